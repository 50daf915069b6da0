// search.cpp -- the driver of dpow_search: its launches, its completion records, its bounds.
//
// dpow_search replaces the reference miner's enumeration loop
// (worker.go:301-400): plan the window into launches (plan.cpp), queue them on
// the context's stream (behind the k = 0 kernel when the window holds k = 0) with at most kDepth in flight,
// and re-verify a hit with the host MD5 before returning it.  Each launch's
// last retiring workgroup writes a completion record (the control block as of
// the end of the launch) to pinned host memory; the host polls that record rather
// than synchronising on events, so a hit is seen one PCIe write after the
// kernel publishes it.  Launches queued behind a hit (or a cancel) are not
// waited for: they retire at once (every worker wave compares its first index
// against Ctrl::best / Ctrl::stop before hashing), in stream order ahead of
// the next search on the context.
#include <string.h>
#include <time.h>

#include <algorithm>

#include "ctx.h"
#include "md5_variants.h"

namespace dpow {

std::atomic<int> g_active[kMaxDevices];
std::mutex g_ctx_mu;
std::vector<dpow_ctx *> g_ctxs;

namespace {

// Internal status of consume(): the window holds nothing below a bound injected
// by dpow_search_bound (reported as DPOW_EXHAUSTED).
constexpr int DPOW_BOUNDED = 3;

// Completion-record wait: spin for the first kSpinNs of a search (time-to-secret) -- or
// longer, up to kSpinMaxNs, for twice the time its first hit is expected in (round 3 spun for
// 200 us only, so an 8-GPU rank's N = 7 search, whose hit comes ~200 us in, saw its records
// and posted its hit one 5-7 us sleep late) -- then poll at kPollNs (20 us in round 2: a
// record waited up to that long to be seen once a search ran past the spin; the thread
// sleeps between polls either way).
constexpr int64_t kSpinNs = 200000;
constexpr int64_t kSpinMaxNs = 4000000;
constexpr long kPollNs = 5000;
constexpr int64_t kNoDeadline = INT64_MAX;
// Deferred queueing.  A launch is queued only once the launches ahead of it are
// expected to finish within kQueueLeadNs, so a hit leaves (almost) nothing queued
// behind it: every queued launch of a persistent grid costs 10-20 us of dispatch
// and retirement even when it claims nothing (profiles/r02_tts_timeline.json),
// which the next search on the stream, and a device synchronize, wait out.  The
// estimate is early on purpose (kEstRate is above every layout's measured rate,
// the fixed cost below the measured one), so a window without a hit runs its
// launches back to back.
constexpr int64_t kQueueLeadNs = 60000;
// (kEstRate: plan.h)
constexpr int64_t kEstFixedNs = 8000;

struct ActiveSearch {
    int dev;
    explicit ActiveSearch(int d) : dev(d) { g_active[dev].fetch_add(1, std::memory_order_relaxed); }
    ~ActiveSearch() { g_active[dev].fetch_sub(1, std::memory_order_relaxed); }
};

// Per-search wait state: the search's start (the spin window), the caller thread's
// timer slack (lowered for the sleeping polls, restored when the search returns --
// the thread is the caller's own, e.g. a cgo goroutine's), and the node slot
// (dpow_node_attach) as last seen.
struct SearchWait {
    int64_t t0 = now_ns();
    int64_t spin_ns = kSpinNs;  // spin_for(): this search's spin window
    TimerSlack slack;
    uint64_t node_seen = DPOW_NO_HIT;  // lowest node best injected into this search
    bool node_stop = false;            // the node slot's stop was seen
    // Early Found fan-out (attached node): the pinned word the running launch's watcher relays
    // Ctrl::best to, the lowest value seen there, and what a hit is verified against.
    const uint64_t *early = nullptr;
    uint64_t early_seen = DPOW_NO_HIT;
    uint64_t own_posted = DPOW_NO_HIT;  // the lowest hit of ours posted early: the slot's best, not a bound
    // Every candidate of this window below `covered` has been searched without a hit: the
    // g_end of the last consumed launch (round 5).  Once an injected bound (another rank's
    // hit, dpow_search_bound) is at or below it, the search is over -- the launches still in
    // flight hold nothing below the bound -- and it returns without waiting for their drain.
    uint64_t covered = 0;
    const uint8_t *nonce = nullptr;
    size_t nonce_len = 0;
    uint32_t ntz = 0;
    uint32_t rbits = 8, base_tb = 0;    // the partition: g is ours iff (g & 255) >> rbits == base_tb >> rbits
};

// The node slot, polled between record polls: a lower best of another rank is
// injected as a bound; a stop marks every launch queued so far stale, so their
// watchers stop them (the search then returns DPOW_CANCELLED).
int poll_node(dpow_ctx *c, SearchWait &sw) {
    dpow_node_slot *n = c->node;
    if (!n) return 0;
    const uint64_t nb = __atomic_load_n(&n->best, __ATOMIC_ACQUIRE);
    if (nb < sw.node_seen) {
        // The running launch's watcher lowers Ctrl::best to it on the device; the host
        // keeps the injected bound (ext_bound) that tells another rank's index from ours.
        // Our own hit, posted early (poll_early), is not a bound.
        sw.node_seen = nb;
        if (nb != sw.own_posted) {
            std::lock_guard<std::mutex> g(c->bound_mu);
            uint64_t cur = c->ext_bound.load(std::memory_order_relaxed);
            if (nb < cur) c->ext_bound.store(nb, std::memory_order_release);
        }
    }
    if (!sw.node_stop && __atomic_load_n(&n->stop, __ATOMIC_ACQUIRE) != 0u) {
        sw.node_stop = true;
        __atomic_store_n(&c->h_cancel[kStaleWord], (uint32_t)c->seq, __ATOMIC_RELEASE);
    }
    return 0;
}

// The early-hit word (attached node): a value below what was seen there is this launch's
// Ctrl::best -- a hit of ours, or a bound that is itself a hit of another rank.  It is
// verified with the host MD5 and posted to the node slot at once, so the other ranks stop at
// it while this launch drains; the search's final answer is still taken from the records.
void poll_early(dpow_ctx *c, SearchWait &sw) {
    const uint64_t g = __atomic_load_n(sw.early, __ATOMIC_ACQUIRE);
    if (g >= sw.early_seen) return;
    sw.early_seen = g;
    // only a hit of this search's partition (Ctrl::best also holds the bounds the watcher relays)
    if ((((uint32_t)g & 0xFFu) >> sw.rbits) != (sw.base_tb >> sw.rbits)) return;
    uint8_t sec[DPOW_MAX_SECRET];
    size_t len = 0;
    if (dpow_secret_from_index(g, sec, &len) != 0) return;
    if (!dpow_verify(sw.nonce, sw.nonce_len, sec, len, sw.ntz)) return;  // not a hit (a bound): left to the record
    if (g < sw.own_posted) sw.own_posted = g;  // before the post: poll_node must not take it for a bound
    dpow_node_post(c->node, g);
    if (c->diag_t[7] < 0) c->diag_t[7] = now_ns() - sw.t0;
}

// Wait for the completion record of launch `seq`, until `deadline` (now_ns()
// clock; kNoDeadline: none).  Returns 1 when the record is there, 0 at the
// deadline, 2 when an injected bound reached what the consumed launches cover
// (SearchWait::covered: nothing of ours is left below it), < 0 on error.  Spins in the first kSpinNs of the search (the record
// of a launch holding a hit is the time-to-secret path), then sleeps between
// polls; the stream is queried now and then so a failed launch, or a stream
// that went idle without writing the record, ends the wait with an error.
int wait_record(dpow_ctx *c, uint64_t seq, int64_t deadline, SearchWait &sw) {
    const uint32_t *p = &c->h_snap[seq % kRing].seq;
    const uint32_t want = (uint32_t)(seq + 1);
    for (uint64_t it = 1;; ++it) {
        if (__atomic_load_n(p, __ATOMIC_ACQUIRE) == want) return 1;
        const int64_t t = now_ns();
        if (t >= deadline) return 0;
        const bool spinning = t - sw.t0 < sw.spin_ns;
        if (spinning ? (it % 4096 == 0) : (it % 16 == 0)) {
            const int alive = stream_liveness(c->slots[seq % kRing].stream, p, want,
                                              "dpow_search: stream idle without the launch's completion record");
            if (alive != 0) return alive;
        }
        if (sw.early && (!spinning || it % 8 == 0)) poll_early(c, sw);
        if (!spinning || it % 64 == 0) {
            if (c->node) {
                const int rc = poll_node(c, sw);
                if (rc < 0) return rc;
            }
            if (c->ext_bound.load(std::memory_order_acquire) <= sw.covered) return 2;
        }
        if (spinning) {
            __builtin_ia32_pause();
        } else {
            sw.slack.lower();
            int64_t ns = kPollNs;
            if (deadline != kNoDeadline && deadline - t < ns) ns = deadline - t;
            const struct timespec ts = {0, (long)ns};
            nanosleep(&ts, nullptr);
        }
    }
}

// Before a record slot is reused: a launch whose record was never consumed (queued behind
// a hit, a cancel or an error, possibly on the other stream) may still be running; wait
// for its record, so it cannot land on the slot's next user.
int retire_slot(dpow_ctx *c, LaunchSlot &s) {
    if (!s.in_flight) return 0;
    const uint32_t *p = &c->h_snap[s.seq % kRing].seq;
    const uint32_t want = (uint32_t)(s.seq + 1);
    for (uint64_t it = 1; __atomic_load_n(p, __ATOMIC_ACQUIRE) != want; ++it) {
        if (it % 1024 == 0) {
            const int alive = stream_liveness(s.stream, p, want,
                                              "dpow_search: stream idle without a queued launch's completion record");
            if (alive < 0) return alive;
            if (alive > 0) break;
        }
        __builtin_ia32_pause();
    }
    s.in_flight = false;
    return 0;
}

// Contexts of `device` used within kRecentNs (the young-search rule above).
int recent_contexts(int device) {
    const int64_t t = now_ns();
    int n = 0;
    std::lock_guard<std::mutex> g(g_ctx_mu);
    for (dpow_ctx *x : g_ctxs)
        if (x->device == device && t - x->last_use.load(std::memory_order_relaxed) < kRecentNs) ++n;
    return n;
}

// One search in flight: what its steps share -- queue the k = 0 launch, queue one md5 launch,
// consume one record -- and what every return, an error's too, owes the context (the
// destructor).  search_window below is the policy that orders the steps.
struct Search {
    dpow_ctx *const c;
    WindowPlanner &planner;
    const uint32_t ntz;
    const uint64_t bound;  // the caller's: nothing at or above it is a hit
    SearchWait sw;
    const uint64_t seq0 = c->seq;
    PlannedLaunch pl;  // the launch to queue next, if `have`
    bool have = false;
    size_t launched = 0, consumed = 0;
    int64_t busy_until = 0;  // expected end of the launches queued so far (now_ns clock)
    // This search's control block (clean: reset by the previous search's launches, or at
    // dpow_open); its md5 launches reset the next one.
    Ctrl *const ctrl = c->d_ctrl + (size_t)c->ctrl_idx * kCtrlStride;
    Ctrl *const ctrl_next = c->d_ctrl + (size_t)((c->ctrl_idx + 1) % kCtrlRing) * kCtrlStride;
    bool md5_queued = false;
    uint64_t bound0 = DPOW_NO_HIT;  // Launch::bound0: the lower of the caller's bound and the node slot's best
    bool window_open = false;       // open_bound_window() ran
    uint32_t done_target = 0;
    uint64_t best = bound;

    Search(dpow_ctx *cc, WindowPlanner &p, uint32_t n, uint64_t b) : c(cc), planner(p), ntz(n), bound(b) {}
    ~Search() {
        // Launches still queued when the search returns -- behind a hit, a bound, a
        // cancel or an error -- are marked stale, so their watchers stop them at once
        // even if the caller clears the cancel flag for its next task before they
        // start.
        if (consumed < launched) __atomic_store_n(&c->h_cancel[kStaleWord], (uint32_t)c->seq, __ATOMIC_RELEASE);
        if (window_open) {
            std::lock_guard<std::mutex> g(c->bound_mu);
            c->searching = false;
        }
        // once an md5 launch is queued, the next search uses the next block
        if (md5_queued) c->ctrl_idx = (c->ctrl_idx + 1) % kCtrlRing;
    }

    // Launch `launched` of the search is on the stream: the diagnostics' launch list, its slot.
    void queued(int32_t kind, uint64_t cands, uint64_t g_end) {
        const size_t li = launched++;
        const uint64_t seq = seq0 + li;
        if (li < dpow_ctx::kDiagLaunches) {
            c->diag_l[li] = {seq, cands, g_end, kind, now_ns(), -1};
            c->diag_nl = li + 1;
        }
        c->slots[seq % kRing] = {seq, true, cands, g_end, c->stream};
        c->seq = seq + 1;
    }

    // Open the window for dpow_search_bound (the bound word starts at "none" for this
    // search; stale launches of the previous one may still read it, harmlessly).
    void open_bound_window(uint64_t node_best) {
        bound0 = node_best < bound ? node_best : bound;
        std::lock_guard<std::mutex> g(c->bound_mu);
        c->ext_bound.store(node_best, std::memory_order_relaxed);
        __atomic_store_n(bound_word(c), (uint64_t)DPOW_NO_HIT, __ATOMIC_RELEASE);
        c->searching = true;
        window_open = true;
    }

    // A window holding k = 0 starts with the k = 0 kernel (search_ctrl.hip), ahead of the
    // first md5 launch on the search stream: launch 0 of the search, with a completion record
    // of its own that holds its own first hit only.  (On a second stream beside the first md5
    // launch it started 2-4 us sooner, but one more busy device queue per process pushed 8
    // processes sharing a GPU into queue oversubscription: profiles/r03_rehearsal_queues.json.)
    int queue_k0() {
        const int rc = retire_slot(c, c->slots[seq0 % kRing]);
        if (rc < 0) return rc;
        c->diag_t[5] = now_ns() - sw.t0;
        StartK0 k0{};
        k0.r = (uint32_t)(pl.L.i_end - pl.L.i_begin);
        k0.base_tb = pl.L.base_tb;
        k0.nblk = pl.info.nblk;
        k0.p = 4 * pl.info.w0 + pl.info.sh;
        k0.ntz = ntz;
        k0.seq = (uint32_t)(seq0 + 1);
        k0.snap = c->d_snap + seq0 % kRing;
        memcpy(k0.iv, pl.L.iv, sizeof k0.iv);
        memcpy(k0.T, pl.L.T, sizeof k0.T);
        const hipError_t e = search_k0(k0, c->stream);
        if (e != hipSuccess) return hip_fail(e, "search_k0");
        c->diag_t[0] = now_ns() - sw.t0;
        queued(0, k0.r, 1ull << 8);
        have = planner.next(pl);
        return 0;
    }

    // Size pl for this search's share of the device, queue it and plan the launch after it.
    int queue_md5() {
        const size_t li = launched;
        const uint64_t seq = seq0 + li;
        int rc = retire_slot(c, c->slots[seq % kRing]);  // the slot's previous user
        if (rc < 0) return rc;
        if (!md5_queued) c->diag_t[6] = now_ns() - sw.t0;
        Launch &L = pl.L;
        // This search's share of the device's resident workgroups (searches sharing the device:
        // plan.h grid_share, cap_shared_launch).
        uint64_t active = (uint64_t)std::max(1, g_active[c->device].load(std::memory_order_relaxed));
        if (active == 1 && !c->solo && now_ns() - sw.t0 < kYoungNs) {
            // A young search that looks alone while other contexts of this process were used on
            // the device recently plans as if they all searched: its first long launch no longer
            // takes the whole device for its full length just because it registered first
            // (round 4: one 16-28 ms full-device launch, config 4's one nonce 8.5-23 ms over runs).
            const int recent = recent_contexts(c->device);
            if (recent > 1) active = (uint64_t)recent;
        }
        uint64_t worker_blocks = 0;
        bool seg_inner = false;
        rc = size_window_launch(planner, pl, ntz, c->cus, active, c->knobs, &worker_blocks, &seg_inner);
        if (rc < 0) return set_error(rc, "dpow_search: launch grid leaves a claim counter without waves");
        done_target += (uint32_t)worker_blocks;  // retirement is counted per workgroup
        L.claim = c->d_claims + (li % kClaimRing) * kClaimSlot;
        L.done_target = done_target;
        L.ctrl = ctrl;
        L.ctrl_next = ctrl_next;
        L.bound0 = bound0;
        L.cancel = c->d_cancel;
        L.stale = c->d_cancel + kStaleWord;
        L.ext_bound = reinterpret_cast<const unsigned long long *>(c->d_cancel + kBoundWord);
        L.snap = c->d_snap + seq % kRing;
        L.seq = (uint32_t)(seq + 1);
        L.node_best = c->d_node ? reinterpret_cast<const unsigned long long *>(&c->d_node->best) : nullptr;
        L.node_stop = c->d_node ? &c->d_node->stop : nullptr;
        L.early = c->d_node ? reinterpret_cast<unsigned long long *>(c->d_cancel + kEarlyWord) + c->ctrl_idx : nullptr;
        const hipError_t e = search_launch((int)pl.info.nblk, (int)pl.info.w0, (int)pl.info.sh, L,
                                           (uint32_t)(worker_blocks + 1), c->stream);
        if (e != hipSuccess) return hip_fail(e, "search_launch");
        if (!md5_queued) c->diag_t[1] = now_ns() - sw.t0;
        queued(L.n_seg != 0u ? 2 : 1, L.i_end - L.i_begin, pl.info.k_end << 8);
        md5_queued = true;
        const int64_t t = now_ns();
        busy_until = std::max(busy_until, t) + kEstFixedNs +
                     (int64_t)((double)(L.i_end - L.i_begin) * (double)active / kEstRate * 1e9);
        have = planner.next(pl);
        return 0;
    }

    // Consume the completion record of the oldest launch in flight (in launch order): FOUND or
    // CANCELLED ends the search, EXHAUSTED goes on, < 0 is an error.  Ctrl::best
    // persists across the launches of a search and later launches hold higher
    // indices, so the first record below the bound carries the answer.
    int consume() {
        const size_t lj = consumed;
        const uint64_t seq = seq0 + lj;
        const int rc = wait_record(c, seq, kNoDeadline, sw);
        if (rc < 0) return rc;
        if (rc == 2) return DPOW_BOUNDED;  // the launch stays in flight; marked stale on return
        LaunchSlot &slot = c->slots[seq % kRing];
        const Snap &sn = c->h_snap[seq % kRing];
        slot.in_flight = false;
        c->stats.launches++;
        c->stats.candidates += slot.candidates;
        if (sn.t_start != 0ull && sn.t_end >= sn.t_start)
            c->stats.kernel_ms += (double)(sn.t_end - sn.t_start) * kRealtimeNs * 1e-6;
        if (consumed == 0) c->diag_t[2] = now_ns() - sw.t0;
        if (lj < dpow_ctx::kDiagLaunches) c->diag_l[lj].seen = now_ns();
        consumed = lj + 1;
        // The watcher may have put the node slot's best into Ctrl::best before this thread
        // saw it: read the slot now (its best only decreases) so ext_bound covers it.
        if (c->node) {
            const int prc = poll_node(c, sw);
            if (prc < 0) return prc;
        }
        if (sn.best < bound) {
            // Ctrl::best = min(this search's hits, bounds injected by dpow_search_bound
            // or from the node slot).  At or above the lowest injected bound it is not a
            // hit of ours.  The search is over only when that bound lies within the
            // launches consumed so far (every candidate below it has been searched);
            // otherwise the later launches still hold candidates below it: go on
            // (they skip chunks at or above Ctrl::best, and a hit of ours there shows
            // in their records as a value below the bound).
            const uint64_t eb = c->ext_bound.load(std::memory_order_acquire);
            if (sn.best >= eb) return eb <= slot.g_end ? DPOW_BOUNDED : DPOW_EXHAUSTED;
            best = sn.best;
            return DPOW_FOUND;
        }
        if (sn.stop != 0u || sw.node_stop || __atomic_load_n(c->h_cancel, __ATOMIC_ACQUIRE) != 0u)
            return DPOW_CANCELLED;
        sw.covered = slot.g_end;
        if (c->ext_bound.load(std::memory_order_acquire) <= sw.covered) return DPOW_BOUNDED;
        return DPOW_EXHAUSTED;
    }
};

}  // namespace

// The body of dpow_search (arguments checked).
int search_window(dpow_ctx *c, const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                  uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, uint64_t *best_global_idx,
                  uint8_t secret_out[DPOW_MAX_SECRET], size_t *secret_len) {
    WindowPlanner planner;
    int rc = planner.init(nonce, nonce_len, ntz, worker_byte, worker_bits, k_begin, k_end);
    if (rc < 0) return set_error(rc, "dpow_search: planning failed");
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    if (c->device >= kMaxDevices) return set_error(DPOW_EINVAL, "dpow_search: device ordinal too large");
    const ActiveSearch active(c->device);
    Search s(c, planner, ntz, *best_global_idx);
    SearchWait &sw = s.sw;
    {   // Spin while the first hit is expected (memoryless: from any start), 2x, within [kSpinNs,
        // kSpinMaxNs].  The expected time is at this search's share of the device (the searches
        // in flight on it).  A search whose hit is not expected within a few spin windows (the
        // sweep, N >= 9, N = 8 on one GPU) spins kSpinNs only: busy-spinning a host core for
        // 4 ms of a long search buys nothing.
        const double searches = (double)std::max(1, g_active[c->device].load(std::memory_order_relaxed));
        const double expect_ns =
            (double)expected_first_hit(ntz, remainder_bits(worker_bits)) / kEstRate * 1e9 * searches;
        sw.spin_ns = expect_ns > 2.0 * (double)kSpinMaxNs
                         ? kSpinNs
                         : (int64_t)std::min<double>(std::max<double>(2.0 * expect_ns, (double)kSpinNs),
                                                     (double)kSpinMaxNs);
    }

    {   // keep the stale mark within 2^30 launches of the present (int32 distance in the watcher)
        uint32_t *st = &c->h_cancel[kStaleWord];
        const uint32_t next = (uint32_t)(c->seq + 1);
        if ((int32_t)(next - __atomic_load_n(st, __ATOMIC_RELAXED)) > (1 << 30))
            __atomic_store_n(st, next - (1u << 30), __ATOMIC_RELAXED);
    }
    // Another rank's hit already on the node slot bounds this search from the start
    // (as an injected bound: a record at or above it is not a hit of ours).
    const uint64_t node_best = c->node ? __atomic_load_n(&c->node->best, __ATOMIC_ACQUIRE) : DPOW_NO_HIT;
    sw.node_seen = node_best;
    sw.covered = k_begin << 8;  // nothing of this window is searched yet
    for (int64_t &t : c->diag_t) t = -1;
    c->diag_nl = 0;
    c->diag_t0 = sw.t0;
    if (c->node) {  // the early Found fan-out: this search's control block's early-hit word
        uint64_t *ew = reinterpret_cast<uint64_t *>(c->h_cancel + kEarlyWord) + c->ctrl_idx;
        __atomic_store_n(ew, (uint64_t)DPOW_NO_HIT, __ATOMIC_RELEASE);
        sw.early = ew;
        sw.nonce = nonce;
        sw.nonce_len = nonce_len;
        sw.ntz = ntz;
        sw.rbits = remainder_bits(worker_bits);
        sw.base_tb = base_thread_byte(worker_byte, worker_bits);
    }
    s.have = planner.next(s.pl);
    c->diag_t[4] = now_ns() - sw.t0;
    if (s.have && s.pl.k0 && (rc = s.queue_k0()) < 0) return rc;
    s.open_bound_window(node_best);

    int status = DPOW_EXHAUSTED;
    while (status == DPOW_EXHAUSTED && s.have) {
        if (sw.node_stop) {
            status = DPOW_CANCELLED;
            break;
        }
        int w = 0;  // wait_record's answer for the oldest launch; 1: consume its record before queueing more
        if (s.launched - s.consumed >= kDepth) {  // the record of the oldest launch decides whether to go on
            w = 1;
        } else if (s.launched > s.consumed && s.busy_until - now_ns() > kQueueLeadNs) {
            // Deferred queueing: wait for the oldest record until the launches ahead
            // are expected to be within kQueueLeadNs of their end.
            w = wait_record(c, s.seq0 + s.consumed, s.busy_until - kQueueLeadNs, sw);
            if (w < 0) return w;
        }
        if (w != 0) {
            const int r = w == 2 ? DPOW_BOUNDED : s.consume();
            if (r < 0) return r;
            if (r != DPOW_EXHAUSTED) status = r;
            continue;
        }
        {   // a launch wholly at or above the bound (the caller's, an injected one) holds nothing
            const uint64_t eb = c->ext_bound.load(std::memory_order_acquire);
            if ((s.pl.info.k_begin << 8) >= (eb < s.bound ? eb : s.bound)) break;
        }
        if ((rc = s.queue_md5()) < 0) return rc;
    }
    while (status == DPOW_EXHAUSTED && s.consumed < s.launched) {  // the window is queued: drain in order
        const int r = s.consume();
        if (r < 0) return r;
        status = r;
    }
    if (status == DPOW_BOUNDED) status = DPOW_EXHAUSTED;  // no hit below the (injected) bound
    c->diag_t[3] = now_ns() - sw.t0;

    if (status == DPOW_FOUND) {
        dpow_secret_from_index(s.best, secret_out, secret_len);
        if (!dpow_verify(nonce, nonce_len, secret_out, *secret_len, ntz)) {
            *secret_len = 0;
            return set_error(DPOW_EVERIFY, "dpow_search: kernel hit failed host MD5 verification");
        }
        *best_global_idx = s.best;
    }
    return status;
}

}  // namespace dpow
