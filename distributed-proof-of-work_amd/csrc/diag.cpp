// diag.cpp -- the dpow_diag_* entry points (include/dpow_diag.h) over the context, the planner
// and the node layer: probes and dumps for tools and tests, off every search's path.
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <thread>
#include <utility>

#include "../../include/dpow_diag.h"
#include "../../include/dpow_worker.h"
#include "ctx.h"
#include "md5_variants.h"

using namespace dpow;

extern "C" {

int dpow_diag_node_post_at(dpow_node_slot *slot, uint64_t global_idx, int64_t t_ns) {
    if (!slot) return set_error(DPOW_EINVAL, "dpow_diag_node_post_at: slot is NULL");
    // One poster thread per process, spinning while requests may come (it exits after 2 s
    // without one): queueing a request costs the caller a lock, not a thread creation --
    // round 3 started a thread per post, on the emulated rank's clock.  The state is never
    // destroyed (the detached thread may still run while the process exits).
    struct Poster {
        std::mutex mu;
        std::vector<std::pair<int64_t, std::pair<dpow_node_slot *, uint64_t>>> q;
        std::atomic<int> pending{0};
        bool alive = false;
    };
    static Poster *const P = new Poster;
    std::lock_guard<std::mutex> g(P->mu);
    P->q.push_back({t_ns, {slot, global_idx}});
    P->pending.fetch_add(1, std::memory_order_release);
    if (!P->alive) {
        P->alive = true;
        std::thread([]() {
            auto mono = []() {
                struct timespec ts;
                clock_gettime(CLOCK_MONOTONIC, &ts);
                return (int64_t)ts.tv_sec * 1000000000 + ts.tv_nsec;
            };
            int64_t idle_since = mono();
            for (;;) {
                if (P->pending.load(std::memory_order_acquire) == 0) {
                    if (mono() - idle_since > 2000000000) {
                        std::lock_guard<std::mutex> g2(P->mu);
                        if (P->pending.load(std::memory_order_acquire) == 0) {
                            P->alive = false;
                            return;
                        }
                    }
                    __builtin_ia32_pause();
                    continue;
                }
                // The earliest request first (a request queued mid-batch with an
                // earlier time waited for the whole batch before): take it, and while waiting
                // for its time go back to the queue whenever another request arrives.
                std::pair<int64_t, std::pair<dpow_node_slot *, uint64_t>> w;
                int rest = 0;  // requests left in the queue when w was taken
                {
                    std::lock_guard<std::mutex> g2(P->mu);
                    auto it = std::min_element(P->q.begin(), P->q.end(),
                                               [](const auto &x, const auto &y) { return x.first < y.first; });
                    w = *it;
                    P->q.erase(it);
                    rest = P->pending.fetch_sub(1, std::memory_order_acq_rel) - 1;
                }
                bool requeued = false;
                for (;;) {
                    const int64_t left = w.first - mono();
                    if (left <= 0) break;
                    if (P->pending.load(std::memory_order_acquire) > rest) {  // a new one: maybe earlier
                        std::lock_guard<std::mutex> g2(P->mu);
                        P->q.push_back(w);
                        P->pending.fetch_add(1, std::memory_order_release);
                        requeued = true;
                        break;
                    }
                    if (left > 100000) {
                        const struct timespec d = {0, (long)std::min<int64_t>(left - 50000, 50000)};
                        nanosleep(&d, nullptr);
                    } else {
                        __builtin_ia32_pause();
                    }
                }
                if (requeued) continue;
                dpow_node_post(w.second.first, w.second.second);
                idle_since = mono();
            }
        }).detach();
    }
    return 0;
}

int dpow_diag_vote_latency(uint32_t world, int reps, double *last_us, double *all_us) {
    if (world < 2 || world > 256 || reps < 1 || !last_us || !all_us)
        return set_error(DPOW_EINVAL, "dpow_diag_vote_latency: world in [2, 256], reps >= 1, outputs non-NULL");
    void *mem = aligned_alloc(64, (size_t)2 * world * sizeof(dpow_node_vote_entry));
    if (!mem) return set_error(DPOW_EINVAL, "dpow_diag_vote_latency: out of memory");
    memset(mem, 0, (size_t)2 * world * sizeof(dpow_node_vote_entry));
    auto *votes = static_cast<dpow_node_vote_entry *>(mem);
    // The ranks on CPUs spread over this thread's affinity set, as a node's processes would be.
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    std::vector<int> cpus;
    if (sched_getaffinity(0, sizeof allowed, &allowed) == 0)
        for (int i = 0; i < CPU_SETSIZE; ++i) {
            if (!CPU_ISSET(i, &allowed)) continue;
            // one hardware thread per core (the first of its siblings): two ranks on SMT
            // siblings would share a core's caches, which a node's processes do not
            char path[96];
            snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", i);
            if (FILE *f = fopen(path, "r")) {
                int first = -1;
                const int n = fscanf(f, "%d", &first);
                fclose(f);
                if (n == 1 && first != i) continue;
            }
            cpus.push_back(i);
        }
    auto pin = [&](uint32_t r) {
        if (cpus.empty()) return;
        cpu_set_t one;
        CPU_ZERO(&one);
        CPU_SET(cpus[(size_t)r * cpus.size() / world], &one);
        (void)pthread_setaffinity_np(pthread_self(), sizeof one, &one);
    };
    std::atomic<int> go{0};
    std::vector<std::atomic<int64_t>> done_at(world);
    for (auto &d : done_at) d.store(0);
    std::atomic<int> failed{0};
    std::vector<std::thread> others;
    for (uint32_t r = 1; r < world; ++r)
        others.emplace_back([&, r]() {
            pin(r);
            for (int rep = 1; rep <= reps; ++rep) {
                while (go.load(std::memory_order_acquire) < rep) __builtin_ia32_pause();
                if (failed.load()) break;  // rank 0 stopped: no rank waits for a vote that will not come
                const int64_t in[3] = {(int64_t)(1000 + r), 1, 1};
                int64_t out[3];
                if (dpow_node_vote(votes, r, world, (uint64_t)rep, in, out, 1000000000) != 0) failed.store(1);
                done_at[r].store(now_ns(), std::memory_order_release);
                while (go.load(std::memory_order_acquire) == rep) __builtin_ia32_pause();  // rank 0 collects
            }
        });
    // Rank 0 (this thread) arrives last: it waits until every other rank has voted and sits in
    // the vote's spin, then votes; last_us is its own vote, all_us the time until every rank
    // holds the result -- the node vote's share of a node's time-to-secret.
    cpu_set_t caller;
    const bool have_caller = pthread_getaffinity_np(pthread_self(), sizeof caller, &caller) == 0;
    pin(0);
    std::vector<double> last, all;
    int64_t t_prev_done = 0;
    for (int rep = 1; rep <= reps && !failed.load(); ++rep) {
        go.store(rep, std::memory_order_release);
        for (uint32_t r = 1; r < world; ++r)
            while (__atomic_load_n(&votes[2 * r + (rep & 1)].epoch, __ATOMIC_ACQUIRE) != (uint64_t)rep &&
                   !failed.load())
                __builtin_ia32_pause();
        for (const int64_t t_wait = now_ns(); now_ns() - t_wait < 2000;) __builtin_ia32_pause();
        const int64_t t0 = now_ns();
        const int64_t in[3] = {1000, 1, 1};
        int64_t out[3];
        if (dpow_node_vote(votes, 0, world, (uint64_t)rep, in, out, 1000000000) != 0 || out[0] != 1000) failed.store(1);
        const int64_t t1 = now_ns();
        int64_t t_all = t1;
        for (uint32_t r = 1; r < world && !failed.load(); ++r) {
            int64_t t;
            while ((t = done_at[r].load(std::memory_order_acquire)) <= t_prev_done && !failed.load())
                __builtin_ia32_pause();
            t_all = std::max(t_all, t);
        }
        t_prev_done = t_all;
        last.push_back((t1 - t0) / 1e3);
        all.push_back((t_all - t0) / 1e3);
    }
    go.store(reps + 1, std::memory_order_release);
    for (auto &t : others) t.join();
    if (have_caller) (void)pthread_setaffinity_np(pthread_self(), sizeof caller, &caller);
    free(mem);
    if (failed.load() || last.empty()) return set_error(DPOW_EPROTO, "dpow_diag_vote_latency: a vote failed");
    std::sort(last.begin(), last.end());
    std::sort(all.begin(), all.end());
    *last_us = last[last.size() / 2];
    *all_us = all[all.size() / 2];
    return 0;
}

namespace {
// The launches of a window as dpow_search sizes them.  recut: a segment-inner launch's claims as
// its kernel gets them (seg_inner_size); without it they stay as size_search_launch cut them, in
// index order, and only n_seg says that the search re-cuts them.
int launch_geometry(const char *who, const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                    uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, uint32_t cus, uint32_t share,
                    int seg_inner_mode, bool recut, dpow_diag_launch *out, size_t max_launches) {
    if (cus == 0 || share == 0) return set_error(DPOW_EINVAL, who);
    WindowPlanner planner;
    const int rc = planner.init(nonce, nonce_len, ntz, worker_byte, worker_bits, k_begin, k_end);
    if (rc < 0) return set_error(rc, who);
    PlannedLaunch pl;
    size_t n = 0;
    LaunchKnobs policy{};
    policy.seg_inner = seg_inner_mode;
    while (planner.next(pl)) {
        if (pl.k0) continue;  // k = 0: the search's k = 0 kernel, not an md5 launch
        // share = searches in flight on the device, as dpow_search sees them (g_active)
        uint64_t wblocks = 0;
        bool seg_inner = false;
        const int r = size_window_launch(planner, pl, ntz, cus, share, policy, &wblocks, &seg_inner, recut);
        if (r < 0) return set_error(r, who);
        if (out && n < max_launches) {
            dpow_diag_launch &d = out[n];
            d.k_begin = pl.info.k_begin;
            d.k_end = pl.info.k_end;
            d.i_begin = pl.L.i_begin;
            d.i_end = pl.L.i_end;
            d.wb_begin = pl.L.wb_begin;
            d.n_wblocks = pl.L.n_wblocks;
            d.n_big = pl.L.n_big;
            d.n_chunks = pl.L.n_chunks;
            d.worker_blocks = wblocks;
            d.chunk = pl.L.chunk;
            d.chunk_tail = pl.L.chunk_tail;
            d.rbits = pl.L.rbits;
            d.wave_block = kWaveBlock;
            d.n_static = pl.L.n_static;
            d.poll_wb = pl.L.poll_wb;
            d.n_seg = pl.L.n_seg;
        }
        ++n;
    }
    return (int)n;
}
}  // namespace

int dpow_diag_launch_geometry(const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                              uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, uint32_t cus, uint32_t share,
                              dpow_diag_launch *out, size_t max_launches) {
    return launch_geometry("dpow_diag_launch_geometry: bad arguments or grid", nonce, nonce_len, ntz, worker_byte,
                           worker_bits, k_begin, k_end, cus, share, -1, false, out, max_launches);
}

int dpow_diag_seg_inner_geometry(const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                                 uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, uint32_t cus, int mode,
                                 dpow_diag_launch *out, size_t max_launches) {
    return launch_geometry("dpow_diag_seg_inner_geometry: bad arguments or grid", nonce, nonce_len, ntz,
                           worker_byte, worker_bits, k_begin, k_end, cus, 1, mode, true, out, max_launches);
}

int dpow_diag_seg_inner_candidate(const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                                  uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, int mode,
                                  uint64_t local_idx, uint32_t iv_out[4], uint32_t words_out[32],
                                  uint32_t *nblk_out) {
    if (!iv_out || !words_out || !nblk_out)
        return set_error(DPOW_EINVAL, "dpow_diag_seg_inner_candidate: NULL argument");
    WindowPlanner planner;
    const int rc = planner.init(nonce, nonce_len, ntz, worker_byte, worker_bits, k_begin, k_end);
    if (rc < 0) return set_error(rc, "dpow_diag_seg_inner_candidate: bad arguments");
    PlannedLaunch pl;
    LaunchKnobs policy{};
    policy.seg_inner = mode;
    while (planner.next(pl)) {
        if (pl.k0) continue;
        uint64_t wblocks = 0;
        bool seg_inner = false;
        const int r = size_window_launch(planner, pl, ntz, 256, 1, policy, &wblocks, &seg_inner);
        if (local_idx < pl.L.i_begin || local_idx >= pl.L.i_end) continue;
        if (r < 0) return set_error(r, "dpow_diag_seg_inner_candidate: sizing failed");
        for (int w = 0; w < 4; ++w) iv_out[w] = pl.L.iv[w];
        memset(words_out, 0, 32 * sizeof(uint32_t));
        candidate_words(pl, local_idx, words_out);
        *nblk_out = pl.info.nblk;
        return seg_inner ? 1 : 0;
    }
    return set_error(DPOW_EINVAL, "dpow_diag_seg_inner_candidate: index outside the window");
}

int dpow_diag_node_alias(dpow_ctx *c, void **cached, void **lookup) {
    if (!c || !cached || !lookup) return set_error(DPOW_EINVAL, "dpow_diag_node_alias: NULL argument");
    if (!c->node) return set_error(DPOW_EINVAL, "dpow_diag_node_alias: no slot attached");
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    *cached = c->d_node;
    DPOW_HIP(hipHostGetDevicePointer(lookup, c->node, 0));
    return 0;
}

int dpow_diag_search_times(dpow_ctx *c, int64_t out[8]) {
    if (!c || !out) return set_error(DPOW_EINVAL, "dpow_diag_search_times: NULL argument");
    for (int i = 0; i < 8; ++i) out[i] = c->diag_t[i];
    return 0;
}

int dpow_diag_search_launches(dpow_ctx *c, int64_t *t0_ns, dpow_diag_launch_time *out, size_t max_launches) {
    if (!c || !t0_ns) return set_error(DPOW_EINVAL, "dpow_diag_search_launches: NULL argument");
    *t0_ns = c->diag_t0;
    const size_t n = c->diag_nl;
    for (size_t i = 0; out && i < n && i < max_launches; ++i) {
        const dpow_ctx::DiagLaunch &d = c->diag_l[i];
        dpow_diag_launch_time &o = out[i];
        o.seq = d.seq;
        o.kind = d.kind;
        o.queued_ns = d.queued;
        o.seen_ns = d.seen;
        o.candidates = d.candidates;
        o.g_end = d.g_end;
        const Snap &sn = c->h_snap[d.seq % kRing];
        const bool rec = __atomic_load_n(&sn.seq, __ATOMIC_ACQUIRE) == (uint32_t)(d.seq + 1);
        o.recorded = rec ? 1 : 0;
        o.t_start_tick = rec ? sn.t_start : 0;
        o.t_end_tick = rec ? sn.t_end : 0;
        o.best = rec ? sn.best : DPOW_NO_HIT;
    }
    return (int)n;
}

int dpow_diag_clock_sync(dpow_ctx *c, int reps, int64_t *offset_ns) {
    if (!c || !offset_ns || reps < 1) return set_error(DPOW_EINVAL, "dpow_diag_clock_sync: bad argument");
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e, "dpow_diag_clock_sync: hipStreamSynchronize");
    unsigned long long *h = nullptr, *d = nullptr;
    if ((e = hipHostMalloc(&h, 64, hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess)
        return hip_fail(e, "dpow_diag_clock_sync: hipHostMalloc");
    if ((e = hipHostGetDevicePointer(reinterpret_cast<void **>(&d), h, 0)) != hipSuccess) {
        (void)hipHostFree(h);
        return hip_fail(e, "dpow_diag_clock_sync: hipHostGetDevicePointer");
    }
    int64_t best = INT64_MAX;
    int rc = 0;
    for (int r = 0; r < reps && rc == 0; ++r) {
        __atomic_store_n(h, 0ull, __ATOMIC_RELEASE);
        if ((e = clock_probe(d, c->stream)) != hipSuccess) {
            rc = hip_fail(e, "dpow_diag_clock_sync: clock_probe");
            break;
        }
        const int64_t t_launch = now_ns();
        unsigned long long tick = 0;
        int64_t t = 0;
        while ((tick = __atomic_load_n(h, __ATOMIC_ACQUIRE)) == 0ull) {
            t = now_ns();
            if (t - t_launch > 1000000000) {
                rc = set_error(DPOW_EHIP, "dpow_diag_clock_sync: the probe's stamp never arrived");
                break;
            }
            __builtin_ia32_pause();
        }
        if (rc) break;
        t = now_ns();
        // The stamp reached host memory at or before t: the least delayed pairing bounds the offset.
        const int64_t off = t - (int64_t)((double)tick * kRealtimeNs);
        if (off < best) best = off;
    }
    e = hipStreamSynchronize(c->stream);
    if (rc == 0 && e != hipSuccess) rc = hip_fail(e, "dpow_diag_clock_sync: hipStreamSynchronize");
    (void)hipHostFree(h);
    if (rc == 0) *offset_ns = best;
    return rc;
}

uint64_t dpow_diag_blocks_per_cu(uint64_t candidates, uint32_t ntz, uint32_t worker_bits) {
    return launch_blocks_per_cu(candidates, ntz, remainder_bits(worker_bits));
}

int dpow_diag_dword_test(const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint64_t k, uint32_t iv_d,
                         uint32_t state_d) {
    std::vector<PlannedLaunch> plan;
    const int n = plan_window(nonce, nonce_len, ntz, 0, 0, k, k + 1, plan);
    if (n != 1) return set_error(n < 0 ? n : DPOW_EINVAL, "dpow_diag_dword_test: bad arguments");
    const Launch &L = plan[0].L;
    const uint32_t nblk = plan[0].info.nblk;
    // one final block: the chaining value is the planner's (midstate or RFC IV)
    if (nblk == 1 && iv_d != L.iv[3]) return set_error(DPOW_EINVAL, "dpow_diag_dword_test: iv_d != iv[3]");
    const uint32_t D = iv_d + state_d;
    const bool pre = use_d_equality(nblk, ntz) ? state_d == L.deq : D <= L.dle;
    return pre && (D & L.dmask) == 0u ? 1 : 0;
}

}  // extern "C"
