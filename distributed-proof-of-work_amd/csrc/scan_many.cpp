// scan_many.cpp -- host side of the batched scan: dpow_scan_batch's launch loop over the batched
// scan kernel (md5_scan_many.hip) on the launch engine (batch_engine.h) and the host helpers
// dpow_scan_plan and dpow_scan_plan_halve.
//
// Launches.  The tasks are worked in array order, by the planner the batched loops share
// (many_plan.h many_next).  A launch takes tasks from a cursor under two
// budgets: kBatchCap local indices (the cancel latency of DESIGN.md section 11) and a hit weight of
// a quarter of the hit list (scan.cpp's slice rule, summed over the launch's parts: DESIGN.md
// section 17).  Only its last task can be cut, at a multiple of 256 local indices from the task's
// begin, and goes on in the next launch.  A task's part of a launch is cut into workgroup
// descriptors of batch_group(the launch's total) local indices, the last one of a task possibly
// shorter.  One bounded launch is in flight at a time and the cancel flag is checked between
// launches, so a return leaves nothing queued.
//
// After each launch the host sorts the launch's entries -- descriptor order is task order, then
// index order, so the sorted words are in output order -- checks that each names a descriptor of
// the launch and an offset inside it and is listed once, recomputes each with the host MD5
// (scan.cpp's step, where a hit's depth comes from) and appends them whole k by whole k.  The hits
// are staged: nothing is written to the caller's tasks or array before the call's last launch has
// been folded.
//
// Overflow.  A launch whose count exceeds its list's capacity is discarded and its parts planned
// again with both budgets halved, down to one launch of 256 candidates, which cannot overflow a
// list of at least 256 entries; the halved budgets stay until the planner is past the discarded
// launch's end.  The weight budget puts that out of reach of an honest digest;
// DPOW_DIAG_SCAN_MANY_LIST=<256..65536>, read per call, shrinks the capacity without changing the
// plan, which is how the path is tested.
#include "scan_many.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/dpow_worker.h"
#include "batch.h"
#include "batch_engine.h"
#include "ctx.h"
#include "many_plan.h"
#include "md5_host.h"
#include "md5_scan_many.h"
#include "queue.h"
#include "scan.h"

namespace dpow {

namespace {

// The budgets for planning again the parts of a launch of `total` local indices and hit weight
// `weight` whose count overflowed its list: half of each, rounded up to a multiple of 256.
ManyBudget scan_many_halve(uint64_t total, uint64_t weight) {
    const auto half = [](uint64_t x) { return std::max<uint64_t>((x / 2 + 255u) & ~255ull, 256u); };
    return ManyBudget{std::min(half(total), kBatchCap), std::min<uint64_t>(half(weight), kScanCap / 4u)};
}

// DPOW_DIAG_SCAN_MANY_LIST: the capacity of this call's hit lists (the plan stays kScanCap's).
uint32_t scan_many_capacity() {
    if (const char *v = getenv("DPOW_DIAG_SCAN_MANY_LIST")) {
        const long c = atol(v);
        if (c >= (long)kScanMinCap && c <= (long)kScanCap) return (uint32_t)c;
    }
    return kScanCap;
}

// The context's buffers.  Device: the task table in the engine's image area, the control words
// behind it (batch_engine.h) with the launch's hit count at +16, then the hit list and the copy of
// the descriptor table of a launch of kQueueCopyBlocks descriptors or more.  Pinned: the task rows
// of the running call, a launch's descriptors, the list's copy, the count, the record.
constexpr size_t kListBytes = (size_t)kScanCap * sizeof(uint32_t);
constexpr size_t kBlocksBytes = (size_t)kScanManyMaxBlocks * sizeof(BatchEntry);
constexpr size_t kManyCountOff = kEngineCtlOff + 16;  // d_mem
constexpr size_t kManyDevListOff = kEngineDevBytes;
constexpr size_t kManyDevBlocksOff = kManyDevListOff + kListBytes;
constexpr size_t kManyDevBytes = kManyDevBlocksOff + kBlocksBytes;
constexpr size_t kManyRowsOff = 0;  // h_mem
constexpr size_t kManyBlocksOff = kManyRowsOff + DPOW_BATCH_MAX * sizeof(BatchTask);
constexpr size_t kManyOutOff = kManyBlocksOff + kBlocksBytes;
constexpr size_t kManyOutCountOff = kManyOutOff + kListBytes;
constexpr size_t kManyRecOff = kManyOutCountOff + 64;
constexpr size_t kManyHostBytes = kManyRecOff + 64;
static_assert(DPOW_BATCH_MAX * sizeof(BatchTask) <= kEngineImageBytes, "the task table fits the image area");
static_assert(kManyDevListOff % 8 == 0 && kManyDevBlocksOff % 32 == 0, "aligned device sections");
static_assert(kManyBlocksOff % 32 == 0 && kManyOutOff % 8 == 0 && kManyOutCountOff % 8 == 0 && kManyRecOff % 8 == 0,
              "aligned pinned sections");
constexpr EngineSections kManyAt{kManyDevListOff, kManyOutOff, kManyRecOff};

const char *const kWho = "dpow_scan_batch";
const char *const kCapEnv = "DPOW_DIAG_SCAN_MANY_CAP";  // (many_plan.h many_cap)

bool cursor_before(const ManyCursor &a, const ManyCursor &b) {
    return a.task != b.task ? a.task < b.task : a.done < b.done;
}

}  // namespace

struct ScanManyState {
    EngineBuffers buf;
};

namespace {

int scan_many_state(ScanManyState **state, hipStream_t stream) {
    if (*state) return 0;
    ScanManyState *s = new (std::nothrow) ScanManyState();
    if (!s) return set_error(DPOW_ENOMEM, "dpow_scan_batch: out of memory");
    const int rc = engine_alloc(s->buf, kManyDevBytes, kManyHostBytes, stream, scan_many_prepare,
                                "dpow_scan_batch: allocation");
    if (rc < 0) delete s;
    else *state = s;
    return rc;
}

}  // namespace

void scan_many_free(ScanManyState *s) {
    if (!s) return;
    engine_free(s->buf);
    delete s;
}

int scan_many_check(const dpow_scan_task *tasks, size_t n_tasks, const dpow_scan_hit *out, size_t max_hits,
                    const size_t *n_out) {
    if (!tasks || !out || !n_out) return set_error(DPOW_EINVAL, "dpow_scan_batch: NULL argument");
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX)
        return set_error(DPOW_EINVAL, "dpow_scan_batch: n_tasks must be in [1, DPOW_BATCH_MAX]");
    if (max_hits < 256) return set_error(DPOW_EINVAL, "dpow_scan_batch: max_hits below 256 (one k's candidates)");
    return many_check_tasks(tasks, n_tasks, kWho);
}

int scan_many_run(ScanManyState **state, hipStream_t stream, const volatile uint32_t *cancel, dpow_scan_task *tasks,
                  size_t n_tasks, dpow_scan_hit *out, size_t max_hits, size_t *n_out, dpow_batch_stats *stats) {
    const size_t n = n_tasks;
    dpow_batch_stats st{};
    // A task's progress: the hits of its local indices [i_begin, i_done) are staged.
    ManyTasks v = many_tasks(tasks, n);
    std::vector<uint64_t> n_hits(n, 0);
    std::vector<dpow_scan_hit> staged;
    // `unfinished`: the status of every task that is not done, DPOW_MORE or DPOW_CANCELLED.
    const auto write_out = [&](int unfinished, bool cancelled_on_entry) {
        uint64_t first = 0;
        for (size_t i = 0; i < n; ++i) {
            dpow_scan_task &t = tasks[i];
            t.status = v.finished(i, cancelled_on_entry) ? DPOW_EXHAUSTED : unfinished;
            t.k_done = v.k_done(i);
            t.first_hit = first;
            t.n_hits = n_hits[i];
            first += n_hits[i];
        }
        if (!staged.empty()) memcpy(out, staged.data(), staged.size() * sizeof(dpow_scan_hit));
        *n_out = staged.size();
        if (stats) *stats = st;
        return 0;
    };
    if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) return write_out(DPOW_CANCELLED, true);  // no launch
    if (!v.any) return write_out(DPOW_EXHAUSTED, false);  // only empty tasks: no launch

    int rc = scan_many_state(state, stream);
    if (rc < 0) return rc;
    EngineBuffers &s = (*state)->buf;

    // The task table: row i is task i's, with its own ntz and prefilter mask.
    if ((rc = many_upload_tasks(tasks, v, s, kManyRowsOff, stream, kWho)) < 0) return rc;
    const BatchTask *const h_rows = reinterpret_cast<const BatchTask *>(s.h_mem + kManyRowsOff);
    const BatchTask *const d_tasks = reinterpret_cast<const BatchTask *>(s.d_mem);
    BatchEntry *const h_blocks = reinterpret_cast<BatchEntry *>(s.h_mem + kManyBlocksOff);
    const uint32_t *const h_out = reinterpret_cast<const uint32_t *>(s.h_mem + kManyOutOff);
    const unsigned long long *const h_count =
        reinterpret_cast<const unsigned long long *>(s.h_mem + kManyOutCountOff);
    // A short descriptor table is read where it is, in pinned memory, one scalar load per workgroup;
    // a long one is first copied to device memory by the upload kernel (queue.h kQueueCopyBlocks).
    uint32_t *const d_blocks = reinterpret_cast<uint32_t *>(s.d_mem + kManyDevBlocksOff);
    const uint32_t *const p_blocks = reinterpret_cast<const uint32_t *>(s.d_h_mem + kManyBlocksOff);  // pinned
    ScanManyLaunch S{};
    S.count = reinterpret_cast<uint32_t *>(s.d_mem + kManyCountOff);
    S.out_count = reinterpret_cast<unsigned long long *>(s.d_h_mem + kManyOutCountOff);
    S.capacity = scan_many_capacity();
    const auto issue = [&](const BatchLaunch &L) {
        S.L = L;
        hipError_t e = hipSuccess;
        const bool copy = L.n_blocks >= kQueueCopyBlocks;
        if (copy) e = batch_upload(d_blocks, p_blocks, (uint32_t)((size_t)L.n_blocks * sizeof(BatchEntry) / 4), stream);
        if (e == hipSuccess)
            e = scan_many_launch(d_tasks, reinterpret_cast<const BatchEntry *>(copy ? d_blocks : p_blocks), S, stream);
        return e == hipSuccess ? 0 : hip_fail(e, "dpow_scan_batch: launch");
    };

    const ManyBudget full{many_cap(kCapEnv), kScanCap / 4u};
    ManyBudget budget = full;
    ManyCursor cur, halved_until;  // the halved budgets hold while cur is before halved_until
    bool halved = false;
    std::vector<ManyPart> parts;
    std::vector<uint32_t> entries;
    std::vector<uint8_t> msg;
    uint32_t group = 0;
    for (;;) {
        if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) return write_out(DPOW_CANCELLED, false);
        if (halved && !cursor_before(cur, halved_until)) {
            budget = full;
            halved = false;
        }
        const ManyCursor start = cur;
        if (!many_next(v.i_begin.data(), v.i_end.data(), v.ntz.data(), n, budget, cur, parts, group)) break;
        uint64_t total = 0, weight = 0;
        for (const ManyPart &p : parts) {
            total += p.hi - p.lo;
            weight += many_weight(p.hi - p.lo, v.ntz[p.task]);
        }
        const size_t n_blocks = many_write_blocks(parts, group, h_blocks, kScanManyMaxBlocks);
        if (n_blocks == 0)
            return set_error(DPOW_EINVAL, "dpow_scan_batch: the launch plan left the descriptor table");  // never expected
        rc = engine_launch(s, kManyAt, (uint32_t)parts.size(), group, (uint32_t)n_blocks, stream,
                           "dpow_scan_batch: stream idle without the launch's completion record", st, issue);
        if (rc < 0) return rc;
        st.candidates += total;
        const uint64_t count = *h_count;
        if (count > total) return set_error(DPOW_EVERIFY, "dpow_scan_batch: more hits counted than candidates hashed");
        if (count > S.capacity) {  // the list is incomplete: discard it, plan its parts again with half the budgets
            if (!halved || cursor_before(halved_until, cur)) halved_until = cur;
            halved = true;
            budget = scan_many_halve(total, weight);
            cur = start;
            continue;
        }
        entries.assign(h_out, h_out + count);
        std::sort(entries.begin(), entries.end());
        // Every entry is a candidate of this launch, and no other entry is the same one.
        for (size_t q = 0; q < entries.size(); ++q) {
            const uint32_t b = scan_many_entry_block(entries[q]);
            if (b >= n_blocks || scan_many_entry_off(entries[q]) >= h_blocks[b].i_end - h_blocks[b].i_begin ||
                (q > 0 && entries[q - 1] == entries[q]))
                return set_error(DPOW_EVERIFY, "dpow_scan_batch: kernel entry outside its launch or listed twice");
        }
        const auto index_of = [&](size_t q) {  // the local index of entry q
            return h_blocks[scan_many_entry_block(entries[q])].i_begin + scan_many_entry_off(entries[q]);
        };
        size_t j = 0, b_end = 0;  // the next entry; the descriptors of the parts so far
        for (const ManyPart &p : parts) {
            const dpow_scan_task &t = tasks[p.task];
            const uint32_t rb = v.rbits[p.task], base_tb = h_rows[p.task].base_tb;
            b_end += (size_t)((p.hi - p.lo + group - 1) / group);
            md5_msg_of_nonce(msg, t.nonce, t.nonce_len);
            uint64_t prev_k = ~0ull;
            // The part's entries: the entries are sorted and the parts' descriptors follow each other.
            for (; j < entries.size() && scan_many_entry_block(entries[j]) < b_end; ++j) {
                const uint64_t i = index_of(j), k = i >> rb;
                if (k != prev_k) {
                    size_t n_k = 1;  // a k's hits are never split over two calls
                    while (j + n_k < entries.size() && scan_many_entry_block(entries[j + n_k]) < b_end &&
                           (index_of(j + n_k) >> rb) == k)
                        ++n_k;
                    if (staged.size() + n_k > max_hits) {  // `out` is full: this task goes on from k
                        v.i_done[p.task] = k << rb;
                        return write_out(DPOW_MORE, false);
                    }
                    prev_k = k;
                }
                staged.emplace_back();
                if (!scan_fill_hit(msg.data(), t.nonce_len, global_of_local(i, rb, base_tb), v.ntz[p.task], staged.back()))
                    return set_error(DPOW_EVERIFY, "dpow_scan_batch: kernel hit failed host MD5 verification");
                n_hits[p.task]++;
            }
            v.i_done[p.task] = p.hi;
        }
    }
    return write_out(DPOW_EXHAUSTED, false);
}

}  // namespace dpow

using namespace dpow;

extern "C" int dpow_scan_plan(const uint64_t *i_begin, const uint64_t *i_end, const uint32_t *ntz, size_t n_tasks,
                              uint64_t cap, uint32_t capacity, dpow_batch_range *out, size_t max_entries,
                              uint64_t *launches_out) {
    if (!i_begin || !i_end || !ntz || !launches_out) return set_error(DPOW_EINVAL, "dpow_scan_plan: NULL argument");
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX)
        return set_error(DPOW_EINVAL, "dpow_scan_plan: n_tasks must be in [1, DPOW_BATCH_MAX]");
    if (cap == 0) cap = kBatchCap;
    if (cap < 256 || cap > kBatchCap) return set_error(DPOW_EINVAL, "dpow_scan_plan: cap outside [256, 2^28]");
    if (capacity == 0) capacity = kScanCap;
    if (capacity < 1024 || capacity > kScanCap)
        return set_error(DPOW_EINVAL, "dpow_scan_plan: capacity outside [1024, 65536]");
    const ManyBudget budget{cap & ~255ull, (uint64_t)(capacity / 4u) & ~255ull};
    for (size_t i = 0; i < n_tasks; ++i) {
        if (i_begin[i] > i_end[i]) return set_error(DPOW_EINVAL, "dpow_scan_plan: i_begin > i_end");
        if (i_end[i] > (DPOW_K_LIMIT << 8)) return set_error(DPOW_ERANGE, "dpow_scan_plan: i_end beyond DPOW_K_LIMIT");
    }
    ManyCursor cur;
    std::vector<ManyPart> parts;
    uint32_t group = 0;
    uint64_t n_out = 0, launch = 0;
    for (; many_next(i_begin, i_end, ntz, n_tasks, budget, cur, parts, group); ++launch) {
        const size_t n_blocks = many_append_ranges(parts, group, launch, out, max_entries, n_out);
        if (n_blocks > kScanManyMaxBlocks)
            return set_error(DPOW_EINVAL, "dpow_scan_plan: a launch beyond its descriptor bound");  // never expected
        n_out += n_blocks;
        if (n_out > (uint64_t)INT32_MAX) return set_error(DPOW_ERANGE, "dpow_scan_plan: too many entries");
    }
    *launches_out = launch;
    return (int)n_out;
}

extern "C" void dpow_scan_plan_halve(uint64_t total, uint64_t weight, uint64_t *cap_out, uint32_t *capacity_out) {
    const ManyBudget b = scan_many_halve(total, weight);
    if (cap_out) *cap_out = b.cap;
    if (capacity_out) *capacity_out = (uint32_t)(4u * b.weight);
}
