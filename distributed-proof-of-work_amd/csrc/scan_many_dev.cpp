// scan_many_dev.cpp -- host side of the batched device scan: dpow_scan_batch_device's launch loop
// over the kernels of md5_scan_many_dev.hip on the launch engine (batch_engine.h), and the host
// helper dpow_scan_batch_device_settle.
//
// Launches.  The tasks are worked in array order and the launches are the batched census's
// (many_plan.h many_next, without a weight budget): a launch takes tasks from a cursor until it
// holds kBatchCap local indices, only its last task can be cut, at a multiple of 256 local indices from the task's begin, and a task's
// part is cut into workgroup descriptors of batch_group(the launch's total).  The list has no
// capacity, hence no hit budget and no overflow path.  A launch of the plan is one mask launch,
// whose completion record the host waits for, and behind it without a wait the rows launch (the row
// pointers of the tasks that begin in it), the place launch and the depth launch, which re-checks
// every entry placed.  The host touches no hit: it reads the launch's total from pinned memory and,
// if the total fits the room left, queues the three for the whole launch; if not -- once per call at
// most, as the call ends there -- it copies the launch's prefix out, decides how many leading
// descriptors' hits fit (dpow_scan_device_cut) and queues them for those.  A descriptor begins at a
// multiple of 256 local indices from its task's begin, so a cut is a k boundary in every partition.
// The cancel flag is checked between launches.
//
// Descriptors.  The kernels behind the mask launch read the launch's descriptors again while the
// host may already write the next launch's, so the pinned table has two halves used in turn; a long
// table is copied to device memory first (queue.h kQueueCopyBlocks), stream-ordered behind the
// readers of the copy before it.  The rows table needs no second half: it is written after the mask
// launch's record, which is behind the launch that read it last.
//
// Verification.  The depth launch counts the entries that are no candidates of their descriptor,
// those not above their predecessor within the task and those shallower than their task's ntz; the
// last rows launch gathers 16 samples with their task, which the host recomputes with its own MD5
// and that task's nonce.  A non-zero count or a failed sample is DPOW_EVERIFY.  The row pointers are
// copied out once per call, by the last rows launch -- O(tasks), never O(hits) -- and the tasks'
// first_hit and n_hits come from that copy.  The function returns after the stream has drained.
#include "scan_many_dev.h"

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
#include "queue.h"
#include "scan_dev.h"

namespace dpow {

static_assert(DPOW_SCAN_DEVICE_MIN_HITS == kBatchMaxGroup, "room for the hits of one descriptor");

bool scan_many_dev_settle(const BatchEntry *blocks, size_t n_fit, const uint64_t *i_begin, uint64_t *i_done,
                          size_t n_tasks, uint32_t &next_row, ScanManyRowEntry *table, uint32_t &n_entries) {
    n_entries = 0;
    for (size_t b = 0; b < n_fit; ++b) {
        const BatchEntry &e = blocks[b];
        if (e.task >= n_tasks || e.i_begin != i_done[e.task] || e.i_end <= e.i_begin) return false;
        if (e.i_begin == i_begin[e.task]) {  // the task begins here: its row, and the empty tasks' before it
            if (next_row > e.task) return false;
            for (; next_row <= e.task; ++next_row) table[n_entries++] = ScanManyRowEntry{next_row, (uint32_t)b};
        }
        i_done[e.task] = e.i_end;
    }
    return true;
}

namespace {

// The context's buffers.  Device: the task table in the engine's image area, the control words
// behind it (batch_engine.h) with the check word at +16, then the totals, their prefix, the
// context's own row pointers, the copy of a long descriptor table and the bitmap.  Pinned: the task
// rows of the running call, the two halves of the descriptor table, the rows table, room for the
// prefix's copy, the launch's total, the record, the check word's copy, the samples, the row
// pointers' copy.
constexpr size_t kBlocksBytes = (size_t)kScanManyMaxBlocks * sizeof(BatchEntry);
constexpr size_t kPrefixBytes = (size_t)kScanManyMaxBlocks * sizeof(uint32_t);
constexpr size_t kRowsBytes = ((size_t)(DPOW_BATCH_MAX + 1) * sizeof(uint64_t) + 63u) & ~(size_t)63u;
constexpr size_t kCheckOff = kEngineCtlOff + 16;  // d_mem
constexpr size_t kTotalsOff = kEngineDevBytes;
constexpr size_t kPrefixOff = kTotalsOff + kPrefixBytes;
constexpr size_t kRowsOff = kPrefixOff + kPrefixBytes;
constexpr size_t kDevBlocksOff = kRowsOff + kRowsBytes;
constexpr size_t kMaskOff = kDevBlocksOff + kBlocksBytes;
constexpr size_t kDevBytes = kMaskOff + kScanManyDevMaskBytes;
constexpr size_t kTaskRowsOff = 0;  // h_mem
constexpr size_t kBlocksOff = kTaskRowsOff + DPOW_BATCH_MAX * sizeof(BatchTask);  // two halves
constexpr size_t kTableOff = kBlocksOff + 2 * kBlocksBytes;
constexpr size_t kOutPrefixOff = kTableOff + DPOW_BATCH_MAX * sizeof(ScanManyRowEntry);
constexpr size_t kOutTotalOff = kOutPrefixOff + kPrefixBytes;
constexpr size_t kRecOff = kOutTotalOff + 64;
constexpr size_t kOutCheckOff = kRecOff + 64;
constexpr size_t kSamplesOff = kOutCheckOff + 64;
constexpr size_t kOutRowsOff = kSamplesOff + kScanManyDevSamples * sizeof(ScanManySample);
constexpr size_t kHostBytes = kOutRowsOff + kRowsBytes;
static_assert(DPOW_BATCH_MAX * sizeof(BatchTask) <= kEngineImageBytes, "the task table fits the image area");
static_assert(kTotalsOff % 8 == 0 && kPrefixOff % 8 == 0 && kRowsOff % 8 == 0 && kDevBlocksOff % 32 == 0 &&
                  kMaskOff % 8 == 0,
              "aligned device sections");
static_assert(kBlocksOff % 32 == 0 && kBlocksBytes % 32 == 0 && kTableOff % 8 == 0 && kOutPrefixOff % 8 == 0 &&
                  kOutTotalOff % 8 == 0 && kRecOff % 8 == 0 && kSamplesOff % 8 == 0 && kOutRowsOff % 8 == 0,
              "aligned pinned sections");
constexpr EngineSections kAt{kTotalsOff, kOutPrefixOff, kRecOff};

const char *const kWho = "dpow_scan_batch_device";
const char *const kCapEnv = "DPOW_DIAG_SCAN_MANY_DEV_CAP";  // (many_plan.h many_cap)

}  // namespace

struct ScanManyDevState {
    EngineBuffers buf;
    hipEvent_t ev[2] = {nullptr, nullptr};  // around the launches queued behind a mask launch
};

namespace {

int scan_many_dev_state(ScanManyDevState **state, hipStream_t stream) {
    if (*state) return 0;
    ScanManyDevState *s = new (std::nothrow) ScanManyDevState();
    if (!s) return set_error(DPOW_ENOMEM, "dpow_scan_batch_device: out of memory");
    int rc = engine_alloc(s->buf, kDevBytes, kHostBytes, stream, scan_many_dev_prepare,
                          "dpow_scan_batch_device: allocation");
    if (rc < 0) {
        delete s;
        return rc;
    }
    hipError_t e = hipSuccess;
    for (hipEvent_t &ev : s->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) {
        rc = hip_fail(e, "dpow_scan_batch_device: allocation");
        scan_many_dev_free(s);
        return rc;
    }
    *state = s;
    return 0;
}

}  // namespace

void scan_many_dev_free(ScanManyDevState *s) {
    if (!s) return;
    engine_free(s->buf);
    for (hipEvent_t ev : s->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete s;
}

int scan_many_dev_check(const dpow_scan_task *tasks, size_t n_tasks, const void *d_idx_out, const void *d_row_out,
                        size_t max_hits, const size_t *n_out) {
    if (!tasks || !d_idx_out || !n_out) return set_error(DPOW_EINVAL, "dpow_scan_batch_device: NULL argument");
    if ((reinterpret_cast<uintptr_t>(d_idx_out) & 7u) != 0u)
        return set_error(DPOW_EINVAL, "dpow_scan_batch_device: indices not 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_row_out) & 7u) != 0u)
        return set_error(DPOW_EINVAL, "dpow_scan_batch_device: rows not 8-byte aligned");
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX)
        return set_error(DPOW_EINVAL, "dpow_scan_batch_device: n_tasks must be in [1, DPOW_BATCH_MAX]");
    if (max_hits < DPOW_SCAN_DEVICE_MIN_HITS)
        return set_error(DPOW_EINVAL, "dpow_scan_batch_device: max_hits below 16384 (one workgroup's candidates)");
    return many_check_tasks(tasks, n_tasks, kWho);
}

int scan_many_dev_run(ScanManyDevState **state, hipStream_t stream, const volatile uint32_t *cancel,
                      dpow_scan_task *tasks, size_t n_tasks, void *d_idx_out, void *d_tz_out, void *d_row_out,
                      size_t max_hits, size_t *n_out, dpow_batch_stats *stats) {
    const size_t n = n_tasks;
    dpow_batch_stats st{};
    // A task's progress: the hits of its local indices [i_begin, i_done) are in the list.
    ManyTasks v = many_tasks(tasks, n);
    // `rows`: the n + 1 row pointers (null: all zero).  `unfinished`: the status of every task that
    // is not done, DPOW_MORE or DPOW_CANCELLED.
    const auto write_out = [&](const uint64_t *rows, int unfinished, bool cancelled_on_entry) {
        for (size_t i = 0; i < n; ++i) {
            dpow_scan_task &t = tasks[i];
            t.status = v.finished(i, cancelled_on_entry) ? DPOW_EXHAUSTED : unfinished;
            t.k_done = v.k_done(i);
            t.first_hit = rows ? rows[i] : 0;
            t.n_hits = rows ? rows[i + 1] - rows[i] : 0;
        }
        *n_out = rows ? (size_t)rows[n] : 0;
        if (stats) *stats = st;
        return 0;
    };
    // A call without a launch: no hit, every row zero (a copy engine's work, no kernel's).
    const auto no_launch = [&](int unfinished, bool cancelled_on_entry) {
        if (d_row_out) {
            hipError_t e = hipMemsetAsync(d_row_out, 0, (n + 1) * sizeof(uint64_t), stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return hip_fail(e, "dpow_scan_batch_device: zeroing the rows");
        }
        return write_out(nullptr, unfinished, cancelled_on_entry);
    };
    if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) return no_launch(DPOW_CANCELLED, true);
    if (!v.any) return no_launch(DPOW_EXHAUSTED, false);  // only empty tasks: no launch, nothing allocated

    int rc = scan_many_dev_state(state, stream);
    if (rc < 0) return rc;
    ScanManyDevState &sd = **state;
    EngineBuffers &s = sd.buf;

    // The task table: row i is task i's, with its own ntz and prefilter mask.
    if ((rc = many_upload_tasks(tasks, v, s, kTaskRowsOff, stream, kWho)) < 0) return rc;
    const BatchTask *const h_rows = reinterpret_cast<const BatchTask *>(s.h_mem + kTaskRowsOff);
    const BatchTask *const d_tasks = reinterpret_cast<const BatchTask *>(s.d_mem);
    unsigned long long *const out = static_cast<unsigned long long *>(d_idx_out);
    uint8_t *const tz_out = static_cast<uint8_t *>(d_tz_out);
    unsigned long long *const rows_dev =
        d_row_out ? static_cast<unsigned long long *>(d_row_out) : reinterpret_cast<unsigned long long *>(s.d_mem + kRowsOff);
    uint32_t *const d_check = reinterpret_cast<uint32_t *>(s.d_mem + kCheckOff);
    BatchEntry *const d_blocks = reinterpret_cast<BatchEntry *>(s.d_mem + kDevBlocksOff);
    ScanManyRowEntry *const h_table = reinterpret_cast<ScanManyRowEntry *>(s.h_mem + kTableOff);
    const unsigned long long *const h_total = reinterpret_cast<const unsigned long long *>(s.h_mem + kOutTotalOff);
    uint32_t *const h_prefix = reinterpret_cast<uint32_t *>(s.h_mem + kOutPrefixOff);
    ScanManyMaskLaunch S{};
    S.mask = reinterpret_cast<unsigned long long *>(s.d_mem + kMaskOff);
    S.totals = reinterpret_cast<uint32_t *>(s.d_mem + kTotalsOff);
    S.prefix = reinterpret_cast<uint32_t *>(s.d_mem + kPrefixOff);
    S.out_total = reinterpret_cast<unsigned long long *>(s.d_h_mem + kOutTotalOff);

    // On an error nothing of ours stays queued behind the return.
    const auto fail = [&](int code) {
        (void)hipStreamSynchronize(stream);
        return code;
    };
    // The time of the launches between the events (they have completed: a later mask launch's record
    // was seen, or the stream has drained).
    bool timed = false;
    const auto collect = [&]() {
        float ms = 0.f;
        if (!timed) return;
        timed = false;
        if (hipEventElapsedTime(&ms, sd.ev[0], sd.ev[1]) == hipSuccess) st.kernel_ms += ms;
        else (void)hipGetLastError();
    };

    const ManyBudget budget{many_cap(kCapEnv), 0};
    ManyCursor cur;
    std::vector<ManyPart> parts;
    uint32_t group = 0, next_row = 0;
    size_t placed_total = 0;
    int unfinished = DPOW_EXHAUSTED;  // (nothing is unfinished when the plan runs out)
    for (uint32_t half = 0;; half ^= 1u) {
        if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) {
            unfinished = DPOW_CANCELLED;
            break;
        }
        if (!many_next(v.i_begin.data(), v.i_end.data(), nullptr, n, budget, cur, parts, group)) break;
        BatchEntry *const h_blocks = reinterpret_cast<BatchEntry *>(s.h_mem + kBlocksOff + half * kBlocksBytes);
        const BatchEntry *const p_blocks =
            reinterpret_cast<const BatchEntry *>(s.d_h_mem + kBlocksOff + half * kBlocksBytes);  // pinned
        uint64_t candidates = 0;
        for (const ManyPart &p : parts) candidates += p.hi - p.lo;
        const size_t n_blocks = many_write_blocks(parts, group, h_blocks, kScanManyMaxBlocks);
        if (n_blocks == 0 || group > kBatchMaxGroup)
            return fail(set_error(DPOW_EINVAL, "dpow_scan_batch_device: the launch plan left the descriptor table"));  // never expected
        // A short descriptor table is read where it is, in pinned memory, one scalar load per
        // workgroup; a long one is first copied to device memory by the upload kernel.
        const bool copy = n_blocks >= kQueueCopyBlocks;
        const BatchEntry *const k_blocks = copy ? d_blocks : p_blocks;
        const auto issue = [&](const BatchLaunch &L) {
            S.L = L;
            hipError_t e = hipSuccess;
            if (copy)
                e = batch_upload(reinterpret_cast<uint32_t *>(d_blocks), reinterpret_cast<const uint32_t *>(p_blocks),
                                 (uint32_t)(n_blocks * sizeof(BatchEntry) / 4), stream);
            if (e == hipSuccess) e = scan_many_mask_launch(d_tasks, k_blocks, S, stream);
            return e == hipSuccess ? 0 : hip_fail(e, "dpow_scan_batch_device: mask launch");
        };
        rc = engine_launch(s, kAt, (uint32_t)parts.size(), group, (uint32_t)n_blocks, stream,
                           "dpow_scan_batch_device: stream idle without the launch's completion record", st, issue);
        if (rc < 0) return fail(rc);
        collect();
        st.candidates += candidates;
        const uint64_t total = *h_total;
        if (total > candidates)
            return fail(set_error(DPOW_EVERIFY, "dpow_scan_batch_device: more hits counted than candidates hashed"));
        const size_t room = max_hits - placed_total;
        size_t n_fit = n_blocks, placed = (size_t)total;
        if (total > room) {  // the cut needs the prefix: once per call at most, as the call ends here
            hipError_t ce = hipMemcpyAsync(h_prefix, S.prefix, n_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
            if (ce == hipSuccess) ce = hipStreamSynchronize(stream);
            if (ce != hipSuccess) return fail(hip_fail(ce, "dpow_scan_batch_device: copying the prefix"));
            if (h_prefix[n_blocks - 1] != total)
                return fail(set_error(DPOW_EVERIFY, "dpow_scan_batch_device: the prefix does not end at the total"));
            n_fit = dpow_scan_device_cut(h_prefix, n_blocks, room);
            placed = n_fit ? h_prefix[n_fit - 1] : 0;
        }
        if (placed > room)
            return fail(set_error(DPOW_EVERIFY, "dpow_scan_batch_device: a prefix that does not ascend"));
        uint32_t n_entries = 0;
        if (!scan_many_dev_settle(h_blocks, n_fit, v.i_begin.data(), v.i_done.data(), n, next_row, h_table, n_entries))
            return fail(set_error(DPOW_EINVAL, "dpow_scan_batch_device: a descriptor out of its task's order"));  // never expected
        // (A launch without a hit whose tasks began earlier queues nothing behind its mask launch.)
        const bool queued = n_entries != 0u || placed != 0u;
        hipError_t e = queued ? hipEventRecord(sd.ev[0], stream) : hipSuccess;
        if (e == hipSuccess && n_entries) {
            ScanManyRowsLaunch R{};
            R.table = reinterpret_cast<const ScanManyRowEntry *>(s.d_h_mem + kTableOff);
            R.prefix = S.prefix;
            R.rows = rows_dev;
            R.base = placed_total;
            R.n_entries = n_entries;
            e = scan_many_rows_launch(R, stream);
            st.launches++;
        }
        if (e == hipSuccess && placed) {
            ScanManyPlaceLaunch P{};
            P.mask = S.mask;
            P.prefix = S.prefix;
            P.out = out;
            P.base = placed_total;
            P.max_hits = max_hits;
            e = scan_many_place_launch(d_tasks, k_blocks, P, (uint32_t)n_fit, stream);
            st.launches++;
            if (e == hipSuccess) {
                ScanManyDepthLaunch D{};
                D.prefix = S.prefix;
                D.idx = out;
                D.tz = tz_out;
                D.rows = rows_dev;
                D.bad = d_check;
                D.base = placed_total;
                D.max_hits = max_hits;
                e = scan_many_depth_launch(d_tasks, k_blocks, D, (uint32_t)n_fit, stream);
                st.launches++;
            }
        }
        if (e == hipSuccess && queued) e = hipEventRecord(sd.ev[1], stream);
        if (e != hipSuccess) return fail(hip_fail(e, "dpow_scan_batch_device: rows, place and depth launches"));
        timed = queued;
        placed_total += placed;
        if (n_fit < n_blocks) {  // the rest of the launch did not fit: the caller submits what is unfinished again
            unfinished = DPOW_MORE;
            break;
        }
    }

    // The rows of the tasks not begun and the end row, the samples, and the wait for everything queued.
    const uint64_t *const h_rows_out = reinterpret_cast<const uint64_t *>(s.h_mem + kOutRowsOff);
    const uint32_t *const h_check = reinterpret_cast<const uint32_t *>(s.h_mem + kOutCheckOff);
    {
        ScanManyRowsLaunch R{};
        R.rows = rows_dev;
        R.fill_begin = next_row;
        R.fill_end = (uint32_t)n + 1u;
        R.fill_value = placed_total;
        R.idx = out;
        R.tz = tz_out;
        R.n = placed_total;
        R.samples = reinterpret_cast<ScanManySample *>(s.d_h_mem + kSamplesOff);
        // (The same launch copies the rows and the check word to pinned memory and zeroes the word
        // for the next call: copy-engine commands for them cost the call more than the launch.)
        R.out_rows = reinterpret_cast<unsigned long long *>(s.d_h_mem + kOutRowsOff);
        R.bad = d_check;
        R.out_bad = reinterpret_cast<uint32_t *>(s.d_h_mem + kOutCheckOff);
        hipError_t e = scan_many_rows_launch(R, stream);
        st.launches++;
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return fail(hip_fail(e, "dpow_scan_batch_device: waiting for the launches"));
    }
    collect();
    // The rows: they begin at 0, do not descend and end at the total.
    for (size_t i = 0; i <= n; ++i)
        if ((i == 0 ? h_rows_out[0] != 0u : h_rows_out[i] < h_rows_out[i - 1]) || h_rows_out[n] != placed_total)
            return set_error(DPOW_EVERIFY, "dpow_scan_batch_device: row pointers that do not ascend to the total");
    if (placed_total) {
        if (h_check[0] != 0u)
            return set_error(DPOW_EVERIFY,
                             "dpow_scan_batch_device: entries outside their descriptor, out of order or shallower than asked for");
        const ScanManySample *const smp = reinterpret_cast<const ScanManySample *>(s.h_mem + kSamplesOff);
        std::vector<uint8_t> msg;
        for (uint32_t q = 0; q < kScanManyDevSamples; ++q) {
            const uint64_t at = (uint64_t)(((unsigned __int128)(placed_total - 1u) * q) / (kScanManyDevSamples - 1u));
            const uint32_t task = smp[q].task;
            bool ok = task < n && h_rows_out[task] <= at && at < h_rows_out[task + 1];
            if (ok) {
                const dpow_scan_task &t = tasks[task];
                const uint64_t g = smp[q].idx;
                uint64_t i;
                ok = local_of_global(g, v.rbits[task], h_rows[task].base_tb, i) && i >= v.i_begin[task] &&
                     i < v.i_done[task];
                if (ok) {
                    const uint32_t tz = md5_depth_of_index(md5_msg_of_nonce(msg, t.nonce, t.nonce_len), t.nonce_len, g);
                    ok = tz >= t.ntz && (!tz_out || smp[q].tz == tz);
                }
            }
            if (!ok)
                return set_error(DPOW_EVERIFY, "dpow_scan_batch_device: a sampled entry failed host MD5 verification");
        }
    }
    return write_out(h_rows_out, unfinished, false);
}

}  // namespace dpow

using namespace dpow;

extern "C" int dpow_scan_batch_device_settle(const dpow_batch_range *blocks, size_t n_fit, const uint64_t *i_begin,
                                             const uint64_t *i_end, size_t n_tasks, uint64_t *i_done,
                                             uint32_t *next_row, uint32_t *row_block, int32_t unfinished,
                                             int32_t *status) {
    if ((!blocks && n_fit) || !i_begin || !i_end || !i_done || !next_row || !row_block || !status)
        return set_error(DPOW_EINVAL, "dpow_scan_batch_device_settle: NULL argument");
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX)
        return set_error(DPOW_EINVAL, "dpow_scan_batch_device_settle: n_tasks must be in [1, DPOW_BATCH_MAX]");
    if (n_fit > kScanManyMaxBlocks)
        return set_error(DPOW_EINVAL, "dpow_scan_batch_device_settle: more descriptors than a launch holds");
    if (*next_row > n_tasks) return set_error(DPOW_EINVAL, "dpow_scan_batch_device_settle: next_row beyond the tasks");
    for (size_t i = 0; i < n_tasks; ++i)
        if (i_begin[i] > i_done[i] || i_done[i] > i_end[i])
            return set_error(DPOW_EINVAL, "dpow_scan_batch_device_settle: progress outside its task");
    std::vector<BatchEntry> entries(n_fit);
    for (size_t b = 0; b < n_fit; ++b) {
        entries[b].i_begin = blocks[b].i_begin;
        entries[b].i_end = blocks[b].i_end;
        entries[b].task = blocks[b].task;
        if (blocks[b].task < n_tasks && blocks[b].i_end > i_end[blocks[b].task])
            return set_error(DPOW_EINVAL, "dpow_scan_batch_device_settle: a descriptor beyond its task");
    }
    std::vector<ScanManyRowEntry> table(n_tasks);
    std::vector<uint64_t> done(i_done, i_done + n_tasks);
    uint32_t next = *next_row, n_entries = 0;
    if (!scan_many_dev_settle(entries.data(), n_fit, i_begin, done.data(), n_tasks, next, table.data(), n_entries))
        return set_error(DPOW_EINVAL, "dpow_scan_batch_device_settle: a descriptor out of its task's order");
    for (size_t i = 0; i < n_tasks; ++i) {
        i_done[i] = done[i];
        row_block[i] = 0xFFFFFFFFu;
        status[i] = done[i] == i_end[i] ? DPOW_EXHAUSTED : unfinished;
    }
    for (uint32_t q = 0; q < n_entries; ++q) row_block[table[q].row] = table[q].first_block;
    *next_row = next;
    return (int)n_entries;
}
