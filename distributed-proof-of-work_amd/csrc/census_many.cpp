// census_many.cpp -- host side of the batched census: dpow_census_batch's launch loop over the
// batched census kernel (md5_census_many.hip) on the launch engine (batch_engine.h) and the host
// helper dpow_census_plan.
//
// Launches.  The tasks are worked in array order, by the planner the batched loops share
// (many_plan.h many_next, without a weight budget).  A launch takes tasks from a cursor until it
// holds kBatchCap local indices; only its last task can be cut, at a multiple of 256 local indices
// from the task's begin, and goes on in the next launch.  A task's part of a launch is cut into
// workgroup descriptors of batch_group(the launch's total) local indices, the last one of a task
// possibly shorter: one descriptor per workgroup, because the tasks of one call differ in size by
// orders of magnitude.  One bounded launch is in flight at a time and the
// cancel flag is checked between launches, so a return leaves nothing queued.
//
// After each launch the host folds the table of every task the launch held into that task's census
// with census.cpp's own step (census_fold_launch): the table's checks, the host MD5 of every
// distinct first index, dpow_census_merge's code.  A task cut by a launch boundary is folded once
// per launch it took part in, as dpow_census_window folds its launches.  Nothing is written to the
// caller's tasks before the call's last launch has been folded.
#include "census_many.h"

#include <string.h>

#include <new>
#include <vector>

#include "../../include/dpow_worker.h"
#include "batch.h"
#include "batch_engine.h"
#include "census.h"
#include "ctx.h"
#include "many_plan.h"
#include "md5_census_many.h"
#include "md5_host.h"
#include "plan.h"
#include "queue.h"

namespace dpow {

namespace {

// The context's buffers.  Device: the task table in the engine's image area, the control words
// behind it (batch_engine.h), then the tasks' tables and the copy of the live-slot list and the
// descriptor table of a launch of kQueueCopyBlocks descriptors or more.  Pinned: the task rows of
// the running call, a launch's live-slot list and, right behind it, its descriptors (one upload
// takes both), the tables' copies, the record.
constexpr size_t kManyTableBytes = (size_t)kCensusTableWords * sizeof(unsigned long long);
constexpr size_t kManySlotsBytes = DPOW_BATCH_MAX * sizeof(uint32_t);
constexpr size_t kManyDevTablesOff = kEngineDevBytes;
constexpr size_t kManyDevSlotsOff = kManyDevTablesOff + DPOW_BATCH_MAX * kManyTableBytes;
constexpr size_t kManyDevBlocksOff = kManyDevSlotsOff + kManySlotsBytes;
constexpr size_t kManyDevBytes = kManyDevBlocksOff + (size_t)kCensusManyMaxBlocks * sizeof(BatchEntry);
constexpr size_t kManyRowsOff = 0;  // h_mem
constexpr size_t kManySlotsOff = kManyRowsOff + DPOW_BATCH_MAX * sizeof(BatchTask);
constexpr size_t kManyBlocksOff = kManySlotsOff + kManySlotsBytes;
constexpr size_t kManyOutOff = kManyBlocksOff + (size_t)kCensusManyMaxBlocks * sizeof(BatchEntry);
constexpr size_t kManyRecOff = kManyOutOff + DPOW_BATCH_MAX * kManyTableBytes;
constexpr size_t kManyHostBytes = kManyRecOff + 64;
static_assert(DPOW_BATCH_MAX * sizeof(BatchTask) <= kEngineImageBytes, "the task table fits the image area");
static_assert(kManyDevTablesOff % 8 == 0 && kManyDevSlotsOff % 4 == 0 && kManyDevBlocksOff % 32 == 0,
              "aligned device sections");
static_assert(kManyBlocksOff % 32 == 0 && kManyOutOff % 8 == 0 && kManyRecOff % 8 == 0, "aligned pinned sections");
constexpr EngineSections kManyAt{kManyDevTablesOff, kManyOutOff, kManyRecOff};

const char *const kWho = "dpow_census_batch";
const char *const kCapEnv = "DPOW_DIAG_CENSUS_MANY_CAP";  // (many_plan.h many_cap)

}  // namespace

struct CensusManyState {
    EngineBuffers buf;
};

namespace {

int census_many_state(CensusManyState **state, hipStream_t stream) {
    if (*state) return 0;
    CensusManyState *s = new (std::nothrow) CensusManyState();
    if (!s) return set_error(DPOW_ENOMEM, "dpow_census_batch: out of memory");
    int rc = engine_alloc(s->buf, kManyDevBytes, kManyHostBytes, stream, census_many_prepare,
                          "dpow_census_batch: allocation");
    if (rc == 0) {
        // The tables as a launch expects them (its last workgroup leaves them so): counts 0, firsts
        // none.  Staged in the pinned copies and sent on the context's own stream.
        unsigned long long *const h = reinterpret_cast<unsigned long long *>(s->buf.h_mem + kManyOutOff);
        for (size_t w = 0; w < (size_t)DPOW_BATCH_MAX * kCensusTableWords; ++w)
            h[w] = w % kCensusTableWords < kCensusDepths ? 0ull : kNoHit;
        hipError_t e;
        if ((e = hipMemcpyAsync(s->buf.d_mem + kManyDevTablesOff, h, DPOW_BATCH_MAX * kManyTableBytes,
                                hipMemcpyHostToDevice, stream)) != hipSuccess ||
            (e = hipStreamSynchronize(stream)) != hipSuccess) {
            engine_free(s->buf);
            rc = hip_fail(e, "dpow_census_batch: allocation");
        } else {
            memset(h, 0, DPOW_BATCH_MAX * kManyTableBytes);
        }
    }
    if (rc < 0) delete s;
    else *state = s;
    return rc;
}

}  // namespace

void census_many_free(CensusManyState *s) {
    if (!s) return;
    engine_free(s->buf);
    delete s;
}

int census_many_check(const dpow_census_task *tasks, size_t n_tasks) {
    if (!tasks) return set_error(DPOW_EINVAL, "dpow_census_batch: tasks is NULL");
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX)
        return set_error(DPOW_EINVAL, "dpow_census_batch: n_tasks must be in [1, DPOW_BATCH_MAX]");
    return many_check_tasks(tasks, n_tasks, kWho);
}

int census_many_run(CensusManyState **state, hipStream_t stream, const volatile uint32_t *cancel,
                    dpow_census_task *tasks, size_t n_tasks, dpow_batch_stats *stats) {
    const size_t n = n_tasks;
    dpow_batch_stats st{};
    // A task's progress: the local indices [i_begin, i_done) are folded into its census.
    ManyTasks v = many_tasks(tasks, n);
    std::vector<dpow_census> census;  // (filled only when a launch is made)
    const auto write_out = [&](bool cancelled_on_entry) {
        for (size_t i = 0; i < n; ++i) {
            dpow_census_task &t = tasks[i];
            if (census.empty()) census_clear(t.census);
            else t.census = census[i];
            t.status = v.finished(i, cancelled_on_entry) ? DPOW_EXHAUSTED : DPOW_CANCELLED;
            t.k_done = v.k_done(i);
        }
        if (stats) *stats = st;
        return 0;
    };
    if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) return write_out(true);  // raised on entry: no launch
    if (!v.any) return write_out(false);                                           // only empty tasks: no launch

    int rc = census_many_state(state, stream);
    if (rc < 0) return rc;
    EngineBuffers &s = (*state)->buf;
    census.resize(n);
    for (dpow_census &c : census) census_clear(c);

    // The task table: row i is task i's (ntz 0, as census.cpp fills its own).
    if ((rc = many_upload_tasks(tasks, v, s, kManyRowsOff, stream, kWho)) < 0) return rc;
    const BatchTask *const h_rows = reinterpret_cast<const BatchTask *>(s.h_mem + kManyRowsOff);
    const BatchTask *const d_tasks = reinterpret_cast<const BatchTask *>(s.d_mem);
    BatchEntry *const h_blocks = reinterpret_cast<BatchEntry *>(s.h_mem + kManyBlocksOff);
    uint32_t *const h_slots = reinterpret_cast<uint32_t *>(s.h_mem + kManySlotsOff);
    const unsigned long long *const h_out = reinterpret_cast<const unsigned long long *>(s.h_mem + kManyOutOff);
    // A short descriptor table is read where it is, in pinned memory, one scalar load per workgroup;
    // a long one is first copied to device memory by the upload kernel (queue.h kQueueCopyBlocks),
    // and the live-slot list in front of it with it: the last workgroup reads a slot per table word.
    uint32_t *const d_slots = reinterpret_cast<uint32_t *>(s.d_mem + kManyDevSlotsOff);
    const uint32_t *const p_slots = reinterpret_cast<const uint32_t *>(s.d_h_mem + kManySlotsOff);  // pinned
    const BatchEntry *const d_blocks = reinterpret_cast<const BatchEntry *>(s.d_mem + kManyDevBlocksOff);
    const BatchEntry *const p_blocks = reinterpret_cast<const BatchEntry *>(s.d_h_mem + kManyBlocksOff);
    const auto issue = [&](const BatchLaunch &L) {
        hipError_t e = hipSuccess;
        const bool copy = L.n_blocks >= kQueueCopyBlocks;
        if (copy)
            e = batch_upload(d_slots, p_slots,
                             (uint32_t)((kManySlotsBytes + (size_t)L.n_blocks * sizeof(BatchEntry)) / 4), stream);
        if (e == hipSuccess)
            e = census_many_launch(d_tasks, copy ? d_blocks : p_blocks, copy ? d_slots : p_slots, L, stream);
        return e == hipSuccess ? 0 : hip_fail(e, "dpow_census_batch: launch");
    };

    const ManyBudget budget{many_cap(kCapEnv), 0};
    ManyCursor cur;
    std::vector<ManyPart> parts;
    std::vector<uint8_t> msg;
    uint32_t group = 0;
    for (;;) {
        if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) break;  // what is not finished stays DPOW_CANCELLED
        if (!many_next(v.i_begin.data(), v.i_end.data(), nullptr, n, budget, cur, parts, group)) break;
        uint64_t total = 0;
        for (size_t q = 0; q < parts.size(); ++q) {
            h_slots[q] = parts[q].task;
            total += parts[q].hi - parts[q].lo;
        }
        const size_t n_blocks = many_write_blocks(parts, group, h_blocks, kCensusManyMaxBlocks);
        if (n_blocks == 0)
            return set_error(DPOW_EINVAL, "dpow_census_batch: the launch plan left the descriptor table");  // never expected
        rc = engine_launch(s, kManyAt, (uint32_t)parts.size(), group, (uint32_t)n_blocks, stream,
                           "dpow_census_batch: stream idle without the launch's completion record", st, issue);
        if (rc < 0) return rc;
        st.candidates += total;
        for (size_t q = 0; q < parts.size(); ++q) {
            const ManyPart &p = parts[q];
            const dpow_census_task &t = tasks[p.task];
            const BatchTask &row = h_rows[p.task];
            const unsigned long long *const table = h_out + q * kCensusTableWords;
            rc = census_fold_launch(kWho, md5_msg_of_nonce(msg, t.nonce, t.nonce_len), t.nonce_len, row.rbits,
                                    row.base_tb, p.lo, p.hi, table, table + kCensusDepths, census[p.task]);
            if (rc < 0) return rc;
            v.i_done[p.task] = p.hi;
        }
    }
    return write_out(false);
}

}  // namespace dpow

using namespace dpow;

extern "C" int dpow_census_plan(const uint64_t *k_begin, const uint64_t *k_end, const uint32_t *worker_bits,
                                size_t n_tasks, uint64_t cap, dpow_batch_range *out, size_t max_entries,
                                uint64_t *launches_out) {
    if (!k_begin || !k_end || !worker_bits || !launches_out)
        return set_error(DPOW_EINVAL, "dpow_census_plan: NULL argument");
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX)
        return set_error(DPOW_EINVAL, "dpow_census_plan: n_tasks must be in [1, DPOW_BATCH_MAX]");
    if (cap == 0) cap = kBatchCap;
    if (cap < 256 || cap > kBatchCap) return set_error(DPOW_EINVAL, "dpow_census_plan: cap outside [256, 2^28]");
    cap &= ~255ull;
    std::vector<uint64_t> i_begin(n_tasks), i_end(n_tasks);
    for (size_t i = 0; i < n_tasks; ++i) {
        if (k_begin[i] > k_end[i]) return set_error(DPOW_EINVAL, "dpow_census_plan: k_begin > k_end");
        if (k_end[i] > DPOW_K_LIMIT) return set_error(DPOW_ERANGE, "dpow_census_plan: k_end beyond DPOW_K_LIMIT");
        const uint32_t rbits = remainder_bits(worker_bits[i]);
        i_begin[i] = k_begin[i] << rbits;
        i_end[i] = k_end[i] << rbits;
    }
    const ManyBudget budget{cap, 0};
    ManyCursor cur;
    std::vector<ManyPart> parts;
    uint32_t group = 0;
    uint64_t n_out = 0, launch = 0;
    for (; many_next(i_begin.data(), i_end.data(), nullptr, n_tasks, budget, cur, parts, group); ++launch) {
        const size_t n_blocks = many_append_ranges(parts, group, launch, out, max_entries, n_out);
        if (n_blocks > kCensusManyMaxBlocks)
            return set_error(DPOW_EINVAL, "dpow_census_plan: a launch beyond its descriptor bound");  // never expected
        n_out += n_blocks;
        if (n_out > (uint64_t)INT32_MAX) return set_error(DPOW_ERANGE, "dpow_census_plan: too many entries");
    }
    *launches_out = launch;
    return (int)n_out;
}
