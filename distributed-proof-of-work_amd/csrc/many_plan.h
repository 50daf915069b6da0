// many_plan.h -- what the three batched host loops (census_many.cpp, scan_many.cpp, scan_many_dev.cpp)
// share: the launch planner, the cut of a launch into workgroup descriptors, the diagnostic budget
// knob, and a call's tasks as local index ranges with their argument check and table upload.  What
// each loop does with a launch's output is its own.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/dpow.h"
#include "batch_engine.h"
#include "plan.h"

namespace dpow {

// (Hidden, as batch_engine.h: nothing here is among the library's dynamic symbols.)
#pragma GCC visibility push(hidden)

// A task's part of one launch: the local indices [lo, hi) of task `task` (k * R + t, absolute).
struct ManyPart {
    uint32_t task;
    uint64_t lo, hi;
};

// Where the planner stands: tasks before `task` are planned, and `done` local indices of `task`.
struct ManyCursor {
    size_t task = 0;
    uint64_t done = 0;
};

// A launch's two budgets: local indices (a multiple of 256, at least 256, at most kBatchCap) and
// hit weight (a multiple of 256, at least 256; unused by a planner without depths).
struct ManyBudget {
    uint64_t cap, weight;
};

// The hit weight of n local indices at depth ntz: ceil(n / 16^min(ntz, 7)), their expected hits
// rounded up (all of them at ntz = 0; from ntz = 7 on 2^28 indices weigh 1).
uint64_t many_weight(uint64_t n, uint32_t ntz);

// The next launch for tasks with local index ranges [i_begin[i], i_end[i]) and depths ntz[i].  It
// takes tasks in array order from the cursor while their local indices total at most b.cap and,
// unless ntz is null, their weights at most b.weight.  Only its last task can be cut, and only at a
// multiple of 256 local indices from the task's begin -- a whole k for every partition width and a
// whole workgroup step.  An empty task has no part.  A launch is never empty: both budgets admit
// 256 indices of any depth.  `group` is batch_group of the launch's total.  False, with no part,
// when nothing is left.
bool many_next(const uint64_t *i_begin, const uint64_t *i_end, const uint32_t *ntz, size_t n, const ManyBudget &b,
               ManyCursor &cur, std::vector<ManyPart> &parts, uint32_t &group);

// The descriptors of one launch, in task order: each part in pieces of `group` local indices, the
// last one of a part possibly shorter.  many_write_blocks writes the launch's table (the first
// max_blocks rows at most) and returns the descriptor count, or 0 when it is outside
// [1, max_blocks]; many_append_ranges writes them as rows of launch `launch` behind the n_out rows
// `out` already holds (null, or short of max_entries rows: those that fit) and returns the count.
size_t many_write_blocks(const std::vector<ManyPart> &parts, uint32_t group, BatchEntry *blocks, size_t max_blocks);
size_t many_append_ranges(const std::vector<ManyPart> &parts, uint32_t group, uint64_t launch, dpow_batch_range *out,
                          size_t max_entries, uint64_t n_out);

// The candidate budget of a call's launches: kBatchCap, or the variable `env`=<256..2^28> rounded
// down to a multiple of 256 (read per call: how the tests put launch seams into small windows).
uint64_t many_cap(const char *env);

// A call's tasks as the planner sees them: task i's local indices [i_begin[i], i_end[i]), of which
// [i_begin[i], i_done[i]) are done with; its remainder bits and its depth (0 where the task type
// has none).
struct ManyTasks {
    std::vector<uint64_t> i_begin, i_end, i_done;
    std::vector<uint32_t> rbits, ntz;
    bool any = false;  // some task is not empty
    explicit ManyTasks(size_t n) : i_begin(n), i_end(n), i_done(n), rbits(n), ntz(n) {}
    // (An empty task is finished.)
    bool finished(size_t i, bool cancelled_on_entry) const { return i_done[i] == i_end[i] && !cancelled_on_entry; }
    uint64_t k_done(size_t i) const { return i_done[i] >> rbits[i]; }  // (a finished task's k_end)
};

inline uint32_t many_ntz(const dpow_scan_task &t) { return t.ntz; }
inline uint32_t many_ntz(const dpow_census_task &) { return 0u; }

template <typename Task>
ManyTasks many_tasks(const Task *tasks, size_t n) {
    ManyTasks v(n);
    for (size_t i = 0; i < n; ++i) {
        v.rbits[i] = remainder_bits(tasks[i].worker_bits);
        v.ntz[i] = many_ntz(tasks[i]);
        v.i_begin[i] = v.i_done[i] = tasks[i].k_begin << v.rbits[i];
        v.i_end[i] = tasks[i].k_end << v.rbits[i];
        v.any = v.any || v.i_begin[i] < v.i_end[i];
    }
    return v;
}

// The tasks' own argument errors (batch_check_task, named after the entry point `who`): 0 or the
// first one's negative code.
template <typename Task>
int many_check_tasks(const Task *tasks, size_t n, const char *who) {
    for (size_t i = 0; i < n; ++i) {
        dpow_batch_task t{};
        t.nonce = tasks[i].nonce;
        t.nonce_len = tasks[i].nonce_len;
        t.worker_byte = tasks[i].worker_byte;
        t.k_begin = tasks[i].k_begin;
        t.k_end = tasks[i].k_end;
        const int rc = batch_check_task(t, who);
        if (rc < 0) return rc;
    }
    return 0;
}

// The task table: row i is task i's, with its depth and prefilter mask, filled in the pinned rows at
// b.h_mem + rows_off (an empty task's row is never read and stays as it is) and uploaded to the
// front of b.d_mem.  0, or the negative code with "`who`: upload: <the HIP error>" set.
template <typename Task>
int many_upload_tasks(const Task *tasks, const ManyTasks &v, EngineBuffers &b, size_t rows_off, hipStream_t stream,
                      const char *who) {
    const size_t n = v.i_begin.size();
    BatchTask *const h_rows = reinterpret_cast<BatchTask *>(b.h_mem + rows_off);
    for (size_t i = 0; i < n; ++i)
        if (v.i_begin[i] < v.i_end[i])
            batch_fill_task(h_rows[i], tasks[i].nonce, tasks[i].nonce_len, v.ntz[i], tasks[i].worker_byte,
                            tasks[i].worker_bits);
    const hipError_t e = batch_upload(reinterpret_cast<uint32_t *>(b.d_mem),
                                      reinterpret_cast<const uint32_t *>(b.d_h_mem + rows_off),
                                      (uint32_t)(n * sizeof(BatchTask) / 4), stream);
    return e == hipSuccess ? 0 : hip_fail(e, (std::string(who) + ": upload").c_str());
}

#pragma GCC visibility pop

}  // namespace dpow
