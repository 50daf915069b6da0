// scan_many.h -- host side of the batched scan (scan_many.cpp), as dpow_api.cpp sees it, and its
// launch planner, a pure host function.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/dpow.h"

namespace dpow {

// A task's part of one launch: the local indices [lo, hi) of task `task` (k * R + t, absolute).
struct ScanManyPart {
    uint32_t task;
    uint64_t lo, hi;
};

// Where the planner stands: tasks before `task` are planned, and `done` local indices of `task`.
struct ScanManyCursor {
    size_t task = 0;
    uint64_t done = 0;
};

// A launch's two budgets: local indices (a multiple of 256, at least 256, at most kBatchCap) and
// hit weight (a multiple of 256, at least 256; the call's own is kScanCap / 4).
struct ScanManyBudget {
    uint64_t cap, weight;
};

// The hit weight of n local indices at depth ntz: ceil(n / 16^min(ntz, 7)), their expected hits
// rounded up (all of them at ntz = 0; from ntz = 7 on 2^28 indices weigh 1).
uint64_t scan_many_weight(uint64_t n, uint32_t ntz);

// The next launch for tasks with local index ranges [i_begin[i], i_end[i]) and depths ntz[i]:
// census_many_next with two budgets.  It takes tasks in array order from the cursor while their
// local indices total at most b.cap and their weights at most b.weight.  Only its last task can be
// cut, and only at a multiple of 256 local indices from the task's begin -- a whole k for every
// partition width and a whole workgroup step.  An empty task has no part.  A launch is never
// empty: both budgets admit 256 indices of any depth.  `group` is batch_group of the launch's
// total.  False, with no part, when nothing is left.
bool scan_many_next(const uint64_t *i_begin, const uint64_t *i_end, const uint32_t *ntz, size_t n,
                    const ScanManyBudget &b, ScanManyCursor &cur, std::vector<ScanManyPart> &parts, uint32_t &group);

// The budgets for planning again the parts of a launch of `total` local indices and hit weight
// `weight` whose count overflowed its list: half of each, rounded up to a multiple of 256.
ScanManyBudget scan_many_halve(uint64_t total, uint64_t weight);

// Device and pinned buffers of a context's batched scans: allocated on its first, freed with it.
struct ScanManyState;
void scan_many_free(ScanManyState *s);  // the context's device is current, its stream drained

// Argument errors of dpow_scan_batch (decided before the device is touched): 0 or a negative code.
int scan_many_check(const dpow_scan_task *tasks, size_t n_tasks, const dpow_scan_hit *out, size_t max_hits,
                    const size_t *n_out);

// The body of dpow_scan_batch (the arguments and the context checked, its device current).
int scan_many_run(ScanManyState **state, hipStream_t stream, const volatile uint32_t *cancel, dpow_scan_task *tasks,
                  size_t n_tasks, dpow_scan_hit *out, size_t max_hits, size_t *n_out, dpow_batch_stats *stats);

}  // namespace dpow
