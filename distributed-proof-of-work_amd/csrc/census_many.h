// census_many.h -- host side of the batched census (census_many.cpp), as dpow_api.cpp sees it, and
// its launch planner, a pure host function.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/dpow.h"

namespace dpow {

// A task's part of one launch: the local indices [lo, hi) of task `task` (k * R + t, absolute).
struct CensusManyPart {
    uint32_t task;
    uint64_t lo, hi;
};

// Where the planner stands: tasks before `task` are planned, and `done` local indices of `task`.
struct CensusManyCursor {
    size_t task = 0;
    uint64_t done = 0;
};

// The next launch for tasks with local index ranges [i_begin[i], i_end[i]): it takes tasks in array
// order from the cursor until it holds `cap` local indices (a multiple of 256, at least 256).  Only
// its last task can be cut, and only at a multiple of 256 local indices from the task's begin -- a
// whole k for every partition width and a whole workgroup step.  An empty task has no part.
// `group` is batch_group of the launch's total.  False, with no part, when nothing is left.
bool census_many_next(const uint64_t *i_begin, const uint64_t *i_end, size_t n, uint64_t cap, CensusManyCursor &cur,
                      std::vector<CensusManyPart> &parts, uint32_t &group);

// The launch budget of this call: kBatchCap, or DPOW_DIAG_CENSUS_MANY_CAP=<256..2^28> rounded down to
// a multiple of 256 (read per call: how the tests put launch seams into small windows).
uint64_t census_many_cap();

// Device and pinned buffers of a context's batched censuses: allocated on its first, freed with it.
struct CensusManyState;
void census_many_free(CensusManyState *s);  // the context's device is current, its stream drained

// Argument errors of dpow_census_batch (decided before the device is touched): 0 or a negative code.
int census_many_check(const dpow_census_task *tasks, size_t n_tasks);

// The body of dpow_census_batch (the arguments and the context checked, its device current).
int census_many_run(CensusManyState **state, hipStream_t stream, const volatile uint32_t *cancel,
                    dpow_census_task *tasks, size_t n_tasks, dpow_batch_stats *stats);

}  // namespace dpow
