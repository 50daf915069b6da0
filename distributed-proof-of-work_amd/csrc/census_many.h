// census_many.h -- host side of the batched census (census_many.cpp), as dpow_api.cpp sees it.  Its
// launches are many_plan.h's, without a weight budget.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"

namespace dpow {

// Device and pinned buffers of a context's batched censuses: allocated on its first, freed with it.
struct CensusManyState;
void census_many_free(CensusManyState *s);  // the context's device is current, its stream drained

// Argument errors of dpow_census_batch (decided before the device is touched): 0 or a negative code.
int census_many_check(const dpow_census_task *tasks, size_t n_tasks);

// The body of dpow_census_batch (the arguments and the context checked, its device current).
int census_many_run(CensusManyState **state, hipStream_t stream, const volatile uint32_t *cancel,
                    dpow_census_task *tasks, size_t n_tasks, dpow_batch_stats *stats);

}  // namespace dpow
