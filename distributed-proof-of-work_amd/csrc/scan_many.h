// scan_many.h -- host side of the batched scan (scan_many.cpp), as dpow_api.cpp sees it.  Its
// launches are many_plan.h's, under both budgets.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"

namespace dpow {

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
