// scan_many_dev.h -- host side of the batched device scan (scan_many_dev.cpp), as dpow_api.cpp sees
// it, and what becomes of the tasks after a launch, a pure host function.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"
#include "md5_scan_many_dev.h"

namespace dpow {

// What the first n_fit descriptors of a launch having been placed means for the tasks.  Each of them
// advances its task's progress i_done (local indices, absolute) to its own end: descriptors are in
// task order and within a task in index order, so a task's progress only grows, and a task none of
// whose descriptors is among the first n_fit keeps its own.  One that begins its task (at
// i_begin[task]) settles that task's row pointer and those of the tasks between next_row and it,
// which are empty: an entry of `table` (room for n_tasks) each, all naming that descriptor; next_row
// moves behind the task.  False when a descriptor names no task of the call or does not begin where
// its task's progress stands (never expected).
bool scan_many_dev_settle(const BatchEntry *blocks, size_t n_fit, const uint64_t *i_begin, uint64_t *i_done,
                          size_t n_tasks, uint32_t &next_row, ScanManyRowEntry *table, uint32_t &n_entries);

// Device and pinned buffers of a context's batched device scans: allocated on its first call that
// makes a launch, freed with it.
struct ScanManyDevState;
void scan_many_dev_free(ScanManyDevState *s);  // the context's device is current, its stream drained

// Argument errors of dpow_scan_batch_device (decided before the device is touched): 0 or a negative code.
int scan_many_dev_check(const dpow_scan_task *tasks, size_t n_tasks, const void *d_idx_out, const void *d_row_out,
                        size_t max_hits, const size_t *n_out);

// The body of dpow_scan_batch_device (the arguments and the context checked, its device current).
int scan_many_dev_run(ScanManyDevState **state, hipStream_t stream, const volatile uint32_t *cancel,
                      dpow_scan_task *tasks, size_t n_tasks, void *d_idx_out, void *d_tz_out, void *d_row_out,
                      size_t max_hits, size_t *n_out, dpow_batch_stats *stats);

}  // namespace dpow
