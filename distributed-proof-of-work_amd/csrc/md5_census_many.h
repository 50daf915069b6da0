// md5_census_many.h -- the batched census (dpow_census_batch): the census of many tasks in one
// pass.  Definitions shared by the gfx950 kernel (md5_census_many.hip), its host loop and planner
// (census_many.cpp).
//
// A census of one small window is a launch and a host round trip, not hashing (DESIGN.md section
// 14: 0.13 ms for 8.4 us of hashing at 2^20 candidates), which is section 11's finding about the
// search.  Here one launch hashes slices of many tasks: one workgroup descriptor per workgroup
// (queue_kernel's shape, BatchEntry's layout: the tasks of one call differ in size by orders of
// magnitude), the census's depth sink per workgroup (md5_census.h: one source for both kernels),
// and one table of 33 counts and 33 first indices per task in device memory instead of one per
// launch.
#pragma once

#include "batch.h"
#include "md5_census.h"

namespace dpow {

// Words of one task's table: cnt[kCensusDepths] then first[kCensusDepths], 8 bytes each.
constexpr uint32_t kCensusTableWords = 2 * kCensusDepths;

// Workgroup descriptors of one launch (census_many_plan).  A launch holds at most kBatchCap local
// indices, cut into descriptors of batch_group(total): fewer than 8192 while the group follows
// total / kBatchBlocks or is kBatchMinGroup (total < 2^21), at most kBatchCap / kBatchMaxGroup =
// 16384 once it is kBatchMaxGroup; and each task of the launch adds at most one shorter descriptor
// at its end.
constexpr uint32_t kCensusManyMaxBlocks = (uint32_t)(kBatchCap / kBatchMaxGroup) + DPOW_BATCH_MAX;
static_assert(kCensusManyMaxBlocks == 20480, "16384 whole descriptors and one partial per task");

#if defined(__HIPCC__)
// One launch of L.n_blocks descriptors.  `tables` is L.best: DPOW_BATCH_MAX tables of
// kCensusTableWords words, the table of task slot s at L.best + s * kCensusTableWords, counts 0 and
// firsts kNoHit whenever no launch is in flight.  L.out_best is the pinned copy: entry q
// (kCensusTableWords words) is the table of slot out_slots[q], q < L.n_live.  L.group is unused.
hipError_t census_many_prepare();
hipError_t census_many_launch(const BatchTask *tasks, const BatchEntry *blocks, const uint32_t *out_slots,
                              const BatchLaunch &L, hipStream_t stream);
#endif

}  // namespace dpow
