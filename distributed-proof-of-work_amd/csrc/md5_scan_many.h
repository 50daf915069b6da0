// md5_scan_many.h -- the batched scan (dpow_scan_batch): every hit of many windows in one pass.
// Definitions shared by the gfx950 kernel (md5_scan_many.hip), its host loop and planner
// (scan_many.cpp).
//
// A scan of one small window is a launch and a host round trip, not hashing (DESIGN.md sections 13
// and 16).  Here one launch hashes slices of many tasks: one workgroup descriptor per workgroup
// (queue_kernel's shape, BatchEntry's layout), the scan's hit sink per workgroup, and one hit list
// per launch whose entries name their descriptor, and through it their task.
#pragma once

#include "batch.h"
#include "md5_scan.h"

namespace dpow {

// An entry of the launch's hit list, one 32-bit word: the descriptor's index in the launch's table
// above the candidate's offset within the descriptor's range.  Descriptors are in task order and,
// within a task, in index order, so the entries sorted as words are in the call's output order.
constexpr uint32_t kScanManyOffBits = 14;
static_assert((1u << kScanManyOffBits) == kBatchMaxGroup, "an offset within a descriptor's range");
DPOW_HD uint32_t scan_many_entry(uint32_t block, uint32_t off) { return (block << kScanManyOffBits) | off; }
DPOW_HD uint32_t scan_many_entry_block(uint32_t e) { return e >> kScanManyOffBits; }
DPOW_HD uint32_t scan_many_entry_off(uint32_t e) { return e & (kBatchMaxGroup - 1u); }

// Workgroup descriptors of one launch (scan_many_next): the batched census's bound by the batched
// census's argument (md5_census_many.h kCensusManyMaxBlocks).  A launch holds at most kBatchCap
// local indices, cut into descriptors of batch_group(total): fewer than 8192 while the group
// follows total / kBatchBlocks or is kBatchMinGroup, at most kBatchCap / kBatchMaxGroup = 16384
// once it is kBatchMaxGroup; and each task of the launch adds at most one shorter descriptor at
// its end.  The hit budget only makes a launch smaller.
constexpr uint32_t kScanManyMaxBlocks = (uint32_t)(kBatchCap / kBatchMaxGroup) + DPOW_BATCH_MAX;
static_assert(kScanManyMaxBlocks == 20480 && kScanManyMaxBlocks <= (1u << (32 - kScanManyOffBits)),
              "16384 whole descriptors and one partial per task; the index fits the entry");

// One launch of L.n_blocks descriptors, passed by value.  Of the engine's BatchLaunch, `best` is
// the device hit list and `out_best` its pinned copy, both of 32-bit words (`capacity` entries of
// kScanCap allocated); n_live and group are unused.
struct ScanManyLaunch {
    BatchLaunch L;
    uint32_t *count;                // device: hits appended so far (zero at launch start; it counts past
                                    //  the capacity; the last workgroup re-zeroes it)
    unsigned long long *out_count;  // pinned: the launch's final count
    uint32_t capacity;              // entries of the lists this launch may use (kScanMinCap..kScanCap)
    uint32_t pad_;
};

#if defined(__HIPCC__)
hipError_t scan_many_prepare();
hipError_t scan_many_launch(const BatchTask *tasks, const BatchEntry *blocks, const ScanManyLaunch &S,
                            hipStream_t stream);
#endif

}  // namespace dpow
