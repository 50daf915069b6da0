// md5_scan_many_dev.h -- the batched device scan (dpow_scan_batch_device): the hits of many windows
// in increasing global index, task after task, left in device memory with their row pointers.
// Definitions shared by the gfx950 kernels (md5_scan_many_dev.hip) and their host loop
// (scan_many_dev.cpp).
//
// The batched scan's task array in (md5_scan_many.h: one workgroup descriptor per workgroup, the task
// rows in a device table), the device scan's output form out (md5_scan_dev.h: a wave's hit ballot is
// a word of a bitmap, a prefix over the workgroups' totals places the list).  A launch of the plan
// takes a mask launch, whose completion record the host waits for, and behind it without a wait the
// rows launch, the place launch and the depth launch.
#pragma once

#include "md5_batch.h"
#include "md5_scan_many.h"

namespace dpow {

// A descriptor's words have a fixed home: descriptor b of a launch owns the kScanManyDevSlotWords
// words from b * kScanManyDevSlotWords, enough for the longest descriptor (kBatchMaxGroup indices),
// whatever the descriptors before it hold (DESIGN.md section 20 says why not packed).
constexpr uint32_t kScanManyDevSlotWords = kBatchMaxGroup / 64;
constexpr size_t kScanManyDevMaskBytes = (size_t)kScanManyMaxBlocks * kScanManyDevSlotWords * sizeof(unsigned long long);
static_assert(kScanManyDevSlotWords == 256 && kScanManyDevMaskBytes == 40u << 20, "20480 slots of 2 KB");

// The mask launch of L.n_blocks descriptors, passed by value.  Of the engine's BatchLaunch, `best`,
// `out_best`, n_live and group are unused.
struct ScanManyMaskLaunch {
    BatchLaunch L;
    unsigned long long *mask;  // device: bit j % 64 of word j / 64 of slot b is the verdict of index i_begin + j
                               //  of descriptor b.  Never zeroed: a launch writes the ceil(len / 64) words of each
                               //  of its descriptors, and nothing may read a word beyond them.
    uint32_t *totals;          // device: hits of descriptor b (every launch writes [0, L.n_blocks))
    uint32_t *prefix;          // device: inclusive prefix of the totals
                               //  (both arrays: kScanManyMaxBlocks entries, 8-byte aligned)
    unsigned long long *out_total;  // pinned: the launch's hits, prefix[L.n_blocks - 1]
};

// The place launch over descriptors [0, n_blocks) of the launch a mask launch has just finished:
// workgroup b stores the global indices of its range's hits to out[base + prefix[b - 1] ...), in order.
struct ScanManyPlaceLaunch {
    const unsigned long long *mask;
    const uint32_t *prefix;
    unsigned long long *out;  // the caller's list
    uint64_t base;            // entries the call has placed before this launch
    uint64_t max_hits;        // entries of `out` (every store is clamped to it)
};

// One row pointer a launch settles: rows[row] = base + (first_block ? prefix[first_block - 1] : 0),
// the place of the first hit of the task whose part begins with descriptor first_block -- and of
// the empty tasks right before it.
struct ScanManyRowEntry {
    uint32_t row, first_block;
};

// One sampled entry of a finished call (pinned): its index, its depth when depths were asked for,
// and the task whose segment it lies in.
struct ScanManySample {
    unsigned long long idx;
    uint32_t tz;
    uint32_t task;
};
constexpr uint32_t kScanManyDevSamples = 16;  // the first, the last and 14 evenly spaced entries

// The rows launch.  Per launch of the plan: the n_entries rows of `table`.  Once behind the call's
// last launch: rows[fill_begin .. fill_end) = fill_value (the tasks not begun and the end row) and,
// when n > 0, the samples of the list's n entries; a sample's task is the last row below fill_begin
// that is at most its place (rows before fill_begin were written by earlier launches).  That launch
// also leaves the host its copies in pinned memory: all fill_end rows and the check word.
struct ScanManyRowsLaunch {
    const ScanManyRowEntry *table;
    const uint32_t *prefix;
    unsigned long long *rows;
    uint64_t base;
    uint32_t n_entries;
    uint32_t fill_begin, fill_end;
    uint32_t pad_;
    uint64_t fill_value;
    const unsigned long long *idx;
    const uint8_t *tz;        // or null
    uint64_t n;               // entries to sample from (0: no samples)
    ScanManySample *samples;  // pinned: kScanManyDevSamples entries
    unsigned long long *out_rows;  // pinned, or null: the copy of rows[0 .. fill_end) for the host
    uint32_t *bad;                 // device: the call's check word (ScanManyDepthLaunch::bad) ...
    uint32_t *out_bad;             // ... pinned, or null: its copy; the word itself is zeroed behind it
};

// The depth launch over descriptors [0, n_blocks) of a launch whose hits have been placed:
// workgroup b takes the entries [base + prefix[b - 1], base + prefix[b]) of the list.  It counts into
// *bad those whose local index lies outside the descriptor's range or in another partition and
// those not strictly above their predecessor within the task (rows[task] is where the task begins);
// with `tz` it re-hashes each with its task's row, stores the depth byte and counts the entries
// shallower than the task's ntz.
struct ScanManyDepthLaunch {
    const uint32_t *prefix;
    const unsigned long long *idx;
    uint8_t *tz;  // or null: the index-only form
    const unsigned long long *rows;
    uint32_t *bad;
    uint64_t base;
    uint64_t max_hits;
};

#if defined(__HIPCC__)
hipError_t scan_many_dev_prepare();
hipError_t scan_many_mask_launch(const BatchTask *tasks, const BatchEntry *blocks, const ScanManyMaskLaunch &S,
                                 hipStream_t stream);
hipError_t scan_many_place_launch(const BatchTask *tasks, const BatchEntry *blocks, const ScanManyPlaceLaunch &P,
                                  uint32_t n_blocks, hipStream_t stream);
hipError_t scan_many_rows_launch(const ScanManyRowsLaunch &R, hipStream_t stream);
hipError_t scan_many_depth_launch(const BatchTask *tasks, const BatchEntry *blocks, const ScanManyDepthLaunch &D,
                                  uint32_t n_blocks, hipStream_t stream);
#endif

}  // namespace dpow
