// md5_scan.h -- the scan (dpow_scan): every hit of a window in one pass.  Definitions shared by the
// gfx950 kernel (md5_scan.hip) and its host loop (scan.cpp).
//
// A search answers "the first hit"; a scan answers "which candidates hit".  The kernel shares the
// candidate assembly and the hash with the batched search (md5_batch.h: the task row, the layout
// as data, the one branch on p / 4) and nothing else: it has no early exit and no atomicMin, its
// hits go to a list.
#pragma once

#include "md5_batch.h"

namespace dpow {

// Entries of the device hit list of one launch: 2^16 global indices, 512 KB.  The slice rule
// (scan.cpp scan_slice) keeps a launch's expected hits at a quarter of it.
constexpr uint32_t kScanCap = 1u << 16;
constexpr uint32_t kScanMinCap = 256;  // one k: what a launch of 256 candidates can append at most

// One launch, passed by value (kernarg segment: the task row is read with scalar loads).  It covers
// the local indices [i_begin, i_end) of `task` in L.n_blocks workgroups of L.group indices each.
// Of the engine's BatchLaunch, `best` is the device hit list and `out_best` its pinned copy
// (`capacity` entries each); n_live is unused.
struct ScanLaunch {
    BatchTask task;
    BatchLaunch L;
    uint64_t i_begin, i_end;
    uint32_t *count;                // device: hits appended so far (zero at launch start; it counts past
                                    //  the capacity; the last workgroup re-zeroes it)
    unsigned long long *out_count;  // pinned: the launch's final count
    uint32_t capacity;              // entries of the lists this launch may use (kScanMinCap..kScanCap)
    uint32_t pad_;
};

#if defined(__HIPCC__)
hipError_t scan_prepare();
hipError_t scan_launch(const ScanLaunch &S, hipStream_t stream);
#endif

}  // namespace dpow
