// md5_scan_dev.h -- the device scan (dpow_scan_device): a window's hits in increasing global index,
// left in device memory.  Definitions shared by the gfx950 kernels (md5_scan_dev.hip) and their
// host loop (scan_dev.cpp).
//
// dpow_scan's kernel appends hits in no order and its host sorts, re-hashes and copies every one.
// Here the order comes from the geometry: a wave's 64 lanes hold 64 consecutive local indices, so
// the wave's hit ballot is a 64-bit piece of the slice's hit bitmap, and a bitmap plus a prefix sum
// of popcounts is the ordered list.  A slice takes two bounded launches: scan_mask_kernel hashes and
// writes the bitmap and each workgroup's hit total (its last workgroup turns the totals into their
// inclusive prefix), scan_place_kernel turns bitmap and prefix into the list.  The list has no
// capacity of its own, so a slice is kBatchCap local indices whatever N.  The kernels share the
// candidate assembly and the hash with the batched search (md5_batch.h) and nothing else.
#pragma once

#include "md5_batch.h"

namespace dpow {

// Local indices per slice (= batch.h kBatchCap), the most workgroups of a slice (its groups are
// batch_group's: at most 16384 indices, and 16384 of them once the slice is 2^28), and the most
// hits of one group -- which is why dpow_scan_device wants room for DPOW_SCAN_DEVICE_MIN_HITS.
constexpr uint64_t kScanDevSlice = 1ull << 28;
constexpr uint32_t kScanDevMaxGroup = 16384;
constexpr uint32_t kScanDevMaxBlocks = (uint32_t)(kScanDevSlice / kScanDevMaxGroup);
constexpr size_t kScanDevMaskBytes = (size_t)(kScanDevSlice / 8);  // one bit per local index: 32 MB

// The mask launch, passed by value (kernarg segment: the task row is read with scalar loads).  It
// covers the local indices [i_begin, i_end) of `task` in L.n_blocks workgroups of L.group indices
// each.  Of the engine's BatchLaunch, `best` and `out_best` are unused.
struct ScanMaskLaunch {
    BatchTask task;
    BatchLaunch L;
    uint64_t i_begin, i_end;
    unsigned long long *mask;  // device: bit (i - i_begin) % 64 of word (i - i_begin) / 64 is index i's
                               //  verdict.  Never zeroed: a launch writes the ceil((i_end - i_begin) / 64)
                               //  words of its slice, and nothing may read a word its slice did not write.
    uint32_t *totals;          // device: hits of workgroup b (every launch writes [0, L.n_blocks))
    uint32_t *prefix;          // device: inclusive prefix of the totals, for the place launch and, copied out,
                               //  for the host's cut of a slice that does not fit
                               //  (both arrays: kScanDevMaxBlocks entries, 8-byte aligned)
    unsigned long long *out_total;  // pinned: the slice's hits, prefix[L.n_blocks - 1]
};

// The place launch over workgroups [0, n_blocks) of the slice a mask launch has just finished:
// workgroup b stores the global indices of its range's hits to out[base + prefix[b - 1] ...), in order.
struct ScanPlaceLaunch {
    const unsigned long long *mask;
    const uint32_t *prefix;
    unsigned long long *out;  // the caller's list
    uint64_t base;            // entries the call has placed before this slice
    uint64_t max_hits;        // entries of `out` (every store is clamped to it)
    uint64_t i_begin, i_end;
    uint32_t group, n_blocks;
    uint32_t rbits, base_tb;
};

// One sampled entry of a finished call (pinned): its index and, when depths were asked for, its depth.
struct ScanDevSample {
    unsigned long long idx;
    uint32_t tz;
    uint32_t pad_;
};
constexpr uint32_t kScanDevSamples = 16;  // the first, the last and 14 evenly spaced entries (digests.cpp kDigestSamples)

// The check launch over the n entries a call has placed.
struct ScanCheckLaunch {
    const unsigned long long *idx;
    const uint8_t *tz;       // or null
    uint64_t n;              // > 0
    uint32_t ntz;
    uint32_t pad_;
    uint32_t *bad;           // device word, added to: entries shallower than ntz or not above their predecessor
    ScanDevSample *samples;  // pinned: kScanDevSamples entries
};

#if defined(__HIPCC__)
hipError_t scan_dev_prepare();
hipError_t scan_mask_launch(const ScanMaskLaunch &S, hipStream_t stream);
hipError_t scan_place_launch(const ScanPlaceLaunch &P, hipStream_t stream);
hipError_t scan_check_launch(const ScanCheckLaunch &C, hipStream_t stream);
#endif

}  // namespace dpow
