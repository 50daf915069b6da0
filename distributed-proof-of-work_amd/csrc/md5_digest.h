// md5_digest.h -- the digests (dpow_digests): MD5 and depth of any listed candidates in one pass.
// Definitions shared by the gfx950 kernel (md5_digest.hip) and its host loop (digests.cpp).
//
// A search, a scan and a census walk a window and report where digests end in zeros; this kernel
// takes a list of global indices of one nonce and reports what it computes for each: all four
// state words and the depth.  It shares the candidate assembly and the hash with the batched
// search (md5_batch.h: the task row, the layout as data, the one branch on p / 4) and nothing else:
// its input is a gather from a list, its sink a full digest per entry, and it has no cross-workgroup
// protocol.
#pragma once

#include "md5_batch.h"

namespace dpow {

// Entries per chunk of dpow_digests' host loop: a chunk is one launch, staged through one of two
// buffer sets (digests.cpp).  DESIGN.md section 15 has the comparison of 2^16, 2^18 and 2^20.
#ifndef DPOW_DIGEST_CHUNK_LOG2
#define DPOW_DIGEST_CHUNK_LOG2 18
#endif
constexpr uint32_t kDigestChunk = 1u << DPOW_DIGEST_CHUNK_LOG2;
constexpr uint32_t kDigestMinChunk = 256;  // one workgroup step
// Entries per launch of dpow_digests_device (lists resident on the device need no staging).
constexpr uint32_t kDigestDeviceSlice = 1u << 24;
static_assert(kDigestChunk >= kDigestMinChunk && kDigestChunk <= kDigestDeviceSlice, "a chunk is one launch");

constexpr uint8_t kDigestBadDepth = 0xFF;  // depth byte of an entry with k >= DPOW_K_LIMIT (device variant)

// One launch, passed by value (kernarg segment: the task row is read with scalar loads).  The task
// row is batch_fill_task's with worker_bits = 0: rbits = 8, base_tb = 0, so the local index of a
// candidate is its global index.  Workgroup b takes entries [b * group, min(n, (b + 1) * group)).
struct DigestLaunch {
    BatchTask task;
    const unsigned long long *idx;  // n global indices (8-byte aligned)
    uint4 *digest;                  // n digests, 16 bytes each (16-byte aligned), or null
    uint8_t *tz;                    // n depth bytes, or null
    uint32_t *bad;                  // device word: entries out of range, added to (never reset here)
    uint32_t n;                     // entries of this launch (<= kDigestDeviceSlice)
    uint32_t group;                 // entries per workgroup, a multiple of 256
};

#if defined(__HIPCC__)
hipError_t digest_prepare();
hipError_t digest_launch(const DigestLaunch &D, uint32_t n_blocks, hipStream_t stream);
#endif

}  // namespace dpow
