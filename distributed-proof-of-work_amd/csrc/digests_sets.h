// digests_sets.h -- the staging of dpow_digests (digests.cpp) as dpow_digests_batch shares it
// (digests_many.cpp): the context's two buffer sets, the call's chunk and staging, a launch's shape.
// Internal: dpow_api.cpp needs none of it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "digests.h"
#include "md5_digest.h"

namespace dpow {

// One buffer set: kDigestChunk indices, digests and depth bytes, in pinned mapped memory and (for the
// "copy" staging, allocated by its first use) in device memory, and the events of its launch.
constexpr size_t kDigestIdxOff = 0;
constexpr size_t kDigestOutOff = kDigestIdxOff + (size_t)kDigestChunk * 8;
constexpr size_t kDigestTzOff = kDigestOutOff + (size_t)kDigestChunk * 16;
constexpr size_t kDigestSetBytes = kDigestTzOff + kDigestChunk;
struct DigestSet {
    char *h_mem = nullptr;    // pinned, mapped
    char *d_h_mem = nullptr;  // device alias of h_mem
    char *d_mem = nullptr;    // device ("copy" staging only)
    hipEvent_t start = nullptr, stop = nullptr;  // around the kernel (timing)
    hipEvent_t done = nullptr;                   // behind the launch's last copy
};

// The context's digest state with both sets allocated for this staging; *sets: its two sets.  (One
// search, batch, scan, census or digest call is in flight per context, so the sets have one user.)
int digests_staging(DigestState **state, hipStream_t stream, bool mapped, const char *who, DigestSet **sets);

uint32_t digest_chunk();           // DPOW_DIAG_DIGEST_CHUNK: the entries per chunk of this call
bool digest_staging_mapped();      // DPOW_DIAG_DIGEST_STAGING: this call's staging
// Workgroups of a launch of `count` entries, `group` (a multiple of 256) each.
uint32_t digest_shape(uint32_t count, uint32_t &group);

}  // namespace dpow
