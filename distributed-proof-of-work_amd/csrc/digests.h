// digests.h -- host side of the digests (digests.cpp), as dpow_api.cpp sees it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"

namespace dpow {

// Device and pinned buffers of a context's digest calls: allocated on its first call, freed with it.
struct DigestState;
void digests_free(DigestState *s);  // the context's device is current, its stream drained

// The body of dpow_digests (the arguments, the list's range and the context checked, its device
// current, n > 0, the cancel flag seen low on entry).
int digests_run(DigestState **state, hipStream_t stream, const volatile uint32_t *cancel, const uint8_t *nonce,
                size_t nonce_len, const uint64_t *global_idx, size_t n, uint8_t *digest_out, uint8_t *tz_out,
                size_t *n_done, dpow_batch_stats *stats);

// The body of dpow_digests_device (the arguments and the context checked, its device current, n > 0).
int digests_run_device(DigestState **state, hipStream_t stream, const uint8_t *nonce, size_t nonce_len,
                       const void *d_global_idx, size_t n, void *d_digest_out, void *d_tz_out,
                       dpow_batch_stats *stats);

}  // namespace dpow
