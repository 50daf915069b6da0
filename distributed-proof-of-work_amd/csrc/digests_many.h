// digests_many.h -- host side of the digests of many nonces (digests_many.cpp), as dpow_api.cpp sees it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"
#include "digests.h"

namespace dpow {

// Device and pinned buffers of a context's dpow_digests_batch and dpow_digests_batch_device calls:
// allocated on its first call, freed with it.  (The host form's staging sets are dpow_digests'.)
struct DigestManyState;
void digests_many_free(DigestManyState *s);  // the context's device is current, its stream drained

// Argument errors that need no context (decided before the device is touched): 0 or a negative code.
int digests_many_check(const dpow_digest_task *tasks, size_t n_tasks, const uint64_t *rows, const uint64_t *global_idx,
                       const size_t *n_done);
int digests_many_check_device(const dpow_digest_task *tasks, size_t n_tasks, const void *d_rows,
                              const void *d_global_idx, const void *d_digest_out);

// The body of dpow_digests_batch (the arguments and the context checked, its device current,
// rows[n_tasks] > 0, the cancel flag seen low on entry).
int digests_many_run(DigestManyState **state, DigestState **sets, hipStream_t stream, const volatile uint32_t *cancel,
                     dpow_digest_task *tasks, size_t n_tasks, const uint64_t *rows, const uint64_t *global_idx,
                     uint8_t *digest_out, uint8_t *tz_out, size_t *n_done, dpow_batch_stats *stats);

// The body of dpow_digests_batch_device (the arguments and the context checked, its device current).
int digests_many_run_device(DigestManyState **state, hipStream_t stream, dpow_digest_task *tasks, size_t n_tasks,
                            const void *d_rows, const void *d_global_idx, size_t n, void *d_digest_out,
                            void *d_tz_out, dpow_batch_stats *stats);

}  // namespace dpow
