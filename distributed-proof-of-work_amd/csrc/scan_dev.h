// scan_dev.h -- host side of the device scan (scan_dev.cpp), as dpow_api.cpp sees it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"

namespace dpow {

// Device and pinned buffers of a context's device scans: allocated on its first call, freed with it.
struct ScanDevState;
void scan_dev_free(ScanDevState *s);  // the context's device is current, its stream drained

// The body of dpow_scan_device (arguments and context checked, the context's device current, the
// window not empty, the cancel flag seen low on entry).
int scan_dev_run(ScanDevState **state, hipStream_t stream, const volatile uint32_t *cancel, const uint8_t *nonce,
                 size_t nonce_len, uint32_t ntz, uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin,
                 uint64_t k_end, void *d_idx_out, void *d_tz_out, size_t max_hits, size_t *n_hits, uint64_t *k_done,
                 dpow_batch_stats *stats);

// The last call's kernel time by kind, in ms: mask launches, place launches, depth launches
// (zeros before the first call).
void scan_dev_times(const ScanDevState *s, double *mask_ms, double *place_ms, double *depth_ms);

}  // namespace dpow
