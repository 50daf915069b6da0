// scan.h -- host side of the scan (scan.cpp), as dpow_api.cpp sees it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"

namespace dpow {

// Local indices per launch of a scan for `ntz` with a hit list of `capacity` entries (DESIGN.md
// section 13): a multiple of 256 in [256, kBatchCap] whose expected hits, slice / 16^min(ntz, 32),
// are at most capacity / 4 wherever the slice is above 256.
uint64_t scan_slice(uint32_t ntz, uint32_t capacity);

// One verified entry, the step dpow_scan and dpow_scan_batch share: `h` for global index g from the
// host MD5 of nonce || secret (msg: the nonce followed by DPOW_MAX_SECRET bytes of room).  False,
// with h.tz the depth found, when that is below ntz.
bool scan_fill_hit(uint8_t *msg, size_t nonce_len, uint64_t g, uint32_t ntz, dpow_scan_hit &h);

// Device and pinned buffers of a context's scans: allocated on its first scan, freed with it.
struct ScanState;
void scan_free(ScanState *s);  // the context's device is current, its stream drained

// The body of dpow_scan (the arguments and the context checked, its device current, the window not
// empty, the cancel flag seen low on entry).
int scan_run(ScanState **state, hipStream_t stream, const volatile uint32_t *cancel, const uint8_t *nonce,
             size_t nonce_len, uint32_t ntz, uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin,
             uint64_t k_end, dpow_scan_hit *out, size_t max_hits, size_t *n_hits, uint64_t *k_done,
             dpow_batch_stats *stats);

}  // namespace dpow
