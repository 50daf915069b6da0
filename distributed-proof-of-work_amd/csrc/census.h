// census.h -- host side of the census (census.cpp), as dpow_api.cpp sees it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"

namespace dpow {

// The census of an empty window: counts 0, firsts DPOW_NO_HIT, depths 0.
void census_clear(dpow_census &c);

// One launch's table -- cnt[33] and first[33] as the kernel left them in pinned memory, of the local
// indices [lo, hi) of a task with partition (rbits, base_tb) -- checked, its first indices
// recomputed with the host MD5 and folded into `into` (census.cpp): the step dpow_census_window
// and dpow_census_batch share.  `msg` holds the task's nonce (nonce_len bytes) in front of
// DPOW_MAX_SECRET free bytes.  0, or DPOW_EVERIFY with "`who`: ..." set.
int census_fold_launch(const char *who, uint8_t *msg, size_t nonce_len, uint32_t rbits, uint32_t base_tb, uint64_t lo,
                       uint64_t hi, const unsigned long long *cnt, const unsigned long long *first, dpow_census &into);

// Device and pinned buffers of a context's censuses: allocated on its first census, freed with it.
struct CensusState;
void census_free(CensusState *s);  // the context's device is current, its stream drained

// The body of dpow_census_window (the arguments and the context checked, its device current, the
// window not empty, the cancel flag seen low on entry, *out cleared).
int census_run(CensusState **state, hipStream_t stream, const volatile uint32_t *cancel, const uint8_t *nonce,
               size_t nonce_len, uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin, uint64_t k_end,
               dpow_census *out, uint64_t *k_done, dpow_batch_stats *stats);

}  // namespace dpow
