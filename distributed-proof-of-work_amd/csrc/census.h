// census.h -- host side of the census (census.cpp), as dpow_api.cpp sees it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"

namespace dpow {

// The census of an empty window: counts 0, firsts DPOW_NO_HIT, depths 0.
void census_clear(dpow_census &c);

// Device and pinned buffers of a context's censuses: allocated on its first census, freed with it.
struct CensusState;
void census_free(CensusState *s);  // the context's device is current, its stream drained

// The body of dpow_census_window (the arguments and the context checked, its device current, the
// window not empty, the cancel flag seen low on entry, *out cleared).
int census_run(CensusState **state, hipStream_t stream, const volatile uint32_t *cancel, const uint8_t *nonce,
               size_t nonce_len, uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin, uint64_t k_end,
               dpow_census *out, uint64_t *k_done, dpow_batch_stats *stats);

}  // namespace dpow
