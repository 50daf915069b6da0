// md5_census.h -- the census (dpow_census_window): depth counts and per-depth first hits of a
// window in one pass.  Definitions shared by the gfx950 kernel (md5_census.hip) and its host loop
// (census.cpp).
//
// A search answers "the first hit at depth N", a scan "which candidates reach depth N"; a census
// answers "how deep does this window go": for every depth d how many candidates end in at least d
// '0' characters and which is the first.  The answer is 33 counts and 33 indices whatever the
// density, so there is no list.  The kernel shares the candidate assembly and the hash with the
// batched search (md5_batch.h: the task row, the layout as data, the one branch on p / 4) and
// nothing else.
#pragma once

#include "md5_batch.h"

namespace dpow {

constexpr uint32_t kCensusDepths = 33;  // depths 0..32 (= DPOW_CENSUS_DEPTHS, include/dpow.h)

// Depths below kCensusRare are counted by wave ballots into wave-uniform registers; a lane that
// reaches kCensusRare goes through the workgroup's table in LDS (md5_census.hip).  2..8: the rare
// test is one mask of the D word.  3 measured best of 2, 3 and 4.
#ifndef DPOW_CENSUS_RARE
#define DPOW_CENSUS_RARE 3
#endif
constexpr uint32_t kCensusRare = DPOW_CENSUS_RARE;
static_assert(kCensusRare >= 2 && kCensusRare <= 8, "the rare test is a mask of the D word");

// One launch, passed by value (kernarg segment: the task row is read with scalar loads).  It covers
// the local indices [i_begin, i_end) of `task` in L.n_blocks workgroups of L.group indices each.
// Of the engine's BatchLaunch, `best` is the launch's device table -- cnt[33] then first[33], 8
// bytes each, counts 0 and firsts kNoHit whenever no launch is in flight (depth 0 stays so: the
// host knows it) -- and `out_best` its pinned copy; n_live is unused.  task.ntz and task.dmask are
// unused.
struct CensusLaunch {
    BatchTask task;
    BatchLaunch L;
    uint64_t i_begin, i_end;
};

#if defined(__HIPCC__)
hipError_t census_prepare();
hipError_t census_launch(const CensusLaunch &C, hipStream_t stream);
#endif

}  // namespace dpow
