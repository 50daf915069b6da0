// md5_census.h -- the census (dpow_census_window): depth counts and per-depth first hits of a
// window in one pass.  Definitions shared by the gfx950 kernel (md5_census.hip) and its host loop
// (census.cpp), and the depth sink's device code, which the batched census's kernel
// (md5_census_many.hip) runs as well.
//
// A search answers "the first hit at depth N", a scan "which candidates reach depth N"; a census
// answers "how deep does this window go": for every depth d how many candidates end in at least d
// '0' characters and which is the first.  The answer is 33 counts and 33 indices whatever the
// density, so there is no list.  The kernel shares the candidate assembly and the hash with the
// batched search (md5_batch.h: the task row, the layout as data, the one branch on p / 4) and
// nothing else.
#pragma once

#include "md5_batch_dev.h"

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
// The depth sink, one source for census_kernel (md5_census.hip) and census_many_kernel
// (md5_census_many.hip); the comment at the top of md5_census.hip describes it.

constexpr uint32_t kNoOff = 0xFFFFFFFFu;  // "no candidate yet" of a first-index offset (offsets are < kBatchMaxGroup)

// One workgroup's range [lo, hi) of the task, with p / 4 a compile-time constant.  First indices
// are kept as offsets from `lo` (32 bits) until the workgroup's flush.
struct CensusGroup {
    const BatchTask *t;
    uint32_t *s_cnt, *s_first;  // the workgroup's table (LDS), depths kCensusRare..32 from the lanes
    uint64_t lo, hi;

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        const BatchRow r = batch_load_row(t);
        // the wave's accumulators of depths 1..kCensusRare - 1 (wave-uniform: SGPRs)
        uint32_t cnt[kCensusRare - 1], first[kCensusRare - 1];
#pragma unroll
        for (uint32_t l = 0; l + 1 < kCensusRare; ++l) cnt[l] = 0u, first[l] = kNoOff;
        const uint32_t rare_mask = tail_nibble_mask(kCensusRare);  // (folded: a constant)
        const uint32_t lane = threadIdx.x & 63u;
        batch_window_steps<W0>(r, lo, hi, [&](uint64_t i0, uint64_t i, bool act, const uint32_t st[4]) {
            // (the ballot builtin on the compare itself: one v_cmp per mask, the active lanes' mask ANDed in)
            const unsigned long long active = __builtin_amdgcn_ballot_w64(act);
#pragma unroll
            for (uint32_t l = 0; l + 1 < kCensusRare; ++l) {
                const unsigned long long m =
                    __builtin_amdgcn_ballot_w64((st[3] & tail_nibble_mask(l + 1u)) == 0u) & active;
                cnt[l] += (uint32_t)__popcll(m);
                if (first[l] == kNoOff) {  // (wave-uniform) set once
                    if (m != 0ull)
                        first[l] = __builtin_amdgcn_readfirstlane((uint32_t)(i0 - lo)) + (uint32_t)__builtin_ctzll(m);
                }
            }
            const bool rare = act && (st[3] & rare_mask) == 0u;
            if ((__builtin_amdgcn_ballot_w64((st[3] & rare_mask) == 0u) & active) != 0ull) {
                if (rare) {
                    const uint32_t depth = trailing_zero_nibbles(st[0], st[1], st[2], st[3]);
                    const uint32_t off = (uint32_t)(i - lo);
                    for (uint32_t d = kCensusRare; d <= depth; ++d) {  // depth <= 32 < kCensusDepths
                        __hip_atomic_fetch_add(s_cnt + d, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_min(s_first + d, off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
        });
        // The wave's accumulators join the workgroup's table.
        if (lane == 0u) {
#pragma unroll
            for (uint32_t l = 0; l + 1 < kCensusRare; ++l) {
                if (cnt[l] != 0u) {
                    __hip_atomic_fetch_add(s_cnt + l + 1u, cnt[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_min(s_first + l + 1u, first[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    }
};

// The workgroup's flush, after the barrier that completes its table: lane d of the first wave, for
// each depth with a non-zero count, issues one agent-scope add on cnt[d] and one agent-scope
// atomicMin on first[d] of `table` (cnt[kCensusDepths] then first[kCensusDepths]), the min skipped
// when a relaxed load already shows a lower index.
__device__ __forceinline__ void census_flush(bool work, uint64_t lo, const uint32_t *s_cnt, const uint32_t *s_first,
                                             uint32_t rbits, uint32_t base_tb, unsigned long long *table) {
    const uint32_t d = threadIdx.x;
    if (work && d >= 1u && d < kCensusDepths && s_cnt[d] != 0u) {
        unsigned long long *const cnt = table, *const first = table + kCensusDepths;
        const unsigned long long g = global_of_local(lo + s_first[d], rbits, base_tb);
        __hip_atomic_fetch_add(cnt + d, (unsigned long long)s_cnt[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_load(first + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > g)
            __hip_atomic_fetch_min(first + d, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

hipError_t census_prepare();
hipError_t census_launch(const CensusLaunch &C, hipStream_t stream);
#endif

}  // namespace dpow
