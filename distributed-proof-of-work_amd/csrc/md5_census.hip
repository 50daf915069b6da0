// md5_census.hip -- the generic kernel of the census (dpow_census_window, census.cpp): for every
// depth d = 1..32, how many candidates of a slice of one task's window end in at least d '0'
// characters, and the lowest of them.
//
// One launch hashes the local indices [i_begin, i_end) of one task.  Workgroup b takes the b-th
// group of L.group indices.  The task row is a kernel argument, so its fields are wave-uniform
// scalar loads; row, hash and step loop are the shared ones (md5_batch_dev.h).
//
// The depth sink.  One candidate in 16 reaches depth 1, so a sink that touched memory per hit would
// be the scan at N = 0 again.  Depths below kCensusRare are counted without memory: per step a wave
// ballots "active and the D word's last d nibbles are zero" for each such d, adds the popcount to a
// wave-uniform accumulator and notes, once, the first index it saw (lanes and steps go up in index
// order, so the first seen is the wave's lowest).  Only under a ballot of lanes whose last
// kCensusRare nibbles are zero (kCensusRare = 3: 1.5 % of wave-steps) do those lanes compute their
// depth and, for each d from kCensusRare to it, add to the workgroup's count and take the minimum
// into the workgroup's first index, both in LDS.  A step without such a lane issues no LDS or
// global memory operation.  Lanes past `hi` hash the clamped index hi - 1 and are counted nowhere.
//
// At the workgroup's end one lane of each wave joins the wave's accumulators to the LDS table, and
// after a barrier lane d of the first wave, for each depth with a non-zero count, issues one
// agent-scope atomic add on the launch's cnt[d] and one agent-scope atomicMin on first[d] (skipped
// when a relaxed load already shows a lower index): two to four of each per workgroup.
//
// Retirement (md5_batch_dev.h): the table is only ever touched by 8-byte agent-scope atomics --
// read-modify-writes here where the scan has entry stores -- drained before the count.  The last
// workgroup copies the 33 counts and 33 indices to pinned memory, re-initialises the device words
// and writes the completion record.
#include <hip/hip_runtime.h>

#include "md5_census.h"

namespace dpow {

namespace {

__device__ __forceinline__ void census_retire(const CensusLaunch &C, uint32_t &s_last) {
    const BatchLaunch &L = C.L;
    if (!launch_count_retired<true>(L, s_last)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x < 2u * kCensusDepths) {
        const uint32_t q = threadIdx.x;
        const unsigned long long v = __hip_atomic_load(L.best + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(L.out_best + q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // the table as the next launch expects it: counts 0, firsts none
        __hip_atomic_store(L.best + q, q < kCensusDepths ? 0ull : kNoHit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    launch_copies_performed();
    launch_write_record(L);
}

__global__ void __launch_bounds__(kBlockThreads) census_kernel(const CensusLaunch C) {
    __shared__ uint32_t s_cnt[kCensusDepths], s_first[kCensusDepths], s_last;
    launch_start_tick(C.L);
    if (threadIdx.x < kCensusDepths) {
        s_cnt[threadIdx.x] = 0u;
        s_first[threadIdx.x] = kNoOff;
    }
    __syncthreads();
    uint64_t lo = 0, hi = 0;
    const bool work = batch_block_range(C.i_begin, C.i_end, blockIdx.x, C.L.group, lo, hi);  // (workgroup-uniform)
    if (work) {
        const CensusGroup g{&C.task, s_cnt, s_first, lo, hi};
        batch_with_w0(__builtin_amdgcn_readfirstlane(C.task.p >> 2), g);
    }
    __syncthreads();  // the table is complete
    census_flush(work, lo, s_cnt, s_first, C.task.rbits, C.task.base_tb, C.L.best);
    census_retire(C, s_last);
}

}  // namespace

hipError_t census_prepare() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(census_kernel));
}

hipError_t census_launch(const CensusLaunch &C, hipStream_t stream) {
    hipLaunchKernelGGL(census_kernel, dim3(C.L.n_blocks), dim3(kBlockThreads), 0, stream, C);
    return hipGetLastError();
}

}  // namespace dpow
