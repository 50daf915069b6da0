// md5_census.hip -- the generic kernel of the census (dpow_census_window, census.cpp): for every
// depth d = 1..32, how many candidates of a slice of one task's window end in at least d '0'
// characters, and the lowest of them.
//
// One launch hashes the local indices [i_begin, i_end) of one task.  Workgroup b takes the b-th
// group of L.group indices, one candidate per lane and 256 per step, in increasing index order.
// The task row is a kernel argument, so its fields are wave-uniform scalar loads; the message
// layout is data and a workgroup branches once on its wave-uniform p / 4 (md5_batch.h), so k = 0,
// every chunk-length boundary and both block counts go through the same code as in batch_kernel
// and scan_kernel.
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
// Ordering (cdna_hip_programming.md 6, Guideline 16, form R1; MI355X_MICROARCH.md "visibility",
// valid forms: 8-byte agent-scope atomics on both sides): scan_retire's form.  The table is only
// ever touched by 8-byte agent-scope atomics -- read-modify-writes here where the scan has entry
// stores; like a write-through store an atomic is performed at the device's coherence point, not in
// this CU's L1 or as a dirty L2 line, and stays counted in vmcnt until then.  Every wave drains
// (s_waitcnt vmcnt(0)) before the workgroup's barrier and one lane then adds to the retirement
// count, so a workgroup's adds and mins are performed before its retirement is counted, without an
// agent-scope release in every workgroup.  The workgroup whose add completes the launch acquires at
// agent scope, reads the 33 counts and 33 indices with atomic loads, copies them to pinned memory,
// re-initialises the device words and writes the completion record last.
//
// No wave waits for another wave or for the host: the grid is bounded, a workgroup's work is
// fixed at its start, and the only cross-workgroup state is the table and the retirement count.
#include <hip/hip_runtime.h>

#include "md5_census.h"

namespace dpow {

namespace {

// Retirement, counted per workgroup, and the copy-out by the workgroup whose count completes the
// launch (md5_scan.hip scan_retire).  Every wave has drained its atomics before the barrier, so the
// count comes after every add and min of the workgroup.
__device__ __forceinline__ void census_retire(const CensusLaunch &C, uint32_t &s_last) {
    const BatchLaunch &L = C.L;
    asm volatile("s_waitcnt vmcnt(0) ; dpow census: adds and mins performed" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t prev = __hip_atomic_fetch_add(L.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev + 1u == L.n_blocks ? 1u : 0u;
    }
    __syncthreads();
    if (s_last == 0u) return;  // (workgroup-uniform)
    // The last workgroup: every other workgroup's adds and mins are performed.  Each wave acquires
    // for its own loads; the loads are atomic (they bypass this CU's L1) as well.
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x < 2u * kCensusDepths) {
        const uint32_t q = threadIdx.x;
        const unsigned long long v = __hip_atomic_load(L.best + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(L.out_best + q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // the table as the next launch expects it: counts 0, firsts none
        __hip_atomic_store(L.best + q, q < kCensusDepths ? 0ull : kNoHit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // every wave's copies before lane 0's record
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0) ; dpow census: copies performed" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(L.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long t_start = __hip_atomic_load(L.t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&L.rec->t_start, t_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&L.rec->t_end, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&L.rec->seq, L.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ void __launch_bounds__(kBlockThreads) census_kernel(const CensusLaunch C) {
    __shared__ uint32_t s_cnt[kCensusDepths], s_first[kCensusDepths], s_last;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(C.L.t0, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
