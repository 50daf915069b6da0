// md5_scan.hip -- the generic kernel of the scan (dpow_scan, scan.cpp): every hit of a slice of one
// task's window, appended to a list.
//
// One launch hashes the local indices [i_begin, i_end) of one task.  Workgroup b takes the b-th
// group of L.group indices, one candidate per lane and 256 per step, in increasing index order.
// The task row is a kernel argument, so its fields are wave-uniform scalar loads; the message
// layout is data and a workgroup branches once on its wave-uniform p / 4 (md5_batch.h), so k = 0,
// every chunk-length boundary and both block counts go through the same code as in batch_kernel.
//
// The hit sink.  There is no early exit and no atomicMin.  Per step the lanes that pass the D-word
// prefilter and the full trailing-zero test are balloted; the first hit lane claims popcount(mask)
// places with one returning atomic add on the launch's count, and every hit lane stores its global
// index to place base + rank if that is below the capacity.  The count keeps counting past the
// capacity, so the host learns the true number and re-runs an overflowed slice in halves.
//
// Ordering (cdna_hip_programming.md 6, Guideline 16, form R1): an entry is an 8-byte relaxed
// agent-scope atomic store (write-through), every wave drains its stores (s_waitcnt vmcnt(0))
// before the workgroup's barrier, and one lane then adds to the retirement count -- so every entry
// of a workgroup is performed before its retirement is counted, without an agent-scope release in
// every workgroup.  The workgroup whose add completes the launch acquires at agent scope, reads
// the count and the entries with atomic loads and copies them to pinned memory: entries, then the
// count, then the completion record.  Waves without hits pay the (empty) drain only.
//
// No wave waits for another wave or for the host: the grid is bounded, a workgroup's work is
// fixed at its start, and the only cross-workgroup state is the hit count and the retirement count.
#include <hip/hip_runtime.h>

#include "md5_scan.h"

namespace dpow {

namespace {

// One workgroup's range [lo, hi) of the task, with p / 4 a compile-time constant (md5_batch.h
// batch_with_w0): 256 candidates per step, one per lane, in increasing index order.
struct ScanGroup {
    const BatchTask *t;
    unsigned long long *hits;  // the launch's device hit list
    uint32_t *count;
    uint32_t capacity;
    uint64_t lo, hi;

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        const uint32_t p = t->p, rbits = t->rbits, base_tb = t->base_tb, ntz = t->ntz, len_bits = t->len_bits;
        const uint32_t dmask = t->dmask;
        // the template and the midstate (wave-uniform: SGPRs)
        uint32_t T[16], iv[4];
#pragma unroll
        for (int w = 0; w < 16; ++w) T[w] = t->T[w];
#pragma unroll
        for (int w = 0; w < 4; ++w) iv[w] = t->iv[w];
        const uint32_t lane = threadIdx.x & 63u;
        for (uint64_t i0 = lo + (threadIdx.x & ~63u); i0 < hi; i0 += kBlockThreads) {  // i0: the wave's first index
            uint64_t i = i0 + lane;
            const bool act = i < hi;
            if (!act) i = hi - 1;
            uint32_t M[32];
            const uint32_t nblk = batch_candidate_words_at<W0>(T, p, rbits, base_tb, len_bits, i, M);
            uint32_t st[4] = {iv[0], iv[1], iv[2], iv[3]};
            batch_md5_block(st, M);
            if constexpr (W0 > 11) {  // p + 1 + L > 55 needs p >= 48
                if (__any(nblk == 2u)) {
                    uint32_t s2[4] = {st[0], st[1], st[2], st[3]};
                    batch_md5_block(s2, M + 16);
#pragma unroll
                    for (int w = 0; w < 4; ++w) st[w] = nblk == 2u ? s2[w] : st[w];
                }
            }
            const bool cand = act && (st[3] & dmask) == 0u;
            if (__ballot(cand) != 0ull) {
                const bool ok = cand && trailing_zero_nibbles(st[0], st[1], st[2], st[3]) >= ntz;
                const unsigned long long m = __ballot(ok);
                if (m != 0ull) {
                    // Wave-aggregated append: the first hit lane claims the wave's places.
                    const uint32_t leader = (uint32_t)(__ffsll((long long)m) - 1);
                    uint32_t base = 0u;
                    if (lane == leader)
                        base = __hip_atomic_fetch_add(count, (uint32_t)__popcll(m), __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
                    base = __builtin_amdgcn_readlane(base, __builtin_amdgcn_readfirstlane(leader));
                    const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    // (base < 2^28 + 64: a launch has at most 2^28 candidates, so `at` does not wrap.)
                    if (ok && at < capacity)
                        __hip_atomic_store(hits + at, (unsigned long long)global_of_local(i, rbits, base_tb),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
};

// Retirement, counted per workgroup, and the copy-out by the workgroup whose count completes the
// launch.  Every wave has drained its entry stores before the barrier, so the count comes after
// every entry of the workgroup (no agent-scope release per workgroup: md5_batch.hip retire_workgroup).
__device__ __forceinline__ void scan_retire(const ScanLaunch &S, uint32_t &s_last) {
    const BatchLaunch &L = S.L;
    asm volatile("s_waitcnt vmcnt(0) ; dpow scan: entries performed" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t prev = __hip_atomic_fetch_add(L.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev + 1u == L.n_blocks ? 1u : 0u;
    }
    __syncthreads();
    if (s_last == 0u) return;  // (workgroup-uniform)
    // The last workgroup: every other workgroup's entries and count adds are performed.  Each wave
    // acquires for its own loads; the loads are atomic (they bypass this CU's L1) as well.
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const uint32_t total = __hip_atomic_load(S.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t n = total < S.capacity ? total : S.capacity;
    for (uint32_t q = threadIdx.x; q < n; q += kBlockThreads) {
        const unsigned long long g = __hip_atomic_load(L.best + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(L.out_best + q, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // every wave's copies before lane 0's count and record
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0) ; dpow scan: copies performed" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(S.out_count, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(S.count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(L.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long t_start = __hip_atomic_load(L.t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&L.rec->t_start, t_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&L.rec->t_end, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&L.rec->seq, L.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ void __launch_bounds__(kBlockThreads) scan_kernel(const ScanLaunch S) {
    __shared__ uint32_t s_last;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(S.L.t0, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint64_t lo, hi;
    if (batch_block_range(S.i_begin, S.i_end, blockIdx.x, S.L.group, lo, hi)) {
        const ScanGroup g{&S.task, S.L.best, S.count, S.capacity, lo, hi};
        batch_with_w0(__builtin_amdgcn_readfirstlane(S.task.p >> 2), g);
    }
    scan_retire(S, s_last);
}

}  // namespace

hipError_t scan_prepare() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(scan_kernel));
}

hipError_t scan_launch(const ScanLaunch &S, hipStream_t stream) {
    hipLaunchKernelGGL(scan_kernel, dim3(S.L.n_blocks), dim3(kBlockThreads), 0, stream, S);
    return hipGetLastError();
}

}  // namespace dpow
