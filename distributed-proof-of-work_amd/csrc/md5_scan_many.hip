// md5_scan_many.hip -- the generic kernel of the batched scan (dpow_scan_batch, scan_many.cpp):
// every hit of many tasks' windows in one launch.
//
// One launch hashes a slice of the local index ranges of the call's next tasks, one descriptor per
// workgroup (md5_batch.hip queue_kernel's shape, BatchEntry's layout): workgroup b hashes
// [i_begin, i_end) -- at most kBatchMaxGroup local indices -- of the task in table slot
// blocks[b].task.  The task's fields, its ntz and its prefilter mask among them, are wave-uniform
// and come from the device task table with scalar loads; the workgroup branches once on its task's
// wave-uniform p / 4 (md5_batch.h), hashes 256 candidates per step, one per lane, in increasing
// index order, lanes past `hi` hashing the clamped index and reported nowhere.
//
// The hit sink is scan_kernel's (md5_scan.hip).  Per step the lanes that pass the D-word prefilter
// and the full trailing-zero test of their own task are balloted; the first hit lane claims
// popcount(mask) places with one returning atomic add on the launch's count, and every hit lane
// stores its entry to place base + rank if that is below the capacity.  An entry is one 32-bit
// word, the workgroup's descriptor index above the candidate's offset in the descriptor's range
// (md5_scan_many.h): one store publishes it whole, and the host rebuilds the task and the index
// from the launch's descriptors.  The count keeps counting past the capacity, so the host learns
// the true number and re-plans an overflowed launch with halved budgets.
//
// Ordering: md5_scan.hip's form unchanged (cdna_hip_programming.md 6, Guideline 16, form R1).  An
// entry is a 4-byte relaxed agent-scope atomic store (write-through), every wave drains its stores
// (s_waitcnt vmcnt(0)) before the workgroup's barrier, and one lane then adds to the retirement
// count -- so every entry of a workgroup is performed before its retirement is counted.  The
// workgroup whose add completes the launch acquires at agent scope, reads the count and the
// entries with atomic loads and copies min(count, capacity) of them to pinned memory, all four
// waves copying with kCopyUnroll words per lane in flight: entries, then the count, then the
// completion record, the device words re-zeroed before it.
//
// No wave waits for another wave or for the host: the grid is bounded, a workgroup's work is
// fixed at its start, and the only cross-workgroup state is the hit count and the retirement count.
#include <hip/hip_runtime.h>

#include "md5_scan_many.h"

namespace dpow {

namespace {

// One workgroup's range [lo, hi) of its task, with p / 4 a compile-time constant (md5_batch.h
// batch_with_w0).  `tag` is the workgroup's descriptor index, shifted to its place in an entry.
struct ScanManyGroup {
    const BatchTask *t;
    uint32_t *hits;  // the launch's device hit list
    uint32_t *count;
    uint32_t capacity, tag;
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
                    // (base < 2^28 + 64: a launch has at most 2^28 candidates, so `at` does not wrap;
                    // i - lo < kBatchMaxGroup: the descriptor's range is at most that long.)
                    if (ok && at < capacity)
                        __hip_atomic_store(hits + at, tag | (uint32_t)(i - lo), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
};

// Retirement (md5_scan.hip scan_retire), with the copy-out of the entries by all four waves of the
// last workgroup.  A lane's kCopyUnroll loads are issued first, then its stores, so that it waits
// for the device's coherence point once per kCopyUnroll words, not once per word.
constexpr uint32_t kCopyUnroll = 8;

__device__ __forceinline__ void scan_many_retire(const ScanManyLaunch &S, uint32_t &s_last) {
    const BatchLaunch &L = S.L;
    asm volatile("s_waitcnt vmcnt(0) ; dpow scan-many: entries performed" ::: "memory");
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
    const uint32_t n = total < S.capacity ? total : S.capacity;  // <= kScanCap: what both lists hold
    const uint32_t *const list = reinterpret_cast<const uint32_t *>(L.best);
    uint32_t *const out = reinterpret_cast<uint32_t *>(L.out_best);
    for (uint32_t q0 = threadIdx.x; q0 < n; q0 += kCopyUnroll * kBlockThreads) {
        uint32_t v[kCopyUnroll];
        // The loads are not predicated: a lane past the end loads the last entry again (n > 0 here)
        // and stores nothing.
#pragma unroll
        for (uint32_t u = 0; u < kCopyUnroll; ++u) {
            const uint32_t q = q0 + u * kBlockThreads < n ? q0 + u * kBlockThreads : n - 1u;
            v[u] = __hip_atomic_load(list + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (uint32_t u = 0; u < kCopyUnroll; ++u) {
            const uint32_t q = q0 + u * kBlockThreads;
            if (q < n) __hip_atomic_store(out + q, v[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    // every wave's copies before lane 0's count and record
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0) ; dpow scan-many: copies performed" ::: "memory");
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

__global__ void __launch_bounds__(kBlockThreads)
    scan_many_kernel(const BatchTask *__restrict__ tasks, const BatchEntry *__restrict__ blocks,
                     const ScanManyLaunch S) {
    __shared__ uint32_t s_last;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(S.L.t0, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const BatchEntry *const e = blocks + blockIdx.x;
    const uint64_t lo = e->i_begin, hi = e->i_end;  // hi - lo <= kBatchMaxGroup (scan_many.cpp)
    const BatchTask *const t = tasks + e->task;     // < DPOW_BATCH_MAX (scan_many.cpp)
    if (lo < hi) {                                  // (workgroup-uniform)
        uint32_t *const list = reinterpret_cast<uint32_t *>(S.L.best);
        const ScanManyGroup g{t, list, S.count, S.capacity, scan_many_entry(blockIdx.x, 0u), lo, hi};
        batch_with_w0(__builtin_amdgcn_readfirstlane(t->p >> 2), g);
    }
    scan_many_retire(S, s_last);
}

}  // namespace

hipError_t scan_many_prepare() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(scan_many_kernel));
}

hipError_t scan_many_launch(const BatchTask *tasks, const BatchEntry *blocks, const ScanManyLaunch &S,
                            hipStream_t stream) {
    hipLaunchKernelGGL(scan_many_kernel, dim3(S.L.n_blocks), dim3(kBlockThreads), 0, stream, tasks, blocks, S);
    return hipGetLastError();
}

}  // namespace dpow
