// md5_batch_dev.h -- device code shared by the generic kernels, the ones that take the message
// layout as data and branch once on p / 4 (md5_batch.h batch_with_w0): batch_kernel, queue_kernel,
// scan_kernel, scan_many_kernel, scan_mask_kernel, census_kernel, census_many_kernel and
// digest_kernel.  What a kernel keeps to itself is its sink and what its last workgroup copies out
// and resets; the task row, the hash of one candidate, the window's step loop, the hit test, the
// wave-aggregated append and the retirement of a workgroup are here.
#pragma once

#include "md5_batch.h"

#if defined(__HIPCC__)

namespace dpow {

// A task row as a workgroup holds it: wave-uniform, read with scalar loads, kept in SGPRs.  (A
// field a kernel does not use is never loaded.)
struct BatchRow {
    uint32_t p, rbits, base_tb, ntz, len_bits, dmask;
    uint32_t T[16], iv[4];
};

__device__ __forceinline__ BatchRow batch_load_row(const BatchTask *t) {
    BatchRow r;
    r.p = t->p, r.rbits = t->rbits, r.base_tb = t->base_tb, r.ntz = t->ntz, r.len_bits = t->len_bits;
    r.dmask = t->dmask;
#pragma unroll
    for (int w = 0; w < 16; ++w) r.T[w] = t->T[w];
#pragma unroll
    for (int w = 0; w < 4; ++w) r.iv[w] = t->iv[w];
    return r;
}

// The MD5 state of local index i of row r, with p / 4 = W0 a compile-time constant.  A wave hashes
// the second final block when any of its lanes needs it; a lane that does not keeps its first.
template <int W0>
__device__ __forceinline__ void batch_hash_at(const BatchRow &r, uint64_t i, uint32_t st[4]) {
    uint32_t M[32];
    const uint32_t nblk = batch_candidate_words_at<W0>(r.T, r.p, r.rbits, r.base_tb, r.len_bits, i, M);
#pragma unroll
    for (int w = 0; w < 4; ++w) st[w] = r.iv[w];
    batch_md5_block(st, M);
    if constexpr (W0 > 11) {  // p + 1 + L > 55 needs p >= 48
        if (__any(nblk == 2u)) {
            uint32_t s2[4] = {st[0], st[1], st[2], st[3]};
            batch_md5_block(s2, M + 16);
#pragma unroll
            for (int w = 0; w < 4; ++w) st[w] = nblk == 2u ? s2[w] : st[w];
        }
    }
}

// A workgroup's sweep of the local indices [lo, hi) of row r: 256 candidates per step, one per
// lane, in increasing index order.  Per wave-step, i0 is the wave's first index, and
// body(i0, i, act, st) gets the lane's index, whether it is below hi (a lane past it hashes the
// clamped index hi - 1 and must be reported nowhere) and the lane's MD5 state.  (batch_kernel and
// scan_kernel write this header out themselves: md5_batch.hip and md5_scan.hip say why.)
template <int W0, typename Body>
__device__ __forceinline__ void batch_window_steps(const BatchRow &r, uint64_t lo, uint64_t hi, Body &&body) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = lo + (threadIdx.x & ~63u); i0 < hi; i0 += kBlockThreads) {
        uint64_t i = i0 + lane;
        const bool act = i < hi;
        if (!act) i = hi - 1;
        uint32_t st[4];
        batch_hash_at<W0>(r, i, st);
        body(i0, i, act, st);
    }
}

// The hit test of one wave-step.  dmask is the prefilter on the D word (BatchTask::dmask); only in
// a wave-step where some active lane passes it does the full test run, and then sink(m, ok) gets
// the wave's mask of hits -- active lanes whose digest ends in at least ntz '0' characters, which
// may be none -- and the lane's own bit.  (The sink is a callback, not a returned mask: a mask
// that had to be zero on the common path cost queue_kernel and scan_mask_kernel scalar
// instructions in every step)
template <typename Sink>
__device__ __forceinline__ void batch_hit_ballot(bool act, const uint32_t st[4], uint32_t dmask, uint32_t ntz,
                                                 Sink &&sink) {
    const bool cand = act && (st[3] & dmask) == 0u;
    if (__ballot(cand) != 0ull) {
        const bool ok = cand && trailing_zero_nibbles(st[0], st[1], st[2], st[3]) >= ntz;
        sink(__ballot(ok), ok);
    }
}

// Wave-aggregated append to a list whose length is *count: the first lane of m (the wave's
// appending lanes, not empty) claims popcount(m) places with one returning add, and each lane of m
// gets its own place, in lane order.  (The caller bounds the result against the list's capacity;
// a launch has at most 2^28 candidates, so the place does not wrap.)
__device__ __forceinline__ uint32_t wave_append_place(unsigned long long m, uint32_t *count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t leader = (uint32_t)(__ffsll((long long)m) - 1);
    uint32_t base = 0u;
    if (lane == leader)
        base = __hip_atomic_fetch_add(count, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __builtin_amdgcn_readlane(base, __builtin_amdgcn_readfirstlane(leader));
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// Words per lane in flight in a last workgroup's copy-out: a lane issues kCopyUnroll loads, then
// their stores, so that it waits for the device's coherence point once per kCopyUnroll words.
constexpr uint32_t kCopyUnroll = 8;

// Retirement: how a launch's results reach the host without the host waiting for the stream.
//
// No wave waits for another wave or for the host.  The only protocol is a count of retired
// workgroups (BatchLaunch::done); the workgroup whose add completes it -- the last -- copies the
// launch's results to pinned memory and writes the completion record (BatchRecord), which the host
// polls.  Three things make that sound (cdna_hip_programming.md 6, Guideline 16, form R1;
// MI355X_MICROARCH.md "visibility").
//
// 1. Performed before counted.  Whatever a workgroup hands to the last one it writes with relaxed
//    agent-scope atomic stores (write-through) or agent-scope atomic read-modify-writes.  Neither
//    stays in the CU's L1 or as a dirty L2 line: both are performed at the device's coherence
//    point, and both stay counted in vmcnt until they are.  So a wave that has drained
//    (s_waitcnt vmcnt(0), launch_count_retired<true>) has nothing left to publish, and after the
//    workgroup's barrier one lane's relaxed add to `done` comes after every such write of the
//    workgroup.  An agent-scope release fence in every workgroup would say the same and costs each
//    an L2 write-back (~0.2 ms per launch of 4096 small workgroups).  A wave whose only write is an
//    atomic whose returned value it consumes has waited for it already and needs no drain
//    (launch_count_retired<false>: batch_kernel's atomicMin).
// 2. The last workgroup reads what the others wrote with agent-scope atomic loads, which bypass its
//    CU's L1, behind one agent-scope acquire fence per wave.
// 3. The record is last.  The copies are relaxed system-scope stores from any wave; a system-scope
//    release, a drain and a barrier (launch_copies_performed) put all of them before lane 0's
//    record, whose seq is a system-scope release store behind the re-zeroing of `done`.  The device
//    words are therefore as the next launch expects them before the host can see the launch end.

// The launch's start tick, from its first workgroup.
__device__ __forceinline__ void launch_start_tick(const BatchLaunch &L) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(L.t0, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Counts this workgroup as retired; true (workgroup-uniform) in the launch's last.  Drain: every
// wave waits for its own stores and atomics first (point 1).
template <bool Drain>
__device__ __forceinline__ bool launch_count_retired(const BatchLaunch &L, uint32_t &s_last) {
    if constexpr (Drain) asm volatile("s_waitcnt vmcnt(0) ; dpow: the wave's writes performed" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t prev = __hip_atomic_fetch_add(L.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev + 1u == L.n_blocks ? 1u : 0u;
    }
    __syncthreads();
    return s_last != 0u;
}

// Every wave's copies before lane 0's record (point 3).
__device__ __forceinline__ void launch_copies_performed() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0) ; dpow: copies performed" ::: "memory");
    __syncthreads();
}

// The completion record, from thread 0 of the last workgroup, behind its own results.
__device__ __forceinline__ void launch_write_record(const BatchLaunch &L) {
    if (threadIdx.x == 0) {
        __hip_atomic_store(L.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long t_start = __hip_atomic_load(L.t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&L.rec->t_start, t_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&L.rec->t_end, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&L.rec->seq, L.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace dpow

#endif
