// md5_scan_dev.hip -- the kernels of the device scan (dpow_scan_device, scan_dev.cpp): a slice's hit
// bitmap and per-workgroup hit totals (scan_mask_kernel), the ordered list from bitmap and prefix
// (scan_place_kernel), and the check of a finished call's list (scan_check_kernel).
//
// scan_mask_kernel.  The geometry is scan_kernel's (md5_scan.hip): workgroup b takes the b-th group
// of L.group local indices of [i_begin, i_end), the task row in the kernarg segment; row, hash,
// step loop and hit test are the shared ones (md5_batch_dev.h).  The sink differs.  A wave's lanes
// hold the 64 consecutive local indices i0 .. i0 + 63 and i0 - i_begin is a multiple of 64 (groups
// are multiples of 256), so the wave's hit ballot is word (i0 - i_begin) / 64 of the slice's
// bitmap, hit or no hit, lanes past the range contributing 0.  A wave runs at most 64 steps, so it
// keeps the words in one register pair -- step s's ballot in lane s, put there by one compare and
// two selects with scalar operands, and only by a step that has a candidate -- and its lanes store them
// behind the loop, one word each.  (One lane storing every step's word as it comes is the same
// bitmap and cost the loop 1 %: DESIGN.md section 18.)  A word is written for every wave-step the
// loop runs, whatever it holds, so the bitmap is never zeroed: it holds stale words of earlier
// slices behind this slice's ceil((i_end - i_begin) / 64), and nothing reads those.  The stores
// are plain: their reader is a later launch.  Behind the loop each wave sums the bits of its words;
// the four sums meet in LDS.  A step without a candidate costs the loop one scalar add more than
// scan_kernel's.
//
// Retirement (md5_batch_dev.h): one lane publishes the workgroup's hit total with a 4-byte relaxed
// agent-scope atomic store, drained before the count.  The last workgroup reads the totals and
// writes their inclusive prefix (at most 16384 groups, uint32: a slice has at most 2^28
// candidates) to a device array for the place launch and the slice's total to pinned memory for
// the host; then it writes the completion record.  It deviates in one thing: the total is lane 0's
// own store and the prefix is read behind the kernel boundary, so nothing has to be ordered before
// the record but lane 0's own stores.  (The host copies the prefix out itself when a slice does not
// fit the caller's room: writing all of it to pinned memory in every launch cost more than the
// sink.)
//
// scan_place_kernel.  A second bounded launch over the leading workgroups of the same slice.
// Workgroup b loads the ceil((hi - lo) / 64) <= 256 bitmap words of its own range, one per thread,
// and the exclusive prefix of b.  These are plain loads, and that is correct: the bitmap and the
// prefix were written by an earlier launch on the same stream, and a kernel boundary makes a
// launch's stores visible to the next whatever their form -- the in-launch protocol above exists
// only for the last workgroup of the mask launch.  A wave takes the exclusive scan of its 64
// popcounts, the wave totals go through LDS, and for every non-zero word (wave-uniformly) lane l
// with bit l set stores global_of_local(lo + 64 word + l) to out[base + rank], rank = the hits
// below it -- consecutive hits are consecutive 8-byte stores.  Every store is clamped to max_hits.
//
// scan_check_kernel.  Over the list of a finished call: counts into one device word the entries
// whose depth is below ntz (when depths exist) and those not strictly above their predecessor, and
// gathers 16 sampled entries into pinned memory for the host's MD5.
//
// No wave waits for another wave or for the host: every grid is bounded, a workgroup's work is fixed
// at its start, and the only cross-workgroup state is the totals, the retirement count and the
// check word.
#include <hip/hip_runtime.h>

#include "md5_batch_dev.h"
#include "md5_scan_dev.h"

namespace dpow {

namespace {

// One workgroup's range [lo, hi) of the task, with p / 4 a compile-time constant.
struct ScanMaskGroup {
    const BatchTask *t;
    unsigned long long *mask;
    uint64_t i_begin, lo, hi;
    uint32_t *wave_hits;  // out: the hits of this wave's steps (wave-uniform)

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        const BatchRow r = batch_load_row(t);
        const uint32_t lane = threadIdx.x & 63u;
        // The wave's words, gathered: lane s holds the ballot of the wave's step s (at most 64 steps:
        // a group is at most 64 x 256 indices), zero until a step with a hit puts its ballot there, and
        // stores it behind the loop.  One store per step from lane 0 cost the loop 1 % (DESIGN.md
        // section 18): its address is 64-bit vector arithmetic.  A step without a candidate costs the
        // loop one scalar add.
        static_assert(kScanDevMaxGroup / kBlockThreads <= 64, "a wave's steps fit its lanes");
        uint32_t w_lo = 0u, w_hi = 0u, step = 0u;
        batch_window_steps<W0>(r, lo, hi, [&](uint64_t, uint64_t, bool act, const uint32_t st[4]) {
            batch_hit_ballot(act, st, r.dmask, r.ntz, [&](unsigned long long m, bool) {
                // The step's word of the bitmap (m and step are wave-uniform: scalar operands of one
                // compare and two selects).
                const bool keeper = lane == step;
                w_lo = keeper ? (uint32_t)m : w_lo;
                w_hi = keeper ? (uint32_t)(m >> 32) : w_hi;
            });
            ++step;
        });
        // The steps this wave ran: those whose first index lo + 64 wave + 256 s is below hi.  Step s's
        // word is (lo - i_begin) / 64 + 4 s + wave, below the slice's ceil((i_end - i_begin) / 64)
        // because hi <= i_end.  Every one of them is stored, hit or no hit.
        const uint64_t first = lo + (threadIdx.x & ~63u);
        const uint32_t steps = first < hi ? (uint32_t)((hi - first + (kBlockThreads - 1)) / kBlockThreads) : 0u;
        if (lane < steps)
            mask[((lo - i_begin) >> 6) + 4u * lane + (threadIdx.x >> 6)] = ((unsigned long long)w_hi << 32) | w_lo;
        // The wave's hits: the bits of its words (the lanes past its steps hold zero).
        uint32_t n = (uint32_t)__popc(w_lo) + (uint32_t)__popc(w_hi);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d);
        *wave_hits = n;
    }
};

// Inclusive scan over a wave's lanes.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

constexpr uint32_t kScanPrefixPer = 8;  // totals per thread and round of the last workgroup's prefix (even)

// The workgroup's total, its retirement, and the prefix by the workgroup whose count completes the
// launch (the header comment has the ordering argument).
__device__ __forceinline__ void scan_mask_retire(const ScanMaskLaunch &S, uint32_t wave_hits, uint32_t *s_wave,
                                                 uint32_t &s_last) {
    const BatchLaunch &L = S.L;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) s_wave[wave] = wave_hits;
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_store(S.totals + blockIdx.x, s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    if (!launch_count_retired<true>(L, s_last)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // A round takes 2048 totals, 8 consecutive ones per thread as four 8-byte loads in flight
    // together: 8 rounds for 16384 workgroups, where one total per thread and round was 64 rounds of
    // one load's latency each.  A pair that starts
    // below n_blocks is loaded and stored whole: the arrays hold kScanDevMaxBlocks entries, and
    // nobody reads entry n_blocks.
    const unsigned long long *const totals2 = reinterpret_cast<const unsigned long long *>(S.totals);
    unsigned long long *const prefix2 = reinterpret_cast<unsigned long long *>(S.prefix);
    uint32_t carry = 0u;
    for (uint32_t q0 = 0u; q0 < L.n_blocks; q0 += kScanPrefixPer * kBlockThreads) {  // (workgroup-uniform trip count)
        const uint32_t q = q0 + kScanPrefixPer * threadIdx.x;
        uint32_t v[kScanPrefixPer];
#pragma unroll
        for (uint32_t j = 0u; j < kScanPrefixPer; j += 2u) {
            const unsigned long long x =
                q + j < L.n_blocks ? __hip_atomic_load(totals2 + ((q + j) >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                   : 0ull;
            v[j] = (uint32_t)x;
            v[j + 1u] = q + j + 1u < L.n_blocks ? (uint32_t)(x >> 32) : 0u;
        }
#pragma unroll
        for (uint32_t j = 1u; j < kScanPrefixPer; ++j) v[j] += v[j - 1u];
        const uint32_t incl = wave_inclusive_scan(v[kScanPrefixPer - 1u], lane);
        __syncthreads();  // the previous round's (and the totals') readers of s_wave are done
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t below = carry + (incl - v[kScanPrefixPer - 1u]);
        for (uint32_t w = 0u; w < wave; ++w) below += s_wave[w];
        carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
#pragma unroll
        for (uint32_t j = 0u; j < kScanPrefixPer; j += 2u) {
            if (q + j < L.n_blocks) {
                const unsigned long long pair = ((unsigned long long)(below + v[j + 1u]) << 32) | (below + v[j]);
                prefix2[(q + j) >> 1] = pair;  // (plain: read by the place launch, or copied out by the host)
            }
        }
    }
    // The host wants the slice's total after every launch and the prefix only for a slice that does
    // not fit the caller's room, so the total alone goes to pinned memory (the prefix as 64 KB of
    // 4-byte stores over the host link was the larger part of this tail: DESIGN.md section 18).
    if (threadIdx.x == 0)
        __hip_atomic_store(S.out_total, (unsigned long long)carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // (No launch_copies_performed: the prefix stores need no order here, their readers are behind the
    // kernel boundary.  The total and the record are lane 0's own, the record's store a system-scope
    // release.)
    launch_write_record(L);
}

__global__ void __launch_bounds__(kBlockThreads) scan_mask_kernel(const ScanMaskLaunch S) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_last;
    launch_start_tick(S.L);
    uint32_t wave_hits = 0u;
    uint64_t lo, hi;
    if (batch_block_range(S.i_begin, S.i_end, blockIdx.x, S.L.group, lo, hi)) {
        const ScanMaskGroup g{&S.task, S.mask, S.i_begin, lo, hi, &wave_hits};
        batch_with_w0(__builtin_amdgcn_readfirstlane(S.task.p >> 2), g);
    }
    scan_mask_retire(S, wave_hits, s_wave, s_last);
}

__global__ void __launch_bounds__(kBlockThreads) scan_place_kernel(const ScanPlaceLaunch P) {
    __shared__ uint32_t s_wave[4];
    uint64_t lo, hi;
    if (!batch_block_range(P.i_begin, P.i_end, blockIdx.x, P.group, lo, hi)) return;  // (workgroup-uniform)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_words = (uint32_t)((hi - lo + 63u) >> 6);  // <= group / 64 <= 256: this range's own words
    const unsigned long long word = threadIdx.x < n_words ? P.mask[((lo - P.i_begin) >> 6) + threadIdx.x] : 0ull;
    const uint32_t incl = wave_inclusive_scan((uint32_t)__popcll(word), lane);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint64_t at = P.base + (blockIdx.x ? P.prefix[blockIdx.x - 1u] : 0u);
    for (uint32_t w = 0u; w < wave; ++w) at += s_wave[w];
    const uint32_t excl = incl - (uint32_t)__popcll(word);
    const uint64_t i_wave = lo + ((uint64_t)wave << 12);  // the local index of this wave's word 0, bit 0
    const unsigned long long below = (1ull << lane) - 1ull;
    for (unsigned long long nz = __ballot(word != 0ull); nz != 0ull; nz &= nz - 1ull) {  // (wave-uniform)
        const uint32_t j = (uint32_t)__builtin_ctzll(nz);
        const unsigned long long m =
            ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(word >> 32), (int)j) << 32) |
            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)word, (int)j);
        const uint64_t to = at + (uint32_t)__builtin_amdgcn_readlane((int)excl, (int)j) + (uint32_t)__popcll(m & below);
        if (((m >> lane) & 1ull) != 0ull && to < P.max_hits)
            P.out[to] = (unsigned long long)global_of_local(i_wave + ((uint64_t)j << 6) + lane, P.rbits, P.base_tb);
    }
}

constexpr uint32_t kScanCheckMaxBlocks = 2048;

__global__ void __launch_bounds__(kBlockThreads) scan_check_kernel(const ScanCheckLaunch C) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * kBlockThreads;
    const uint64_t rounds = (C.n + stride - 1u) / stride;  // (uniform: every lane runs every ballot)
    uint32_t n_bad = 0u;                                   // wave-uniform
    uint64_t j = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    for (uint64_t r = 0u; r < rounds; ++r, j += stride) {
        const bool act = j < C.n;
        const bool shallow = act && C.tz != nullptr && C.tz[j] < C.ntz;
        const bool unordered = act && j > 0u && C.idx[j] <= C.idx[j - 1u];
        n_bad += (uint32_t)__popcll(__ballot(shallow)) + (uint32_t)__popcll(__ballot(unordered));
    }
    if (n_bad != 0u && lane == 0u) __hip_atomic_fetch_add(C.bad, n_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x == 0 && threadIdx.x < kScanDevSamples) {
        const uint64_t q = (C.n - 1u) / (kScanDevSamples - 1u) * threadIdx.x +
                           (C.n - 1u) % (kScanDevSamples - 1u) * threadIdx.x / (kScanDevSamples - 1u);
        // (= (n - 1) * threadIdx.x / 15 without the product's overflow; the host reads the samples
        // after the stream has drained)
        C.samples[threadIdx.x].idx = C.idx[q];
        C.samples[threadIdx.x].tz = C.tz != nullptr ? C.tz[q] : 0u;
    }
}

}  // namespace

hipError_t scan_dev_prepare() {
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(scan_mask_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(scan_place_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(scan_check_kernel));
    return e;
}

hipError_t scan_mask_launch(const ScanMaskLaunch &S, hipStream_t stream) {
    hipLaunchKernelGGL(scan_mask_kernel, dim3(S.L.n_blocks), dim3(kBlockThreads), 0, stream, S);
    return hipGetLastError();
}

hipError_t scan_place_launch(const ScanPlaceLaunch &P, hipStream_t stream) {
    hipLaunchKernelGGL(scan_place_kernel, dim3(P.n_blocks), dim3(kBlockThreads), 0, stream, P);
    return hipGetLastError();
}

hipError_t scan_check_launch(const ScanCheckLaunch &C, hipStream_t stream) {
    const uint64_t want = (C.n + kBlockThreads - 1u) / kBlockThreads;
    const uint32_t n_blocks = (uint32_t)(want < kScanCheckMaxBlocks ? want : kScanCheckMaxBlocks);
    hipLaunchKernelGGL(scan_check_kernel, dim3(n_blocks), dim3(kBlockThreads), 0, stream, C);
    return hipGetLastError();
}

}  // namespace dpow
