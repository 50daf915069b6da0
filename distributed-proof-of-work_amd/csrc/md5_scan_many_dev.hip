// md5_scan_many_dev.hip -- the kernels of the batched device scan (dpow_scan_batch_device,
// scan_many_dev.cpp): the hit bitmap and per-descriptor hit totals of one launch of many tasks
// (scan_many_mask_kernel), the ordered list from bitmap and prefix (scan_many_place_kernel), the
// tasks' row pointers and the call's samples (scan_many_rows_kernel), and the re-check and the
// depths of the entries placed (scan_many_depth_kernel).
//
// scan_many_mask_kernel.  The geometry is scan_many_kernel's (md5_scan_many.hip): workgroup b
// hashes the descriptor blocks[b] -- [i_begin, i_end), at most kBatchMaxGroup local indices, of the
// task in table slot blocks[b].task -- and the task's fields come from the device task table; row,
// hash, step loop and hit test are the shared ones (md5_batch_dev.h).  The sink is
// scan_mask_kernel's (md5_scan_dev.hip): a wave's lanes hold 64 consecutive local indices and a
// wave's first index is a multiple of 64 from the descriptor's begin, so its hit ballot is a word of
// the descriptor's bitmap; step s's ballot is gathered into lane s and the lanes store their words
// behind the loop, hit or no hit.  The descriptor's words live in slot b of the bitmap
// (md5_scan_many_dev.h), word 4 s + wave for the indices from i_begin + 64 (4 s + wave), so no
// descriptor needs to know what the others hold.  The bitmap is never zeroed: every word of every
// step run is written, and nothing reads beyond a descriptor's own ceil(len / 64) words.  The stores
// are plain: their reader is a later launch.
//
// Retirement (md5_batch_dev.h): one lane publishes the workgroup's hit total with a 4-byte relaxed
// agent-scope atomic store, drained before the count.  The last workgroup, behind an acquire fence,
// reads the totals and writes their inclusive prefix -- at most kScanManyMaxBlocks = 20480
// descriptors, 10 rounds of 2048, uint32: a launch has at most 2^28 candidates -- to a device array
// for the launches behind it, and the launch's total alone to pinned memory; then the completion
// record.  As in scan_mask_kernel the total is lane 0's own store and the prefix is read behind the
// kernel boundary, so nothing has to be ordered before the record but lane 0's own stores.
//
// scan_many_place_kernel.  One workgroup per leading descriptor of the same launch: it loads its
// slot's ceil(len / 64) <= 256 words, one per thread, and prefix[b - 1] (plain loads: written by an
// earlier launch on the same stream), takes rbits and base_tb from its task's row, and lane l of a
// word with bit l set stores global_of_local(...) to out[base + rank], clamped to max_hits.
//
// scan_many_rows_kernel.  The tasks' row pointers, on the device: per launch of the plan the rows of
// the tasks whose first part lies in it (and of the empty tasks before them) from a host table of
// (row, first descriptor); behind the call's last launch the rows of the tasks not begun, the end
// row, and 16 samples of the list with their task for the host's MD5.
//
// scan_many_depth_kernel.  Workgroup b walks the entries [prefix[b - 1], prefix[b]) it finds in the
// list: an independent gather, as digest_kernel is for the device scan, but one launch for every
// task of the launch.  It counts into one device word the entries that are not candidates of its
// descriptor and those not strictly above their predecessor within the task, and -- when depths are
// asked for -- re-hashes each entry with its task's row through batch_hash_at, stores the depth byte
// and counts the entries shallower than the task's ntz.
//
// No wave waits for another wave or for the host: every grid is bounded, a workgroup's work is fixed
// at its start, and the only cross-workgroup state is the totals, the retirement count and the
// check word.
//
// wave_inclusive_scan and the prefix rounds are a second copy of md5_scan_dev.hip's (DESIGN.md
// section 20): that unit is pinned to its three kernels and its constants by the tests.
#include <hip/hip_runtime.h>

#include "md5_batch_dev.h"
#include "md5_scan_many_dev.h"

namespace dpow {

namespace {

// One workgroup's descriptor [lo, hi) of its task, with p / 4 a compile-time constant; `slot` is the
// descriptor's own kScanManyDevSlotWords words.
struct ScanManyMaskGroup {
    const BatchTask *t;
    unsigned long long *slot;
    uint64_t lo, hi;
    uint32_t *wave_hits;  // out: the hits of this wave's steps (wave-uniform)

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        const BatchRow r = batch_load_row(t);
        const uint32_t lane = threadIdx.x & 63u;
        // The wave's words, gathered: lane s holds the ballot of the wave's step s (at most 64 steps:
        // a descriptor is at most 64 x 256 indices), zero until a step with a hit puts its ballot there.
        static_assert(kBatchMaxGroup / kBlockThreads <= 64, "a wave's steps fit its lanes");
        uint32_t w_lo = 0u, w_hi = 0u, step = 0u;
        batch_window_steps<W0>(r, lo, hi, [&](uint64_t, uint64_t, bool act, const uint32_t st[4]) {
            batch_hit_ballot(act, st, r.dmask, r.ntz, [&](unsigned long long m, bool) {
                const bool keeper = lane == step;  // (m and step are wave-uniform)
                w_lo = keeper ? (uint32_t)m : w_lo;
                w_hi = keeper ? (uint32_t)(m >> 32) : w_hi;
            });
            ++step;
        });
        // The steps this wave ran: those whose first index lo + 64 wave + 256 s is below hi.  Step s's
        // word is 4 s + wave, below ceil((hi - lo) / 64) <= kScanManyDevSlotWords.  Every one is stored.
        const uint64_t first = lo + (threadIdx.x & ~63u);
        const uint32_t steps = first < hi ? (uint32_t)((hi - first + (kBlockThreads - 1)) / kBlockThreads) : 0u;
        if (lane < steps) slot[4u * lane + (threadIdx.x >> 6)] = ((unsigned long long)w_hi << 32) | w_lo;
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

constexpr uint32_t kScanManyPrefixPer = 8;  // totals per thread and round of the last workgroup's prefix (even)
static_assert(kScanManyMaxBlocks % 2u == 0u, "a pair that starts below n_blocks lies within the arrays");

// The workgroup's total, its retirement, and the prefix by the workgroup whose count completes the
// launch (the header comment has the ordering argument).
__device__ __forceinline__ void scan_many_mask_retire(const ScanManyMaskLaunch &S, uint32_t wave_hits,
                                                      uint32_t *s_wave, uint32_t &s_last) {
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
    // together: 10 rounds for 20480 descriptors.  A pair that starts below n_blocks is loaded and
    // stored whole: the arrays hold kScanManyMaxBlocks entries, and nobody reads entry n_blocks.
    const unsigned long long *const totals2 = reinterpret_cast<const unsigned long long *>(S.totals);
    unsigned long long *const prefix2 = reinterpret_cast<unsigned long long *>(S.prefix);
    uint32_t carry = 0u;
    for (uint32_t q0 = 0u; q0 < L.n_blocks; q0 += kScanManyPrefixPer * kBlockThreads) {  // (workgroup-uniform trip count)
        const uint32_t q = q0 + kScanManyPrefixPer * threadIdx.x;
        uint32_t v[kScanManyPrefixPer];
#pragma unroll
        for (uint32_t j = 0u; j < kScanManyPrefixPer; j += 2u) {
            const unsigned long long x =
                q + j < L.n_blocks ? __hip_atomic_load(totals2 + ((q + j) >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                   : 0ull;
            v[j] = (uint32_t)x;
            v[j + 1u] = q + j + 1u < L.n_blocks ? (uint32_t)(x >> 32) : 0u;
        }
#pragma unroll
        for (uint32_t j = 1u; j < kScanManyPrefixPer; ++j) v[j] += v[j - 1u];
        const uint32_t incl = wave_inclusive_scan(v[kScanManyPrefixPer - 1u], lane);
        __syncthreads();  // the previous round's (and the totals') readers of s_wave are done
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t below = carry + (incl - v[kScanManyPrefixPer - 1u]);
        for (uint32_t w = 0u; w < wave; ++w) below += s_wave[w];
        carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
#pragma unroll
        for (uint32_t j = 0u; j < kScanManyPrefixPer; j += 2u) {
            if (q + j < L.n_blocks) {
                const unsigned long long pair = ((unsigned long long)(below + v[j + 1u]) << 32) | (below + v[j]);
                prefix2[(q + j) >> 1] = pair;  // (plain: read by the launches behind this one, or copied out by the host)
            }
        }
    }
    if (threadIdx.x == 0)
        __hip_atomic_store(S.out_total, (unsigned long long)carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // (No launch_copies_performed: the prefix stores need no order here, their readers are behind the
    // kernel boundary.  The total and the record are lane 0's own, the record's store a system-scope
    // release.)
    launch_write_record(L);
}

__global__ void __launch_bounds__(kBlockThreads)
    scan_many_mask_kernel(const BatchTask *__restrict__ tasks, const BatchEntry *__restrict__ blocks,
                          const ScanManyMaskLaunch S) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_last;
    launch_start_tick(S.L);
    const BatchEntry *const e = blocks + blockIdx.x;
    const uint64_t lo = e->i_begin, hi = e->i_end;  // hi - lo <= kBatchMaxGroup (scan_many_dev.cpp)
    const BatchTask *const t = tasks + e->task;     // < DPOW_BATCH_MAX (scan_many_dev.cpp)
    uint32_t wave_hits = 0u;
    if (lo < hi) {  // (workgroup-uniform)
        const ScanManyMaskGroup g{t, S.mask + (size_t)blockIdx.x * kScanManyDevSlotWords, lo, hi, &wave_hits};
        batch_with_w0(__builtin_amdgcn_readfirstlane(t->p >> 2), g);
    }
    scan_many_mask_retire(S, wave_hits, s_wave, s_last);
}

__global__ void __launch_bounds__(kBlockThreads)
    scan_many_place_kernel(const BatchTask *__restrict__ tasks, const BatchEntry *__restrict__ blocks,
                           const ScanManyPlaceLaunch P) {
    __shared__ uint32_t s_wave[4];
    const BatchEntry *const e = blocks + blockIdx.x;
    const uint64_t lo = e->i_begin, hi = e->i_end;
    if (lo >= hi) return;  // (workgroup-uniform)
    const BatchTask *const t = tasks + e->task;
    const uint32_t rbits = t->rbits, base_tb = t->base_tb;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t len = hi - lo < kBatchMaxGroup ? hi - lo : kBatchMaxGroup;
    const uint32_t n_words = (uint32_t)((len + 63u) >> 6);  // <= kScanManyDevSlotWords: this descriptor's own words
    const unsigned long long word =
        threadIdx.x < n_words ? P.mask[(size_t)blockIdx.x * kScanManyDevSlotWords + threadIdx.x] : 0ull;
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
            P.out[to] = (unsigned long long)global_of_local(i_wave + ((uint64_t)j << 6) + lane, rbits, base_tb);
    }
}

__global__ void __launch_bounds__(kBlockThreads) scan_many_rows_kernel(const ScanManyRowsLaunch R) {
    const uint32_t q = blockIdx.x * kBlockThreads + threadIdx.x;
    if (q < R.n_entries) {
        const ScanManyRowEntry e = R.table[q];
        R.rows[e.row] = R.base + (e.first_block ? R.prefix[e.first_block - 1u] : 0u);
    }
    if (q < R.fill_end - R.fill_begin) R.rows[R.fill_begin + q] = R.fill_value;
    // The host's copies, read after the stream has drained: every row (those below fill_begin are
    // earlier launches') and the check word, which goes back to zero for the next call.
    if (R.out_rows != nullptr && q < R.fill_end) R.out_rows[q] = q >= R.fill_begin ? R.fill_value : R.rows[q];
    if (R.out_bad != nullptr && q == 0u) {
        *R.out_bad = __hip_atomic_load(R.bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(R.bad, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (R.n != 0u && blockIdx.x == 0 && threadIdx.x < kScanManyDevSamples) {
        const uint64_t at = (R.n - 1u) / (kScanManyDevSamples - 1u) * threadIdx.x +
                            (R.n - 1u) % (kScanManyDevSamples - 1u) * threadIdx.x / (kScanManyDevSamples - 1u);
        // (= (n - 1) * threadIdx.x / 15 without the product's overflow.)  The sample's task: the last
        // row below fill_begin that is at most `at` (rows[0] = 0 is; those rows are earlier launches').
        uint32_t a = 0u, b = R.fill_begin;  // rows[a] <= at, and rows[b] > at or b == fill_begin
        while (b - a > 1u) {
            const uint32_t mid = a + (b - a) / 2u;
            if (R.rows[mid] <= at) a = mid;
            else b = mid;
        }
        R.samples[threadIdx.x].idx = R.idx[at];
        R.samples[threadIdx.x].tz = R.tz != nullptr ? R.tz[at] : 0u;
        R.samples[threadIdx.x].task = a;
    }
}

// One workgroup's entries [e_lo, e_hi) of the list, all of descriptor [lo, hi) of task row t.
struct ScanManyDepthGroup {
    const BatchTask *t;
    const unsigned long long *idx;
    uint8_t *tz;
    uint64_t e_lo, e_hi, e_task;  // e_task: where the task's segment begins
    uint64_t lo, hi;
    uint32_t *n_bad;  // out, wave-uniform

    // The entry's local index under the task's partition; false when it is another partition's.
    static __device__ __forceinline__ bool local_of(unsigned long long g, uint32_t rbits, uint32_t base_tb, uint64_t &i) {
        const uint32_t tb = (uint32_t)(g & 255u);
        i = ((g >> 8) << rbits) | (tb & ((1u << rbits) - 1u));
        return (tb >> rbits) == (base_tb >> rbits);
    }

    template <bool Hash, int W0>
    __device__ __forceinline__ void run() const {
        const BatchRow r = batch_load_row(t);
        const uint32_t lane = threadIdx.x & 63u;
        uint32_t bad = 0u;
        for (uint64_t e0 = e_lo + (threadIdx.x & ~63u); e0 < e_hi; e0 += kBlockThreads) {  // e0: the wave's first entry
            const uint64_t e = e0 + lane;
            const bool act = e < e_hi;
            const unsigned long long g = act ? idx[e] : 0ull;
            uint64_t i;
            const bool mine = local_of(g, r.rbits, r.base_tb, i) && i >= lo && i < hi;
            const bool unordered = act && e > e_task && g <= idx[e - 1u];
            bad += (uint32_t)__popcll(__ballot(act && !mine)) + (uint32_t)__popcll(__ballot(unordered));
            if constexpr (Hash) {
                uint32_t st[4];
                batch_hash_at<W0>(r, mine ? i : lo, st);  // (a lane without an entry of this descriptor hashes lo)
                const uint32_t depth = trailing_zero_nibbles(st[0], st[1], st[2], st[3]);
                if (act) tz[e] = (uint8_t)depth;
                bad += (uint32_t)__popcll(__ballot(act && mine && depth < r.ntz));
            }
        }
        *n_bad = bad;
    }

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        run<true, W0>();
    }
};

__global__ void __launch_bounds__(kBlockThreads)
    scan_many_depth_kernel(const BatchTask *__restrict__ tasks, const BatchEntry *__restrict__ blocks,
                           const ScanManyDepthLaunch D) {
    const BatchEntry *const e = blocks + blockIdx.x;
    const uint64_t lo = e->i_begin, hi = e->i_end;
    uint64_t e_lo = D.base + (blockIdx.x ? D.prefix[blockIdx.x - 1u] : 0u), e_hi = D.base + D.prefix[blockIdx.x];
    if (e_hi > D.max_hits) e_hi = D.max_hits;
    if (lo >= hi || e_lo >= e_hi) return;  // (workgroup-uniform)
    const BatchTask *const t = tasks + e->task;
    uint32_t n_bad = 0u;
    const ScanManyDepthGroup g{t, D.idx, D.tz, e_lo, e_hi, D.rows[e->task], lo, hi, &n_bad};
    if (D.tz != nullptr) batch_with_w0(__builtin_amdgcn_readfirstlane(t->p >> 2), g);
    else g.run<false, 0>();  // the index-only form: no hash, hence no layout
    if (n_bad != 0u && (threadIdx.x & 63u) == 0u)
        __hip_atomic_fetch_add(D.bad, n_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

hipError_t scan_many_dev_prepare() {
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(scan_many_mask_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(scan_many_place_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(scan_many_rows_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(scan_many_depth_kernel));
    return e;
}

hipError_t scan_many_mask_launch(const BatchTask *tasks, const BatchEntry *blocks, const ScanManyMaskLaunch &S,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(scan_many_mask_kernel, dim3(S.L.n_blocks), dim3(kBlockThreads), 0, stream, tasks, blocks, S);
    return hipGetLastError();
}

hipError_t scan_many_place_launch(const BatchTask *tasks, const BatchEntry *blocks, const ScanManyPlaceLaunch &P,
                                  uint32_t n_blocks, hipStream_t stream) {
    hipLaunchKernelGGL(scan_many_place_kernel, dim3(n_blocks), dim3(kBlockThreads), 0, stream, tasks, blocks, P);
    return hipGetLastError();
}

hipError_t scan_many_rows_launch(const ScanManyRowsLaunch &R, hipStream_t stream) {
    const uint32_t fill = R.out_rows != nullptr ? R.fill_end : R.fill_end - R.fill_begin;
    const uint32_t want = R.n_entries > fill ? R.n_entries : fill;
    const uint32_t n_blocks = want ? (want + kBlockThreads - 1u) / kBlockThreads : 1u;
    hipLaunchKernelGGL(scan_many_rows_kernel, dim3(n_blocks), dim3(kBlockThreads), 0, stream, R);
    return hipGetLastError();
}

hipError_t scan_many_depth_launch(const BatchTask *tasks, const BatchEntry *blocks, const ScanManyDepthLaunch &D,
                                  uint32_t n_blocks, hipStream_t stream) {
    hipLaunchKernelGGL(scan_many_depth_kernel, dim3(n_blocks), dim3(kBlockThreads), 0, stream, tasks, blocks, D);
    return hipGetLastError();
}

}  // namespace dpow
