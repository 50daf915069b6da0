// md5_digest_many.hip -- the generic kernel of the digests of many nonces (dpow_digests_batch,
// dpow_digests_batch_device, digests_many.cpp): the MD5 and the depth of every entry of a list in
// CSR order over many tasks.
//
// One launch hashes D.n entries.  Workgroup b takes the b-th group of D.group entries, one entry per
// lane and 256 per step, as digest_kernel does (md5_digest.hip); row, hash and the branch on p / 4
// are the shared ones (md5_batch_dev.h).  What is new is where the task row comes from: entry e of
// the launch is position D.e_base + e of the list, and the rows say which task a position belongs
// to.
//
// One task.  A workgroup bisects the rows for the task of its first position; when its whole range
// lies in that task it runs digest_kernel's loop with the row loaded once.
//
// Seams.  Otherwise every wave-step walks the tasks that meet its 64 positions (md5_digest_many.h
// digest_many_walk): a bisection for the first, wave-uniform scalar code from the hint of the wave's
// last step, then forward.  Each non-empty overlap is one pass with that task's row in SGPRs and one
// batch_with_w0 branch on its p / 4; the lanes of other tasks hash index 0 and store nothing.  A
// list has at most n / 64 + n_tasks + (number of waves) passes, as a seam adds at most one pass to
// one wave; the price is the worst case, tasks of one entry: 64 passes per wave, every hash done 64
// times over.  There is no per-lane task row, no message word indexed at run
// time and no scratch.
//
// Outputs.  As digest_kernel's: an entry with k >= DPOW_K_LIMIT gets a zero digest and the depth
// byte 0xFF and is counted in D.ctl[0]; so does a position no pass covered (outside
// [rows[0], rows[n_tasks]) when the rows are valid), counted in D.ctl[1].  A pass adds its entries
// shallower than its task's ntz to the task's word of D.shallow.
//
// Visibility.  Outputs are plain stores, read by nobody within the launch; the counts are relaxed
// agent-scope adds, read by the host after the stream has drained.  No wave waits for another wave
// or for the host: the grid is bounded and a workgroup's work is fixed at its start.
//
// Garbage rows.  The rows are device memory the host never checked.  The walk reads
// rows[0 .. n_tasks] only, names no task >= n_tasks, keeps every pass within the wave's own
// positions and ends within n_tasks steps (md5_digest_many.h), so rows that descend cost wrong
// digests, never a store outside the launch's entries or a wave that does not end.
#include <hip/hip_runtime.h>

#include "md5_batch_dev.h"
#include "md5_digest_many.h"

namespace dpow {

namespace {

constexpr unsigned long long kDigestKLimit = (1ull << 55) - 1ull;  // = DPOW_K_LIMIT (include/dpow.h)

// A wave's add of the lanes in m (not empty) to a 32-bit count.
__device__ __forceinline__ void wave_count(uint32_t *word, unsigned long long m, uint32_t lane) {
    if (lane == (uint32_t)(__ffsll((long long)m) - 1))
        __hip_atomic_fetch_add(word, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup's entries [lo, hi) of the launch, all of task row t: digest_kernel's loop, and the
// wave's shallow entries in one add behind it.
struct DigestManyOneTask {
    const BatchTask *t;
    const DigestManyLaunch &D;
    unsigned long long *shallow;  // the task's word
    uint32_t lo, hi;

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        const BatchRow r = batch_load_row(t);
        const uint32_t lane = threadIdx.x & 63u;
        uint32_t n_shallow = 0u;  // (wave-uniform)
        for (uint32_t e0 = lo + (threadIdx.x & ~63u); e0 < hi; e0 += kBlockThreads) {  // e0: the wave's first entry
            const uint32_t e = e0 + lane;
            const bool act = e < hi;
            const unsigned long long g = act ? D.idx[e] : 0ull;
            const bool out_of_range = (g >> 8) >= kDigestKLimit;  // (never for a lane past the list)
            uint32_t st[4];
            batch_hash_at<W0>(r, out_of_range ? 0ull : g, st);
            uint32_t depth = trailing_zero_nibbles(st[0], st[1], st[2], st[3]);
            n_shallow += (uint32_t)__popcll(__ballot(act && !out_of_range && depth < r.ntz));
            if (out_of_range) {
                st[0] = st[1] = st[2] = st[3] = 0u;
                depth = kDigestBadDepth;
            }
            if (D.digest != nullptr && act) D.digest[e] = make_uint4(st[0], st[1], st[2], st[3]);
            if (D.tz != nullptr && act) D.tz[e] = (uint8_t)depth;
            const unsigned long long m = __ballot(out_of_range);
            if (m != 0ull) wave_count(D.ctl, m, lane);
        }
        if (n_shallow != 0u && lane == 0u)
            __hip_atomic_fetch_add(shallow, (unsigned long long)n_shallow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// One pass of a wave-step: the lanes in `mine` hold entries of task row t.
struct DigestManyPass {
    const BatchTask *t;
    const DigestManyLaunch &D;
    unsigned long long *shallow;  // the task's word
    uint32_t e;                   // the lane's entry of the launch
    unsigned long long g;         // its index, 0 where out of range
    bool mine, out_of_range;

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        const BatchRow r = batch_load_row(t);
        const uint32_t lane = threadIdx.x & 63u;
        uint32_t st[4];
        batch_hash_at<W0>(r, mine ? g : 0ull, st);  // (a lane of another task hashes index 0)
        uint32_t depth = trailing_zero_nibbles(st[0], st[1], st[2], st[3]);
        const unsigned long long m = __ballot(mine && !out_of_range && depth < r.ntz);
        if (out_of_range) {
            st[0] = st[1] = st[2] = st[3] = 0u;
            depth = kDigestBadDepth;
        }
        if (D.digest != nullptr && mine) D.digest[e] = make_uint4(st[0], st[1], st[2], st[3]);
        if (D.tz != nullptr && mine) D.tz[e] = (uint8_t)depth;
        if (m != 0ull && lane == (uint32_t)(__ffsll((long long)m) - 1))
            __hip_atomic_fetch_add(shallow, (unsigned long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__global__ void __launch_bounds__(kBlockThreads)
    digest_many_kernel(const BatchTask *__restrict__ tasks, const unsigned long long *__restrict__ rows,
                       const DigestManyLaunch D) {
    const uint64_t lo64 = (uint64_t)blockIdx.x * D.group;
    if (lo64 >= D.n) return;  // (workgroup-uniform)
    const uint32_t lo = (uint32_t)lo64;
    const uint32_t hi = D.n - lo > D.group ? lo + D.group : D.n;
    const uint32_t lane = threadIdx.x & 63u;

    // The workgroup's whole range in one task: digest_kernel's loop.
    const uint32_t t_first = digest_many_find(rows, D.n_tasks, 0u, D.e_base + lo);
    if (rows[t_first] <= D.e_base + lo && rows[t_first + 1u] >= D.e_base + hi) {
        const DigestManyOneTask one{tasks + t_first, D, D.shallow + t_first, lo, hi};
        batch_with_w0(__builtin_amdgcn_readfirstlane(tasks[t_first].p >> 2), one);
        return;
    }

    uint32_t hint = t_first;  // rows[hint] <= the wave's first position, or hint == 0
    for (uint32_t e0v = lo + (threadIdx.x & ~63u); e0v < hi; e0v += kBlockThreads) {
        // The wave's first entry and its hint are the same in every lane: scalar from here on (the
        // loop's exit test is per lane to the compiler, and with it whatever the loop carries).
        const uint32_t e0 = __builtin_amdgcn_readfirstlane(e0v);
        hint = __builtin_amdgcn_readfirstlane(hint);
        const uint32_t e = e0 + lane;
        const bool act = e < hi;
        const unsigned long long g = act ? D.idx[e] : 0ull;
        const bool out_of_range = (g >> 8) >= kDigestKLimit;
        const uint64_t pos = D.e_base + e;
        const uint64_t p_first = D.e_base + e0, p_end = D.e_base + (hi - e0 > 64u ? e0 + 64u : hi);
        bool covered = false;
        hint = digest_many_walk(rows, D.n_tasks, hint, p_first, p_end, [&](uint32_t t, uint64_t p_lo, uint64_t p_hi) {
            const bool mine = pos >= p_lo && pos < p_hi;  // (p_hi <= p_end: an active lane)
            covered = covered || mine;
            const DigestManyPass pass{tasks + t, D, D.shallow + t, e, out_of_range ? 0ull : g, mine, out_of_range};
            batch_with_w0(__builtin_amdgcn_readfirstlane(tasks[t].p >> 2), pass);
        });
        const unsigned long long bad = __ballot(out_of_range);
        if (bad != 0ull) wave_count(D.ctl, bad, lane);
        const bool bare = act && !covered;
        const unsigned long long none = __ballot(bare);
        if (none != 0ull) {
            if (D.digest != nullptr && bare) D.digest[e] = make_uint4(0u, 0u, 0u, 0u);
            if (D.tz != nullptr && bare) D.tz[e] = kDigestBadDepth;
            wave_count(D.ctl + 1, none, lane);
        }
    }
}

}  // namespace

hipError_t digest_many_prepare() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(digest_many_kernel));
}

hipError_t digest_many_launch(const BatchTask *tasks, const DigestManyLaunch &D, uint32_t n_blocks, hipStream_t stream) {
    hipLaunchKernelGGL(digest_many_kernel, dim3(n_blocks), dim3(kBlockThreads), 0, stream, tasks, D.rows, D);
    return hipGetLastError();
}

}  // namespace dpow
