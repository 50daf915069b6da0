// md5_digest.hip -- the generic kernel of the digests (dpow_digests, digests.cpp): the MD5 and the
// depth of every entry of a list of global indices of one nonce.
//
// One launch hashes D.n entries.  Workgroup b takes the b-th group of D.group entries, one entry per
// lane and 256 per step.  The task row is a kernel argument, so its fields are wave-uniform scalar
// loads; row and hash are the shared ones (md5_batch_dev.h).  What differs from the window kernels
// is that the lanes of a wave hold unrelated candidates: the chunk length, and for p >= 48 the block
// count, vary per lane, which the shared assembly already derives from the lane's own k.
//
// Each lane loads its own 8-byte index (a wave's 64 loads are one contiguous 512 bytes), range-
// checks it, hashes, and stores the four state words as one 16-byte store and the depth as a byte.
// Lanes past D.n load and store nothing; an entry with k >= DPOW_K_LIMIT gets a zero digest and the
// depth byte 0xFF and is counted; a null output is a wave-uniform skip.
//
// Visibility.  Outputs are plain stores, read by nobody within the launch: they are visible at the
// kernel boundary, and the host waits for the stream (an event) before it reads them.  There is no
// in-kernel hand-off, hence no retirement count and no completion record.  The only cross-workgroup
// state is the out-of-range count: one relaxed agent-scope add per wave that has such a lane, read
// by the host after the stream has drained.
//
// No wave waits for another wave or for the host: the grid is bounded and a workgroup's work is
// fixed at its start.
#include <hip/hip_runtime.h>

#include "md5_batch_dev.h"
#include "md5_digest.h"

namespace dpow {

namespace {

constexpr unsigned long long kDigestKLimit = (1ull << 55) - 1ull;  // = DPOW_K_LIMIT (include/dpow.h)

// One workgroup's entries [lo, hi) of the list, with p / 4 a compile-time constant (md5_batch.h
// batch_with_w0): 256 entries per step, one per lane.
struct DigestGroup {
    const BatchTask *t;
    const unsigned long long *idx;
    uint4 *digest;
    uint8_t *tz;
    uint32_t *bad;
    uint32_t lo, hi;

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        const BatchRow r = batch_load_row(t);
        const uint32_t lane = threadIdx.x & 63u;
        for (uint32_t e0 = lo + (threadIdx.x & ~63u); e0 < hi; e0 += kBlockThreads) {  // e0: the wave's first entry
            const uint32_t e = e0 + lane;
            const bool act = e < hi;
            const unsigned long long g = act ? idx[e] : 0ull;
            const bool out_of_range = (g >> 8) >= kDigestKLimit;  // (never for a lane past the list)
            uint32_t st[4];
            batch_hash_at<W0>(r, out_of_range ? 0ull : g, st);
            uint32_t depth = trailing_zero_nibbles(st[0], st[1], st[2], st[3]);
            if (out_of_range) {
                st[0] = st[1] = st[2] = st[3] = 0u;
                depth = kDigestBadDepth;
            }
            if (digest != nullptr && act) digest[e] = make_uint4(st[0], st[1], st[2], st[3]);
            if (tz != nullptr && act) tz[e] = (uint8_t)depth;
            const unsigned long long m = __ballot(out_of_range);
            if (m != 0ull && lane == (uint32_t)(__ffsll((long long)m) - 1))
                __hip_atomic_fetch_add(bad, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};

__global__ void __launch_bounds__(kBlockThreads) digest_kernel(const DigestLaunch D) {
    const uint64_t lo = (uint64_t)blockIdx.x * D.group;
    if (lo >= D.n) return;  // (workgroup-uniform)
    const uint32_t hi = D.n - (uint32_t)lo > D.group ? (uint32_t)lo + D.group : D.n;
    const DigestGroup g{&D.task, D.idx, D.digest, D.tz, D.bad, (uint32_t)lo, hi};
    batch_with_w0(__builtin_amdgcn_readfirstlane(D.task.p >> 2), g);
}

}  // namespace

hipError_t digest_prepare() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(digest_kernel));
}

hipError_t digest_launch(const DigestLaunch &D, uint32_t n_blocks, hipStream_t stream) {
    hipLaunchKernelGGL(digest_kernel, dim3(n_blocks), dim3(kBlockThreads), 0, stream, D);
    return hipGetLastError();
}

}  // namespace dpow
