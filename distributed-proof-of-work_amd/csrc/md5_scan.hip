// md5_scan.hip -- the generic kernel of the scan (dpow_scan, scan.cpp): every hit of a slice of one
// task's window, appended to a list.
//
// One launch hashes the local indices [i_begin, i_end) of one task.  Workgroup b takes the b-th
// group of L.group indices.  The task row is a kernel argument, so its fields are wave-uniform
// scalar loads; row, hash and hit test are the shared ones (md5_batch_dev.h), the step loop is
// written out here.
//
// The hit sink.  There is no early exit and no atomicMin.  Per step the first hit lane claims
// popcount(mask) places with one returning atomic add on the launch's count
// (wave_append_place), and every hit lane stores its global index to its place if that is below
// the capacity.  The count keeps counting past the capacity, so the host learns the true number
// and re-runs an overflowed slice in halves.
//
// Retirement (md5_batch_dev.h): an entry is an 8-byte relaxed agent-scope atomic store, drained
// before the count.  The last workgroup copies min(count, capacity) entries to pinned memory, then
// the count, re-zeroes the device count and writes the completion record.  Waves without hits pay
// the (empty) drain only.
#include <hip/hip_runtime.h>

#include "md5_batch_dev.h"
#include "md5_scan.h"

namespace dpow {

namespace {

// One workgroup's range [lo, hi) of the task, with p / 4 a compile-time constant.
struct ScanGroup {
    const BatchTask *t;
    unsigned long long *hits;  // the launch's device hit list
    uint32_t *count;
    uint32_t capacity;
    uint64_t lo, hi;

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        const BatchRow r = batch_load_row(t);
        // (Its own loop header: through batch_window_steps this kernel's no-hit rate measured 0.5 %
        // below the parent's)
        const uint32_t lane = threadIdx.x & 63u;
        for (uint64_t i0 = lo + (threadIdx.x & ~63u); i0 < hi; i0 += kBlockThreads) {  // i0: the wave's first index
            uint64_t i = i0 + lane;
            const bool act = i < hi;
            if (!act) i = hi - 1;
            uint32_t st[4];
            batch_hash_at<W0>(r, i, st);
            batch_hit_ballot(act, st, r.dmask, r.ntz, [&](unsigned long long m, bool ok) {
                if (m != 0ull) {
                    const uint32_t at = wave_append_place(m, count);
                    if (ok && at < capacity)
                        __hip_atomic_store(hits + at, (unsigned long long)global_of_local(i, r.rbits, r.base_tb),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            });
        }
    }
};

__device__ __forceinline__ void scan_retire(const ScanLaunch &S, uint32_t &s_last) {
    const BatchLaunch &L = S.L;
    if (!launch_count_retired<true>(L, s_last)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const uint32_t total = __hip_atomic_load(S.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t n = total < S.capacity ? total : S.capacity;
    for (uint32_t q = threadIdx.x; q < n; q += kBlockThreads) {
        const unsigned long long g = __hip_atomic_load(L.best + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(L.out_best + q, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    launch_copies_performed();
    if (threadIdx.x == 0) {
        __hip_atomic_store(S.out_count, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(S.count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    launch_write_record(L);
}

__global__ void __launch_bounds__(kBlockThreads) scan_kernel(const ScanLaunch S) {
    __shared__ uint32_t s_last;
    launch_start_tick(S.L);
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
