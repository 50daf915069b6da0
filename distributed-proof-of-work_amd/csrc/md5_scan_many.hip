// md5_scan_many.hip -- the generic kernel of the batched scan (dpow_scan_batch, scan_many.cpp):
// every hit of many tasks' windows in one launch.
//
// One launch hashes a slice of the local index ranges of the call's next tasks, one descriptor per
// workgroup (md5_batch.hip queue_kernel's shape, BatchEntry's layout): workgroup b hashes
// [i_begin, i_end) -- at most kBatchMaxGroup local indices -- of the task in table slot
// blocks[b].task.  The task's fields, its ntz and its prefilter mask among them, come from the
// device task table; row, hash, step loop and hit test are the shared ones (md5_batch_dev.h).
//
// The hit sink is scan_kernel's (md5_scan.hip, wave_append_place) with another entry: one 32-bit
// word, the workgroup's descriptor index above the candidate's offset in the descriptor's range
// (md5_scan_many.h).  One store publishes it whole, and the host rebuilds the task and the index
// from the launch's descriptors.  The count keeps counting past the capacity, so the host learns
// the true number and re-plans an overflowed launch with halved budgets.
//
// Retirement (md5_batch_dev.h): an entry is a 4-byte relaxed agent-scope atomic store, drained
// before the count.  The last workgroup copies min(count, capacity) entries to pinned memory, all
// four waves copying with kCopyUnroll words per lane in flight, then the count, re-zeroes the
// device count and writes the completion record.
#include <hip/hip_runtime.h>

#include "md5_batch_dev.h"
#include "md5_scan_many.h"

namespace dpow {

namespace {

// One workgroup's range [lo, hi) of its task, with p / 4 a compile-time constant.  `tag` is the
// workgroup's descriptor index, shifted to its place in an entry.
struct ScanManyGroup {
    const BatchTask *t;
    uint32_t *hits;  // the launch's device hit list
    uint32_t *count;
    uint32_t capacity, tag;
    uint64_t lo, hi;

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        const BatchRow r = batch_load_row(t);
        batch_window_steps<W0>(r, lo, hi, [&](uint64_t, uint64_t i, bool act, const uint32_t st[4]) {
            batch_hit_ballot(act, st, r.dmask, r.ntz, [&](unsigned long long m, bool ok) {
                if (m != 0ull) {
                    const uint32_t at = wave_append_place(m, count);
                    // (i - lo < kBatchMaxGroup: the descriptor's range is at most that long.)
                    if (ok && at < capacity)
                        __hip_atomic_store(hits + at, tag | (uint32_t)(i - lo), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                }
            });
        });
    }
};

__device__ __forceinline__ void scan_many_retire(const ScanManyLaunch &S, uint32_t &s_last) {
    const BatchLaunch &L = S.L;
    if (!launch_count_retired<true>(L, s_last)) return;
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
    launch_copies_performed();
    if (threadIdx.x == 0) {
        __hip_atomic_store(S.out_count, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(S.count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    launch_write_record(L);
}

__global__ void __launch_bounds__(kBlockThreads)
    scan_many_kernel(const BatchTask *__restrict__ tasks, const BatchEntry *__restrict__ blocks,
                     const ScanManyLaunch S) {
    __shared__ uint32_t s_last;
    launch_start_tick(S.L);
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
