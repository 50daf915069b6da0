// md5_batch.hip -- the generic kernel of the batched search (dpow_search_batch, batch.cpp) and,
// further down, its second entry point for the task queue (queue_kernel, queue.cpp).
//
// One launch hashes a slice of every live task's window.  Workgroup b takes row b / n_live of
// live entry b % n_live (chunk-major: a task's early indices are dispatched first), one candidate
// per lane and 256 per step, in increasing index order.  The task's fields are wave-uniform and
// come from the task table with scalar loads; the message layout is data (md5_batch.h
// batch_candidate_words), so k = 0, every chunk-length boundary and both block counts go through
// the same code; a workgroup branches once on its task's wave-uniform p / 4, so that the word
// positions of the variable bytes are compile-time constants inside the hash.  A wave hashes the
// second final block when any of its lanes needs it.
//
// Exactness: a hit goes to the task's best with atomicMin on the global index, which is monotone
// in the local index.  A workgroup stops at the first step whose lowest global index is at or
// above the task's current best; best only ever holds the task's bound or a hit, so no candidate
// below the final best is skipped.
//
// Retirement (md5_batch_dev.h): the only cross-workgroup state besides the tasks' best words is the
// retirement count, whose last increment copies the live tasks' best values and the completion
// record to pinned memory (retire_workgroup, the one tail of both entry points).
#include <hip/hip_runtime.h>

#include "md5_batch_dev.h"

namespace dpow {

namespace {

// One workgroup's range [lo, hi) of one task, with p / 4 a compile-time constant.
struct BatchGroup {
    const BatchTask *t;
    unsigned long long *bp;  // the task's best
    uint64_t lo, hi;

    template <int W0>
    __device__ __forceinline__ void operator()() const {
        const BatchRow r = batch_load_row(t);
        const uint32_t lane = threadIdx.x & 63u;
        // The task's best is read one step ahead (the load is in flight while the step hashes); a
        // value one step old only delays the early exit, it skips nothing.
        unsigned long long best = __hip_atomic_load(bp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (Its own loop header, not batch_window_steps: the early exit in front of the hash is part
        // of the exactness argument above, and through the shared loop with a pre-step predicate
        // queue_kernel's rate measured below the parent's)
        for (uint64_t i0 = lo + (threadIdx.x & ~63u); i0 < hi; i0 += kBlockThreads) {  // i0: the wave's first index
            if (global_of_local(i0, r.rbits, r.base_tb) >= best) break;
            best = __hip_atomic_load(bp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint64_t i = i0 + lane;
            const bool act = i < hi;
            if (!act) i = hi - 1;
            uint32_t st[4];
            batch_hash_at<W0>(r, i, st);
            batch_hit_ballot(act, st, r.dmask, r.ntz, [&](unsigned long long m, bool) {
                if (m != 0ull && lane == (uint32_t)(__ffsll((long long)m) - 1)) {
                    // The returned value is consumed, so the wave waits for the atomic: it is
                    // performed before the workgroup's retirement count (below).
                    const unsigned long long prev =
                        __hip_atomic_fetch_min(bp, (unsigned long long)global_of_local(i, r.rbits, r.base_tb),
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("; dpow batch: atomicMin performed (%0)" ::"v"(prev));
                }
            });
        }
    }
};

// Retirement.  Each wave's atomicMin has been performed already (the hit path consumes the
// returning atomic's result), so the count needs no drain.  The last workgroup copies the live
// tasks' best values out -- out_best[q] = best of table slot slot_of(q) -- and writes the
// completion record, from one wave: the wave's own release fence orders its copies before its lane
// 0's record, without a second barrier.
template <typename SlotOf>
__device__ __forceinline__ void retire_workgroup(const BatchLaunch &L, uint32_t &s_last, SlotOf slot_of) {
    if (launch_count_retired<false>(L, s_last) && threadIdx.x < 64u) {
        for (uint32_t q = threadIdx.x; q < L.n_live; q += 64u) {
            const unsigned long long b =
                __hip_atomic_load(L.best + slot_of(q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(L.out_best + q, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // the wave's stores before its lane 0's record
        launch_write_record(L);
    }
}

__global__ void __launch_bounds__(kBlockThreads)
    batch_kernel(const BatchTask *__restrict__ tasks, const BatchEntry *__restrict__ map, const BatchLaunch L) {
    __shared__ uint32_t s_last;
    launch_start_tick(L);
    const uint32_t row = blockIdx.x / L.n_live;
    const uint32_t j = blockIdx.x - row * L.n_live;
    const BatchEntry *const e = map + j;
    uint64_t lo, hi;
    if (batch_block_range(e->i_begin, e->i_end, row, L.group, lo, hi)) {
        const uint32_t ti = e->task;
        const BatchGroup g{tasks + ti, L.best + ti, lo, hi};
        batch_with_w0(__builtin_amdgcn_readfirstlane(g.t->p >> 2), g);
    }
    retire_workgroup(L, s_last, [map](uint32_t q) { return map[q].task; });
}

// The upload image, pinned host memory to device memory (batch_upload).
__global__ void __launch_bounds__(kBlockThreads)
    batch_upload_kernel(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint32_t n_words) {
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += gridDim.x * blockDim.x) dst[w] = src[w];
}

// The task queue's launch (queue.cpp): one descriptor per workgroup.  The live tasks of a queue
// have different ages, so their slices differ by orders of magnitude and a (row, entry) grid would
// be mostly empty; here workgroup b hashes [i_begin, i_end) (at most kBatchMaxGroup local indices)
// of the task in table slot blocks[b].task, through the same BatchGroup as batch_kernel.  The
// descriptors are read with one scalar load per workgroup: from pinned memory where the table is
// short, as batch_kernel reads its map, else from the device copy the upload kernel made
// (queue.h kQueueCopyBlocks).  Retirement as in batch_kernel; the last workgroup copies out the best values of
// the launch's live-slot list out_slots[0..L.n_live), which is not the block list.
__global__ void __launch_bounds__(kBlockThreads)
    queue_kernel(const BatchTask *__restrict__ tasks, const BatchEntry *__restrict__ blocks,
                 const uint32_t *__restrict__ out_slots, const BatchLaunch L) {
    __shared__ uint32_t s_last;
    launch_start_tick(L);
    const BatchEntry *const e = blocks + blockIdx.x;
    const uint64_t lo = e->i_begin, hi = e->i_end;
    if (lo < hi) {
        const uint32_t ti = e->task;
        const BatchGroup g{tasks + ti, L.best + ti, lo, hi};
        batch_with_w0(__builtin_amdgcn_readfirstlane(g.t->p >> 2), g);
    }
    retire_workgroup(L, s_last, [out_slots](uint32_t q) { return out_slots[q]; });
}

// The rows of the task table that changed since the queue's last launch (newly filled slots), from
// pinned host memory to their slots: the task row and the slot's best.  In stream order before the
// launch that reads them and after the launch that last used the slot.
__global__ void __launch_bounds__(kBlockThreads)
    queue_upload_kernel(uint32_t *__restrict__ tasks, uint32_t *__restrict__ best, const QueueRow *__restrict__ rows,
                        uint32_t n_rows) {
    constexpr uint32_t kTaskWords = sizeof(BatchTask) / 4, kWords = kTaskWords + 2;
    const uint32_t n = n_rows * kWords;
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < n; w += gridDim.x * blockDim.x) {
        const uint32_t r = w / kWords, c = w - r * kWords;
        const uint32_t slot = rows[r].slot;
        const uint32_t v = reinterpret_cast<const uint32_t *>(rows + r)[c];  // the best follows the task row
        if (c < kTaskWords) tasks[slot * kTaskWords + c] = v;
        else best[slot * 2u + (c - kTaskWords)] = v;
    }
}

}  // namespace

hipError_t batch_prepare() {
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(batch_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(batch_upload_kernel));
    return e;
}

hipError_t queue_prepare() {
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(queue_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(queue_upload_kernel));
    return e;
}

hipError_t queue_upload(BatchTask *tasks, unsigned long long *best, const QueueRow *rows, uint32_t n_rows,
                        hipStream_t stream) {
    if (n_rows == 0u) return hipSuccess;
    const uint32_t words = n_rows * (uint32_t)(sizeof(BatchTask) / 4 + 2);
    const uint32_t blocks = (words + kBlockThreads - 1u) / kBlockThreads;
    hipLaunchKernelGGL(queue_upload_kernel, dim3(blocks), dim3(kBlockThreads), 0, stream,
                       reinterpret_cast<uint32_t *>(tasks), reinterpret_cast<uint32_t *>(best), rows, n_rows);
    return hipGetLastError();
}

hipError_t queue_launch(const BatchTask *tasks, const BatchEntry *blocks, const uint32_t *out_slots,
                        const BatchLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(queue_kernel, dim3(L.n_blocks), dim3(kBlockThreads), 0, stream, tasks, blocks, out_slots, L);
    return hipGetLastError();
}

hipError_t batch_upload(uint32_t *dst, const uint32_t *src, uint32_t n_words, hipStream_t stream) {
    const uint32_t blocks = (n_words + 4u * kBlockThreads - 1u) / (4u * kBlockThreads);
    hipLaunchKernelGGL(batch_upload_kernel, dim3(blocks ? blocks : 1u), dim3(kBlockThreads), 0, stream, dst, src,
                       n_words);
    return hipGetLastError();
}

hipError_t batch_launch(const BatchTask *tasks, const BatchEntry *map, const BatchLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(batch_kernel, dim3(L.n_blocks), dim3(kBlockThreads), 0, stream, tasks, map, L);
    return hipGetLastError();
}

}  // namespace dpow
