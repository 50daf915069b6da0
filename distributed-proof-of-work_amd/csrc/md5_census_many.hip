// md5_census_many.hip -- the generic kernel of the batched census (dpow_census_batch,
// census_many.cpp): the census of many tasks in one launch.
//
// One launch hashes a slice of the local index ranges of the call's next tasks, one descriptor per
// workgroup (md5_batch.hip queue_kernel's shape, BatchEntry's layout): workgroup b hashes
// [i_begin, i_end) -- at most kBatchMaxGroup local indices -- of the task in table slot
// blocks[b].task.  The task's fields are wave-uniform and come from the device task table with
// scalar loads; the workgroup branches once on its task's wave-uniform p / 4 and runs the census's
// depth sink (md5_census.h CensusGroup, the source census_kernel runs): depths below kCensusRare in
// wave registers by ballot and popcount, the rest in the workgroup's LDS table, lanes past `hi`
// hashing the clamped index and counted nowhere.
//
// The tables.  Device memory holds one table per task slot, cnt[33] then first[33], 8 bytes a word,
// counts 0 and firsts kNoHit whenever no launch is in flight.  A workgroup's flush is
// census_kernel's (md5_census.h census_flush) into the table of its descriptor's slot: at most one
// agent-scope add and one guarded agent-scope atomicMin per depth with a non-zero count.  The
// workgroups of one task, and of different tasks, meet nowhere else.
//
// Retirement (md5_batch_dev.h): the table words are only ever touched by 8-byte agent-scope
// atomics, drained before the count.  The last workgroup copies the tables of the launch's
// live-slot list to pinned memory -- entry q is the table of slot out_slots[q], as queue_kernel
// copies its best values -- re-initialises those tables and writes the completion record.
#include <hip/hip_runtime.h>

#include "md5_census_many.h"

namespace dpow {

namespace {

// The copy-out of n_live tables by all four waves of the last workgroup.  Word w of the copy is
// word w % kCensusTableWords of the table of slot out_slots[w / kCensusTableWords].  A lane's
// kCopyUnroll slot loads are issued first, then its kCopyUnroll table loads, then the stores, so
// that it waits for the slot list, too, once per kCopyUnroll words.
__device__ __forceinline__ void census_many_retire(const BatchLaunch &L, const uint32_t *__restrict__ out_slots,
                                                   uint32_t &s_last) {
    if (!launch_count_retired<true>(L, s_last)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const uint32_t n_words = L.n_live * kCensusTableWords;  // <= DPOW_BATCH_MAX * 66
    for (uint32_t w0 = threadIdx.x; w0 < n_words; w0 += kCopyUnroll * kBlockThreads) {
        uint32_t off[kCopyUnroll];  // the word's place in the tables; bit 31: a first, not a count
        unsigned long long v[kCopyUnroll];
        // The loads are not predicated: a lane past the end loads the last word again (n_words > 0
        // here) and stores nothing.  The slots first: a table load waits for its slot alone.
#pragma unroll
        for (uint32_t u = 0; u < kCopyUnroll; ++u) {
            const uint32_t w = w0 + u * kBlockThreads < n_words ? w0 + u * kBlockThreads : n_words - 1u;
            off[u] = out_slots[w / kCensusTableWords];
        }
#pragma unroll
        for (uint32_t u = 0; u < kCopyUnroll; ++u) {
            const uint32_t w = w0 + u * kBlockThreads < n_words ? w0 + u * kBlockThreads : n_words - 1u;
            const uint32_t c = w % kCensusTableWords;
            off[u] = off[u] * kCensusTableWords + c;  // < DPOW_BATCH_MAX * 66
            v[u] = __hip_atomic_load(L.best + off[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            off[u] |= c < kCensusDepths ? 0u : 0x80000000u;
        }
#pragma unroll
        for (uint32_t u = 0; u < kCopyUnroll; ++u) {
            const uint32_t w = w0 + u * kBlockThreads;
            if (w < n_words) {
                __hip_atomic_store(L.out_best + w, v[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                // the table as the next launch expects it: counts 0, firsts none
                __hip_atomic_store(L.best + (off[u] & 0x7FFFFFFFu), (off[u] >> 31) != 0u ? kNoHit : 0ull,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    launch_copies_performed();
    launch_write_record(L);
}

__global__ void __launch_bounds__(kBlockThreads)
    census_many_kernel(const BatchTask *__restrict__ tasks, const BatchEntry *__restrict__ blocks,
                       const uint32_t *__restrict__ out_slots, const BatchLaunch L) {
    __shared__ uint32_t s_cnt[kCensusDepths], s_first[kCensusDepths], s_last;
    launch_start_tick(L);
    if (threadIdx.x < kCensusDepths) {
        s_cnt[threadIdx.x] = 0u;
        s_first[threadIdx.x] = kNoOff;
    }
    __syncthreads();
    const BatchEntry *const e = blocks + blockIdx.x;
    const uint64_t lo = e->i_begin, hi = e->i_end;
    const uint32_t ti = e->task;  // < DPOW_BATCH_MAX (census_many.cpp)
    const BatchTask *const t = tasks + ti;
    const bool work = lo < hi;  // (workgroup-uniform)
    if (work) {
        const CensusGroup g{t, s_cnt, s_first, lo, hi};
        batch_with_w0(__builtin_amdgcn_readfirstlane(t->p >> 2), g);
    }
    __syncthreads();  // the table is complete
    census_flush(work, lo, s_cnt, s_first, t->rbits, t->base_tb, L.best + (size_t)ti * kCensusTableWords);
    census_many_retire(L, out_slots, s_last);
}

}  // namespace

hipError_t census_many_prepare() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(census_many_kernel));
}

hipError_t census_many_launch(const BatchTask *tasks, const BatchEntry *blocks, const uint32_t *out_slots,
                              const BatchLaunch &L, hipStream_t stream) {
    hipLaunchKernelGGL(census_many_kernel, dim3(L.n_blocks), dim3(kBlockThreads), 0, stream, tasks, blocks, out_slots,
                       L);
    return hipGetLastError();
}

}  // namespace dpow
