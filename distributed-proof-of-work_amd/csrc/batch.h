// batch.h -- host side of the batched search (batch.cpp), as dpow_api.cpp sees it, and the round
// schedule that the task queue's planner (queue.h) is built from.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"

namespace dpow {

// Round schedule of a batch (DESIGN.md "Batched search").  Round r hashes about
// kBatchFirst * 4^r candidates, at most kBatchCap, split evenly over the live tasks.
constexpr uint64_t kBatchFirst = 1ull << 20;  // ~5 us of hashing: one round trip's worth
constexpr uint64_t kBatchCap = 1ull << 28;    // 1-3 ms of hashing: the cancel flag's latency
constexpr uint64_t kBatchMinSlice = 256;      // one workgroup step
constexpr uint32_t kBatchBlocks = 4096;       // workgroups a launch aims for (16 per CU)
constexpr uint32_t kBatchMinGroup = 256, kBatchMaxGroup = 16384;  // local indices per workgroup

// What a batch hashes in all in round `step`; the task queue's budget of a task of that age.
uint64_t batch_budget(uint32_t step);
// Local indices per workgroup of a launch whose slices, as planned, sum to `total`.
uint32_t batch_group(uint64_t total);

struct BatchRound {
    uint64_t slice;  // local indices per live task
    uint32_t group;  // local indices per workgroup
    uint32_t rows;   // workgroups per live task
};
// The round's shape for n_live tasks whose longest remaining range is max_left local indices.
BatchRound batch_round(uint32_t round, size_t n_live, uint64_t max_left);

uint64_t pow2_floor(uint64_t x);  // 0 for 0
uint64_t pow2_ceil(uint64_t x);

// Device and pinned buffers of a context's batches: allocated on its first batch, freed with it.
struct BatchState;
void batch_free(BatchState *s);  // the context's device is current, its stream drained

// Argument errors of dpow_search_batch (decided before the device is touched): 0 or a negative code.
int batch_check(const dpow_batch_task *tasks, size_t n_tasks);

// The body of dpow_search_batch (the context checked, its device current).
int batch_run(BatchState **state, hipStream_t stream, const volatile uint32_t *cancel, dpow_batch_task *tasks,
              size_t n_tasks, dpow_batch_stats *stats);

}  // namespace dpow
