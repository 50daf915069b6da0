// queue.h -- the task queue's launch planner (queue.cpp), a pure host function.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "batch.h"

namespace dpow {

// A launch that holds tasks of different ages hashes at most kQueueSpread times the youngest
// task's budget (DESIGN.md "Task queue"): a fresh task beside old ones waits for 2^24 candidates
// at most, about 0.14 ms of the generic kernel.
constexpr uint64_t kQueueSpread = 16;
// Workgroup descriptors of one launch.  The slices of a launch sum to at most kBatchCap +
// DPOW_BATCH_MAX * kBatchMinSlice, cut into blocks of the launch's group: at most 8192 blocks
// while the group follows total / kBatchBlocks, at most 16448 once it is kBatchMaxGroup, and one
// partial block per task more.
constexpr uint32_t kQueueMaxBlocks = 32768;

// From this many descriptors on, a launch's table is copied to device memory first (one more small
// kernel on the stream) instead of being read from pinned memory by each workgroup: read in place,
// 16384 descriptors cost a 2^28-candidate launch about a third of its rate (82-92 against 122 GH/s,
// profiles/queue_rate.json), some 40-60 ns each; the copy costs a few microseconds, so it pays
// from a few hundred descriptors on.
constexpr uint32_t kQueueCopyBlocks = 256;

struct QueueBlock {
    uint32_t task;     // index into the planner's inputs
    uint32_t ordinal;  // of the block within its task's slice
    uint64_t lo, hi;   // relative to the task's current position
};

struct QueuePlan {
    uint64_t budget = 0;              // Bd
    uint32_t group = 0;               // local indices per workgroup
    std::vector<uint64_t> slice;      // per task
    std::vector<uint32_t> rows;       // per task: its block count
    std::vector<QueueBlock> blocks;   // descriptor order: by ordinal, then by task
};

// One launch for n live tasks: left[i] > 0 local indices to go, age[i] launches taken part in (its
// budget is batch_budget(age[i]), the launch's group batch_group of the slices as planned).
// `spread` is kQueueSpread but for the A/B override of dpow_queue_open (DPOW_DIAG_QUEUE_SPREAD).
void queue_plan(const uint64_t *left, const uint32_t *age, size_t n, QueuePlan &plan, uint64_t spread = kQueueSpread);

}  // namespace dpow
