// many_plan.cpp -- the launch planner and the descriptor cut of the batched host loops (many_plan.h).
#include "many_plan.h"

#include <stdlib.h>

#include <algorithm>

#include "batch.h"

namespace dpow {

uint64_t many_weight(uint64_t n, uint32_t ntz) {
    const uint32_t shift = 4u * std::min(ntz, 7u);
    return (n + (1ull << shift) - 1ull) >> shift;
}

bool many_next(const uint64_t *i_begin, const uint64_t *i_end, const uint32_t *ntz, size_t n, const ManyBudget &b,
               ManyCursor &cur, std::vector<ManyPart> &parts, uint32_t &group) {
    parts.clear();
    uint64_t used = 0, weight = 0;
    while (cur.task < n) {
        const uint64_t lo = i_begin[cur.task] + cur.done, end = i_end[cur.task];
        if (lo >= end) {  // an empty task, or one just finished
            cur.task++;
            cur.done = 0;
            continue;
        }
        // The most this task may add: the indices left of the first budget, and the most whose
        // weight is left of the second (ceil(m / 16^e) <= w exactly when m <= w * 16^e).
        const uint64_t left = end - lo;
        uint64_t room = b.cap - used;
        if (ntz) room = std::min(room, (b.weight - weight) << (4u * std::min(ntz[cur.task], 7u)));
        const uint64_t take = left <= room ? left : room & ~255ull;
        if (take == 0) break;  // (never of an empty launch: both budgets are at least 256)
        parts.push_back(ManyPart{(uint32_t)cur.task, lo, lo + take});
        used += take;
        if (ntz) weight += many_weight(take, ntz[cur.task]);
        if (take < left) {
            cur.done += take;
            break;
        }
        cur.task++;
        cur.done = 0;
    }
    group = batch_group(used);
    return !parts.empty();
}

namespace {

// The walk: emit(b, task, lo, hi, rows) per descriptor b, `rows` the descriptors of its part.
template <typename Emit>
size_t many_blocks(const std::vector<ManyPart> &parts, uint32_t group, Emit &&emit) {
    size_t n_blocks = 0;
    for (const ManyPart &p : parts) {
        const uint32_t rows = (uint32_t)((p.hi - p.lo + group - 1) / group);
        for (uint64_t lo = p.lo; lo < p.hi; lo += group, ++n_blocks)
            emit(n_blocks, p.task, lo, p.hi - lo > group ? lo + group : p.hi, rows);
    }
    return n_blocks;
}

}  // namespace

size_t many_write_blocks(const std::vector<ManyPart> &parts, uint32_t group, BatchEntry *blocks, size_t max_blocks) {
    const size_t n_blocks = many_blocks(parts, group, [&](size_t b, uint32_t task, uint64_t lo, uint64_t hi, uint32_t) {
        if (b >= max_blocks) return;
        BatchEntry &e = blocks[b];
        e.i_begin = lo;
        e.i_end = hi;
        e.task = task;
        e.pad_[0] = e.pad_[1] = e.pad_[2] = 0;
    });
    return n_blocks <= max_blocks ? n_blocks : 0;
}

size_t many_append_ranges(const std::vector<ManyPart> &parts, uint32_t group, uint64_t launch, dpow_batch_range *out,
                          size_t max_entries, uint64_t n_out) {
    return many_blocks(parts, group, [&](size_t b, uint32_t task, uint64_t lo, uint64_t hi, uint32_t rows) {
        if (!out || n_out + b >= max_entries) return;
        dpow_batch_range &o = out[n_out + b];
        o.launch = (uint32_t)launch;
        o.task = task;
        o.i_begin = lo;
        o.i_end = hi;
        o.group = group;
        o.rows = rows;
    });
}

uint64_t many_cap(const char *env) {
    if (const char *v = getenv(env)) {
        const long long c = atoll(v);
        if (c >= 256 && (uint64_t)c <= kBatchCap) return (uint64_t)c & ~255ull;
    }
    return kBatchCap;
}

}  // namespace dpow
