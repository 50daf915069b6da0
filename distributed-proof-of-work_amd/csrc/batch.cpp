// batch.cpp -- host side of the batched search: dpow_search_batch's round loop over the generic
// kernel (md5_batch.hip) on the launch engine (batch_engine.h), the round schedule and planner, and
// the host helpers dpow_batch_candidate / dpow_batch_plan / dpow_batch_plan_block.
//
// Rounds.  Round r covers the next slice of every live (undecided) task's local index range,
// the same slice for every task: kBatchFirst * 4^r candidates in all (capped at kBatchCap) split
// evenly over the live tasks, a power of two.  After each launch the host reads the live tasks'
// best values from pinned memory, verifies and retires the tasks that hit, drops the exhausted
// ones, checks the cancel flag and plans the next round from the survivors.  One launch is in
// flight at a time and every launch is bounded, so a return leaves nothing queued.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/dpow.h"
#include "../../include/dpow_worker.h"
#include "batch.h"
#include "batch_engine.h"
#include "ctx.h"
#include "md5_batch.h"
#include "plan.h"

namespace dpow {

uint64_t pow2_floor(uint64_t x) { return x ? 1ull << (63 - __builtin_clzll(x)) : 0; }
uint64_t pow2_ceil(uint64_t x) { return x <= 1 ? 1 : pow2_floor(x - 1) << 1; }

uint64_t batch_budget(uint32_t step) { return std::min(kBatchFirst << (2 * std::min<uint32_t>(step, 8u)), kBatchCap); }

uint32_t batch_group(uint64_t total) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(pow2_floor(total / kBatchBlocks), kBatchMinGroup),
                                        kBatchMaxGroup);
}

namespace {

// A live task of the round loop (its partition: what settling it needs, kept out of pinned memory).
struct Live {
    uint32_t task;
    uint64_t i_cur, i_end;
    uint32_t rbits, base_tb;
};

// The entries of one round for `live` (in order), and the round's shape.
BatchRound plan_round(uint32_t round, const std::vector<Live> &live, std::vector<BatchEntry> &entries) {
    uint64_t max_left = 0;
    for (const Live &l : live) max_left = std::max(max_left, l.i_end - l.i_cur);
    const BatchRound r = batch_round(round, live.size(), max_left);
    entries.resize(live.size());
    for (size_t j = 0; j < live.size(); ++j) {
        BatchEntry &e = entries[j];
        memset(&e, 0, sizeof e);
        e.task = live[j].task;
        e.i_begin = live[j].i_cur;
        e.i_end = live[j].i_end - live[j].i_cur > r.slice ? live[j].i_cur + r.slice : live[j].i_end;
    }
    return r;
}

}  // namespace

BatchRound batch_round(uint32_t round, size_t n_live, uint64_t max_left) {
    uint64_t slice = std::max(pow2_floor(batch_budget(round) / (uint64_t)std::max<size_t>(n_live, 1)), kBatchMinSlice);
    slice = std::min(slice, pow2_ceil(max_left));  // no rows past the longest range left
    BatchRound r;
    r.slice = slice;
    r.group = batch_group(slice * (uint64_t)n_live);
    r.rows = (uint32_t)((slice + r.group - 1) / r.group);
    return r;
}

// The context's buffers.  Device: the upload image [BatchTask x n][best x n] of the running batch,
// the control words behind (batch_engine.h).  Pinned: the upload image, the launch map, out_best,
// the record.
struct BatchState {
    EngineBuffers buf;
};

namespace {
constexpr size_t kBatchMapOff = kEngineImageBytes;  // h_mem, behind the upload image
constexpr size_t kBatchOutOff = kBatchMapOff + DPOW_BATCH_MAX * sizeof(BatchEntry);
constexpr size_t kBatchRecOff = kBatchOutOff + DPOW_BATCH_MAX * sizeof(unsigned long long);
constexpr size_t kBatchHostBytes = kBatchRecOff + 64;

int batch_state(BatchState **state, hipStream_t stream) {
    if (*state) return 0;
    BatchState *s = new (std::nothrow) BatchState();
    if (!s) return set_error(DPOW_ENOMEM, "dpow_search_batch: out of memory");
    const int rc = engine_alloc(s->buf, kEngineDevBytes, kBatchHostBytes, stream, batch_prepare,
                                "dpow_search_batch: allocation");
    if (rc < 0) delete s;
    else *state = s;
    return rc;
}

}  // namespace

void batch_free(BatchState *s) {
    if (!s) return;
    engine_free(s->buf);
    delete s;
}

int batch_check(const dpow_batch_task *tasks, size_t n_tasks) {
    if (!tasks) return set_error(DPOW_EINVAL, "dpow_search_batch: tasks is NULL");
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX)
        return set_error(DPOW_EINVAL, "dpow_search_batch: n_tasks must be in [1, DPOW_BATCH_MAX]");
    for (size_t i = 0; i < n_tasks; ++i) {
        const int rc = batch_check_task(tasks[i], "dpow_search_batch");
        if (rc < 0) return rc;
    }
    return 0;
}

int batch_run(BatchState **state, hipStream_t stream, const volatile uint32_t *cancel, dpow_batch_task *tasks,
              size_t n_tasks, dpow_batch_stats *stats) {
    const size_t n = n_tasks;
    dpow_batch_stats st{};
    std::vector<int32_t> status(n, DPOW_CANCELLED);
    std::vector<uint64_t> hit(n, DPOW_NO_HIT);
    auto write_out = [&]() {
        for (size_t i = 0; i < n; ++i) {
            tasks[i].status = status[i];
            tasks[i].secret_len = 0;
            if (status[i] == DPOW_FOUND)
                engine_write_hit(hit[i], tasks[i].secret, tasks[i].secret_len, tasks[i].best_global_idx);
        }
        if (stats) *stats = st;
    };
    if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) {  // raised on entry: no launch
        write_out();
        return 0;
    }
    int rc = batch_state(state, stream);
    if (rc < 0) return rc;
    EngineBuffers &s = (*state)->buf;
    const EngineSections at{n * sizeof(BatchTask), kBatchOutOff, kBatchRecOff};

    // The upload image [BatchTask x n][best x n] and the live list.
    BatchTask *img_tasks = reinterpret_cast<BatchTask *>(s.h_mem);
    unsigned long long *img_best = reinterpret_cast<unsigned long long *>(s.h_mem + at.best);
    std::vector<Live> live;
    live.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const dpow_batch_task &t = tasks[i];
        batch_fill_task(img_tasks[i], t.nonce, t.nonce_len, t.ntz, t.worker_byte, t.worker_bits);
        img_best[i] = t.best_global_idx;
        const uint32_t rbits = img_tasks[i].rbits;
        if (window_needs_no_launch(t.k_begin, t.k_end, t.best_global_idx)) {
            status[i] = DPOW_EXHAUSTED;
            continue;
        }
        live.push_back(Live{(uint32_t)i, t.k_begin << rbits, t.k_end << rbits, rbits, img_tasks[i].base_tb});
    }
    if (!live.empty()) {
        const hipError_t e =
            batch_upload(reinterpret_cast<uint32_t *>(s.d_mem), reinterpret_cast<const uint32_t *>(s.d_h_mem),
                         (uint32_t)(n * (sizeof(BatchTask) + sizeof(unsigned long long)) / 4), stream);
        if (e != hipSuccess) return hip_fail(e, "dpow_search_batch: upload");
    }
    BatchEntry *const h_map = reinterpret_cast<BatchEntry *>(s.h_mem + kBatchMapOff);
    const unsigned long long *const h_out = reinterpret_cast<const unsigned long long *>(s.h_mem + kBatchOutOff);
    const BatchEntry *const d_map = reinterpret_cast<const BatchEntry *>(s.d_h_mem + kBatchMapOff);
    const auto issue = [&](const BatchLaunch &L) {
        const hipError_t e = batch_launch(reinterpret_cast<const BatchTask *>(s.d_mem), d_map, L, stream);
        return e == hipSuccess ? 0 : hip_fail(e, "dpow_search_batch: launch");
    };
    std::vector<BatchEntry> entries;
    std::vector<Live> next;
    for (uint32_t round = 0; !live.empty(); ++round) {
        if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) break;  // the live tasks stay DPOW_CANCELLED
        const BatchRound r = plan_round(round, live, entries);
        memcpy(h_map, entries.data(), entries.size() * sizeof(BatchEntry));
        const uint32_t n_live = (uint32_t)live.size();
        rc = engine_launch(s, at, n_live, r.group, r.rows * n_live, stream,
                           "dpow_search_batch: stream idle without the launch's completion record", st, issue);
        if (rc < 0) return rc;
        next.clear();
        for (size_t j = 0; j < live.size(); ++j) {
            const Live &l = live[j];
            const dpow_batch_task &t = tasks[l.task];
            st.candidates += entries[j].i_end - entries[j].i_begin;
            const uint64_t b = h_out[j];
            switch (engine_settle(t.nonce, t.nonce_len, t.ntz, l.rbits, l.base_tb, t.best_global_idx, entries[j].i_end,
                                  l.i_end, b)) {
                case Settled::kVerifyFailed:
                    return set_error(DPOW_EVERIFY, "dpow_search_batch: kernel hit failed host MD5 verification");
                case Settled::kFound:
                    status[l.task] = DPOW_FOUND;
                    hit[l.task] = b;
                    break;
                case Settled::kExhausted: status[l.task] = DPOW_EXHAUSTED; break;
                case Settled::kLive: next.push_back(Live{l.task, entries[j].i_end, l.i_end, l.rbits, l.base_tb}); break;
            }
        }
        live.swap(next);
    }
    write_out();
    return 0;
}

}  // namespace dpow

using namespace dpow;

extern "C" {

int dpow_batch_candidate(const uint8_t *nonce, size_t nonce_len, uint32_t worker_byte, uint32_t worker_bits,
                         uint64_t local_idx, uint32_t iv_out[4], uint32_t words_out[32], uint32_t *nblk_out) {
    if (!iv_out || !words_out || !nblk_out || (nonce_len && !nonce))
        return set_error(DPOW_EINVAL, "dpow_batch_candidate: NULL argument");
    if (nonce_len > DPOW_MAX_NONCE || worker_byte > 255u)
        return set_error(DPOW_EINVAL, "dpow_batch_candidate: bad nonce length or worker_byte");
    if ((local_idx >> remainder_bits(worker_bits)) >= DPOW_K_LIMIT)
        return set_error(DPOW_ERANGE, "dpow_batch_candidate: k beyond DPOW_K_LIMIT");
    BatchTask t;
    batch_fill_task(t, nonce, nonce_len, 0, worker_byte, worker_bits);
    for (int w = 0; w < 4; ++w) iv_out[w] = t.iv[w];
    *nblk_out = batch_candidate_words(t.T, t.p, t.rbits, t.base_tb, t.len_bits, local_idx, words_out);
    return 0;
}

int dpow_batch_plan(const uint64_t *k_begin, const uint64_t *k_end, const uint32_t *worker_bits, size_t n_tasks,
                    dpow_batch_range *out, size_t max_entries, uint64_t *launches_out) {
    if (!k_begin || !k_end || !worker_bits || !launches_out)
        return set_error(DPOW_EINVAL, "dpow_batch_plan: NULL argument");
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX)
        return set_error(DPOW_EINVAL, "dpow_batch_plan: n_tasks must be in [1, DPOW_BATCH_MAX]");
    std::vector<Live> live, next;
    for (size_t i = 0; i < n_tasks; ++i) {
        if (k_begin[i] > k_end[i]) return set_error(DPOW_EINVAL, "dpow_batch_plan: k_begin > k_end");
        if (k_end[i] > DPOW_K_LIMIT) return set_error(DPOW_ERANGE, "dpow_batch_plan: k_end beyond DPOW_K_LIMIT");
        const uint32_t rbits = remainder_bits(worker_bits[i]);
        if (k_begin[i] < k_end[i]) live.push_back(Live{(uint32_t)i, k_begin[i] << rbits, k_end[i] << rbits});
    }
    std::vector<BatchEntry> entries;
    uint64_t n_out = 0, launch = 0;
    for (uint32_t round = 0; !live.empty(); ++round, ++launch) {
        const BatchRound r = plan_round(round, live, entries);
        next.clear();
        for (size_t j = 0; j < live.size(); ++j) {
            if (out && n_out < max_entries) {
                dpow_batch_range &o = out[n_out];
                o.launch = (uint32_t)launch;
                o.task = entries[j].task;
                o.i_begin = entries[j].i_begin;
                o.i_end = entries[j].i_end;
                o.group = r.group;
                o.rows = r.rows;
            }
            ++n_out;
            if (entries[j].i_end < live[j].i_end) next.push_back(Live{live[j].task, entries[j].i_end, live[j].i_end});
        }
        live.swap(next);
        if (n_out > (uint64_t)INT32_MAX) return set_error(DPOW_ERANGE, "dpow_batch_plan: too many entries");
    }
    *launches_out = launch;
    return (int)n_out;
}

int dpow_batch_plan_block(const dpow_batch_range *entries, uint32_t n_live, uint32_t block, uint32_t *task,
                          uint64_t *lo, uint64_t *hi) {
    if (!entries || !task || !lo || !hi || n_live == 0)
        return set_error(DPOW_EINVAL, "dpow_batch_plan_block: bad argument");
    const uint32_t row = block / n_live, j = block - row * n_live;
    if (row >= entries[j].rows) return set_error(DPOW_EINVAL, "dpow_batch_plan_block: block outside the launch's grid");
    *task = entries[j].task;
    return batch_block_range(entries[j].i_begin, entries[j].i_end, row, entries[j].group, *lo, *hi) ? 1 : 0;
}

}  // extern "C"
