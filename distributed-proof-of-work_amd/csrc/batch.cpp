// batch.cpp -- host side of the batched search: dpow_search_batch's round loop over the generic
// kernel (md5_batch.hip), its round planner, and the host helpers dpow_batch_candidate /
// dpow_batch_plan / dpow_batch_plan_block.
//
// Rounds.  Round r covers the next slice of every live (undecided) task's local index range,
// the same slice for every task: kBatchFirst * 4^r candidates in all (capped at kBatchCap) split
// evenly over the live tasks, a power of two.  After each launch the host reads the live tasks'
// best values from pinned memory, verifies and retires the tasks that hit, drops the exhausted
// ones, checks the cancel flag and plans the next round from the survivors.  One launch is in
// flight at a time and every launch is bounded, so a return leaves nothing queued.
#include <hip/hip_runtime.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dpow.h"
#include "../../include/dpow_worker.h"
#include "batch.h"
#include "ctx.h"
#include "md5_batch.h"
#include "md5_host.h"
#include "plan.h"

namespace dpow {

uint64_t pow2_floor(uint64_t x) { return x ? 1ull << (63 - __builtin_clzll(x)) : 0; }
uint64_t pow2_ceil(uint64_t x) { return x <= 1 ? 1 : pow2_floor(x - 1) << 1; }

// Midstate, final-block template and partition of one task.
void batch_fill_task(BatchTask &t, const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                     uint32_t worker_bits) {
    memset(&t, 0, sizeof t);
    for (int w = 0; w < 4; ++w) t.iv[w] = kMd5IV[w];
    uint32_t M[16];
    size_t off = 0;
    for (; off + 64 <= nonce_len; off += 64) {
        for (int w = 0; w < 16; ++w) M[w] = load_le32(nonce + off + 4 * w);
        md5_compress(t.iv, M);
    }
    uint8_t tail[64] = {0};
    if (nonce_len > off) memcpy(tail, nonce + off, nonce_len - off);
    for (int w = 0; w < 16; ++w) t.T[w] = load_le32(tail + 4 * w);
    t.p = (uint32_t)(nonce_len - off);
    t.rbits = remainder_bits(worker_bits);
    t.base_tb = base_thread_byte(worker_byte, worker_bits);
    t.ntz = ntz;
    t.len_bits = 8u * (uint32_t)(nonce_len + 1);
    t.dmask = tail_nibble_mask(ntz < 8u ? ntz : 8u);
}

namespace {

// A live task of the round loop.
struct Live {
    uint32_t task;
    uint64_t i_cur, i_end;
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
    const uint64_t target = std::min(kBatchFirst << (2 * std::min<uint32_t>(round, 8u)), kBatchCap);
    uint64_t slice = std::max(pow2_floor(target / (uint64_t)std::max<size_t>(n_live, 1)), kBatchMinSlice);
    slice = std::min(slice, pow2_ceil(max_left));  // no rows past the longest range left
    const uint64_t total = slice * (uint64_t)n_live;
    const uint64_t group = std::min<uint64_t>(std::max<uint64_t>(pow2_floor(total / kBatchBlocks), kBatchMinGroup),
                                              kBatchMaxGroup);
    BatchRound r;
    r.slice = slice;
    r.group = (uint32_t)group;
    r.rows = (uint32_t)((slice + group - 1) / group);
    return r;
}

struct BatchState {
    char *d_mem = nullptr;     // device: [BatchTask x n][best x n] of the running batch, the control words behind
    char *h_mem = nullptr;     // pinned, mapped: the upload image, the launch map, out_best, the record
    char *d_h_mem = nullptr;   // device alias of h_mem
    uint32_t seq = 0;
};

namespace {
constexpr size_t kImageBytes = DPOW_BATCH_MAX * (sizeof(BatchTask) + sizeof(unsigned long long));
constexpr size_t kCtlOff = kImageBytes;                      // d_mem: done (u32) at +0, t0 (u64) at +8
constexpr size_t kDevBytes = kImageBytes + 64;
constexpr size_t kMapOff = kImageBytes;                      // h_mem
constexpr size_t kOutOff = kMapOff + DPOW_BATCH_MAX * sizeof(BatchEntry);
constexpr size_t kRecOff = kOutOff + DPOW_BATCH_MAX * sizeof(unsigned long long);
constexpr size_t kHostBytes = kRecOff + 64;

int batch_state(BatchState **state, hipStream_t stream) {
    if (*state) return 0;
    BatchState *s = new (std::nothrow) BatchState();
    if (!s) return set_error(DPOW_ENOMEM, "dpow_search_batch: out of memory");
    hipError_t e;
    if ((e = hipMalloc(&s->d_mem, kDevBytes)) != hipSuccess ||
        (e = hipHostMalloc(&s->h_mem, kHostBytes, hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void **>(&s->d_h_mem), s->h_mem, 0)) != hipSuccess ||
        (e = hipMemsetAsync(s->d_mem + kCtlOff, 0, 64, stream)) != hipSuccess ||
        (e = hipStreamSynchronize(stream)) != hipSuccess || (e = batch_prepare()) != hipSuccess) {
        batch_free(s);
        return hip_fail(e, "dpow_search_batch: allocation");
    }
    memset(s->h_mem, 0, kHostBytes);
    *state = s;
    return 0;
}

}  // namespace

// Wait for the completion record of launch `seq`: spin at first (a small round's record is a
// few microseconds away), then sleep between polls; the stream is queried now and then so a
// failed launch ends the wait with an error.
int batch_wait_record(const BatchRecord *rec, uint32_t seq, hipStream_t stream, const char *idle_msg) {
    const int64_t t0 = now_ns();
    for (uint64_t it = 1;; ++it) {
        if (__atomic_load_n(&rec->seq, __ATOMIC_ACQUIRE) == seq) return 0;
        const bool spinning = now_ns() - t0 < 200000;
        if (spinning ? (it % 4096 == 0) : (it % 16 == 0)) {
            const int alive = stream_liveness(stream, &rec->seq, seq, idle_msg);
            if (alive != 0) return alive < 0 ? alive : 0;
        }
        if (spinning) {
            __builtin_ia32_pause();
        } else {
            const struct timespec ts = {0, 5000};
            nanosleep(&ts, nullptr);
        }
    }
}

int batch_check_task(const dpow_batch_task &t, const char *who) {
    const std::string w(who);
    if (t.nonce_len && !t.nonce) return set_error(DPOW_EINVAL, w + ": nonce is NULL");
    if (t.nonce_len > DPOW_MAX_NONCE) return set_error(DPOW_EINVAL, w + ": nonce longer than DPOW_MAX_NONCE");
    if (t.worker_byte > 255u) return set_error(DPOW_EINVAL, w + ": worker_byte > 255");
    if (t.k_begin > t.k_end) return set_error(DPOW_EINVAL, w + ": k_begin > k_end");
    if (t.k_end > DPOW_K_LIMIT) return set_error(DPOW_ERANGE, w + ": k_end beyond DPOW_K_LIMIT");
    return 0;
}

void batch_free(BatchState *s) {
    if (!s) return;
    if (s->d_mem) (void)hipFree(s->d_mem);
    if (s->h_mem) (void)hipHostFree(s->h_mem);
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
            if (status[i] != DPOW_FOUND) continue;
            size_t len = 0;
            dpow_secret_from_index(hit[i], tasks[i].secret, &len);
            tasks[i].secret_len = (uint32_t)len;
            tasks[i].best_global_idx = hit[i];
        }
        if (stats) *stats = st;
    };
    if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) {  // raised on entry: no launch
        write_out();
        return 0;
    }
    int rc = batch_state(state, stream);
    if (rc < 0) return rc;
    BatchState *s = *state;

    // The upload image [BatchTask x n][best x n] and the live list.  A task with an empty
    // window, or whose window starts at or above its bound, is exhausted without a launch.
    BatchTask *img_tasks = reinterpret_cast<BatchTask *>(s->h_mem);
    unsigned long long *img_best = reinterpret_cast<unsigned long long *>(s->h_mem + n * sizeof(BatchTask));
    std::vector<Live> live;
    live.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const dpow_batch_task &t = tasks[i];
        batch_fill_task(img_tasks[i], t.nonce, t.nonce_len, t.ntz, t.worker_byte, t.worker_bits);
        img_best[i] = t.best_global_idx;
        const uint32_t rbits = img_tasks[i].rbits;
        if (t.k_begin >= t.k_end || (t.k_begin << 8) >= t.best_global_idx) {
            status[i] = DPOW_EXHAUSTED;
            continue;
        }
        live.push_back(Live{(uint32_t)i, t.k_begin << rbits, t.k_end << rbits});
    }
    if (!live.empty()) {
        const hipError_t e =
            batch_upload(reinterpret_cast<uint32_t *>(s->d_mem), reinterpret_cast<const uint32_t *>(s->d_h_mem),
                         (uint32_t)(n * (sizeof(BatchTask) + sizeof(unsigned long long)) / 4), stream);
        if (e != hipSuccess) return hip_fail(e, "dpow_search_batch: upload");
    }
    BatchEntry *const h_map = reinterpret_cast<BatchEntry *>(s->h_mem + kMapOff);
    const unsigned long long *const h_out = reinterpret_cast<const unsigned long long *>(s->h_mem + kOutOff);
    const BatchRecord *const h_rec = reinterpret_cast<const BatchRecord *>(s->h_mem + kRecOff);
    std::vector<BatchEntry> entries;
    std::vector<Live> next;
    for (uint32_t round = 0; !live.empty(); ++round) {
        if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) break;  // the live tasks stay DPOW_CANCELLED
        const BatchRound r = plan_round(round, live, entries);
        memcpy(h_map, entries.data(), entries.size() * sizeof(BatchEntry));
        BatchLaunch L{};
        L.best = reinterpret_cast<unsigned long long *>(s->d_mem + n * sizeof(BatchTask));
        L.out_best = reinterpret_cast<unsigned long long *>(s->d_h_mem + kOutOff);
        L.rec = reinterpret_cast<BatchRecord *>(s->d_h_mem + kRecOff);
        L.done = reinterpret_cast<uint32_t *>(s->d_mem + kCtlOff);
        L.t0 = reinterpret_cast<unsigned long long *>(s->d_mem + kCtlOff + 8);
        L.n_live = (uint32_t)live.size();
        L.group = r.group;
        L.n_blocks = r.rows * L.n_live;
        if (++s->seq == 0u) s->seq = 1u;
        L.seq = s->seq;
        const hipError_t e = batch_launch(reinterpret_cast<const BatchTask *>(s->d_mem),
                                          reinterpret_cast<const BatchEntry *>(s->d_h_mem + kMapOff), L, stream);
        if (e != hipSuccess) return hip_fail(e, "dpow_search_batch: launch");
        if ((rc = batch_wait_record(h_rec, L.seq, stream,
                                    "dpow_search_batch: stream idle without the launch's completion record")) < 0)
            return rc;
        st.launches++;
        st.rounds++;
        if (h_rec->t_start != 0ull && h_rec->t_end >= h_rec->t_start)
            st.kernel_ms += (double)(h_rec->t_end - h_rec->t_start) * kRealtimeNs * 1e-6;
        next.clear();
        for (size_t j = 0; j < live.size(); ++j) {
            const Live &l = live[j];
            const dpow_batch_task &t = tasks[l.task];
            st.candidates += entries[j].i_end - entries[j].i_begin;
            const uint64_t b = h_out[j];
            if (b < t.best_global_idx) {  // below the bound: a hit, re-verified on the host
                uint8_t sec[DPOW_MAX_SECRET];
                size_t len = 0;
                dpow_secret_from_index(b, sec, &len);
                if (!dpow_verify(t.nonce, t.nonce_len, sec, len, t.ntz))
                    return set_error(DPOW_EVERIFY, "dpow_search_batch: kernel hit failed host MD5 verification");
                status[l.task] = DPOW_FOUND;
                hit[l.task] = b;
                continue;
            }
            const uint64_t cur = entries[j].i_end;
            const BatchTask &bt = img_tasks[l.task];
            if (cur >= l.i_end || global_of_local(cur, bt.rbits, bt.base_tb) >= t.best_global_idx) {
                status[l.task] = DPOW_EXHAUSTED;
                continue;
            }
            next.push_back(Live{l.task, cur, l.i_end});
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
