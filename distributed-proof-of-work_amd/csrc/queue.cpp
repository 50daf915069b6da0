// queue.cpp -- the task queue (dpow_queue_*): the batched search as a service on one GPU.
//
// Tasks are submitted, cancelled and collected one by one from any thread while one pump thread
// keeps launching the generic kernel's queue entry point (md5_batch.hip queue_kernel) over whatever
// is live.  A task lives in one of DPOW_BATCH_MAX slots of a device task table from the launch
// after its arrival until the launch that decides it (or that was in flight at its cancel) has
// retired.  The pump, per launch: free the slots of decided tasks, place arrivals (their rows go
// up with a kernel on the queue's stream, so a reused slot is rewritten in stream order), plan,
// launch, wait for the completion record, read the live slots' best values, verify every hit with
// the host MD5, decide, and age the survivors.  One launch is in flight; every launch is bounded.
// The buffers, the launch up to its record and a task's fate after it are the launch engine's
// (batch_engine.h), shared with dpow_search_batch.
//
// Planner (queue_plan, a pure host function; DESIGN.md "Task queue").  A task of age a (launches
// it took part in) has the budget b = batch_budget(a) of a batch's round a.  A
// launch hashes Bd = min(max b, kQueueSpread * min b): a launch that holds a fresh task stays
// short.  Task i's ceiling is max(pow2_floor(min(b_i, Bd) / n_live), kBatchMinSlice), its share
// of a batch of this size at its own age within this launch's budget; every task but those of
// the oldest age takes its ceiling, and the oldest age class splits what is left of Bd evenly (a
// power of two, at least its ceiling).  With one age only this is batch_round's slice and group.
//
// Exactness is the batch's: a slot's best holds the task's bound or one of its own hits, slices
// go up in index order, and a workgroup skips only indices above its slot's best.
#include "queue.h"

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/dpow.h"
#include "../../include/dpow_worker.h"
#include "batch_engine.h"
#include "ctx.h"
#include "md5_batch.h"
#include "plan.h"

namespace dpow {

void queue_plan(const uint64_t *left, const uint32_t *age, size_t n, QueuePlan &plan, uint64_t spread) {
    plan.slice.assign(n, 0);
    plan.rows.assign(n, 0);
    plan.blocks.clear();
    plan.budget = 0;
    plan.group = kBatchMinGroup;
    if (n == 0) return;
    uint64_t min_b = ~0ull, max_b = 0, max_left = 0;
    uint32_t max_age = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t b = batch_budget(age[i]);
        min_b = std::min(min_b, b);
        max_b = std::max(max_b, b);
        max_age = std::max(max_age, age[i]);
        max_left = std::max(max_left, left[i]);
    }
    const uint64_t budget = std::min(max_b, spread * min_b);
    const uint64_t longest = pow2_ceil(max_left);  // no blocks past the longest range left (batch_round)
    auto ceiling = [&](uint32_t a) {
        return std::max(pow2_floor(std::min(batch_budget(a), budget) / (uint64_t)n), kBatchMinSlice);
    };
    // `total` sums the slices as planned, before a task's own end cuts its slice short: what
    // batch_round takes for the group.
    uint64_t used = 0, total = 0;
    size_t n_old = 0;
    for (size_t i = 0; i < n; ++i) {
        if (age[i] == max_age) {
            ++n_old;
            continue;
        }
        const uint64_t s = std::min(ceiling(age[i]), longest);
        plan.slice[i] = std::min(s, left[i]);
        used += plan.slice[i];
        total += s;
    }
    const uint64_t rest = budget > used ? budget - used : 0;
    const uint64_t share = std::min(std::max(pow2_floor(rest / (uint64_t)n_old), ceiling(max_age)), longest);
    for (size_t i = 0; i < n; ++i) {
        if (age[i] != max_age) continue;
        plan.slice[i] = std::min(share, left[i]);
        total += share;
    }
    const uint64_t group = batch_group(total);
    plan.budget = budget;
    plan.group = (uint32_t)group;
    // Blocks by ordinal, then by task: every task's early indices are dispatched first.  `active`
    // holds the tasks with blocks left, in task order; the loop costs the block count.
    std::vector<uint32_t> active;
    active.reserve(n);
    size_t n_blocks = 0;
    for (size_t i = 0; i < n; ++i) {
        plan.rows[i] = (uint32_t)((plan.slice[i] + group - 1) / group);
        n_blocks += plan.rows[i];
        if (plan.rows[i]) active.push_back((uint32_t)i);
    }
    plan.blocks.reserve(n_blocks);
    for (uint32_t r = 0; !active.empty(); ++r) {
        size_t keep = 0;
        for (const uint32_t i : active) {
            const uint64_t lo = (uint64_t)r * group;
            const uint64_t hi = std::min(lo + group, plan.slice[i]);
            plan.blocks.push_back(QueueBlock{i, r, lo, hi});
            if (r + 1u < plan.rows[i]) active[keep++] = i;
        }
        active.resize(keep);
    }
}

namespace {

struct QTask {
    uint64_t ticket = 0, user = 0;
    std::vector<uint8_t> nonce;
    uint32_t ntz = 0, worker_byte = 0, worker_bits = 0;
    uint32_t rbits = 0, base_tb = 0;
    uint64_t i_cur = 0, i_end = 0, bound = DPOW_NO_HIT;
    uint32_t age = 0;      // launches the task took part in
    int64_t t_submit = 0;
    bool decided = false;  // its result exists (its slot is freed once no launch can write it)
};

// The queue's buffers (dpow_queue::buf).  Pinned: the rows of newly filled slots, a launch's
// descriptors, its live-slot list, out_best, the record.  Device: the task table, the best words and
// the control words (batch_engine.h), then the descriptor table of a launch of kQueueCopyBlocks or more.
constexpr size_t kQueueRowsOff = 0;
constexpr size_t kQueueBlocksOff = kQueueRowsOff + DPOW_BATCH_MAX * sizeof(QueueRow);
constexpr size_t kQueueSlotsOff = kQueueBlocksOff + (size_t)kQueueMaxBlocks * sizeof(BatchEntry);
constexpr size_t kQueueOutOff = kQueueSlotsOff + DPOW_BATCH_MAX * sizeof(uint32_t);
constexpr size_t kQueueRecOff = kQueueOutOff + DPOW_BATCH_MAX * sizeof(unsigned long long);
constexpr size_t kQueueHostBytes = kQueueRecOff + 64;
constexpr size_t kQueueBestOff = DPOW_BATCH_MAX * sizeof(BatchTask);
constexpr size_t kQueueDevBlocksOff = kEngineDevBytes;
constexpr size_t kQueueDevBytes = kQueueDevBlocksOff + (size_t)kQueueMaxBlocks * sizeof(BatchEntry);
static_assert(kQueueBlocksOff % 32 == 0 && kQueueOutOff % 8 == 0 && kQueueRecOff % 8 == 0, "aligned sections");
constexpr EngineSections kQueueAt{kQueueBestOff, kQueueOutOff, kQueueRecOff};

const char *const kIdleMsg = "dpow_queue: stream idle without the launch's completion record";

}  // namespace

}  // namespace dpow

using namespace dpow;

struct dpow_queue {
    int device = 0;
    dpow_ctx *ctx = nullptr;  // private: its stream carries the queue's launches
    EngineBuffers buf;        // seq and the device side: the pump's alone

    std::mutex mu;
    std::condition_variable pump_cv;  // arrivals, close
    std::condition_variable res_cv;   // a result was added
    std::unordered_map<uint64_t, std::shared_ptr<QTask>> undecided;
    std::deque<std::shared_ptr<QTask>> arrivals;   // submitted, not yet in a slot
    std::vector<std::shared_ptr<QTask>> slot_task;  // DPOW_BATCH_MAX
    std::vector<uint32_t> free_slots;
    std::vector<uint32_t> live_slots;               // slots that hold a task, decided or not
    std::map<uint64_t, dpow_queue_result> done;     // results not yet collected, by ticket
    std::deque<uint64_t> done_order;                // tickets in the order decided (collected ones linger)
    int failed = 0;
    std::string fail_msg;
    bool closing = false;
    uint64_t next_ticket = 1;
    uint64_t spread = kQueueSpread;  // DPOW_DIAG_QUEUE_SPREAD at open: the A/B behind the constant (tools/queue_rate.py)
    dpow_batch_stats stats{};
    std::thread pump;

    // The task's result, available from now on.  Under mu.
    void decide(QTask &t, int32_t status, uint64_t hit) {
        dpow_queue_result r;
        memset(&r, 0, sizeof r);
        r.ticket = t.ticket;
        r.user = t.user;
        r.status = status;
        r.global_idx = DPOW_NO_HIT;
        if (status == DPOW_FOUND) engine_write_hit(hit, r.secret, r.secret_len, r.global_idx);
        r.launches = t.age;
        r.queued_ms = (double)(now_ns() - t.t_submit) * 1e-6;
        t.decided = true;
        undecided.erase(t.ticket);
        done.emplace(t.ticket, r);
        while (!done_order.empty() && !done.count(done_order.front())) done_order.pop_front();  // dpow_queue_wait took them
        done_order.push_back(t.ticket);
        res_cv.notify_all();
    }

    // A launch failed: the queue is over.  Under mu.
    void fail(int code, const std::string &msg) {
        failed = code;
        fail_msg = msg;
        std::vector<std::shared_ptr<QTask>> all;
        for (auto &kv : undecided) all.push_back(kv.second);
        std::sort(all.begin(), all.end(), [](const auto &a, const auto &b) { return a->ticket < b->ticket; });
        for (auto &t : all) decide(*t, code, DPOW_NO_HIT);
        arrivals.clear();
        res_cv.notify_all();
    }

    void pump_main() {
        TimerSlack slack;  // the pump's waits poll with short sleeps (batch_wait_record)
        slack.lower();
        std::unique_lock<std::mutex> g(mu);
        if (hipSetDevice(device) != hipSuccess) {
            fail(DPOW_EHIP, "dpow_queue: hipSetDevice failed in the pump thread");
            return;
        }
        QueueRow *const h_rows = reinterpret_cast<QueueRow *>(buf.h_mem + kQueueRowsOff);
        BatchEntry *const h_blocks = reinterpret_cast<BatchEntry *>(buf.h_mem + kQueueBlocksOff);
        uint32_t *const h_slots = reinterpret_cast<uint32_t *>(buf.h_mem + kQueueSlotsOff);
        const unsigned long long *const h_out = reinterpret_cast<const unsigned long long *>(buf.h_mem + kQueueOutOff);
        BatchTask *const d_tasks = reinterpret_cast<BatchTask *>(buf.d_mem);
        uint32_t *const d_blocks = reinterpret_cast<uint32_t *>(buf.d_mem + kQueueDevBlocksOff);
        const uint32_t *const p_blocks = reinterpret_cast<const uint32_t *>(buf.d_h_mem + kQueueBlocksOff);  // pinned
        uint32_t n_rows = 0;
        // The rows of new slots, then the launch.  A short descriptor table is read where it is, in
        // pinned memory, one scalar load per workgroup; a long one is first copied to device memory
        // by the upload kernel (queue.h kQueueCopyBlocks).
        const auto issue = [&](const BatchLaunch &L) {
            hipError_t e = queue_upload(d_tasks, L.best, reinterpret_cast<const QueueRow *>(buf.d_h_mem + kQueueRowsOff),
                                        n_rows, ctx->stream);
            const bool copy = L.n_blocks >= kQueueCopyBlocks;
            if (e == hipSuccess && copy)
                e = batch_upload(d_blocks, p_blocks, L.n_blocks * (uint32_t)(sizeof(BatchEntry) / 4), ctx->stream);
            if (e == hipSuccess)
                e = queue_launch(d_tasks, reinterpret_cast<const BatchEntry *>(copy ? d_blocks : p_blocks),
                                 reinterpret_cast<const uint32_t *>(buf.d_h_mem + kQueueSlotsOff), L, ctx->stream);
            return e == hipSuccess ? 0 : hip_fail(e, "dpow_queue: launch");
        };
        dpow_batch_stats run{};  // launches, rounds and kernel time, counted with the mutex dropped
        std::vector<std::shared_ptr<QTask>> in_launch;
        std::vector<uint64_t> left;
        std::vector<uint32_t> age;
        QueuePlan plan;
        for (;;) {
            // No launch is in flight here: the slots of decided tasks are free.
            size_t keep = 0;
            for (const uint32_t s : live_slots) {
                if (slot_task[s]->decided) {
                    slot_task[s].reset();
                    free_slots.push_back(s);
                } else {
                    live_slots[keep++] = s;
                }
            }
            live_slots.resize(keep);
            n_rows = 0;
            while (!arrivals.empty() && !free_slots.empty()) {
                std::shared_ptr<QTask> t = arrivals.front();
                arrivals.pop_front();
                if (t->decided) continue;  // cancelled before it was placed
                const uint32_t s = free_slots.back();
                free_slots.pop_back();
                slot_task[s] = t;
                live_slots.push_back(s);
                QueueRow &row = h_rows[n_rows++];
                batch_fill_task(row.t, t->nonce.data(), t->nonce.size(), t->ntz, t->worker_byte, t->worker_bits);
                row.best = t->bound;
                row.slot = s;
                row.pad_ = 0;
            }
            if (live_slots.empty()) {
                if (closing) return;
                pump_cv.wait(g);
                continue;
            }
            if (!std::is_sorted(live_slots.begin(), live_slots.end())) std::sort(live_slots.begin(), live_slots.end());
            const size_t n = live_slots.size();
            in_launch.resize(n);
            left.resize(n);
            age.resize(n);
            for (size_t j = 0; j < n; ++j) {
                in_launch[j] = slot_task[live_slots[j]];
                left[j] = in_launch[j]->i_end - in_launch[j]->i_cur;
                age[j] = in_launch[j]->age;
                h_slots[j] = live_slots[j];
            }
            queue_plan(left.data(), age.data(), n, plan, spread);
            if (plan.blocks.empty() || plan.blocks.size() > kQueueMaxBlocks) {
                fail(DPOW_EINVAL, "dpow_queue: the launch plan left the descriptor table");  // never expected
                return;
            }
            for (size_t b = 0; b < plan.blocks.size(); ++b) {
                const QueueBlock &pb = plan.blocks[b];
                BatchEntry &e = h_blocks[b];
                e.i_begin = in_launch[pb.task]->i_cur + pb.lo;
                e.i_end = in_launch[pb.task]->i_cur + pb.hi;
                e.task = live_slots[pb.task];
                e.pad_[0] = e.pad_[1] = e.pad_[2] = 0;
            }
            g.unlock();  // round the upload, the launch and the wait
            const int rc = engine_launch(buf, kQueueAt, (uint32_t)n, plan.group, (uint32_t)plan.blocks.size(), ctx->stream,
                                         kIdleMsg, run, issue);
            g.lock();
            if (rc < 0) {
                fail(rc, dpow_last_error());
                return;
            }
            stats.launches = run.launches;
            stats.rounds = run.rounds;
            stats.kernel_ms = run.kernel_ms;
            for (size_t j = 0; j < n; ++j) {
                QTask &t = *in_launch[j];
                stats.candidates += plan.slice[j];
                t.age++;
                if (t.decided) continue;  // cancelled while the launch ran: the kill wins over its hit
                const uint64_t b = h_out[j];
                t.i_cur += plan.slice[j];
                switch (engine_settle(t.nonce.data(), t.nonce.size(), t.ntz, t.rbits, t.base_tb, t.bound, t.i_cur,
                                      t.i_end, b)) {
                    case Settled::kVerifyFailed:
                        fail(DPOW_EVERIFY, "dpow_queue: kernel hit failed host MD5 verification");
                        return;
                    case Settled::kFound: decide(t, DPOW_FOUND, b); break;
                    case Settled::kExhausted: decide(t, DPOW_EXHAUSTED, DPOW_NO_HIT); break;
                    case Settled::kLive: break;
                }
            }
            for (auto &t : in_launch) t.reset();
        }
    }
};

namespace {

// Hand out one collected result; a failed queue's code travels as the calling thread's error too.
int hand_out(dpow_queue *q, std::map<uint64_t, dpow_queue_result>::iterator it, dpow_queue_result *out) {
    *out = it->second;
    q->done.erase(it);
    if (out->status < 0) (void)set_error(out->status, q->fail_msg);
    return 1;
}

template <typename Pred>
bool wait_results(dpow_queue *q, std::unique_lock<std::mutex> &g, int timeout_ms, Pred ready) {
    if (timeout_ms < 0) {
        q->res_cv.wait(g, ready);
        return true;
    }
    return q->res_cv.wait_for(g, std::chrono::milliseconds(timeout_ms), ready);
}

}  // namespace

extern "C" {

int dpow_queue_open(int device, dpow_queue **out) {
    if (!out) return set_error(DPOW_EINVAL, "dpow_queue_open: out is NULL");
    *out = nullptr;
    dpow_ctx *ctx = nullptr;
    const int rc = dpow_open(device, &ctx);  // no device, a bad ordinal: its errors
    if (rc < 0) return rc;
    dpow_queue *q = new (std::nothrow) dpow_queue();
    if (!q) {
        dpow_close(ctx);
        return set_error(DPOW_ENOMEM, "dpow_queue_open: out of memory");
    }
    q->device = device;
    q->ctx = ctx;
    if (const char *sp = getenv("DPOW_DIAG_QUEUE_SPREAD")) {
        const long v = atol(sp);
        if (v >= 1 && v <= 256) q->spread = (uint64_t)v;  // Bd stays within kBatchCap: the block table holds any launch
    }
    const DeviceScope on_device(device);
    const char *const who = "dpow_queue_open: allocation";
    const int arc = on_device.e != hipSuccess
                        ? hip_fail(on_device.e, who)
                        : engine_alloc(q->buf, kQueueDevBytes, kQueueHostBytes, ctx->stream, queue_prepare, who);
    if (arc < 0) {
        dpow_close(ctx);  // (leaves the thread's error as it is)
        delete q;
        return arc;
    }
    q->slot_task.resize(DPOW_BATCH_MAX);
    q->free_slots.reserve(DPOW_BATCH_MAX);
    for (uint32_t s = DPOW_BATCH_MAX; s-- > 0;) q->free_slots.push_back(s);  // slot 0 first
    q->live_slots.reserve(DPOW_BATCH_MAX);
    q->pump = std::thread([q] { q->pump_main(); });
    *out = q;
    return 0;
}

void dpow_queue_close(dpow_queue *q) {
    if (!q) return;
    {
        std::lock_guard<std::mutex> g(q->mu);
        q->closing = true;
        std::vector<std::shared_ptr<QTask>> all;
        for (auto &kv : q->undecided) all.push_back(kv.second);
        for (auto &t : all) q->decide(*t, DPOW_CANCELLED, DPOW_NO_HIT);
        q->arrivals.clear();
        q->pump_cv.notify_all();
    }
    if (q->pump.joinable()) q->pump.join();  // after the launch in flight has retired
    {
        const DeviceScope on_device(q->device);
        (void)hipStreamSynchronize(q->ctx->stream);
        engine_free(q->buf);
    }
    dpow_close(q->ctx);
    delete q;
}

int dpow_queue_submit(dpow_queue *q, const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                      uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, uint64_t bound, uint64_t user,
                      uint64_t *ticket) {
    dpow_batch_task a;  // the task's own errors first: they need no queue
    memset(&a, 0, sizeof a);
    a.nonce = nonce;
    a.nonce_len = nonce_len;
    a.ntz = ntz;
    a.worker_byte = worker_byte;
    a.worker_bits = worker_bits;
    a.k_begin = k_begin;
    a.k_end = k_end;
    const int rc = batch_check_task(a, "dpow_queue_submit");
    if (rc < 0) return rc;
    if (!q || !ticket) return set_error(DPOW_EINVAL, "dpow_queue_submit: NULL argument");
    auto t = std::make_shared<QTask>();
    if (nonce_len) t->nonce.assign(nonce, nonce + nonce_len);
    t->user = user;
    t->ntz = ntz;
    t->worker_byte = worker_byte;
    t->worker_bits = worker_bits;
    t->rbits = remainder_bits(worker_bits);
    t->base_tb = base_thread_byte(worker_byte, worker_bits);
    t->i_cur = k_begin << t->rbits;
    t->i_end = k_end << t->rbits;
    t->bound = bound;
    t->t_submit = now_ns();
    std::lock_guard<std::mutex> g(q->mu);
    if (q->failed) return set_error(q->failed, q->fail_msg);
    if (q->closing) return set_error(DPOW_EINVAL, "dpow_queue_submit: the queue is closing");
    // Tickets out: undecided tasks and results nobody has collected yet.  Both hold memory, and a
    // caller that never collects must not grow the queue without bound.
    if (q->undecided.size() + q->done.size() >= DPOW_BATCH_MAX)
        return set_error(DPOW_EAGAIN, "dpow_queue_submit: DPOW_BATCH_MAX tasks are undecided or not yet collected");
    t->ticket = q->next_ticket++;
    *ticket = t->ticket;
    if (window_needs_no_launch(k_begin, k_end, bound)) {  // as dpow_search_batch
        q->decide(*t, DPOW_EXHAUSTED, DPOW_NO_HIT);
        return 0;
    }
    q->undecided.emplace(t->ticket, t);
    q->arrivals.push_back(t);
    q->pump_cv.notify_one();
    return 0;
}

int dpow_queue_cancel(dpow_queue *q, uint64_t ticket) {
    if (!q) return set_error(DPOW_EINVAL, "dpow_queue_cancel: queue is NULL");
    std::lock_guard<std::mutex> g(q->mu);
    auto it = q->undecided.find(ticket);
    if (it == q->undecided.end()) return 0;
    // Decided at once; the pump frees its slot once the launch in flight (which may still write
    // the slot's best) has retired, and drops it from the arrivals if it has no slot yet.
    const std::shared_ptr<QTask> t = it->second;
    q->decide(*t, DPOW_CANCELLED, DPOW_NO_HIT);
    return 1;
}

int dpow_queue_next(dpow_queue *q, dpow_queue_result *out, int timeout_ms) {
    if (!q || !out) return set_error(DPOW_EINVAL, "dpow_queue_next: NULL argument");
    std::unique_lock<std::mutex> g(q->mu);
    auto drop_collected = [&] {  // tickets dpow_queue_wait took
        while (!q->done_order.empty() && !q->done.count(q->done_order.front())) q->done_order.pop_front();
    };
    if (!wait_results(q, g, timeout_ms, [&] {
            drop_collected();
            return !q->done_order.empty() || q->failed != 0;
        }))
        return 0;
    if (q->done_order.empty()) return set_error(q->failed, q->fail_msg);
    const auto it = q->done.find(q->done_order.front());
    q->done_order.pop_front();
    return hand_out(q, it, out);
}

int dpow_queue_wait(dpow_queue *q, uint64_t ticket, dpow_queue_result *out, int timeout_ms) {
    if (!q || !out) return set_error(DPOW_EINVAL, "dpow_queue_wait: NULL argument");
    std::unique_lock<std::mutex> g(q->mu);
    if (!wait_results(q, g, timeout_ms, [&] { return q->done.count(ticket) || !q->undecided.count(ticket); }))
        return 0;
    const auto it = q->done.find(ticket);
    if (it == q->done.end())
        return set_error(DPOW_EINVAL, "dpow_queue_wait: the ticket is neither undecided nor waiting to be collected");
    return hand_out(q, it, out);
}

int dpow_queue_stats(dpow_queue *q, dpow_batch_stats *out, uint32_t *live, uint32_t *uncollected) {
    if (!q) return set_error(DPOW_EINVAL, "dpow_queue_stats: queue is NULL");
    std::lock_guard<std::mutex> g(q->mu);
    if (out) *out = q->stats;
    if (live) *live = (uint32_t)q->undecided.size();
    if (uncollected) *uncollected = (uint32_t)q->done.size();
    return 0;
}

int dpow_queue_plan(const uint64_t *left, const uint32_t *age, size_t n_tasks, dpow_batch_range *out,
                    size_t max_blocks, uint64_t *budget_out) {
    if (!left || !age || !budget_out) return set_error(DPOW_EINVAL, "dpow_queue_plan: NULL argument");
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX)
        return set_error(DPOW_EINVAL, "dpow_queue_plan: n_tasks must be in [1, DPOW_BATCH_MAX]");
    for (size_t i = 0; i < n_tasks; ++i)
        if (left[i] == 0) return set_error(DPOW_EINVAL, "dpow_queue_plan: a live task has indices left");
    QueuePlan plan;
    queue_plan(left, age, n_tasks, plan);
    for (size_t b = 0; b < plan.blocks.size() && b < max_blocks && out; ++b) {
        const QueueBlock &pb = plan.blocks[b];
        dpow_batch_range &o = out[b];
        o.launch = 0;
        o.task = pb.task;
        o.i_begin = pb.lo;
        o.i_end = pb.hi;
        o.group = plan.group;
        o.rows = plan.rows[pb.task];
    }
    *budget_out = plan.budget;
    return (int)plan.blocks.size();
}

}  // extern "C"
