// batch_engine.h -- what the batched search (batch.cpp) and the task queue (queue.cpp) share on the
// host: a task's table row and its argument errors (`who`: the entry point named in the message),
// the device and pinned buffers of one user, one launch of the generic kernel (md5_batch.hip) up to
// its completion record (the stream-liveness check included; `idle_msg`: the error text when the
// stream went idle without the record), and what becomes of one task after a launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dpow.h"
#include "ctx.h"
#include "md5_batch.h"

namespace dpow {

void batch_fill_task(BatchTask &t, const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                     uint32_t worker_bits);
int batch_check_task(const dpow_batch_task &t, const char *who);
int batch_wait_record(const BatchRecord *rec, uint32_t seq, hipStream_t stream, const char *idle_msg);

// (Hidden, as ctx.h: the engine's functions, the inline and template ones included, stay out of the
// library's dynamic symbols.)
#pragma GCC visibility push(hidden)

// The buffers of one user.  Device memory starts the same way for both: the task table and the
// tasks' best words within the first kEngineImageBytes bytes, then 64 control bytes -- done (u32)
// at +0, t0 (u64) at +8 -- that are zero whenever no launch is in flight.  What follows, and the
// sections of the pinned memory, are the user's own.
struct EngineBuffers {
    char *d_mem = nullptr;
    char *h_mem = nullptr;    // pinned, mapped
    char *d_h_mem = nullptr;  // device alias of h_mem
    uint32_t seq = 0;         // of the last launch (0: none yet)
};
constexpr size_t kEngineImageBytes = DPOW_BATCH_MAX * (sizeof(BatchTask) + sizeof(unsigned long long));
constexpr size_t kEngineCtlOff = kEngineImageBytes;  // d_mem
constexpr size_t kEngineDevBytes = kEngineCtlOff + 64;

// Allocates and zeroes (the device's current, `stream` its user's); `prepare` loads the user's
// kernels.  0, or the negative code with "`who`: <the HIP error>" set and nothing left allocated.
int engine_alloc(EngineBuffers &b, size_t dev_bytes, size_t host_bytes, hipStream_t stream, hipError_t (*prepare)(),
                 const char *who);
void engine_free(EngineBuffers &b);  // the device is current, the stream drained

// Where one user keeps what a launch needs.
struct EngineSections {
    size_t best;  // d_mem: the tasks' best words
    size_t out;   // h_mem: out_best of the launch's live entries
    size_t rec;   // h_mem: the completion record
};

// One launch: fills BatchLaunch, runs issue(L) -- the user's upload and launch calls, 0 or a negative
// code with the error set -- waits for the completion record and counts the launch into `st`.
template <typename Issue>
int engine_launch(EngineBuffers &b, const EngineSections &at, uint32_t n_live, uint32_t group, uint32_t n_blocks,
                  hipStream_t stream, const char *idle_msg, dpow_batch_stats &st, Issue &&issue) {
    BatchLaunch L{};
    L.best = reinterpret_cast<unsigned long long *>(b.d_mem + at.best);
    L.out_best = reinterpret_cast<unsigned long long *>(b.d_h_mem + at.out);
    L.rec = reinterpret_cast<BatchRecord *>(b.d_h_mem + at.rec);
    L.done = reinterpret_cast<uint32_t *>(b.d_mem + kEngineCtlOff);
    L.t0 = reinterpret_cast<unsigned long long *>(b.d_mem + kEngineCtlOff + 8);
    L.n_live = n_live;
    L.group = group;
    L.n_blocks = n_blocks;
    if (++b.seq == 0u) b.seq = 1u;
    L.seq = b.seq;
    int rc = issue(L);
    const BatchRecord *const rec = reinterpret_cast<const BatchRecord *>(b.h_mem + at.rec);
    if (rc < 0 || (rc = batch_wait_record(rec, L.seq, stream, idle_msg)) < 0) return rc;
    st.launches++;
    st.rounds++;
    if (rec->t_start != 0ull && rec->t_end >= rec->t_start)
        st.kernel_ms += (double)(rec->t_end - rec->t_start) * kRealtimeNs * 1e-6;
    return 0;
}

// A window that is empty, or that starts at or above its bound, is exhausted without a launch.
inline bool window_needs_no_launch(uint64_t k_begin, uint64_t k_end, uint64_t bound) {
    return k_begin >= k_end || (k_begin << 8) >= bound;
}

// The local index of global index g under the partition (rbits, base_tb), the inverse of
// global_of_local; false when g's threadByte is another partition's (i is then meaningless).
inline bool local_of_global(uint64_t g, uint32_t rbits, uint32_t base_tb, uint64_t &i) {
    const uint32_t tb = (uint32_t)(g & 255u);
    i = ((g >> 8) << rbits) | (tb & ((1u << rbits) - 1u));
    return (tb >> rbits) == (base_tb >> rbits);
}

// One task after a launch that covered its local indices up to `cur` (of i_end) and left `best` in
// out_best.  A value below the bound is a hit, re-verified with the host MD5.
enum class Settled { kLive, kFound, kExhausted, kVerifyFailed };
inline Settled engine_settle(const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t rbits, uint32_t base_tb,
                             uint64_t bound, uint64_t cur, uint64_t i_end, uint64_t best) {
    if (best < bound) {
        uint8_t sec[DPOW_MAX_SECRET];
        size_t len = 0;
        dpow_secret_from_index(best, sec, &len);
        return dpow_verify(nonce, nonce_len, sec, len, ntz) ? Settled::kFound : Settled::kVerifyFailed;
    }
    return cur >= i_end || global_of_local(cur, rbits, base_tb) >= bound ? Settled::kExhausted : Settled::kLive;
}

// The result fields of a task found at global index `hit`.
inline void engine_write_hit(uint64_t hit, uint8_t secret[DPOW_MAX_SECRET], uint32_t &secret_len,
                             uint64_t &global_idx) {
    size_t len = 0;
    dpow_secret_from_index(hit, secret, &len);
    secret_len = (uint32_t)len;
    global_idx = hit;
}

#pragma GCC visibility pop

}  // namespace dpow
