// batch_engine.cpp -- the launch engine of the batched search and the task queue (batch_engine.h).
#include "batch_engine.h"

#include <string.h>
#include <time.h>

#include <string>

#include "../../include/dpow_worker.h"
#include "md5_host.h"
#include "plan.h"

namespace dpow {

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

int batch_check_task(const dpow_batch_task &t, const char *who) {
    const std::string w(who);
    if (t.nonce_len && !t.nonce) return set_error(DPOW_EINVAL, w + ": nonce is NULL");
    if (t.nonce_len > DPOW_MAX_NONCE) return set_error(DPOW_EINVAL, w + ": nonce longer than DPOW_MAX_NONCE");
    if (t.worker_byte > 255u) return set_error(DPOW_EINVAL, w + ": worker_byte > 255");
    if (t.k_begin > t.k_end) return set_error(DPOW_EINVAL, w + ": k_begin > k_end");
    if (t.k_end > DPOW_K_LIMIT) return set_error(DPOW_ERANGE, w + ": k_end beyond DPOW_K_LIMIT");
    return 0;
}

int engine_alloc(EngineBuffers &b, size_t dev_bytes, size_t host_bytes, hipStream_t stream, hipError_t (*prepare)(),
                 const char *who) {
    hipError_t e;
    if ((e = hipMalloc(&b.d_mem, dev_bytes)) != hipSuccess ||
        (e = hipHostMalloc(&b.h_mem, host_bytes, hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void **>(&b.d_h_mem), b.h_mem, 0)) != hipSuccess ||
        (e = hipMemsetAsync(b.d_mem + kEngineCtlOff, 0, 64, stream)) != hipSuccess ||
        (e = hipStreamSynchronize(stream)) != hipSuccess || (e = prepare()) != hipSuccess) {
        engine_free(b);
        return hip_fail(e, who);
    }
    memset(b.h_mem, 0, host_bytes);
    return 0;
}

void engine_free(EngineBuffers &b) {
    if (b.d_mem) (void)hipFree(b.d_mem);
    if (b.h_mem) (void)hipHostFree(b.h_mem);
    b = EngineBuffers{};
}

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

}  // namespace dpow
