// digests.cpp -- host side of the digests: dpow_digests' chunk loop and dpow_digests_device's launch
// loop over the digest kernel (md5_digest.hip), and the pure host helper dpow_digest_of_index.
//
// Chunks.  The caller's list goes up in chunks of kDigestChunk entries, one launch per chunk, through
// two buffer sets used in turn: while chunk i hashes, the host moves chunk i + 1's indices into the
// other set and queues its launch behind chunk i, then waits for chunk i and moves its outputs to the
// caller's arrays.  Device and pinned memory are O(chunk) whatever n is.  The cancel flag is checked
// before each chunk is queued; a call never returns with a launch in flight.
// DPOW_DIAG_DIGEST_CHUNK=<256..kDigestChunk>, read per call, shrinks the chunk, which is how the
// chunk seams and the reuse of both sets are tested.
//
// Staging.  A buffer set is one block of pinned host memory mapped into the device (indices, digests,
// depth bytes).  "mapped": the kernel loads the indices from it and stores the outputs to it over the
// host link; the stores are visible to the host once the launch's event has completed.  "copy": the
// same block is the source and target of hipMemcpyAsync calls around a launch that works on device
// buffers.  DESIGN.md section 15 has both measured; DPOW_DIAG_DIGEST_STAGING=mapped|copy, read per
// call, overrides the choice (kDigestStagingMapped) for that comparison.
//
// Verification.  Re-hashing every entry on the host would cost what the call saves, so the host
// samples: of each chunk it recomputes the first entry, the last entry and 14 evenly spaced ones with
// dpow_digest_of_index's code and compares every output the caller asked for; a mismatch is
// DPOW_EVERIFY.  dpow_digests_device verifies nothing: its data never reaches the host.
#include "digests.h"
#include "digests_sets.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/dpow_worker.h"
#include "batch.h"
#include "batch_engine.h"
#include "ctx.h"
#include "md5_digest.h"
#include "md5_host.h"

namespace dpow {

namespace {

#ifndef DPOW_DIGEST_STAGING_MAPPED
#define DPOW_DIGEST_STAGING_MAPPED 1
#endif
constexpr bool kDigestStagingMapped = DPOW_DIGEST_STAGING_MAPPED != 0;
constexpr uint32_t kDigestSamples = 16;  // per chunk: the first, the last and 14 evenly spaced entries

}  // namespace

// The context's buffers.  Device: 64 control bytes, the out-of-range count (u32) at +0, zero between
// calls of the device variant.  Pinned: the count's copy.
struct DigestState {
    DigestSet set[2];
    char *d_ctl = nullptr;
    uint32_t *h_bad = nullptr;
    hipEvent_t start = nullptr, stop = nullptr;  // dpow_digests_device's launches
};

namespace {

void digest_state_free(DigestState *s) {
    for (DigestSet &b : s->set) {
        if (b.h_mem) (void)hipHostFree(b.h_mem);
        if (b.d_mem) (void)hipFree(b.d_mem);
        if (b.start) (void)hipEventDestroy(b.start);
        if (b.stop) (void)hipEventDestroy(b.stop);
        if (b.done) (void)hipEventDestroy(b.done);
    }
    if (s->d_ctl) (void)hipFree(s->d_ctl);
    if (s->h_bad) (void)hipHostFree(s->h_bad);
    if (s->start) (void)hipEventDestroy(s->start);
    if (s->stop) (void)hipEventDestroy(s->stop);
    delete s;
}

// The control words, the events and the kernel: what both entry points need.
int digest_state(DigestState **state, hipStream_t stream, const char *who) {
    if (*state) return 0;
    DigestState *s = new (std::nothrow) DigestState();
    if (!s) return set_error(DPOW_ENOMEM, std::string(who) + ": out of memory");
    hipError_t e;
    if ((e = hipMalloc(&s->d_ctl, 64)) != hipSuccess ||
        (e = hipHostMalloc(&s->h_bad, 64, hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess ||
        (e = hipEventCreate(&s->start)) != hipSuccess || (e = hipEventCreate(&s->stop)) != hipSuccess ||
        (e = hipMemsetAsync(s->d_ctl, 0, 64, stream)) != hipSuccess ||
        (e = hipStreamSynchronize(stream)) != hipSuccess || (e = digest_prepare()) != hipSuccess) {
        digest_state_free(s);
        return hip_fail(e, who);
    }
    *state = s;
    return 0;
}

// The two buffer sets of dpow_digests (the device variant needs none).
int digest_sets(DigestState &s, bool mapped) {
    hipError_t e = hipSuccess;
    for (DigestSet &b : s.set) {
        if (!b.h_mem &&
            ((e = hipHostMalloc(&b.h_mem, kDigestSetBytes, hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess ||
             (e = hipHostGetDevicePointer(reinterpret_cast<void **>(&b.d_h_mem), b.h_mem, 0)) != hipSuccess ||
             (e = hipEventCreate(&b.start)) != hipSuccess || (e = hipEventCreate(&b.stop)) != hipSuccess ||
             (e = hipEventCreateWithFlags(&b.done, hipEventDisableTiming)) != hipSuccess))
            break;
        if (!mapped && !b.d_mem && (e = hipMalloc(&b.d_mem, kDigestSetBytes)) != hipSuccess) break;
    }
    // (What was allocated stays with the state and is freed with the context.)
    return e == hipSuccess ? 0 : hip_fail(e, "dpow_digests: allocation");
}

}  // namespace

void digests_free(DigestState *s) {
    if (s) digest_state_free(s);
}

// DPOW_DIAG_DIGEST_CHUNK: the entries per chunk of this call.
uint32_t digest_chunk() {
    if (const char *v = getenv("DPOW_DIAG_DIGEST_CHUNK")) {
        const long c = atol(v);
        if (c >= (long)kDigestMinChunk && c <= (long)kDigestChunk) return (uint32_t)c;
    }
    return kDigestChunk;
}

// DPOW_DIAG_DIGEST_STAGING: this call's staging.
bool digest_staging_mapped() {
    if (const char *v = getenv("DPOW_DIAG_DIGEST_STAGING")) {
        if (!strcmp(v, "mapped")) return true;
        if (!strcmp(v, "copy")) return false;
    }
    return kDigestStagingMapped;
}

// Workgroups of a launch of `count` entries, `group` (a multiple of 256) each.
uint32_t digest_shape(uint32_t count, uint32_t &group) {
    group = batch_group(count);
    return (count + group - 1) / group;
}

int digests_staging(DigestState **state, hipStream_t stream, bool mapped, const char *who, DigestSet **sets) {
    int rc = digest_state(state, stream, who);
    if (rc < 0 || (rc = digest_sets(**state, mapped)) < 0) return rc;
    *sets = (*state)->set;
    return 0;
}

int digests_run(DigestState **state, hipStream_t stream, const volatile uint32_t *cancel, const uint8_t *nonce,
                size_t nonce_len, const uint64_t *global_idx, size_t n, uint8_t *digest_out, uint8_t *tz_out,
                size_t *n_done, dpow_batch_stats *stats) {
    dpow_batch_stats st{};
    const auto finish = [&](int code, size_t done) {
        *n_done = done;
        st.candidates = done;
        if (stats) *stats = st;
        return code;
    };
    int rc = digest_state(state, stream, "dpow_digests: allocation");
    if (rc < 0) return rc;
    DigestState &s = **state;
    const bool mapped = digest_staging_mapped();
    if ((rc = digest_sets(s, mapped)) < 0) return rc;
    const size_t chunk = digest_chunk();

    DigestLaunch D{};
    batch_fill_task(D.task, nonce, nonce_len, 0u, 0u, 0u);
    D.bad = reinterpret_cast<uint32_t *>(s.d_ctl);
    std::vector<uint8_t> msg(nonce_len + DPOW_MAX_SECRET);
    if (nonce_len) memcpy(msg.data(), nonce, nonce_len);

    // Chunk c covers entries [c * chunk, min(n, (c + 1) * chunk)) through set c % 2.
    const size_t n_chunks = (n + chunk - 1) / chunk;
    const auto count_of = [&](size_t c) { return (uint32_t)std::min(chunk, n - c * chunk); };
    const auto fill = [&](size_t c) {
        memcpy(s.set[c & 1].h_mem + kDigestIdxOff, global_idx + c * chunk, (size_t)count_of(c) * 8);
    };
    const auto issue = [&](size_t c) -> int {
        DigestSet &b = s.set[c & 1];
        const uint32_t count = count_of(c);
        char *const base = mapped ? b.d_h_mem : b.d_mem;
        D.idx = reinterpret_cast<const unsigned long long *>(base + kDigestIdxOff);
        D.digest = digest_out ? reinterpret_cast<uint4 *>(base + kDigestOutOff) : nullptr;
        D.tz = tz_out ? reinterpret_cast<uint8_t *>(base + kDigestTzOff) : nullptr;
        D.n = count;
        const uint32_t n_blocks = digest_shape(count, D.group);
        if (!mapped)
            DPOW_HIP(hipMemcpyAsync(b.d_mem + kDigestIdxOff, b.h_mem + kDigestIdxOff, (size_t)count * 8,
                                    hipMemcpyHostToDevice, stream));
        DPOW_HIP(hipEventRecord(b.start, stream));
        const hipError_t e = digest_launch(D, n_blocks, stream);
        if (e != hipSuccess) return hip_fail(e, "dpow_digests: launch");
        DPOW_HIP(hipEventRecord(b.stop, stream));
        if (!mapped) {
            if (digest_out)
                DPOW_HIP(hipMemcpyAsync(b.h_mem + kDigestOutOff, b.d_mem + kDigestOutOff, (size_t)count * 16,
                                        hipMemcpyDeviceToHost, stream));
            if (tz_out)
                DPOW_HIP(hipMemcpyAsync(b.h_mem + kDigestTzOff, b.d_mem + kDigestTzOff, count,
                                        hipMemcpyDeviceToHost, stream));
        }
        DPOW_HIP(hipEventRecord(b.done, stream));
        return 0;
    };
    // On an error nothing of ours stays queued behind the return.
    const auto fail = [&](int code) {
        (void)hipStreamSynchronize(stream);
        return code;
    };

    fill(0);
    if ((rc = issue(0)) < 0) return fail(rc);
    for (size_t c = 0; c < n_chunks; ++c) {
        DigestSet &b = s.set[c & 1];
        bool cancelled = false;
        if (c + 1 < n_chunks) {
            fill(c + 1);  // (set (c + 1) % 2 was drained when chunk c - 1 ended)
            cancelled = __atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u;
            if (!cancelled && (rc = issue(c + 1)) < 0) return fail(rc);
        }
        hipError_t e = hipEventSynchronize(b.done);
        if (e != hipSuccess) return fail(hip_fail(e, "dpow_digests: waiting for a chunk"));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, b.start, b.stop) == hipSuccess) st.kernel_ms += ms;
        else (void)hipGetLastError();
        st.launches++;
        st.rounds++;
        const size_t first = c * chunk;
        const uint32_t count = count_of(c);
        const uint8_t *const h_digest = reinterpret_cast<const uint8_t *>(b.h_mem + kDigestOutOff);
        const uint8_t *const h_tz = reinterpret_cast<const uint8_t *>(b.h_mem + kDigestTzOff);
        for (uint32_t q = 0; q < kDigestSamples; ++q) {
            const size_t j = (size_t)(count - 1) * q / (kDigestSamples - 1);
            uint8_t d[16];
            const uint32_t tz = md5_depth_of_index(msg.data(), nonce_len, global_idx[first + j], d);
            if ((digest_out && memcmp(h_digest + 16 * j, d, 16) != 0) || (tz_out && h_tz[j] != tz))
                return fail(set_error(DPOW_EVERIFY, "dpow_digests: a sampled entry failed host MD5 verification"));
        }
        if (digest_out) memcpy(digest_out + 16 * first, h_digest, (size_t)count * 16);
        if (tz_out) memcpy(tz_out + first, h_tz, count);
        if (cancelled) return finish(DPOW_CANCELLED, first + count);
    }
    return finish(DPOW_EXHAUSTED, n);
}

int digests_run_device(DigestState **state, hipStream_t stream, const uint8_t *nonce, size_t nonce_len,
                       const void *d_global_idx, size_t n, void *d_digest_out, void *d_tz_out,
                       dpow_batch_stats *stats) {
    dpow_batch_stats st{};
    int rc = digest_state(state, stream, "dpow_digests_device: allocation");
    if (rc < 0) return rc;
    DigestState &s = **state;
    DigestLaunch D{};
    batch_fill_task(D.task, nonce, nonce_len, 0u, 0u, 0u);
    D.bad = reinterpret_cast<uint32_t *>(s.d_ctl);
    // One bounded launch per kDigestDeviceSlice entries, back to back on the stream; the count of
    // out-of-range entries is read once, behind the last one.
    DPOW_HIP(hipEventRecord(s.start, stream));
    for (size_t first = 0; first < n; first += kDigestDeviceSlice) {
        const uint32_t count = (uint32_t)std::min<size_t>(kDigestDeviceSlice, n - first);
        D.idx = static_cast<const unsigned long long *>(d_global_idx) + first;
        D.digest = d_digest_out ? static_cast<uint4 *>(d_digest_out) + first : nullptr;
        D.tz = d_tz_out ? static_cast<uint8_t *>(d_tz_out) + first : nullptr;
        D.n = count;
        const uint32_t n_blocks = digest_shape(count, D.group);
        const hipError_t e = digest_launch(D, n_blocks, stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(stream);
            return hip_fail(e, "dpow_digests_device: launch");
        }
        st.launches++;
        st.rounds++;
    }
    hipError_t e;
    if ((e = hipEventRecord(s.stop, stream)) != hipSuccess ||
        (e = hipMemcpyAsync(s.h_bad, s.d_ctl, sizeof(uint32_t), hipMemcpyDeviceToHost, stream)) != hipSuccess ||
        (e = hipMemsetAsync(s.d_ctl, 0, 64, stream)) != hipSuccess ||  // zero for the next call
        (e = hipStreamSynchronize(stream)) != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        return hip_fail(e, "dpow_digests_device: waiting for the launches");
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.start, s.stop) == hipSuccess) st.kernel_ms = ms;
    else (void)hipGetLastError();
    st.candidates = n;
    if (stats) *stats = st;
    if (*s.h_bad != 0u) return set_error(DPOW_ERANGE, "dpow_digests_device: an entry beyond DPOW_K_LIMIT");
    return DPOW_EXHAUSTED;
}

}  // namespace dpow

extern "C" int dpow_digest_of_index(const uint8_t *nonce, size_t nonce_len, uint64_t global_idx,
                                    uint8_t digest_out[16], uint32_t *tz_out) {
    if (nonce_len && !nonce) return dpow::set_error(DPOW_EINVAL, "dpow_digest_of_index: nonce is NULL");
    if (!digest_out && !tz_out) return dpow::set_error(DPOW_EINVAL, "dpow_digest_of_index: both outputs are NULL");
    if ((global_idx >> 8) >= DPOW_K_LIMIT)
        return dpow::set_error(DPOW_ERANGE, "dpow_digest_of_index: index beyond DPOW_K_LIMIT");
    uint8_t stack[256 + DPOW_MAX_SECRET];
    std::vector<uint8_t> heap;
    uint8_t *msg = stack;
    if (nonce_len > 256) {
        heap.resize(nonce_len + DPOW_MAX_SECRET);
        msg = heap.data();
    }
    if (nonce_len) memcpy(msg, nonce, nonce_len);
    uint8_t d[16];
    const uint32_t tz = dpow::md5_depth_of_index(msg, nonce_len, global_idx, d);
    if (digest_out) memcpy(digest_out, d, 16);
    if (tz_out) *tz_out = tz;
    return 0;
}
