// digests_many.cpp -- host side of the digests of many nonces: dpow_digests_batch's chunk loop and
// dpow_digests_batch_device's launch loop over digest_many_kernel (md5_digest_many.hip), and the
// host helper dpow_digests_batch_walk.
//
// Both forms fill one task row per task (batch_fill_task with worker_bits = 0 and the task's ntz)
// in pinned memory and copy the table to the device with the upload kernel, as scan_many_dev.cpp
// does; the per-task shallow words and the two count words are zeroed on the stream per call and
// copied out behind the last launch.  Host work is O(tasks) + O(chunks or launches).
//
// Host form.  The rows go up once per call, behind the table.  The list goes up in dpow_digests'
// chunks through dpow_digests' two staging sets (digests_sets.h), chunk c's launch with
// e_base = c * chunk, so chunk seams fall wherever they fall in the tasks.  The cancel flag is
// checked before each chunk is queued; a call never returns with a launch in flight.  Of each chunk
// the host recomputes 16 samples, each with its own task's nonce, the task found by bisecting the
// rows; a mismatch with an output asked for is DPOW_EVERIFY.
//
// Device form.  The rows stay where the caller has them, unread by the host before the launches:
// one bounded launch per kDigestDeviceSlice entries, back to back, then the copies of the rows, the
// shallow words and the count words, and one stream drain.  It verifies nothing on the host.
#include "digests_many.h"

#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/dpow_worker.h"
#include "batch.h"
#include "batch_engine.h"
#include "ctx.h"
#include "digests_sets.h"
#include "md5_digest_many.h"
#include "md5_host.h"

namespace dpow {

namespace {

constexpr uint32_t kDigestManySamples = 16;  // per chunk: the first, the last and 14 evenly spaced entries

// Device: the task table, the rows (host form), then the count words ([0] out of range, [1]
// uncovered) with the tasks' shallow words behind them, zeroed and copied out as one block.  Pinned:
// the table and the rows of the running call, and the copies of the counts and the rows.
constexpr size_t kRowsBytes = ((size_t)(DPOW_BATCH_MAX + 1) * sizeof(uint64_t) + 63u) & ~(size_t)63u;
constexpr size_t kCountBytes = 64 + (size_t)DPOW_BATCH_MAX * sizeof(uint64_t);
constexpr size_t kTableOff = 0;  // d_mem and h_mem
constexpr size_t kRowsOff = kTableOff + (size_t)DPOW_BATCH_MAX * sizeof(BatchTask);
constexpr size_t kCountOff = kRowsOff + kRowsBytes;
constexpr size_t kDevBytes = kCountOff + kCountBytes;
constexpr size_t kOutRowsOff = kDevBytes;  // h_mem only
constexpr size_t kHostBytes = kOutRowsOff + kRowsBytes;
static_assert(kRowsOff % 8 == 0 && kCountOff % 8 == 0 && kOutRowsOff % 8 == 0, "aligned sections");

}  // namespace

struct DigestManyState {
    char *d_mem = nullptr;
    char *h_mem = nullptr;    // pinned, mapped
    char *d_h_mem = nullptr;  // device alias of h_mem
    hipEvent_t start = nullptr, stop = nullptr;  // dpow_digests_batch_device's launches
};

void digests_many_free(DigestManyState *s) {
    if (!s) return;
    if (s->d_mem) (void)hipFree(s->d_mem);
    if (s->h_mem) (void)hipHostFree(s->h_mem);
    if (s->start) (void)hipEventDestroy(s->start);
    if (s->stop) (void)hipEventDestroy(s->stop);
    delete s;
}

namespace {

int digests_many_state(DigestManyState **state, const char *who) {
    if (*state) return 0;
    DigestManyState *s = new (std::nothrow) DigestManyState();
    if (!s) return set_error(DPOW_ENOMEM, std::string(who) + ": out of memory");
    hipError_t e;
    if ((e = hipMalloc(&s->d_mem, kDevBytes)) != hipSuccess ||
        (e = hipHostMalloc(&s->h_mem, kHostBytes, hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void **>(&s->d_h_mem), s->h_mem, 0)) != hipSuccess ||
        (e = hipEventCreate(&s->start)) != hipSuccess || (e = hipEventCreate(&s->stop)) != hipSuccess ||
        (e = digest_many_prepare()) != hipSuccess || (e = batch_prepare()) != hipSuccess) {
        digests_many_free(s);
        return hip_fail(e, who);
    }
    *state = s;
    return 0;
}

int check_tasks(const dpow_digest_task *tasks, size_t n_tasks, const std::string &w) {
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX) return set_error(DPOW_EINVAL, w + ": n_tasks must be in [1, DPOW_BATCH_MAX]");
    for (size_t i = 0; i < n_tasks; ++i) {
        if (tasks[i].nonce_len && !tasks[i].nonce) return set_error(DPOW_EINVAL, w + ": nonce is NULL");
        if (tasks[i].nonce_len > DPOW_MAX_NONCE) return set_error(DPOW_EINVAL, w + ": nonce longer than DPOW_MAX_NONCE");
    }
    return 0;
}

// The task table of the call, and the zeroed counts: queued on the stream, nothing waited for.
int upload_table(DigestManyState &s, hipStream_t stream, const dpow_digest_task *tasks, size_t n, const char *who) {
    BatchTask *const h_table = reinterpret_cast<BatchTask *>(s.h_mem + kTableOff);
    for (size_t i = 0; i < n; ++i) batch_fill_task(h_table[i], tasks[i].nonce, tasks[i].nonce_len, tasks[i].ntz, 0u, 0u);
    hipError_t e = batch_upload(reinterpret_cast<uint32_t *>(s.d_mem + kTableOff),
                                reinterpret_cast<const uint32_t *>(s.d_h_mem + kTableOff),
                                (uint32_t)(n * sizeof(BatchTask) / 4), stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.d_mem + kCountOff, 0, 64 + n * sizeof(uint64_t), stream);
    return e == hipSuccess ? 0 : hip_fail(e, who);
}

DigestManyLaunch launch_base(DigestManyState &s, const void *d_rows, size_t n) {
    DigestManyLaunch D{};
    D.rows = static_cast<const unsigned long long *>(d_rows);
    D.ctl = reinterpret_cast<uint32_t *>(s.d_mem + kCountOff);
    D.shallow = reinterpret_cast<unsigned long long *>(s.d_mem + kCountOff + 64);
    D.n_tasks = (uint32_t)n;
    return D;
}

}  // namespace

int digests_many_check(const dpow_digest_task *tasks, size_t n_tasks, const uint64_t *rows, const uint64_t *global_idx,
                       const size_t *n_done) {
    const std::string w("dpow_digests_batch");
    if (!tasks || !rows || !global_idx || !n_done) return set_error(DPOW_EINVAL, w + ": NULL argument");
    const int rc = check_tasks(tasks, n_tasks, w);
    if (rc < 0) return rc;
    if (rows[0] != 0u) return set_error(DPOW_EINVAL, w + ": rows[0] is not 0");
    for (size_t i = 0; i < n_tasks; ++i)
        if (rows[i + 1] < rows[i]) return set_error(DPOW_EINVAL, w + ": a descending row");
    for (uint64_t j = 0; j < rows[n_tasks]; ++j)
        if ((global_idx[j] >> 8) >= DPOW_K_LIMIT) return set_error(DPOW_ERANGE, w + ": an entry beyond DPOW_K_LIMIT");
    return 0;
}

int digests_many_check_device(const dpow_digest_task *tasks, size_t n_tasks, const void *d_rows,
                              const void *d_global_idx, const void *d_digest_out) {
    const std::string w("dpow_digests_batch_device");
    if (!tasks || !d_rows || !d_global_idx) return set_error(DPOW_EINVAL, w + ": NULL argument");
    if ((reinterpret_cast<uintptr_t>(d_rows) & 7u) != 0u || (reinterpret_cast<uintptr_t>(d_global_idx) & 7u) != 0u ||
        (reinterpret_cast<uintptr_t>(d_digest_out) & 15u) != 0u)
        return set_error(DPOW_EINVAL, w + ": rows or indices not 8-byte or digests not 16-byte aligned");
    return check_tasks(tasks, n_tasks, w);
}

int digests_many_run(DigestManyState **state, DigestState **sets_state, hipStream_t stream,
                     const volatile uint32_t *cancel, dpow_digest_task *tasks, size_t n_tasks, const uint64_t *rows,
                     const uint64_t *global_idx, uint8_t *digest_out, uint8_t *tz_out, size_t *n_done,
                     dpow_batch_stats *stats) {
    const size_t n = (size_t)rows[n_tasks];
    dpow_batch_stats st{};
    int rc = digests_many_state(state, "dpow_digests_batch: allocation");
    if (rc < 0) return rc;
    DigestManyState &s = **state;
    const bool mapped = digest_staging_mapped();
    DigestSet *set = nullptr;
    if ((rc = digests_staging(sets_state, stream, mapped, "dpow_digests_batch: allocation", &set)) < 0) return rc;
    const size_t chunk = digest_chunk();

    // On an error nothing of ours stays queued behind the return.
    const auto fail = [&](int code) {
        (void)hipStreamSynchronize(stream);
        return code;
    };
    if ((rc = upload_table(s, stream, tasks, n_tasks, "dpow_digests_batch: upload")) < 0) return fail(rc);
    memcpy(s.h_mem + kRowsOff, rows, (n_tasks + 1) * sizeof(uint64_t));
    {
        const hipError_t e = batch_upload(reinterpret_cast<uint32_t *>(s.d_mem + kRowsOff),
                                          reinterpret_cast<const uint32_t *>(s.d_h_mem + kRowsOff),
                                          (uint32_t)((n_tasks + 1) * sizeof(uint64_t) / 4), stream);
        if (e != hipSuccess) return fail(hip_fail(e, "dpow_digests_batch: upload"));
    }
    DigestManyLaunch D = launch_base(s, s.d_mem + kRowsOff, n_tasks);

    // The counts behind the launches queued so far, which have completed: the tasks' n_shallow.
    const auto finish = [&](int code, size_t done) {
        const uint64_t *const h_count = reinterpret_cast<const uint64_t *>(s.h_mem + kCountOff);
        hipError_t e = hipMemcpyAsync(s.h_mem + kCountOff, s.d_mem + kCountOff, 64 + n_tasks * sizeof(uint64_t),
                                      hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return fail(hip_fail(e, "dpow_digests_batch: copying the counts"));
        if (h_count[0] != 0u)  // (the list's range was checked on entry, and the rows cover every entry)
            return set_error(DPOW_EVERIFY, "dpow_digests_batch: the kernel counted entries out of range or uncovered");
        for (size_t i = 0; i < n_tasks; ++i) tasks[i].n_shallow = h_count[8 + i];
        *n_done = done;
        st.candidates = done;
        if (stats) *stats = st;
        return code;
    };

    // Chunk c covers entries [c * chunk, min(n, (c + 1) * chunk)) through set c % 2.
    const size_t n_chunks = (n + chunk - 1) / chunk;
    const auto count_of = [&](size_t c) { return (uint32_t)std::min(chunk, n - c * chunk); };
    const auto fill = [&](size_t c) {
        memcpy(set[c & 1].h_mem + kDigestIdxOff, global_idx + c * chunk, (size_t)count_of(c) * 8);
    };
    const auto issue = [&](size_t c) -> int {
        DigestSet &b = set[c & 1];
        const uint32_t count = count_of(c);
        char *const base = mapped ? b.d_h_mem : b.d_mem;
        D.idx = reinterpret_cast<const unsigned long long *>(base + kDigestIdxOff);
        D.digest = digest_out ? reinterpret_cast<uint4 *>(base + kDigestOutOff) : nullptr;
        D.tz = tz_out ? reinterpret_cast<uint8_t *>(base + kDigestTzOff) : nullptr;
        D.e_base = c * chunk;
        D.n = count;
        const uint32_t n_blocks = digest_shape(count, D.group);
        if (!mapped)
            DPOW_HIP(hipMemcpyAsync(b.d_mem + kDigestIdxOff, b.h_mem + kDigestIdxOff, (size_t)count * 8,
                                    hipMemcpyHostToDevice, stream));
        DPOW_HIP(hipEventRecord(b.start, stream));
        const hipError_t e = digest_many_launch(reinterpret_cast<const BatchTask *>(s.d_mem + kTableOff), D, n_blocks, stream);
        if (e != hipSuccess) return hip_fail(e, "dpow_digests_batch: launch");
        DPOW_HIP(hipEventRecord(b.stop, stream));
        if (!mapped) {
            if (digest_out)
                DPOW_HIP(hipMemcpyAsync(b.h_mem + kDigestOutOff, b.d_mem + kDigestOutOff, (size_t)count * 16,
                                        hipMemcpyDeviceToHost, stream));
            if (tz_out)
                DPOW_HIP(hipMemcpyAsync(b.h_mem + kDigestTzOff, b.d_mem + kDigestTzOff, count, hipMemcpyDeviceToHost,
                                        stream));
        }
        DPOW_HIP(hipEventRecord(b.done, stream));
        return 0;
    };

    std::vector<uint8_t> msg;
    fill(0);
    if ((rc = issue(0)) < 0) return fail(rc);
    for (size_t c = 0; c < n_chunks; ++c) {
        DigestSet &b = set[c & 1];
        bool cancelled = false;
        if (c + 1 < n_chunks) {
            fill(c + 1);  // (set (c + 1) % 2 was drained when chunk c - 1 ended)
            cancelled = __atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u;
            if (!cancelled && (rc = issue(c + 1)) < 0) return fail(rc);
        }
        hipError_t e = hipEventSynchronize(b.done);
        if (e != hipSuccess) return fail(hip_fail(e, "dpow_digests_batch: waiting for a chunk"));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, b.start, b.stop) == hipSuccess) st.kernel_ms += ms;
        else (void)hipGetLastError();
        st.launches++;
        st.rounds++;
        const size_t first = c * chunk;
        const uint32_t count = count_of(c);
        const uint8_t *const h_digest = reinterpret_cast<const uint8_t *>(b.h_mem + kDigestOutOff);
        const uint8_t *const h_tz = reinterpret_cast<const uint8_t *>(b.h_mem + kDigestTzOff);
        for (uint32_t q = 0; (digest_out || tz_out) && q < kDigestManySamples; ++q) {
            const size_t j = (size_t)(count - 1) * q / (kDigestManySamples - 1);
            // The sample's task: the last row at most its position (the empty tasks there are skipped).
            const size_t t = (size_t)(std::upper_bound(rows, rows + n_tasks + 1, (uint64_t)(first + j)) - rows) - 1;
            uint8_t d[16];
            const uint32_t tz = md5_depth_of_index(md5_msg_of_nonce(msg, tasks[t].nonce, tasks[t].nonce_len),
                                                   tasks[t].nonce_len, global_idx[first + j], d);
            if ((digest_out && memcmp(h_digest + 16 * j, d, 16) != 0) || (tz_out && h_tz[j] != tz))
                return fail(set_error(DPOW_EVERIFY, "dpow_digests_batch: a sampled entry failed host MD5 verification"));
        }
        if (digest_out) memcpy(digest_out + 16 * first, h_digest, (size_t)count * 16);
        if (tz_out) memcpy(tz_out + first, h_tz, count);
        if (cancelled) return finish(DPOW_CANCELLED, first + count);
    }
    return finish(DPOW_EXHAUSTED, n);
}

int digests_many_run_device(DigestManyState **state, hipStream_t stream, dpow_digest_task *tasks, size_t n_tasks,
                            const void *d_rows, const void *d_global_idx, size_t n, void *d_digest_out,
                            void *d_tz_out, dpow_batch_stats *stats) {
    dpow_batch_stats st{};
    int rc = digests_many_state(state, "dpow_digests_batch_device: allocation");
    if (rc < 0) return rc;
    DigestManyState &s = **state;
    const auto fail = [&](int code) {
        (void)hipStreamSynchronize(stream);
        return code;
    };
    if ((rc = upload_table(s, stream, tasks, n_tasks, "dpow_digests_batch_device: upload")) < 0) return fail(rc);
    DigestManyLaunch D = launch_base(s, d_rows, n_tasks);
    // One bounded launch per kDigestDeviceSlice entries, back to back on the stream; the rows and
    // the counts are read once, behind the last one.
    hipError_t e = hipEventRecord(s.start, stream);
    for (size_t first = 0; e == hipSuccess && first < n; first += kDigestDeviceSlice) {
        const uint32_t count = (uint32_t)std::min<size_t>(kDigestDeviceSlice, n - first);
        D.idx = static_cast<const unsigned long long *>(d_global_idx) + first;
        D.digest = d_digest_out ? static_cast<uint4 *>(d_digest_out) + first : nullptr;
        D.tz = d_tz_out ? static_cast<uint8_t *>(d_tz_out) + first : nullptr;
        D.e_base = first;
        D.n = count;
        const uint32_t n_blocks = digest_shape(count, D.group);
        e = digest_many_launch(reinterpret_cast<const BatchTask *>(s.d_mem + kTableOff), D, n_blocks, stream);
        st.launches++;
        st.rounds++;
    }
    if (e != hipSuccess || (e = hipEventRecord(s.stop, stream)) != hipSuccess ||
        (e = hipMemcpyAsync(s.h_mem + kOutRowsOff, d_rows, (n_tasks + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                            stream)) != hipSuccess ||
        (e = hipMemcpyAsync(s.h_mem + kCountOff, s.d_mem + kCountOff, 64 + n_tasks * sizeof(uint64_t),
                            hipMemcpyDeviceToHost, stream)) != hipSuccess ||
        (e = hipStreamSynchronize(stream)) != hipSuccess)
        return fail(hip_fail(e, "dpow_digests_batch_device: the launches and the copies behind them"));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.start, s.stop) == hipSuccess) st.kernel_ms = ms;
    else (void)hipGetLastError();
    const uint64_t *const h_rows = reinterpret_cast<const uint64_t *>(s.h_mem + kOutRowsOff);
    const uint64_t *const h_count = reinterpret_cast<const uint64_t *>(s.h_mem + kCountOff);
    for (size_t i = 0; i < n_tasks; ++i) {
        tasks[i].n_entries = h_rows[i + 1] - h_rows[i];
        tasks[i].n_shallow = h_count[8 + i];
    }
    st.candidates = n;
    if (stats) *stats = st;
    const uint32_t *const h_ctl = reinterpret_cast<const uint32_t *>(s.h_mem + kCountOff);
    if (h_ctl[1] != 0u)
        return set_error(DPOW_EINVAL, "dpow_digests_batch_device: entries outside [rows[0], rows[n_tasks])");
    if (h_ctl[0] != 0u) return set_error(DPOW_ERANGE, "dpow_digests_batch_device: an entry beyond DPOW_K_LIMIT");
    return DPOW_EXHAUSTED;
}

}  // namespace dpow

using namespace dpow;

extern "C" int dpow_digests_batch_walk(const uint64_t *rows, size_t n_tasks, uint64_t e_first, uint64_t e_end,
                                       dpow_digest_pass *out, size_t max_passes) {
    if (!rows || (!out && max_passes)) return set_error(DPOW_EINVAL, "dpow_digests_batch_walk: NULL argument");
    if (n_tasks == 0 || n_tasks > DPOW_BATCH_MAX)
        return set_error(DPOW_EINVAL, "dpow_digests_batch_walk: n_tasks must be in [1, DPOW_BATCH_MAX]");
    if (e_end < e_first || e_end - e_first > 64u)
        return set_error(DPOW_EINVAL, "dpow_digests_batch_walk: a wave has at most 64 entries");
    size_t n = 0;
    digest_many_walk(reinterpret_cast<const unsigned long long *>(rows), (uint32_t)n_tasks, 0u, e_first, e_end,
                     [&](uint32_t t, uint64_t lo, uint64_t hi) {
                         if (n < max_passes) out[n] = dpow_digest_pass{lo, hi, t, 0u};
                         ++n;
                     });
    return (int)n;
}
