// scan_dev.cpp -- host side of the device scan: dpow_scan_device's slice loop over the kernels of
// md5_scan_dev.hip on the launch engine (batch_engine.h), and the host helper dpow_scan_device_cut.
//
// Slices.  The window goes up in slices of up to kBatchCap local indices, in index order.  A slice
// is one mask launch, whose completion record the host waits for, and -- when the slice has hits --
// one place launch and, when depths were asked for, the digest kernel (md5_digest.hip) over the
// entries just placed, both queued behind it without a wait.  The host touches no hit: after the
// mask launch it reads the slice's total from pinned memory and, if the total fits the room left,
// queues the place launch for the whole slice; if not -- once per call at most, as the call ends
// there -- it copies the slice's prefix out, decides how many leading workgroups' hits fit
// (dpow_scan_device_cut) and queues the place launch for those.
// A workgroup's range is a multiple of 256 local indices, so a cut is a k boundary in every
// partition and a k's hits are never split.  The cancel flag is checked between slices.
//
// Verification.  Re-hashing every entry on the host would cost what the call saves (digests.cpp).
// The depths come from the digest kernel, an independent gather that re-hashes every placed entry;
// scan_check_kernel then counts, over the whole list, the entries shallower than ntz and those not
// strictly above their predecessor, and gathers 16 samples that the host recomputes with its own
// MD5.  A non-zero count or a failed sample is DPOW_EVERIFY.  The function returns after the stream
// has drained, so the outputs are complete on return.
#include "scan_dev.h"

#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/dpow_worker.h"
#include "batch.h"
#include "batch_engine.h"
#include "ctx.h"
#include "md5_digest.h"
#include "md5_host.h"
#include "md5_scan_dev.h"

namespace dpow {

static_assert(kScanDevSlice == kBatchCap && kScanDevMaxGroup == kBatchMaxGroup, "a slice is one engine launch");
static_assert(DPOW_SCAN_DEVICE_MIN_HITS == kScanDevMaxGroup, "room for the hits of one workgroup");

// The context's buffers.  Device: the totals and their prefix in the engine's image area, the control
// words behind it (batch_engine.h) with the check word at +16 and the digest kernel's out-of-range
// count at +20, then the bitmap.  Pinned: room for the prefix's copy, the slice's total, the record,
// the two words' copies, the samples.
struct ScanDevState {
    EngineBuffers buf;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // around a slice's place launch and its depth launches
    double ms[3] = {0.0, 0.0, 0.0};                  // the last call's mask, place and depth time
};

namespace {

constexpr size_t kTotalsOff = 0;  // d_mem
constexpr size_t kPrefixOff = kTotalsOff + kScanDevMaxBlocks * sizeof(uint32_t);
static_assert(kPrefixOff + kScanDevMaxBlocks * sizeof(uint32_t) <= kEngineImageBytes, "both fit the image area");
constexpr size_t kCheckOff = kEngineCtlOff + 16;  // the check word, then the digest kernel's count
constexpr size_t kMaskOff = kEngineDevBytes;
static_assert(kMaskOff % 8 == 0, "the bitmap's words are 8-byte aligned");
constexpr size_t kDevBytes = kMaskOff + kScanDevMaskBytes;
constexpr size_t kOutPrefixOff = 0;  // h_mem
constexpr size_t kOutTotalOff = kOutPrefixOff + kScanDevMaxBlocks * sizeof(uint32_t);
constexpr size_t kRecOff = kOutTotalOff + 64;
constexpr size_t kOutCheckOff = kRecOff + 64;
constexpr size_t kSamplesOff = kOutCheckOff + 64;
constexpr size_t kHostBytes = kSamplesOff + kScanDevSamples * sizeof(ScanDevSample);

int scan_dev_state(ScanDevState **state, hipStream_t stream) {
    if (*state) return 0;
    ScanDevState *s = new (std::nothrow) ScanDevState();
    if (!s) return set_error(DPOW_ENOMEM, "dpow_scan_device: out of memory");
    int rc = engine_alloc(s->buf, kDevBytes, kHostBytes, stream, scan_dev_prepare, "dpow_scan_device: allocation");
    if (rc == 0) {
        hipError_t e = digest_prepare();
        for (hipEvent_t &ev : s->ev)
            if (e == hipSuccess) e = hipEventCreate(&ev);
        if (e != hipSuccess) {
            rc = hip_fail(e, "dpow_scan_device: allocation");
            scan_dev_free(s);
            return rc;
        }
        *state = s;
    } else {
        delete s;
    }
    return rc;
}

}  // namespace

void scan_dev_free(ScanDevState *s) {
    if (!s) return;
    engine_free(s->buf);
    for (hipEvent_t ev : s->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete s;
}

void scan_dev_times(const ScanDevState *s, double *mask_ms, double *place_ms, double *depth_ms) {
    *mask_ms = s ? s->ms[0] : 0.0;
    *place_ms = s ? s->ms[1] : 0.0;
    *depth_ms = s ? s->ms[2] : 0.0;
}

// Leading workgroups whose hits fit `room`: the inclusive prefix is non-decreasing, so they are the
// entries that are at most `room`.
size_t scan_dev_cut(const uint32_t *inclusive_prefix, size_t n_groups, size_t room) {
    return (size_t)(std::upper_bound(inclusive_prefix, inclusive_prefix + n_groups, room,
                                     [](size_t r, uint32_t p) { return r < (size_t)p; }) -
                    inclusive_prefix);
}

int scan_dev_run(ScanDevState **state, hipStream_t stream, const volatile uint32_t *cancel, const uint8_t *nonce,
                 size_t nonce_len, uint32_t ntz, uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin,
                 uint64_t k_end, void *d_idx_out, void *d_tz_out, size_t max_hits, size_t *n_hits, uint64_t *k_done,
                 dpow_batch_stats *stats) {
    dpow_batch_stats st{};
    int rc = scan_dev_state(state, stream);
    if (rc < 0) return rc;
    ScanDevState &sd = **state;
    EngineBuffers &s = sd.buf;
    const EngineSections at{0, kOutPrefixOff, kRecOff};
    sd.ms[0] = sd.ms[1] = sd.ms[2] = 0.0;

    ScanMaskLaunch S{};
    batch_fill_task(S.task, nonce, nonce_len, ntz, worker_byte, worker_bits);
    const uint32_t rbits = S.task.rbits, base_tb = S.task.base_tb;
    S.mask = reinterpret_cast<unsigned long long *>(s.d_mem + kMaskOff);
    S.totals = reinterpret_cast<uint32_t *>(s.d_mem + kTotalsOff);
    S.prefix = reinterpret_cast<uint32_t *>(s.d_mem + kPrefixOff);
    S.out_total = reinterpret_cast<unsigned long long *>(s.d_h_mem + kOutTotalOff);
    const unsigned long long *const h_total = reinterpret_cast<const unsigned long long *>(s.h_mem + kOutTotalOff);
    uint32_t *const h_prefix = reinterpret_cast<uint32_t *>(s.h_mem + kOutPrefixOff);
    const auto issue = [&](const BatchLaunch &L) {
        S.L = L;
        const hipError_t e = scan_mask_launch(S, stream);
        return e == hipSuccess ? 0 : hip_fail(e, "dpow_scan_device: mask launch");
    };
    DigestLaunch D{};
    batch_fill_task(D.task, nonce, nonce_len, 0u, 0u, 0u);  // global indices are its local ones
    D.bad = reinterpret_cast<uint32_t *>(s.d_mem + kCheckOff) + 1;
    unsigned long long *const out = static_cast<unsigned long long *>(d_idx_out);
    uint8_t *const tz_out = static_cast<uint8_t *>(d_tz_out);

    // On an error nothing of ours stays queued behind the return.
    const auto fail = [&](int code) {
        (void)hipStreamSynchronize(stream);
        return code;
    };
    // The time of the slice whose place and depth launches lie between the events (they have
    // completed: a later launch's record was seen, or the stream has drained).
    bool timed = false;
    const auto collect = [&]() {
        float ms = 0.f;
        if (!timed) return;
        timed = false;
        if (hipEventElapsedTime(&ms, sd.ev[0], sd.ev[1]) == hipSuccess) sd.ms[1] += ms;
        else (void)hipGetLastError();
        if (hipEventElapsedTime(&ms, sd.ev[1], sd.ev[2]) == hipSuccess) sd.ms[2] += ms;
        else (void)hipGetLastError();
    };

    const uint64_t i_end = k_end << rbits;
    uint64_t i_cur = k_begin << rbits;
    size_t n_out = 0;
    int status = DPOW_EXHAUSTED;
    while (i_cur < i_end) {
        if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) {
            status = DPOW_CANCELLED;
            break;
        }
        const uint64_t lo = i_cur, hi = i_end - lo > kScanDevSlice ? lo + kScanDevSlice : i_end;
        S.i_begin = lo;
        S.i_end = hi;
        const uint32_t group = batch_group(hi - lo);
        const uint32_t n_blocks = (uint32_t)((hi - lo + group - 1) / group);
        if (n_blocks > kScanDevMaxBlocks) return fail(set_error(DPOW_EINVAL, "dpow_scan_device: slice geometry"));
        rc = engine_launch(s, at, 0u, group, n_blocks, stream,
                           "dpow_scan_device: stream idle without the launch's completion record", st, issue);
        if (rc < 0) return fail(rc);
        collect();
        st.candidates += hi - lo;
        const uint64_t total = *h_total;
        if (total > hi - lo)
            return fail(set_error(DPOW_EVERIFY, "dpow_scan_device: more hits counted than candidates hashed"));
        const size_t room = max_hits - n_out;
        uint32_t n_fit = n_blocks;
        size_t placed = (size_t)total;
        if (total > room) {  // the cut needs the prefix: once per call at most, as the call ends here
            hipError_t ce = hipMemcpyAsync(h_prefix, S.prefix, n_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
            if (ce == hipSuccess) ce = hipStreamSynchronize(stream);
            if (ce != hipSuccess) return fail(hip_fail(ce, "dpow_scan_device: copying the prefix"));
            if (h_prefix[n_blocks - 1] != total)
                return fail(set_error(DPOW_EVERIFY, "dpow_scan_device: the prefix does not end at the total"));
            n_fit = (uint32_t)scan_dev_cut(h_prefix, n_blocks, room);
            placed = n_fit ? h_prefix[n_fit - 1] : 0;
        }
        if (placed > room) return fail(set_error(DPOW_EVERIFY, "dpow_scan_device: a prefix that does not ascend"));
        if (placed) {
            ScanPlaceLaunch P{};
            P.mask = S.mask;
            P.prefix = S.prefix;
            P.out = out;
            P.base = n_out;
            P.max_hits = max_hits;
            P.i_begin = lo;
            P.i_end = hi;
            P.group = group;
            P.n_blocks = n_fit;
            P.rbits = rbits;
            P.base_tb = base_tb;
            hipError_t e = hipEventRecord(sd.ev[0], stream);
            if (e == hipSuccess) e = scan_place_launch(P, stream);
            if (e == hipSuccess) e = hipEventRecord(sd.ev[1], stream);
            if (e != hipSuccess) return fail(hip_fail(e, "dpow_scan_device: place launch"));
            st.launches++;
            // Depths: the digest kernel over the entries just placed, stream-ordered behind them.
            for (size_t first = 0; tz_out && first < placed; first += kDigestDeviceSlice) {
                const uint32_t count = (uint32_t)std::min<size_t>(kDigestDeviceSlice, placed - first);
                D.idx = out + n_out + first;
                D.digest = nullptr;
                D.tz = tz_out + n_out + first;
                D.n = count;
                D.group = batch_group(count);
                if ((e = digest_launch(D, (count + D.group - 1) / D.group, stream)) != hipSuccess)
                    return fail(hip_fail(e, "dpow_scan_device: depth launch"));
                st.launches++;
            }
            if ((e = hipEventRecord(sd.ev[2], stream)) != hipSuccess)
                return fail(hip_fail(e, "dpow_scan_device: place launch"));
            timed = true;
            n_out += placed;
        }
        if (n_fit < n_blocks) {  // the rest of the slice did not fit: the caller continues from this k
            i_cur = lo + (uint64_t)n_fit * group;
            status = DPOW_MORE;
            break;
        }
        i_cur = hi;
    }
    const uint64_t k_at = i_cur >> rbits;

    // The list's check, and the wait for everything queued.
    uint32_t *const d_check = reinterpret_cast<uint32_t *>(s.d_mem + kCheckOff);
    const uint32_t *const h_check = reinterpret_cast<const uint32_t *>(s.h_mem + kOutCheckOff);
    hipError_t e = hipSuccess;
    if (n_out) {
        ScanCheckLaunch C{};
        C.idx = out;
        C.tz = tz_out;
        C.n = n_out;
        C.ntz = ntz;
        C.bad = d_check;
        C.samples = reinterpret_cast<ScanDevSample *>(s.d_h_mem + kSamplesOff);
        if ((e = scan_check_launch(C, stream)) == hipSuccess) {
            st.launches++;
            e = hipMemcpyAsync(s.h_mem + kOutCheckOff, d_check, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        }
        if (e == hipSuccess) e = hipMemsetAsync(d_check, 0, 2 * sizeof(uint32_t), stream);  // zero for the next call
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(hip_fail(e, "dpow_scan_device: waiting for the launches"));
    collect();
    sd.ms[0] = st.kernel_ms;
    st.kernel_ms += sd.ms[1] + sd.ms[2];
    if (n_out) {
        if (h_check[0] != 0u)
            return set_error(DPOW_EVERIFY, "dpow_scan_device: entries out of order or shallower than asked for");
        if (h_check[1] != 0u) return set_error(DPOW_EVERIFY, "dpow_scan_device: an entry beyond DPOW_K_LIMIT");
        const ScanDevSample *const smp = reinterpret_cast<const ScanDevSample *>(s.h_mem + kSamplesOff);
        std::vector<uint8_t> msg(nonce_len + DPOW_MAX_SECRET);
        if (nonce_len) memcpy(msg.data(), nonce, nonce_len);
        for (uint32_t q = 0; q < kScanDevSamples; ++q) {
            const uint64_t g = smp[q].idx;
            uint64_t i;
            bool ok = local_of_global(g, rbits, base_tb, i) && (g >> 8) >= k_begin && (g >> 8) < k_at &&
                      (q == 0 || g >= smp[q - 1].idx);
            if (ok) {
                const uint32_t tz = md5_depth_of_index(msg.data(), nonce_len, g);
                ok = tz >= ntz && (!tz_out || smp[q].tz == tz);
            }
            if (!ok) return set_error(DPOW_EVERIFY, "dpow_scan_device: a sampled entry failed host MD5 verification");
        }
    }
    *n_hits = n_out;
    *k_done = k_at;
    if (stats) *stats = st;
    return status;
}

}  // namespace dpow

extern "C" size_t dpow_scan_device_cut(const uint32_t *inclusive_prefix, size_t n_groups, size_t room) {
    if (!inclusive_prefix) return 0;
    return dpow::scan_dev_cut(inclusive_prefix, n_groups, room);
}
