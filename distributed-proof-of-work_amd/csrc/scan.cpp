// scan.cpp -- host side of the scan: dpow_scan's slice loop over the scan kernel (md5_scan.hip) on
// the launch engine (batch_engine.h), the slice rule and the host helper dpow_scan_slice.
//
// Slices.  The window goes up in slices of local indices, in index order, one bounded launch per
// slice.  A slice is a multiple of 256 local indices, so its ends are k boundaries in every
// partition (a k has 256 >> worker_bits local indices).  After each launch the host sorts the
// slice's entries (the device appends them in no order), recomputes each with the host MD5 -- which
// is where a hit's depth comes from -- appends them to the caller's array whole k by whole k, and
// checks the cancel flag.  One launch is in flight at a time, so a return leaves nothing queued.
//
// Overflow.  A launch whose count exceeds its list's capacity is discarded and its range re-run in
// halves, down to 256 candidates, which cannot overflow a list of at least 256 entries.  The slice
// rule (scan_slice) puts that out of reach of an honest digest; DPOW_DIAG_SCAN_CAP=<256..65536>,
// read per call, shrinks the capacity without changing the slice rule, which is how the path is
// tested.
#include "scan.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/dpow_worker.h"
#include "batch.h"
#include "batch_engine.h"
#include "ctx.h"
#include "md5_host.h"
#include "md5_scan.h"

namespace dpow {

// Expected hits of a slice are slice / 16^ntz for uniform digests.  The rule keeps them at a quarter
// of the capacity C: slice = (C / 4) * 16^min(ntz, 32), at most kBatchCap (the cancel latency of
// DESIGN.md section 11), at least 256.  For ntz = 0 every candidate hits and the slice holds C / 4
// of them exactly.  For ntz >= 1 the hits of a slice are binomial with mean m <= C / 4, and an
// overflow needs more than 4 m of them: by the Chernoff bound P(X >= 4 m) <= (e^3 / 4^4)^m
// < 0.079^m, and the rule is only tight where m = C / 4 = 16384 (a smaller m at the kBatchCap
// clamp leaves a factor above 4): below 10^-18000 per launch.
uint64_t scan_slice(uint32_t ntz, uint32_t capacity) {
    uint64_t slice = capacity / 4u;
    for (uint32_t e = std::min(ntz, 32u); e > 0u && slice < kBatchCap; --e) slice *= 16u;
    slice = std::min(slice, kBatchCap) & ~255ull;
    return std::max<uint64_t>(slice, 256u);
}

bool scan_fill_hit(uint8_t *msg, size_t nonce_len, uint64_t g, uint32_t ntz, dpow_scan_hit &h) {
    size_t len = 0;
    h.tz = md5_depth_of_index(msg, nonce_len, g, nullptr, &len);
    memcpy(h.secret, msg + nonce_len, len);
    memset(h.secret + len, 0, DPOW_MAX_SECRET - len);
    if (h.tz < ntz) return false;
    h.global_idx = g;
    h.secret_len = (uint32_t)len;
    return true;
}

// The context's buffers.  Device: the hit list in the engine's image area, the control words behind
// it (batch_engine.h) with the launch's hit count at +16.  Pinned: the list's copy, the count, the
// record.
struct ScanState {
    EngineBuffers buf;
};

namespace {

static_assert(kScanCap * sizeof(unsigned long long) <= kEngineImageBytes, "the hit list fits the image area");
constexpr size_t kScanCountOff = kEngineCtlOff + 16;  // d_mem
constexpr size_t kScanOutOff = 0;                     // h_mem
constexpr size_t kScanOutCountOff = kScanOutOff + kScanCap * sizeof(unsigned long long);
constexpr size_t kScanRecOff = kScanOutCountOff + 64;
constexpr size_t kScanHostBytes = kScanRecOff + 64;

int scan_state(ScanState **state, hipStream_t stream) {
    if (*state) return 0;
    ScanState *s = new (std::nothrow) ScanState();
    if (!s) return set_error(DPOW_ENOMEM, "dpow_scan: out of memory");
    const int rc = engine_alloc(s->buf, kEngineDevBytes, kScanHostBytes, stream, scan_prepare, "dpow_scan: allocation");
    if (rc < 0) delete s;
    else *state = s;
    return rc;
}

// DPOW_DIAG_SCAN_CAP: the capacity of this call's hit lists (the slice rule stays kScanCap's).
uint32_t scan_capacity() {
    if (const char *v = getenv("DPOW_DIAG_SCAN_CAP")) {
        const long c = atol(v);
        if (c >= (long)kScanMinCap && c <= (long)kScanCap) return (uint32_t)c;
    }
    return kScanCap;
}

}  // namespace

void scan_free(ScanState *s) {
    if (!s) return;
    engine_free(s->buf);
    delete s;
}

int scan_run(ScanState **state, hipStream_t stream, const volatile uint32_t *cancel, const uint8_t *nonce,
             size_t nonce_len, uint32_t ntz, uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin,
             uint64_t k_end, dpow_scan_hit *out, size_t max_hits, size_t *n_hits, uint64_t *k_done,
             dpow_batch_stats *stats) {
    dpow_batch_stats st{};
    size_t n_out = 0;
    const auto finish = [&](int code, uint64_t k) {
        *n_hits = n_out;
        *k_done = k;
        if (stats) *stats = st;
        return code;
    };
    int rc = scan_state(state, stream);
    if (rc < 0) return rc;
    EngineBuffers &s = (*state)->buf;
    const EngineSections at{0, kScanOutOff, kScanRecOff};

    ScanLaunch S{};
    batch_fill_task(S.task, nonce, nonce_len, ntz, worker_byte, worker_bits);
    const uint32_t rbits = S.task.rbits, base_tb = S.task.base_tb;
    S.count = reinterpret_cast<uint32_t *>(s.d_mem + kScanCountOff);
    S.out_count = reinterpret_cast<unsigned long long *>(s.d_h_mem + kScanOutCountOff);
    S.capacity = scan_capacity();
    const unsigned long long *const h_out = reinterpret_cast<const unsigned long long *>(s.h_mem + kScanOutOff);
    const unsigned long long *const h_count =
        reinterpret_cast<const unsigned long long *>(s.h_mem + kScanOutCountOff);
    const auto issue = [&](const BatchLaunch &L) {
        S.L = L;
        const hipError_t e = scan_launch(S, stream);
        return e == hipSuccess ? 0 : hip_fail(e, "dpow_scan: launch");
    };

    const uint64_t slice = scan_slice(ntz, kScanCap);
    const uint64_t i_end = k_end << rbits;
    uint64_t i_cur = k_begin << rbits;
    uint64_t slice_end = i_cur, step = slice;  // step: halved while an overflowed slice is re-run
    std::vector<uint64_t> hits;
    std::vector<uint8_t> msg(nonce_len + DPOW_MAX_SECRET);
    if (nonce_len) memcpy(msg.data(), nonce, nonce_len);
    while (i_cur < i_end) {
        if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) return finish(DPOW_CANCELLED, i_cur >> rbits);
        if (i_cur >= slice_end) {  // the next slice of the rule
            slice_end = i_end - i_cur > slice ? i_cur + slice : i_end;
            step = slice;
        }
        const uint64_t lo = i_cur, hi = slice_end - lo > step ? lo + step : slice_end;
        S.i_begin = lo;
        S.i_end = hi;
        const uint32_t group = batch_group(hi - lo);
        rc = engine_launch(s, at, 0u, group, (uint32_t)((hi - lo + group - 1) / group), stream,
                           "dpow_scan: stream idle without the launch's completion record", st, issue);
        if (rc < 0) return rc;
        st.candidates += hi - lo;
        const uint64_t count = *h_count;
        if (count > hi - lo) return set_error(DPOW_EVERIFY, "dpow_scan: more hits counted than candidates hashed");
        if (count > S.capacity) {  // the list is incomplete: discard it, re-run the range in halves
            step = std::max<uint64_t>(((hi - lo) / 2 + 255u) & ~255ull, 256u);
            continue;
        }
        hits.assign(h_out, h_out + count);
        std::sort(hits.begin(), hits.end());
        uint64_t prev_k = ~0ull;
        for (size_t j = 0; j < hits.size(); ++j) {
            const uint64_t g = hits[j];
            // The entry is a candidate of this launch, and no other entry is the same one.
            uint64_t i;
            if (!local_of_global(g, rbits, base_tb, i) || (g >> 8) >= k_end || i < lo || i >= hi ||
                (j > 0 && hits[j - 1] == g))
                return set_error(DPOW_EVERIFY, "dpow_scan: kernel entry outside its launch or listed twice");
            if ((g >> 8) != prev_k) {
                size_t n_k = 1;  // a k's hits are never split over two calls
                while (j + n_k < hits.size() && (hits[j + n_k] >> 8) == (g >> 8)) ++n_k;
                if (n_out + n_k > max_hits) return finish(DPOW_MORE, g >> 8);
                prev_k = g >> 8;
            }
            if (!scan_fill_hit(msg.data(), nonce_len, g, ntz, out[n_out]))
                return set_error(DPOW_EVERIFY, "dpow_scan: kernel hit failed host MD5 verification");
            ++n_out;
        }
        i_cur = hi;
    }
    return finish(DPOW_EXHAUSTED, k_end);
}

}  // namespace dpow

extern "C" uint64_t dpow_scan_slice(uint32_t ntz, uint32_t capacity) {
    const uint32_t c = std::min(std::max(capacity, dpow::kScanMinCap), dpow::kScanCap);
    return dpow::scan_slice(ntz, c);
}
