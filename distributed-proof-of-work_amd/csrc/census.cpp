// census.cpp -- host side of the census: dpow_census_window's launch loop over the census kernel
// (md5_census.hip) on the launch engine (batch_engine.h), and the pure host fold dpow_census_merge.
//
// Launches.  The window goes up in index order, kBatchCap local indices per launch except the
// last, one bounded launch in flight at a time; the cancel flag is checked between launches.  A
// launch's answer is 33 counts and 33 indices whatever the density, so there is no slice rule and
// no re-run path, and the host's work per launch is O(33): it checks the launch's table (below),
// recomputes each distinct first index with the host MD5 -- which is where first_tz comes from --
// and folds the launch into the caller's census with the code of dpow_census_merge.  Depth 0 (the
// launch's size and its first candidate) is the host's own.
#include "census.h"

#include <string.h>

#include <string>
#include <vector>

#include "../../include/dpow_worker.h"
#include "batch.h"
#include "batch_engine.h"
#include "ctx.h"
#include "md5_census.h"
#include "md5_host.h"

namespace dpow {

static_assert(kCensusDepths == DPOW_CENSUS_DEPTHS, "the kernel's table and the ABI's struct have the same depths");

void census_clear(dpow_census &c) {
    memset(&c, 0, sizeof c);
    for (uint32_t d = 0; d < kCensusDepths; ++d) c.first_ge[d] = DPOW_NO_HIT;
}

namespace {

// Self-consistent (include/dpow.h): counts do not increase with d, a count is non-zero exactly
// where its first is set, the set firsts do not decrease with d, first_tz[d] >= d where set, and
// deepest is the largest d with a non-zero count (0 of an empty census).
bool census_consistent(const dpow_census &c) {
    uint32_t deepest = 0;
    for (uint32_t d = 0; d < kCensusDepths; ++d) {
        const bool set = c.first_ge[d] != DPOW_NO_HIT;
        if ((c.count_ge[d] > 0) != set) return false;
        if (d > 0 && c.count_ge[d] > c.count_ge[d - 1]) return false;
        if (!set) continue;
        if (d > 0 && c.first_ge[d] < c.first_ge[d - 1]) return false;  // (d - 1 is set: its count is no smaller)
        if (c.first_tz[d] < d) return false;
        deepest = d;
    }
    return c.deepest == deepest;
}

// dpow_census_merge on references: `next` is the census of a window wholly above `into`'s.
bool census_merge(dpow_census &into, const dpow_census &next) {
    if (!census_consistent(into) || !census_consistent(next)) return false;
    // The set firsts go up with d: next's lowest is its first_ge[0], into's highest its first_ge[deepest].
    if (next.count_ge[0] > 0 && into.count_ge[0] > 0 && next.first_ge[0] <= into.first_ge[into.deepest]) return false;
    for (uint32_t d = 0; d < kCensusDepths; ++d) {
        into.count_ge[d] += next.count_ge[d];
        if (into.first_ge[d] == DPOW_NO_HIT) {
            into.first_ge[d] = next.first_ge[d];
            into.first_tz[d] = next.first_tz[d];
        }
    }
    if (next.deepest > into.deepest) into.deepest = next.deepest;
    return true;
}

}  // namespace

// One launch's table folded into `into`: the launch covered the local indices [lo, hi) of a task
// with partition (rbits, base_tb); cnt and first are its 33 counts and 33 indices as the kernel left
// them in pinned memory.  Depth 0 (the launch's size and its first candidate) is the host's own.
// The table is checked -- no more counted than hashed, every first index a candidate of this
// launch's range and partition -- each distinct first index is recomputed with the host MD5, which
// is where first_tz comes from, and the launch is folded with the code of dpow_census_merge.  `msg`
// holds the task's nonce (nonce_len bytes) in front of DPOW_MAX_SECRET free bytes.  0, or
// DPOW_EVERIFY with "`who`: ..." set.
int census_fold_launch(const char *who, uint8_t *msg, size_t nonce_len, uint32_t rbits, uint32_t base_tb, uint64_t lo,
                       uint64_t hi, const unsigned long long *cnt, const unsigned long long *first, dpow_census &into) {
    const std::string w(who);
    dpow_census one;
    census_clear(one);
    one.count_ge[0] = hi - lo;
    one.first_ge[0] = global_of_local(lo, rbits, base_tb);
    for (uint32_t d = 1; d < kCensusDepths; ++d) {
        one.count_ge[d] = cnt[d];
        one.first_ge[d] = first[d];
    }
    if (one.count_ge[1] > hi - lo) return set_error(DPOW_EVERIFY, w + ": more candidates counted than hashed");
    for (uint32_t d = 0; d < kCensusDepths; ++d) {
        const uint64_t g = one.first_ge[d];
        if (g == DPOW_NO_HIT) continue;
        // The index is a candidate of this launch's range and partition.
        uint64_t i;
        if (!local_of_global(g, rbits, base_tb, i) || i < lo || i >= hi)
            return set_error(DPOW_EVERIFY, w + ": kernel index outside its launch");
        if (d > 0 && g == one.first_ge[d - 1]) {
            one.first_tz[d] = one.first_tz[d - 1];
        } else {
            one.first_tz[d] = md5_depth_of_index(msg, nonce_len, g);
        }
        if (one.first_tz[d] < d) return set_error(DPOW_EVERIFY, w + ": kernel index failed host MD5 verification");
        one.deepest = d;
    }
    // (census_merge checks both sides: the launch's table is self-consistent, or it is refused.)
    if (!census_merge(into, one))
        return set_error(DPOW_EVERIFY, w + ": the launch's counts and indices contradict each other");
    return 0;
}

// The context's buffers.  Device: the launch's table (cnt[33], first[33]) in the engine's image
// area, the control words behind it (batch_engine.h).  Pinned: the table's copy, the record.
struct CensusState {
    EngineBuffers buf;
};

namespace {

constexpr size_t kCensusTableBytes = 2 * kCensusDepths * sizeof(unsigned long long);
static_assert(kCensusTableBytes <= kEngineImageBytes, "the table fits the image area");
constexpr size_t kCensusOutOff = 0;  // h_mem
constexpr size_t kCensusRecOff = (kCensusOutOff + kCensusTableBytes + 63) & ~(size_t)63;
constexpr size_t kCensusHostBytes = kCensusRecOff + 64;

int census_state(CensusState **state, hipStream_t stream) {
    if (*state) return 0;
    CensusState *s = new (std::nothrow) CensusState();
    if (!s) return set_error(DPOW_ENOMEM, "dpow_census_window: out of memory");
    int rc = engine_alloc(s->buf, kEngineDevBytes, kCensusHostBytes, stream, census_prepare,
                          "dpow_census_window: allocation");
    if (rc == 0) {
        // The table as a launch expects it (its last workgroup leaves it so): counts 0, firsts none.
        // Staged in the pinned copy and sent on the context's own stream.
        unsigned long long *const h = reinterpret_cast<unsigned long long *>(s->buf.h_mem + kCensusOutOff);
        for (uint32_t q = 0; q < 2 * kCensusDepths; ++q) h[q] = q < kCensusDepths ? 0ull : kNoHit;
        hipError_t e;
        if ((e = hipMemcpyAsync(s->buf.d_mem, h, kCensusTableBytes, hipMemcpyHostToDevice, stream)) != hipSuccess ||
            (e = hipStreamSynchronize(stream)) != hipSuccess) {
            engine_free(s->buf);
            rc = hip_fail(e, "dpow_census_window: allocation");
        } else {
            memset(h, 0, kCensusTableBytes);
        }
    }
    if (rc < 0) delete s;
    else *state = s;
    return rc;
}

}  // namespace

void census_free(CensusState *s) {
    if (!s) return;
    engine_free(s->buf);
    delete s;
}

int census_run(CensusState **state, hipStream_t stream, const volatile uint32_t *cancel, const uint8_t *nonce,
               size_t nonce_len, uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin, uint64_t k_end,
               dpow_census *out, uint64_t *k_done, dpow_batch_stats *stats) {
    dpow_batch_stats st{};
    const auto finish = [&](int code, uint64_t k) {
        *k_done = k;
        if (stats) *stats = st;
        return code;
    };
    int rc = census_state(state, stream);
    if (rc < 0) return rc;
    EngineBuffers &s = (*state)->buf;
    const EngineSections at{0, kCensusOutOff, kCensusRecOff};

    CensusLaunch C{};
    batch_fill_task(C.task, nonce, nonce_len, 0u, worker_byte, worker_bits);
    const uint32_t rbits = C.task.rbits, base_tb = C.task.base_tb;
    const unsigned long long *const h_cnt = reinterpret_cast<const unsigned long long *>(s.h_mem + kCensusOutOff);
    const unsigned long long *const h_first = h_cnt + kCensusDepths;
    const auto issue = [&](const BatchLaunch &L) {
        C.L = L;
        const hipError_t e = census_launch(C, stream);
        return e == hipSuccess ? 0 : hip_fail(e, "dpow_census_window: launch");
    };

    const uint64_t i_end = k_end << rbits;
    std::vector<uint8_t> msg(nonce_len + DPOW_MAX_SECRET);
    if (nonce_len) memcpy(msg.data(), nonce, nonce_len);
    for (uint64_t lo = k_begin << rbits; lo < i_end;) {
        if (__atomic_load_n(cancel, __ATOMIC_ACQUIRE) != 0u) return finish(DPOW_CANCELLED, lo >> rbits);
        const uint64_t hi = i_end - lo > kBatchCap ? lo + kBatchCap : i_end;
        C.i_begin = lo;
        C.i_end = hi;
        const uint32_t group = batch_group(hi - lo);
        rc = engine_launch(s, at, 0u, group, (uint32_t)((hi - lo + group - 1) / group), stream,
                           "dpow_census_window: stream idle without the launch's completion record", st, issue);
        if (rc < 0) return rc;
        st.candidates += hi - lo;

        rc = census_fold_launch("dpow_census_window", msg.data(), nonce_len, rbits, base_tb, lo, hi, h_cnt, h_first, *out);
        if (rc < 0) return rc;
        lo = hi;
    }
    return finish(DPOW_EXHAUSTED, k_end);
}

}  // namespace dpow

extern "C" int dpow_census_merge(dpow_census *into, const dpow_census *next) {
    if (!into || !next) return dpow::set_error(DPOW_EINVAL, "dpow_census_merge: NULL argument");
    if (!dpow::census_merge(*into, *next))
        return dpow::set_error(DPOW_EINVAL, "dpow_census_merge: a census is not self-consistent, or next is not above into");
    return 0;
}
