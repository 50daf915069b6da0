// md5_launch_ctl.h -- what a search kernel does beside hashing: the watcher workgroup, the claim
// counters, retirement and the completion record (publish), and the diagnostic wave trace.
#pragma once
#include "md5_kernel_tune.h"

namespace dpow {
namespace DPOW_KNS {

// The wave trace of DPOW_WAVE_TRACE builds (tools/wave_trace*.py, tools/search_timeline.py):
// every worker wave records kTraceFields words -- {start, first claim, exit} in s_memrealtime
// ticks (100 MHz), its hashed wave-blocks, the start of its last chunk and that chunk's claim
// index, why it left the claim loop (1 counters drained, 2 a chunk at or above the best, 3 stop,
// 4 left a chunk before its last group) and when it found a hit of its own (0: none).  Slot
// kTraceWaves - 1 is the watcher's: start, the first node best relayed, the first early-hit
// relay, exit.  Slot kTraceWaves - 2 is the publisher's retirement: its claims performed, its
// barrier passed, its count made, the record released.
// In every other build WaveTrace's members are empty, and so is every call of them.
constexpr uint32_t kTraceWaves = 8192;
constexpr uint32_t kTraceFields = 8;
#if DPOW_WAVE_TRACE
static __device__ unsigned long long g_wave_trace[kTraceWaves * kTraceFields];
#define DPOW_TRACED(...) { __VA_ARGS__ }
#else
#define DPOW_TRACED(...) {}
#endif
struct WaveTrace {
    unsigned long long t_start, t_first, n_wb, t_last, c_last, reason, t_hit, t_claims, t_bar;
    static DPOW_DEV unsigned long long now() { return __builtin_amdgcn_s_memrealtime(); }
    DPOW_DEV void start() DPOW_TRACED(t_start = now(); t_first = n_wb = t_last = c_last = reason = t_hit = 0;)
    DPOW_DEV void first_claim(uint64_t claim) DPOW_TRACED(t_first = now() + (claim & 0);)
    DPOW_DEV void chunk(uint64_t claim) DPOW_TRACED(t_last = now(); c_last = claim;)
    DPOW_DEV void wave_block() DPOW_TRACED(++n_wb;)
    DPOW_DEV void hit(bool h) DPOW_TRACED(if (h && t_hit == 0) t_hit = now();)
    DPOW_DEV void left(uint32_t why) DPOW_TRACED(reason = why;)
    DPOW_DEV void store(uint32_t lane) DPOW_TRACED(
        const uint32_t wave = (blockIdx.x - 1u) * (kBlockThreads / 64) + threadIdx.x / 64u;
        if (lane == 0 && wave < kTraceWaves) {
            unsigned long long *w = g_wave_trace + kTraceFields * wave;
            w[0] = t_start; w[1] = t_first; w[2] = now(); w[3] = n_wb;
            w[4] = t_last; w[5] = c_last; w[6] = reason; w[7] = t_hit;
        })
    DPOW_DEV void claims_performed() DPOW_TRACED(t_claims = now();)
    DPOW_DEV void barrier_passed() DPOW_TRACED(t_bar = now();)
    // prev: Ctrl::done before this workgroup's count of n
    DPOW_DEV void counted(const Launch &L, uint32_t prev, uint32_t n) DPOW_TRACED(
        if (prev + n == L.done_target) {
            unsigned long long *r = g_wave_trace + kTraceFields * (kTraceWaves - 2);
            r[0] = t_claims; r[1] = t_bar; r[2] = now() + (prev & 0);
        })
    static DPOW_DEV void released() DPOW_TRACED(g_wave_trace[kTraceFields * (kTraceWaves - 2) + 3] = now();)
    // the watcher's record: f = 0 start (clears 1, 2), 1 / 2 the first relay of its kind, 3 exit
    static DPOW_DEV void watch(int f) DPOW_TRACED(
        unsigned long long *w = g_wave_trace + kTraceFields * (kTraceWaves - 1);
        if (f == 0 || f == 3 || w[f] == 0) w[f] = now();
        if (f == 0) w[1] = w[2] = 0;)
};
#undef DPOW_TRACED

// The launch's completion record, written by the workgroup that retires last: the control block
// after every hit of this launch (and of earlier ones) was performed, then `seq` with release,
// which the host polls.  Out of line, and not in the watcher: either inlined form makes the
// register allocator spill SGPRs inside the hash loop (tools/isa_loop.py: 7-11 v_readlane per
// wave-block, -3.5 % throughput).
//
// It also resets the next search's control block (ctrl_next): every launch of this search
// runs before any of the next one's (stream order), so the next search needs no reset
// kernel in front of its first launch.
// (Some two-block kernels pass ctrl_next = null and publish() derives it from ctrl -- the
// ring is kCtrlRing * 128 bytes, aligned to its size -- where that keeps SGPR spill reloads
// out of their hash loop (KernelTune::kPoll).  The one-block kernels pass it: deriving it there
// moved the sweep kernel's register assignment and cost it 0.6 % (218.1 -> 216.8 GH/s,
// profiles/r03_ab_publish.log).)
__device__ __attribute__((noinline)) void publish(Ctrl *ctrl, Snap *snap, uint32_t seq, unsigned long long *claim,
                                                  Ctrl *ctrl_next) {
    if (ctrl_next == nullptr) {
        constexpr uintptr_t kRingBytes = kCtrlRing * kCtrlStride * sizeof(Ctrl);
        const uintptr_t a = reinterpret_cast<uintptr_t>(ctrl);
        ctrl_next =
            reinterpret_cast<Ctrl *>((a & ~(kRingBytes - 1)) | ((a + kCtrlStride * sizeof(Ctrl)) & (kRingBytes - 1)));
    }
    // Every workgroup has left its claim loop: recycle the counter slot (claim[1]: the
    // launch's start time, written by the watcher).
    const unsigned long long t_start = __hip_atomic_load(&claim[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t x = 0; x < kClaimCounters; ++x) claim[x * kClaimStride] = 0ull;
    claim[1] = 0ull;
    ctrl_next->best = kNoHit;
    ctrl_next->stop = 0u;
    ctrl_next->done = 0u;
    const unsigned long long best = __hip_atomic_load(&ctrl->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t stop = __hip_atomic_load(&ctrl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&snap->best, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&snap->stop, stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&snap->t_start, t_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&snap->t_end, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&snap->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    WaveTrace::released();
}

// A workgroup's retirement: the one whose count completes the launch (done: Ctrl::done with its
// count) publishes the completion record.
DPOW_DEV void retire(const Launch &L, uint32_t done, Ctrl *ctrl_next) {
    if (done == L.done_target) publish(L.ctrl, L.snap, L.seq, L.claim, ctrl_next);
}

// Workgroup 0, one lane: relays the host cancel flag to Ctrl::stop while the launch runs; exits
// once every worker workgroup has retired.  A launch that was still queued when its search
// returned CANCELLED stops too, even after the caller cleared the flag for its next task: the
// host marks every launch up to the last one it queued as stale (int32 sequence distance).
//
// With a node slot attached (Launch::node_best / node_stop: the node's shared host memory,
// mapped), it relays the node's Found fan-out the same way: a lower best of another rank goes to
// Ctrl::best (atomicMin) -- the waves stop at it at their next group -- and a raised node stop
// stops the launch.  The host injecting the same best through a kernel on a second stream (round
// 2's dpow_search_bound) took 50-160 us to start that kernel beside the running grid (measured
// early in round 3 with a stop-latency probe whose log did not survive;
// tools/small_search_probe.py --stop measures the stop as it is now).
//
// The bound injected by dpow_search_bound (a pinned host word) is relayed the same way.
//
// With a node slot attached it also relays Ctrl::best the other way, to the pinned early-hit
// word (Launch::early): a hit of this launch reaches the host ~1 us after the wave's
// atomicMin, which verifies it and posts it to the node slot at once -- the other ranks stop
// at it while this launch is still draining the chunks below it (round 3: the post waited
// for the completion record, the drain plus ~5 us).
//
// It also stamps the launch's start (s_memrealtime into the claim slot's spare word): the
// watcher workgroup is dispatched first, and the kernel time in the completion record
// replaces per-launch HIP timing events, whose profiling packets cost the host ~4.5 us per
// launch on the time-to-secret path (tools/small_search_probe.py, DPOW_DIAG_NO_EVENTS).
DPOW_DEV void watcher(const Launch &L) {
    if (threadIdx.x != 0) return;
    __hip_atomic_store(&L.claim[1], __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long node_seen = ~0ull, bound_seen = L.bound0, early_seen = kNoHit;
    WaveTrace::watch(0);
    // Every word of a poll is loaded at once and waited for together: one round trip to the
    // host's pinned pages per poll.  Round 4's loop consumed each load before issuing the next -- the completion count, the best, then the flags, the bound
    // and the node's words: four round trips, ~8 us per poll under load
    // (tools/search_timeline.py, profiles/r05_ab.json[r05s/]), which every relay waited for:
    // an owner's hit to its early-hit word, another rank's posted hit into Ctrl::best, the
    // watcher's own exit behind the last workgroup (the next launch's start).  The node slot's
    // words are read through pointers selected inside the loop (without a slot: the launch's
    // own bound and cancel words), so the selection stays out of the kernel's entry block.
    for (;;) {
        const unsigned long long *const nbp = L.node_best ? L.node_best : L.ext_bound;
        const uint32_t *const nsp = L.node_stop ? L.node_stop : L.cancel;
        const uint32_t done = __hip_atomic_load(&L.ctrl->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long b = __hip_atomic_load(&L.ctrl->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t stale = __hip_atomic_load(L.stale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint32_t cancel = __hip_atomic_load(L.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const unsigned long long eb = __hip_atomic_load(L.ext_bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const unsigned long long nb = __hip_atomic_load(nbp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint32_t nstop = __hip_atomic_load(nsp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (done >= L.done_target) {
            WaveTrace::watch(3);
            return;
        }
        if (L.early && b < early_seen) {
            WaveTrace::watch(2);
            early_seen = b;
            __hip_atomic_store(L.early, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        bool stop = cancel != 0u || (int32_t)(stale - L.seq) >= 0;
        if (eb < bound_seen) {
            bound_seen = eb;
            __hip_atomic_fetch_min(&L.ctrl->best, eb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (L.node_best) {
            if (nb < node_seen) {
                if (nb < kNoHit) WaveTrace::watch(1);
                node_seen = nb;
                __hip_atomic_fetch_min(&L.ctrl->best, nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            stop = stop || nstop != 0u;
        }
        if (stop) {
            __hip_atomic_store(&L.ctrl->stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        __builtin_amdgcn_s_sleep(kWatchSleep);
    }
}

// One returning atomic per claim, by lane 0 (claim_issue); its result stays in lane 0's VGPR
// until claim_take broadcasts it to the wave -- the wave waits for the atomic only there.  The
// counter's n-th claim is chunk n * kClaimCounters + x.  The AMDGPU atomic optimizer rewrites an
// atomic on a uniform address into a wave-wide reduction that reads the returned value at once,
// which would put the atomic's latency back in front of the chunk it was issued ahead of.  A
// lane-varying (opaque) zero offset keeps the address divergent to the compiler, so the claim
// stays a plain one-lane returning atomic, waited for only where claim_take reads it.
template <bool kOpaque>
DPOW_DEV unsigned long long claim_issue(unsigned long long *ctr, uint32_t lane) {
    unsigned long long v = 0;
    if constexpr (kOpaque) {
        uint32_t z;
        asm volatile("v_mov_b32 %0, 0" : "=v"(z));
        ctr += z;
    }
    if (lane == 0) v = __hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return v;
}

// base: the first counter-handed claim (Launch::n_static with static first claims, else 0).
DPOW_DEV uint64_t claim_take(unsigned long long v, uint32_t x, uint64_t base) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (((uint64_t)hi << 32) | lo) * kClaimCounters + x + base;
}

DPOW_DEV uint64_t claim_next(unsigned long long *ctr, uint32_t x, uint32_t lane, uint64_t base) {
    return claim_take(claim_issue<false>(ctr, lane), x, base);
}

DPOW_DEV uint64_t lane_range_mask(int64_t lo, int64_t hi) {
    lo = lo < 0 ? 0 : (lo > 64 ? 64 : lo);
    hi = hi < 0 ? 0 : (hi > 64 ? 64 : hi);
    if (hi <= lo) return 0;
    const uint64_t upto_hi = hi == 64 ? ~0ull : ((1ull << hi) - 1ull);
    const uint64_t below_lo = lo == 64 ? ~0ull : ((1ull << lo) - 1ull);
    return upto_hi & ~below_lo;
}

}  // namespace DPOW_KNS
}  // namespace dpow
