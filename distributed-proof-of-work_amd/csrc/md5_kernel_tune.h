// md5_kernel_tune.h -- every build choice of the search kernels (md5_search_kernel.h): the -D
// knobs, the unit's namespace, the launch-control constants and KernelTune, the one place that
// decides a layout's pipe start, VGPR-constant cap, poll source and SGPR budget.
#pragma once
#include <hip/hip_runtime.h>

#include "dpow_common.h"

// DPOW_VLS = 1 (md5_variant.hip's "_ls" translation units): the SH = 0 kernels of launches
// below k = 2^24, whose template is chunk length 0's and which may span chunk lengths 1..3
// (Launch::seg0 == kLsegBase): the pad word W0 + 1 and the bit-length word are segment
// words.  0: every other launch.  Separate kernels, in their own namespace: holding the
// bit-length word's K + M in VGPRs cost the sweep kernel 2 % through register assignment
// alone, with an identical instruction count (217.3 -> 214.0 GH/s in an A/B early in round 3;
// that log did not survive the session).
#ifndef DPOW_VLS
#define DPOW_VLS 0
#endif
// DPOW_VSI = 1 (md5_variant.hip's "_si" translation unit): the segment-inner kernels of the
// one-block SH = 0 D-equality layouts (md5_search_si.h search_body_si): a wave keeps its
// wave-block and walks the launch's 2^24-k segments as its inner loop, so everything that depends
// on word W0 alone is computed once per wave-block and reused for every segment.  Their own unit
// and namespace: the other units' kernels keep their code.
#ifndef DPOW_VSI
#define DPOW_VSI 0
#endif
// Build choices of the segment-inner unit (A/B builds: Makefile SIFLAGS): the pipe start, s_nop in
// front of the worker path (code placement) and whether the segment word's K + M constants live
// in VGPRs (a v_mov each per iteration) or SGPRs.  Same-box sweep of one start for every covered
// W0 (profiles/seg_inner_lead_sweep.json; GH/s on the 16-segment bench step, index order first):
//   W0   index  lead 2     3     4     5     6     7   5 + VGPR constants
//    0   217.0   224.4 224.9 200.1 225.7 215.2 221.1   224.4
//    1   217.8   226.8 207.0 200.2 226.2 226.6 224.8   229.1
//    2   224.6   208.2 229.5 207.2 232.9 231.5 228.4   233.2
//    3   227.8   232.7 212.0 207.2 236.6 235.9 233.8   236.7
// The index-ordered kernels' starts (lead_listed: 2, 4, 3, 3) do not carry over: 4 is the worst
// start of every layout here (-8 to -9 % against index order), 5 the best of every one.
#ifndef DPOW_SI_LEAD
#define DPOW_SI_LEAD 5
#endif
#ifndef DPOW_SI_PAD
#define DPOW_SI_PAD 0
#endif
#ifndef DPOW_SI_VSEG
#define DPOW_SI_VSEG 1
#endif
#if DPOW_VLS && DPOW_VSI
#error "DPOW_VLS and DPOW_VSI are separate units"
#endif
#if DPOW_VLS
#define DPOW_KNS lsk
#elif DPOW_VSI
#define DPOW_KNS sik
#else
#define DPOW_KNS k
#endif
// SGPR budget: <= 80 allocated SGPRs admit 8 four-wave workgroups per CU
// (8 waves per SIMD, MI355X_MICROARCH.md "Residency").  Literal K constants are
// rematerialised by SALU moves, which co-issue beside other waves' VALU.  The budgets are
// tuning values (tools/isa_loop.py builds with others); DESIGN.md records the A/B
// measurements of the alternatives that were removed from this file in round 6.
#ifndef DPOW_NUM_SGPR
#define DPOW_NUM_SGPR 72
#endif
#ifndef DPOW_NUM_SGPR_LONG
#define DPOW_NUM_SGPR_LONG 96  // long-nonce and two-block layouts (KernelTune::kSgpr 1)
#endif
#ifndef DPOW_NUM_SGPR_W15
#define DPOW_NUM_SGPR_W15 100  // two-block layouts at W0 = 15 (KernelTune::kSgpr 2)
#endif
// Diagnostic builds only (tools/wave_trace.py, tools/wave_trace_node.py): every worker wave
// records its times and counts (md5_launch_ctl.h WaveTrace), read back with dpow_diag_wave_trace.
#ifndef DPOW_WAVE_TRACE
#define DPOW_WAVE_TRACE 0
#endif
// A/B builds only: one choice for every narrow kernel, over narrow_knobs (tools/lead_sweep.py)
#ifndef DPOW_NLEAD
#define DPOW_NLEAD 0   // pipe start
#endif
#ifndef DPOW_NCAP
#define DPOW_NCAP 0    // VGPR-constant cap
#endif
#ifndef DPOW_NPOLL
#define DPOW_NPOLL -1  // KernelTune::kPoll 0 / 1
#endif
#ifndef DPOW_NSGPR
#define DPOW_NSGPR 0   // SGPR budget class 1 / 2
#endif

#define DPOW_DEV __device__ __forceinline__
#define DPOW_DEV_CONST __host__ __device__ constexpr

namespace dpow {
namespace DPOW_KNS {

static_assert(DPOW_POLL_WB > 0, "the chunk loop polls per group of wave-blocks");
constexpr int kSgprLongW0 = 8;
// The watcher's poll interval, s_sleep units of 64 cycles (round 4: 32).
constexpr int kWatchSleep = 16;
// Retirement counted per claim counter, then on Ctrl::done: in the chunk-length-spanning
// units only -- the launches of short searches, below k = 2^24 -- so that the other units'
// kernels (the sweep's among them) keep their code.
constexpr bool kXcdRetire = DPOW_VLS != 0;
// Static first claims (the "_ls" kernels: the short launches below k = 2^24 that the
// time-to-secret path runs): worker wave w's first claim is chunk w, so a wave starts
// hashing without waiting for a contended counter -- at 4 workgroups per CU the start-up
// burst of 8k claim atomics on 8 counters held the median wave 5 us and the slowest 10 us
// before its first wave-block (tools/wave_trace_tts.py).  Its claim-ahead atomic then
// hides behind that first chunk.  The counters hand out chunks from Launch::n_static on.
// (plan.cpp sets Launch::n_static for exactly those launches.)
constexpr bool kStaticFirst = DPOW_VLS != 0;
// The code-placement pad of the sweep kernels (search_body): 63 s_nop.
constexpr int kPad4B = 63;

// The build choices of the narrow SH = 3 kernels (hash_wave_block KSPAN = false, the kernels of
// launches with R >= 64): pipe start (0: the general kernel's), VGPR-constant cap (0: the
// general's), poll source (-1: the general's) and SGPR budget class (-1: the general's; 1 = 96,
// 2 = 100).  Each row is the per-layout argmax of round 6's same-box sweeps of builds with one
// choice for every narrow kernel (tools/lead_sweep.py; profiles/r06_narrow_sweep.json).  on =
// false: no narrow build beat the layout's general kernel (<1,0,3>), or the layout was not swept
// (<1,12..13,3>: chunks below 2^24 only), so it runs the general kernel for every R.
struct NarrowKnobs {
    bool on;
    int lead, cap, poll, sgpr;
};
constexpr NarrowKnobs narrow_knobs(int nblk, int w0) {
    if (nblk == 1) {
        switch (w0) {
            case 1: case 2: case 3: case 5: case 6: case 11:
                    return {true, 2, 0, 0, 1};
            case 4: return {true, 1, 0, -1, -1};
            case 7: return {true, 2, 0, -1, 1};
            case 8: return {true, 3, 0, 0, -1};
            case 9: return {true, 4, 0, -1, -1};
            case 10: return {true, 2, 0, 0, -1};
            default: return {false, 0, 0, -1, -1};
        }
    }
    switch (w0) {
        case 12: return {true, 3, 0, 0, -1};
        case 13: return {true, 3, 0, -1, -1};
        case 14: return {true, 2, 24, -1, -1};
        case 15: return {true, 2, 0, 0, -1};
        default: return {false, 0, 0, -1, -1};
    }
}

// The general kernels' listed pipe starts (0: none, the rule's 4).  Which start issues best
// depends on the layout; the table is the argmax of a per-layout sweep of builds with one start
// for every layout, 1..6 (tools/lead_sweep.py, profiles/r02_lead_sweep.json), where a start beats
// 4 by >= 0.8 %.  The headline <1,1,0> keeps 4.
// (round 4: the same sweep over the round-4 kernels, profiles/r04_lead_sweep.json, moved the
// entries marked r4 -- a start that beats the table's by >= 1 % -- and dropped <1,10,1..2>'s
// 3, now 7.4 % below 4)
constexpr int lead_listed(int nblk, int w0, int sh) {
    if (nblk == 1) {
        switch (w0 * 4 + sh) {
            case 0 * 4 + 0: return 2;  // +1.3 %
            case 0 * 4 + 3: return 2;  // r4 +1.1 %
            case 2 * 4 + 0: return 3;  // +2.0 %
            case 2 * 4 + 1: return 1;  // r4 +1.2 % (round 2: 2)
            case 2 * 4 + 2: return 1;  // r4 +1.2 % (round 2: 2)
            case 3 * 4 + 0: return 3;  // +2.2 %
            case 3 * 4 + 1: return 3;  // r4 +1.2 %
            case 3 * 4 + 2: return 3;  // r4 +1.1 %
            case 3 * 4 + 3: return 1;  // +2.0 %
            case 4 * 4 + 0: return 2;  // r4 +1.5 %
            case 4 * 4 + 3: return 2;  // +1.0 %
            case 6 * 4 + 3: return 2;  // r4 +1.4 %
            case 8 * 4 + 3: return 3;  // +2.2 %
            case 9 * 4 + 0: return 2;  // +3.7 %
            case 9 * 4 + 1: return 3;  // r4 +2.3 %
            case 9 * 4 + 2: return 3;  // r4 +2.3 %
            case 9 * 4 + 3: return 3;  // +1.6 %
            case 10 * 4 + 3: return 5; // +1.8 %
            default: return 0;
        }
    }
    switch (w0 * 4 + sh) {
        case 12 * 4 + 3: return 1;  // +4.3 %
        case 14 * 4 + 1: return 2;  // +5.0 %
        case 14 * 4 + 2: return 2;  // +5.1 %
        case 14 * 4 + 3: return 1;  // +4.3 %
        case 15 * 4 + 0: return 2;  // +4.5 %
        case 15 * 4 + 1: return 2;  // r4 +2.2 %
        case 15 * 4 + 2: return 2;  // r4 +2.3 %
        case 15 * 4 + 3: return 1;  // +5.7 %
        default: return 0;
    }
}

// The tuning of kernel <NBLK, W0, SH> (KS: its KSPAN; kNarrow = SH = 3's narrow kernel).  Each
// member is the layout's rule, unless the layout is listed (kN: narrow_knobs' row for a narrow
// kernel; else the general kernels' exceptions), unless an A/B build's macro overrides both.
template <int NBLK, int W0, int SH, bool KS = true>
struct KernelTune {
    static constexpr bool kNarrow = SH == 3 && !KS;
    static constexpr NarrowKnobs kN = kNarrow ? narrow_knobs(NBLK, W0) : NarrowKnobs{false, 0, 0, -1, -1};

    // kLead: the first hand-ordered step of block 0 is W0 + kLead.  Rule: 4, the first step whose
    // four state words are all per-lane; before it the compiler schedules the steps (some state
    // words are wave-uniform there, and it exploits that).
    static constexpr int kLeadListed = kN.lead > 0 ? kN.lead : lead_listed(NBLK, W0, SH);
    static constexpr int kLead = DPOW_VSI && DPOW_SI_LEAD > 0 ? DPOW_SI_LEAD
                                 : kNarrow && DPOW_NLEAD > 0  ? DPOW_NLEAD
                                 : kLeadListed > 0            ? kLeadListed
                                                              : 4;

    // kCap: K + M constants held in VGPRs (VgprK).  VGPRs the layout uses without them
    // (-Rpass-analysis=kernel-resource-usage): one block 34-39 (SH = 0) / 43-49 (SH != 0), two
    // blocks 41-43 / 49-53; each constant costs about one more.  The grid runs 6 waves per SIMD,
    // so up to 80 VGPRs cost no occupancy that is used; the caps keep every kernel within 72
    // (7 waves: a queued launch's workgroups still start beside a draining one).  The
    // segment-word constants count against them first.  Round 1's caps for <= 64 VGPRs (14
    // one-block / 10 two-block for SH != 0) left the two-block layouts with 4-11 SGPR spill
    // reloads per wave-block.
    // (listed, round 4, profiles/r04_lead_sweep.json: a cap of 24 for <1,7,1..2> +1.9-2.0 %,
    // <1,4,3> +1.5 %, <1,5,3> +1.0 %; elsewhere it is no better, or costs up to 3 %)
    static constexpr int kCapRule = NBLK == 1 ? (SH == 0 ? 24 : SH == 3 ? 14 : 18) : (SH == 3 ? 20 : 26);
    static constexpr bool kCap24 =
        NBLK == 1 && ((W0 == 7 && (SH == 1 || SH == 2)) || (SH == 3 && (W0 == 4 || W0 == 5)));
    static constexpr int kCap = kNarrow && DPOW_NCAP > 0 ? DPOW_NCAP : kN.cap > 0 ? kN.cap : kCap24 ? 24 : kCapRule;

    // kPoll: whether the kernel reads the poll group (Launch::poll_wb) and the next search's control
    // block (Launch::ctrl_next) from the launch, or uses the compile-time group and derives the
    // block in publish().  Rule: the one-block kernels and SH = 1..2 read them.  The two-block
    // kernels sit at their SGPR budget, and which choice leaves their hash loop free of SGPR spill
    // reloads depends on the layout's register assignment, not on the count of live values
    // (tools/isa_loop.py over all four combinations; the two flags chosen alike leave every
    // two-block layout at 0-1 reloads per wave-block except <2,12,0> (4 in every combination) and
    // <2,15,0> / <2,15,3> (3); one reload-heavy choice for all of them cost 3-4 % at <2,14,1>,
    // <2,14,3>, <2,15,1> against round 2's build in a same-box A/B): listed, <2,15,0> and
    // <2,14..15,3> read them too.
    static constexpr bool kPollRule = NBLK == 1 || SH == 1 || SH == 2;
    static constexpr bool kPollListed = (SH == 0 && W0 == 15) || (SH == 3 && W0 >= 14);
    static constexpr bool kPoll = kNarrow && DPOW_NPOLL >= 0 ? DPOW_NPOLL != 0
                                  : kN.poll >= 0             ? kN.poll != 0
                                                             : kPollRule || kPollListed;

    // kSgpr: the SGPR budget class (0: DPOW_NUM_SGPR, 1: _LONG, 2: _W15).  The grid is 6 four-wave
    // workgroups per CU (6 waves per SIMD, dpow_api.cpp), so a budget that still admits 7 waves costs
    // no occupancy.  Rule: the short-nonce layouts keep the round-1 budget (72: no spill in the
    // hash loop; 8 waves admitted, so the next queued launch's workgroups start beside a draining
    // one); layouts with many launch-uniform K + M constants -- long nonces and two final blocks --
    // get 96: at 72 the compiler spills them to VGPR lanes and reloads each with a v_readlane in
    // every wave-block (tools/isa_loop.py: 4-41 per wave-block; 0 at 96).
    // Listed, kW15: the two-block W0 = 15 layouts get 100: at 96 three of them kept 3 spill reloads
    // per wave-block in every kPoll choice, at 100 they keep 0-1.  Round 4's per-layout sweep of a
    // 100 budget for every long layout (tools/lead_sweep.py, profiles/r04_lead_sweep.json) added
    // <2,13,3> (+1.5 %), <2,14,3> (+0.7 %) and <1,11,3> (+2.6 %); elsewhere 100 is within +-0.3 %
    // of 96.  7 waves still fit.
    // Listed, kShort96: short-nonce one-block layouts that take 96 instead of 72: every one-block
    // kernel at 96 against the build before, per layout (round 6, profiles/r06_narrow_sweep.json
    // ab6 at workerBits 0: SH = 1-2 +0.5 to +1.5 %, SH = 0 at W0 3 and 5-7 +0.8 to +1.2 %; ab5,
    // SH = 3's general kernels at workerBits 3: W0 2-5 +0.5 to +0.9 %, W0 7 +6.6 %, where 72 left 7
    // spill reloads per wave-block).  The rest were within noise or slower (<1,0,3> -3 %, <1,6,3>
    // -3 %); the sweep kernel <1,1,0> keeps its code.  Not the "_ls" units.
    // (The attribute takes no template-dependent value: md5_search_kernel.h defines one kernel
    // template per class, and md5_variant.hip instantiates the one kSgpr selects.)
    static constexpr int kSgprRule = NBLK == 2 || W0 >= kSgprLongW0 ? 1 : 0;
    static constexpr bool kW15 = (NBLK == 2 && W0 == 15) || (NBLK == 2 && SH == 3 && (W0 == 13 || W0 == 14)) ||
                                 (NBLK == 1 && W0 == 11 && SH == 3);
    static constexpr bool kShort96 = NBLK == 1 && !DPOW_VLS && KS && W0 < kSgprLongW0 &&
                                     (SH == 1 || SH == 2 || (SH == 0 && (W0 == 3 || W0 >= 5)) ||
                                      (SH == 3 && ((W0 >= 2 && W0 <= 5) || W0 == 7)));
    static constexpr int kSgpr = kNarrow && DPOW_NSGPR > 0 ? DPOW_NSGPR
                                 : kN.sgpr > 0             ? kN.sgpr
                                 : kW15                    ? 2
                                 : kShort96                ? 1
                                                           : kSgprRule;
};

}  // namespace DPOW_KNS
}  // namespace dpow
