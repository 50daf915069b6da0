// md5_hash.h -- the MD5 of the search kernels: which K + M constants live where (VgprK, StepWord),
// the compiler-scheduled steps (md5_steps), the hand-ordered two-candidate pipeline (pipe::), the
// final-block compression (md5_tail) and the full digest test of a candidate (full_check).
#pragma once
#include "md5_kernel_tune.h"

namespace dpow {
namespace DPOW_KNS {

// State-word roles of step I (a is written from b, c, d) and its bitop3 truth table.
template <int I> struct Roles {
    static constexpr int a = (64 - I) % 4, b = (a + 1) % 4, c = (a + 2) % 4, d = (a + 3) % 4;
};
template <int I>
constexpr uint32_t tt() {
    return I / 16 == 0 ? kBop3F : I / 16 == 1 ? kBop3G : I / 16 == 2 ? kBop3H : kBop3I;
}

template <int I>
DPOW_DEV uint32_t md5_fn(uint32_t x, uint32_t y, uint32_t z) {
    return __builtin_amdgcn_bitop3_b32(x, y, z, tt<I>());
}

// Launch-uniform K + M constants kept in VGPRs (every lane the same value).  Layouts with long
// nonces need up to ~50 distinct K + M constants in the pipelined steps (every nonce word, four
// times per block).  Under the 80-SGPR budget of 8 waves/SIMD the compiler spills them to VGPR
// lanes and reloads each with a v_readlane -- a VALU instruction -- on every use (28-54 per
// wave-block in the two-block kernels).  Copied once per wave into VGPRs with an opaque v_mov (so
// they are not folded back to SGPRs), they cost nothing in the loop: v_add3_u32 reads a VGPR
// operand at the same rate.  Capped (KernelTune::kCap) so the kernel stays within 72 VGPRs.
struct KConst {
    uint32_t v[128];  // [64 * BLK + I]; only the entries VgprK selects are set
};

// Segment words: the message word(s) holding the chunk bytes above k's low 24 bits (byte p + 4
// on; k >> 24 is one byte for L = 4, two for L = 5).  They are launch-uniform within a 2^24-k
// segment, and a launch spans segments (plan.cpp), so their K + M constants are re-derived per
// wave when it enters another segment: word W0 + 1 always, W0 + 2 when SH = 3 (the two-byte
// field of L = 5 crosses into it).
// For SH != 0 word W0 + 1 also holds the top bytes of V; its K + M is then wave-uniform per
// wave-block anyway (VarWords::hi_s, which carries the segment addition too), so only SH = 0's
// W0 + 1 and SH = 3's W0 + 2 are VGPR-held segment words.
// SH = 0 kernels also serve launches spanning chunk-length segments (Launch::lspan):
// there the bit-length word (16 NBLK - 2) and W0 + 1 (the pad of L = 3) change per segment.
template <int NBLK, int W0, int SH>
DPOW_DEV_CONST bool seg_word(int m) {
    return (SH == 0 && m == W0 + 1) || (SH == 3 && m == W0 + 2 && m != 16 * NBLK - 2) ||
           (DPOW_VLS && SH == 0 && (m == W0 + 1 || m == 16 * NBLK - 2));
}

// KS: the KSPAN argument of the kernel (hash_wave_block).
template <int NBLK, int W0, int SH, bool KS = true>
struct VgprK {
    using Tune = KernelTune<NBLK, W0, SH, KS>;
    // The hash loop's hand-ordered steps of block 0 (its ONLY_D md5_tail with kNC candidates):
    // [kI0, kEnd0).
    static constexpr int kEnd0 = NBLK == 1 ? 62 : 64;
    static constexpr int kI0 = W0 + Tune::kLead < kEnd0 ? W0 + Tune::kLead : kEnd0;
    // Steps the hash loop runs (ONLY_D: the last block stops after step 61).
    static constexpr bool run(int blk, int i) { return !(blk == NBLK - 1 && i >= 62); }
    // Steps reading a segment word: always held in VGPRs (updated at segment changes).
    // (the segment-inner unit rewrites them every iteration of its segment loop; built with
    // DPOW_SI_VSEG = 0 it takes them from SGPRs instead: StepWord::km's seg_add path)
    static constexpr bool segw(int blk, int i) { return seg_word<NBLK, W0, SH>(16 * blk + md5_word(i)) && run(blk, i); }
    static constexpr bool seg(int blk, int i) { return (!DPOW_VSI || DPOW_SI_VSEG) && segw(blk, i); }
    static constexpr bool eligible(int blk, int i) {
        const int m = 16 * blk + md5_word(i);
        const bool zero = m > W0 + 2 && m != 16 * NBLK - 2;
        const bool lane = m == W0 || (SH != 0 && m == W0 + 1);
        const bool piped = blk > 0 || i >= kI0;
        return !zero && !lane && piped && run(blk, i) && !segw(blk, i);
    }
    static constexpr int rank(int blk, int i) {
        int r = 0;
        for (int b = 0; b < NBLK; ++b)
            for (int j = 0; j < 64; ++j) {
                if (b == blk && j == i) return r;
                if (eligible(b, j)) ++r;
            }
        return r;
    }
    static constexpr int count_seg() {
        int r = 0;
        for (int b = 0; b < NBLK; ++b)
            for (int j = 0; j < 64; ++j) r += seg(b, j) ? 1 : 0;
        return r;
    }
    static constexpr bool use(int blk, int i) {
        return seg(blk, i) || (eligible(blk, i) && rank(blk, i) < Tune::kCap - count_seg());
    }
};

template <int NBLK, int W0, int SH, int BLK, int I, bool KS>
DPOW_DEV void kconst_init(KConst &kc, const Launch &L) {
    if constexpr (BLK < NBLK) {
        if constexpr (VgprK<NBLK, W0, SH, KS>::use(BLK, I))
            asm("v_mov_b32 %0, %1" : "=v"(kc.v[64 * BLK + I]) : "s"(L.KT[64 * BLK + I]));
        if constexpr (I + 1 < 64) kconst_init<NBLK, W0, SH, BLK, I + 1, KS>(kc, L);
        else kconst_init<NBLK, W0, SH, BLK + 1, 0, KS>(kc, L);
    }
}

// Additions to the segment words (W0 + 1, W0 + 2) for 2^24-k segment `seg`
// (dpow_common.h seg_word_deltas).
template <int W0, int SH>
DPOW_DEV void seg_deltas(const Launch &L, uint32_t seg, uint32_t &d1, uint32_t &d2) {
    seg_word_deltas(L.T[W0 + 1], L.T[W0 + 2], seg, L.seg_first, SH, d1, d2);
}

// Addition to segment word m: d[0] to W0 + 1, d[1] to W0 + 2, d[2] to the bit-length word
// (where W0 + 1 is the bit-length word, plan.cpp puts the whole difference in d[2]).
template <int NBLK, int W0>
DPOW_DEV uint32_t seg_add(int m, const uint32_t (&d)[3]) {
    return m == 16 * NBLK - 2 ? d[2] : m == W0 + 1 ? d[0] : d[1];
}

// The segment-word additions of segment sg (seg_id): for SH = 0 below k = 2^24 the
// chunk-length deltas against the template's chunk length 0 (lseg_deltas: no Launch field is
// read -- plain kernarg reads here were hoisted out of the claim loop into SGPRs and pushed
// its wave-uniform index arithmetic onto the VALU, +10 VALU per wave-block in <1,1,0>,
// tools/isa_loop.py), else the 2^24-k field (seg_word_deltas); d0 = the addition to W0.
template <int NBLK, int W0, int SH>
DPOW_DEV void seg_all_deltas(const Launch &L, uint32_t sg, uint32_t &d0, uint32_t (&d)[3]) {
    d0 = d[0] = d[1] = d[2] = 0u;
    if (sg >= kLsegBase) {
        if constexpr (SH == 0 && DPOW_VLS) {
            lseg_deltas((sg - kLsegBase) & 3u, d0, d[0], d[2]);
            if constexpr (W0 + 1 == 16 * NBLK - 2) {  // W0 + 1 is the bit-length word
                d[2] += d[0];
                d[0] = 0u;
            }
        }
    } else {
        seg_deltas<W0, SH>(L, sg, d[0], d[1]);
    }
}

// Re-derive the VGPR-held K + M constants of the segment words (wave-uniform,
// once per segment change: a rare branch).
template <int NBLK, int W0, int SH, int BLK, int I, bool KS>
DPOW_DEV void kconst_seg(KConst &kc, const Launch &L, const uint32_t (&d)[3]) {
    if constexpr (BLK < NBLK) {
        if constexpr (VgprK<NBLK, W0, SH, KS>::seg(BLK, I)) {
            constexpr int m = 16 * BLK + md5_word(I);
            const uint32_t k = L.KT[64 * BLK + I] + seg_add<NBLK, W0>(m, d);
            asm volatile("v_mov_b32 %0, %1" : "=v"(kc.v[64 * BLK + I]) : "s"(k));
        }
        if constexpr (I + 1 < 64) kconst_seg<NBLK, W0, SH, BLK, I + 1, KS>(kc, L, d);
        else kconst_seg<NBLK, W0, SH, BLK + 1, 0, KS>(kc, L, d);
    }
}

// Per-candidate variable message parts.  KSPAN: the lanes may span several k (R < 64), so
// SH = 3's word W0 + 1 differs per lane (lane_k); without it that word's K + M is wave-uniform.
template <bool KSPAN>
struct VarWords {
    static constexpr bool kSpan = KSPAN;
    uint32_t lo_s[kNC];  // wave-uniform part of V << 8*SH (word W0)
    uint32_t lo_v;       // per-lane part of V << 8*SH (the same for every slot)
    uint32_t hi_s[kNC];  // SH != 0: the wave-uniform part of word W0+1's addition -- V >> (32 - 8 SH)
                         //  (uniform: a lane's k offset never carries into those bits) plus the
                         //  segment addition d1
    uint32_t lane_k;     // SH = 3: the per-lane part of V >> 8 (the lane's k offset; 0 when R >= 64,
                         //  and not read without KSPAN)
    const KConst *kc;    // launch-uniform K + M constants held in VGPRs (segment words: current segment)
    uint32_t seg_d[3];   // segment-word additions (seg_add) for the steps that read them from L.KT
                         //  (full_check's steps 62-63 of the last block only; the hash loop holds them
                         //  all in kc)
#if DPOW_VSI
    uint32_t w0km[4][kNC];  // K + M of round r's step reading word W0 (per lane; loop-invariant in the
                            //  segment loop, where seg_d[0] is the current segment's addition to word W0 + 1)
#endif
};

// Step of round r (block-relative) that reads message word w.
constexpr int step_of_word(int r, int w) {
    for (int i = 16 * r; i < 16 * r + 16; ++i)
        if (md5_word(i) == w) return i;
    return -1;
}

// K + M of step I of block BLK for candidate j (the message word M includes the
// candidate's variable bytes when the step reads word W0, or W0 + 1 for SH != 0).
template <int NBLK, int W0, int SH, int BLK, int I, bool KS>
struct StepWord {
    static constexpr int m = 16 * BLK + md5_word(I);
    // Words past the variable bytes, the chunk tail and the 0x80 pad -- every
    // word after W0 + 2 except the bit-length word -- are zero for every launch
    // of this layout (plan.cpp), so K + M folds to the literal K: no SGPR.
    static constexpr bool zero_word = m > W0 + 2 && m != 16 * NBLK - 2;
    static constexpr bool per_lane = m == W0 || (SH == 3 && KS && m == W0 + 1);  // K + M differs per lane
    static constexpr bool vgpr_k = VgprK<NBLK, W0, SH, KS>::use(BLK, I);
    static constexpr bool seg = seg_word<NBLK, W0, SH>(m);
    static DPOW_DEV uint32_t km(const Launch &L, const VarWords<KS> &v, int j) {
        uint32_t k = zero_word ? kMd5K[I] : vgpr_k ? v.kc->v[64 * BLK + I] : L.KT[64 * BLK + I];
        if constexpr (seg && !vgpr_k) k += seg_add<NBLK, W0>(m, v.seg_d);
#if DPOW_VSI
        if constexpr (m == W0) k = v.w0km[I / 16][j];
#else
        if constexpr (m == W0) k = (k + v.lo_s[j]) + v.lo_v;
#endif
        if constexpr (SH != 0 && m == W0 + 1) {
            k += v.hi_s[j];                        // SALU: K + M stays uniform
            if constexpr (SH == 3 && KS) k += v.lane_k;  // the one VALU add of the step
        }
        return k;
    }
};

// Steps [I, IE) of block BLK for NCAND candidates, left to the compiler.
template <int NBLK, int W0, int SH, int BLK, int I, int IE, int NCAND, class V>
DPOW_DEV void md5_steps(uint32_t (&x)[4][kNC], const Launch &L, const V &v) {
    if constexpr (I < IE) {
        using R = Roles<I>;
#pragma unroll
        for (int j = 0; j < NCAND; ++j) {
            const uint32_t km = StepWord<NBLK, W0, SH, BLK, I, V::kSpan>::km(L, v, j);
            const uint32_t f = md5_fn<I>(x[R::b][j], x[R::c][j], x[R::d][j]);
            x[R::a][j] = x[R::b][j] + __builtin_rotateleft32(x[R::a][j] + f + km, md5_shift(I));
        }
        md5_steps<NBLK, W0, SH, BLK, I + 1, IE, NCAND>(x, L, v);
    }
}

// ---------------------------------------------------------------------------
// Two candidates, issue order fixed by hand.  Each MD5 step is four VALU instructions, two full
// rate (v_bitop3_b32, v_add_u32) and two half rate (v_add3_u32, v_alignbit_b32), strictly
// dependent within a candidate.  Candidate q runs half a step behind candidate p and the two
// chains alternate instruction by instruction (DPOW_PIPE_BODY below), with s_nop padding after
// the half-rate instructions.  One asm statement per step pair: the compiler keeps the order,
// allocates the registers and places the SALU moves of the K constants, and adds no padding of
// its own inside the group (these plain VALU ops are interlocked in hardware; one asm statement
// per instruction got a conservative s_nop after every VOP3).  Against the compiler-scheduled
// loop: 170 -> 214.7 GH/s.  The probes that led here are dpow_diag_valu_rate kinds 20-27
// (profiles/r01_valu_probe_order.log).
namespace pipe {

// Wait states after each instruction kind of a group (-1: none).  A VALU instruction issued right
// behind the one it depends on holds the SIMD's issue for the whole dependency latency -- every
// wave on the SIMD waits -- while an s_nop holds only its own wave and lets the other waves
// issue; the padding after the half-rate instructions pays even where nothing depends on them.
// Measured on the sweep (order 1, profiles/r01_ab_nop.log): no padding 170 GH/s; s_nop 0 after
// each rotate 192.5; plus s_nop 0 / 1 / 2 / 3 after each add3 200.7 / 203.6 / 209.1 / 205.4;
// s_nop 1 after the rotate instead 191; any padding after the full-rate ops 168-185; no rotate
// padding 179-180.  Order 2 (profiles/r01_ab_order.log): the same s_nop 0 / s_nop 2 is best,
// 214.7; no padding 170.7; add3 padding 1 or 3: 210.
#define DPOW_PAD_R "s_nop 0\n\t"  // after v_alignbit_b32 (the rotate; the next add reads it)
#define DPOW_PAD_A "s_nop 2\n\t"  // after v_add3_u32

// Order of a step pair (B bop3, A add3, R rotate, D add; p at step I, q finishing
// step I-1 then starting step I): p.B q.R p.A q.D p.R q.B p.D q.A -- the two chains
// strictly alternate, so every dependency is two instructions apart (F H H F H F F H);
// 214.7 GH/s.  (p.B q.R q.D p.A q.B p.R p.D q.A -- F and H strictly alternate, but each
// rotate sits right before its add -- 209.1 GH/s; two pairs interleaved at NC = 4 with
// both properties, every dependency >= 3 apart: 191 GH/s at best.
// profiles/r01_ab_order.log.)
#define DPOW_PIPE_BODY                                        \
    "v_bitop3_b32 %[fp], %[pb], %[pc], %[pd] bitop3:%[tt]\n\t" \
    "v_alignbit_b32 %[rq], %[tq], %[tq], %[sq]\n\t" DPOW_PAD_R \
    "v_add3_u32 %[tp], %[pa], %[fp], %[kp]\n\t" DPOW_PAD_A     \
    "v_add_u32_e32 %[qb], %[qc], %[rq]\n\t"                   \
    "v_alignbit_b32 %[tp], %[tp], %[tp], %[sp]\n\t" DPOW_PAD_R \
    "v_bitop3_b32 %[fq], %[qb], %[qc], %[qd] bitop3:%[tt]\n\t" \
    "v_add_u32_e32 %[pa], %[pb], %[tp]\n\t"                   \
    "v_add3_u32 %[tq], %[qa], %[fq], %[kq]\n\t" DPOW_PAD_A

#define DPOW_PIPE_PRO                                         \
    "v_bitop3_b32 %[fp], %[pb], %[pc], %[pd] bitop3:%[tt]\n\t" \
    "v_add3_u32 %[tp], %[pa], %[fp], %[kp]\n\t" DPOW_PAD_A     \
    "v_bitop3_b32 %[fq], %[qb], %[qc], %[qd] bitop3:%[tt]\n\t" \
    "v_alignbit_b32 %[tp], %[tp], %[tp], %[sp]\n\t" DPOW_PAD_R \
    "v_add_u32_e32 %[pa], %[pb], %[tp]\n\t"                   \
    "v_add3_u32 %[tq], %[qa], %[fq], %[kq]\n\t" DPOW_PAD_A

// The two groups' statements, KC the constraint of kp / kq: "v" where K + M differs per lane
// or is held in a VGPR (StepWord), else "s".
#define DPOW_PIPE_BODY_ASM(KC)                                                                                        \
    asm volatile(DPOW_PIPE_BODY                                                                                       \
                 : [pa] "+&v"(x[R::a][J]), [qb] "=&v"(x[R::b][J + 1]), [tq] "+v"(tq), [fp] "=&v"(fp),                 \
                   [fq] "=&v"(fq), [rq] "=&v"(rq), [tp] "=&v"(tp)                                                     \
                 : [pb] "v"(x[R::b][J]), [pc] "v"(x[R::c][J]), [pd] "v"(x[R::d][J]), [qc] "v"(x[R::c][J + 1]),        \
                   [qd] "v"(x[R::d][J + 1]), [qa] "v"(x[R::a][J + 1]), [kp] KC(kp), [kq] KC(kq),                      \
                   [tt] "i"(tt<I>()), [sp] "i"(32 - md5_shift(I)), [sq] "i"(32 - md5_shift(I - 1)))
#define DPOW_PIPE_PRO_ASM(KC)                                                                                         \
    asm volatile(DPOW_PIPE_PRO                                                                                        \
                 : [pa] "+&v"(x[R::a][J]), [tq] "=&v"(tq), [fp] "=&v"(fp), [fq] "=&v"(fq), [tp] "=&v"(tp)             \
                 : [pb] "v"(x[R::b][J]), [pc] "v"(x[R::c][J]), [pd] "v"(x[R::d][J]), [qb] "v"(x[R::b][J + 1]),        \
                   [qc] "v"(x[R::c][J + 1]), [qd] "v"(x[R::d][J + 1]), [qa] "v"(x[R::a][J + 1]), [kp] KC(kp),         \
                   [kq] KC(kq), [tt] "i"(tt<I0>()), [sp] "i"(32 - md5_shift(I0)))

// One step pair of candidates p = J, q = J + 1 at step I (q finishes step I-1, whose add3 is in
// tq, and starts step I).  p's state word a is written in the middle of the group (`+&v`,
// early-clobber): where the pipeline starts before W0 + 4, p's and q's state words can still be
// the same wave-uniform value, and a plain `+v` lets the register allocator hand q's input that
// same register, which the group then overwrites before q reads it (a wrong hash in <1,0,0> at
// start W0 + 2, caught by test_nonce_lengths_golden / tests/soak/layout_check.py).
template <int NBLK, int W0, int SH, int BLK, int I, int J, class V>
DPOW_DEV void body(uint32_t (&x)[4][kNC], uint32_t &tq, const Launch &L, const V &v) {
    using R = Roles<I>;  // q's step I-1 writes x[R::b][q] from x[R::c][q]
    using W = StepWord<NBLK, W0, SH, BLK, I, V::kSpan>;
    const uint32_t kp = W::km(L, v, J), kq = W::km(L, v, J + 1);
    uint32_t fp, fq, rq, tp;
    if constexpr (W::per_lane || W::vgpr_k) DPOW_PIPE_BODY_ASM("v");
    else DPOW_PIPE_BODY_ASM("s");
}

// Prologue of a pair at its first pipelined step I0: q's step I0 is left half done.
template <int NBLK, int W0, int SH, int BLK, int I0, int J, class V>
DPOW_DEV void prologue(uint32_t (&x)[4][kNC], uint32_t &tq, const Launch &L, const V &v) {
    using R = Roles<I0>;
    using W = StepWord<NBLK, W0, SH, BLK, I0, V::kSpan>;
    const uint32_t kp = W::km(L, v, J), kq = W::km(L, v, J + 1);
    uint32_t fp, fq, tp;
    if constexpr (W::per_lane || W::vgpr_k) DPOW_PIPE_PRO_ASM("v");
    else DPOW_PIPE_PRO_ASM("s");
}

constexpr int kPairs = kNC / 2;

// Step pairs I .. IE-1 of every candidate pair, the pairs' groups interleaved.
template <int NBLK, int W0, int SH, int BLK, int I, int IE, class V>
DPOW_DEV void run(uint32_t (&x)[4][kNC], uint32_t (&tq)[kPairs], const Launch &L, const V &v) {
    if constexpr (I < IE) {
        body<NBLK, W0, SH, BLK, I, 0>(x, tq[0], L, v);
        if constexpr (kPairs > 1) body<NBLK, W0, SH, BLK, I, 2>(x, tq[1], L, v);
        run<NBLK, W0, SH, BLK, I + 1, IE>(x, tq, L, v);
    }
}

// Steps [I0, IE) of block BLK for all candidates in the alternating order.
template <int NBLK, int W0, int SH, int BLK, int I0, int IE, class V>
DPOW_DEV void steps(uint32_t (&x)[4][kNC], const Launch &L, const V &v) {
    static_assert(kNC == 2 || kNC == 4, "the pipelined path runs one or two candidate pairs");
    if constexpr (I0 < IE) {
        uint32_t tq[kPairs];
        prologue<NBLK, W0, SH, BLK, I0, 0>(x, tq[0], L, v);
        if constexpr (kPairs > 1) prologue<NBLK, W0, SH, BLK, I0, 2>(x, tq[1], L, v);
        run<NBLK, W0, SH, BLK, I0 + 1, IE>(x, tq, L, v);
        // epilogue: each q finishes step IE-1
        using E = Roles<IE - 1>;
#pragma unroll
        for (int p = 0; p < kPairs; ++p)
            x[E::a][2 * p + 1] = x[E::b][2 * p + 1] + __builtin_rotateleft32(tq[p], md5_shift(IE - 1));
    }
}

#undef DPOW_PIPE_BODY_ASM
#undef DPOW_PIPE_PRO_ASM
#undef DPOW_PIPE_BODY
#undef DPOW_PIPE_PRO
#undef DPOW_PAD_R
#undef DPOW_PAD_A

}  // namespace pipe

// Final-block compression(s) of NCAND candidates; returns the digest words.  With ONLY_D the last
// block stops after step 61, which writes D (steps 62-63 only feed A..C): out[3] is exact,
// out[0..2] are not computed.  With RAW_D (one final block) out[3] is the state word without the
// chaining value: D = iv[3] + out[3], which the D-equality test compares against -iv[3].
template <int NBLK, int W0, int SH, int NCAND, bool ONLY_D = false, bool RAW_D = false, class V>
DPOW_DEV void md5_tail(uint32_t (&out)[4][kNC], const Launch &L, const V &v) {
    static_assert(!RAW_D || (ONLY_D && NBLK == 1), "RAW_D: D word of one final block");
    uint32_t x[4][kNC];
#pragma unroll
    for (int j = 0; j < NCAND; ++j) {
        x[0][j] = L.iv[0]; x[1][j] = L.iv[1]; x[2][j] = L.iv[2]; x[3][j] = L.iv[3];
    }
    // The hand-ordered pipeline starts at step VgprK::kI0 = W0 + KernelTune::kLead of the first
    // block (all four state words are per-lane from W0 + 4 on; earlier steps are wave-uniform or
    // partly so, and the compiler folds them).
    using K = VgprK<NBLK, W0, SH, V::kSpan>;
    constexpr bool kPipe = NCAND == kNC && (kNC == 2 || kNC == 4);
    static_assert(!kPipe || ONLY_D, "VgprK::kEnd0 / kI0 are the hash loop's: the pipeline runs ONLY_D");
    constexpr int kEnd0 = ONLY_D ? K::kEnd0 : 64;
    constexpr int kI0 = kPipe ? K::kI0 : kEnd0;
    md5_steps<NBLK, W0, SH, 0, 0, kI0, NCAND>(x, L, v);
    if constexpr (kPipe) pipe::steps<NBLK, W0, SH, 0, kI0, kEnd0>(x, L, v);
#pragma unroll
    for (int j = 0; j < NCAND; ++j)
#pragma unroll
        for (int w = 0; w < 4; ++w) out[w][j] = (RAW_D && w == 3) ? x[w][j] : L.iv[w] + x[w][j];
    if constexpr (NBLK == 2) {
        constexpr int kEnd1 = ONLY_D ? 62 : 64;
#pragma unroll
        for (int j = 0; j < NCAND; ++j)
#pragma unroll
            for (int w = 0; w < 4; ++w) x[w][j] = out[w][j];
        if constexpr (kPipe)
            pipe::steps<NBLK, W0, SH, 1, 0, kEnd1>(x, L, v);
        else
            md5_steps<NBLK, W0, SH, 1, 0, kEnd1, NCAND>(x, L, v);
#pragma unroll
        for (int j = 0; j < NCAND; ++j)
#pragma unroll
            for (int w = 0; w < 4; ++w) out[w][j] += x[w][j];
    }
}

// V = vs + loff (wave-uniform + per-lane) of slot j.  The lane offset holds the thread-byte bits
// below R and the k bits below 64 / R; vs is zero in both (i0 is a multiple of 64), so the sum
// never carries and V's bits above the lane's k offset are wave-uniform: V >> 24 and V >> 16 are
// uniform, and V >> 8 = (vs >> 8) + (loff >> 8).  d1 = the segment addition to word W0 + 1.
template <int SH, class V>
DPOW_DEV void var_words(V &v, int j, uint32_t vs, uint32_t loff, uint32_t d1) {
    v.lo_s[j] = vs << (8 * SH);
    v.lo_v = loff << (8 * SH);
    if constexpr (SH != 0) {
        v.hi_s[j] = (vs >> (32 - 8 * SH)) + d1;
        v.lane_k = SH == 3 && V::kSpan ? loff >> 8 : 0u;
    } else {
        v.hi_s[j] = 0u;
        v.lane_k = 0u;
    }
}

#if DPOW_VSI
// The four K + M values of word W0 for slot j (one final block), from lo_s / lo_v.
template <int W0, class V>
DPOW_DEV void w0km_fill(V &v, int j, const Launch &L) {
    constexpr int i0 = step_of_word(0, W0), i1 = step_of_word(1, W0), i2 = step_of_word(2, W0),
                  i3 = step_of_word(3, W0);
    v.w0km[0][j] = (L.KT[i0] + v.lo_s[j]) + v.lo_v;
    v.w0km[1][j] = (L.KT[i1] + v.lo_s[j]) + v.lo_v;
    v.w0km[2][j] = (L.KT[i2] + v.lo_s[j]) + v.lo_v;
    v.w0km[3][j] = (L.KT[i3] + v.lo_s[j]) + v.lo_v;
}
#endif

// Full digest test of one lane's candidate (rare path: only when the D-word
// test passed and ntz > 8, i.e. probability 2^-32 per candidate).
// loff: the lane offset, plus (SH = 0) the segment's addition to word W0 (search_body lov);
// sd: the segment's word additions (seg_all_deltas), computed by the caller outside the
// per-lane branch (a dynamic kernarg index inside it moved the hash loop's wave-uniform
// index arithmetic onto the VALU: +10 VALU per wave-block in <1,1,0>, tools/isa_loop.py).
// KS: the kernel's KSPAN (kc holds the constants VgprK<.., KS> selects).
template <int NBLK, int W0, int SH, bool KS>
DPOW_DEV bool full_check(const Launch &L, const KConst &kc, uint32_t vs, uint32_t loff, const uint32_t (&sd)[3]) {
    VarWords<KS> v;
    v.kc = &kc;
    v.seg_d[0] = sd[0];
    v.seg_d[1] = sd[1];
    v.seg_d[2] = sd[2];
    var_words<SH>(v, 0, vs, loff, v.seg_d[0]);
#if DPOW_VSI
    w0km_fill<W0>(v, 0, L);
#endif
    uint32_t out[4][kNC];
    md5_tail<NBLK, W0, SH, 1>(out, L, v);
    return trailing_zero_nibbles(out[0][0], out[1][0], out[2][0], out[3][0]) >= L.ntz;
}

}  // namespace DPOW_KNS
}  // namespace dpow
