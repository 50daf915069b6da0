// md5_search_si.h -- the segment-inner body of the search kernel (DPOW_VSI, md5_variant.hip's
// "_si" unit only; included by md5_search_kernel.h), for launches in segment-inner order
// (Launch::n_seg != 0; one final block, SH = 0, the D-equality test).
//
// The launch's window lies in n_seg consecutive 2^24-k segments from segment seg_first.
// Its wave-blocks are those of ONE segment's local-index range: wave-block b is the 64 * kNC
// indices from offset o = b * 64 * kNC of a segment (wb_begin = the first segment's first
// index, n_wblocks = a segment's wave-blocks), and the wave that claims it hashes it in every
// segment s whose copy wb_begin + (s << (24 + rbits)) + o intersects [i_begin, i_end), s
// increasing.  Word W0 (threadByte | k_lo24 << 8) depends on o and the lane only, word W0 + 1
// (k >> 24) on s only, so per wave-block and slot the wave computes once
//   - step W0 whole (its inputs: the uniform state of steps 0 .. W0 - 1 and the lane's W0),
//   - a + F(b, c, d) of step W0 + 1 (F's inputs are the step-W0 word and uniform words),
//   - K + M[W0] of the three later steps that read word W0,
// and each segment's hash starts at step W0 + 1 with add(P, K + M[W0 + 1]), rotate, add.
//
// Exactness: the answer is still the atomicMin over global indices.  (o, s) -> index is
// increasing in s, so a wave-block leaves its segment loop at the first s whose first index
// is at or above the best seen, or on a hit of its own; a claim whose first wave-block has no
// segment below the best ends the wave (every later wave-block lies higher in every segment).
// Every candidate below the returned index is hashed.
#pragma once

namespace dpow {
namespace DPOW_KNS {

constexpr uint32_t kSegLimitNone = 0xFFFFFFFFu;

// Smallest local index whose global index is >= g (global_of_local is increasing).
DPOW_DEV uint64_t local_ceil_of_global(uint64_t g, uint32_t rbits, uint32_t base_tb) {
    const uint64_t k = g >> 8;
    const uint32_t tb = (uint32_t)(g & 0xFFu);
    if (tb < base_tb) return k << rbits;
    const uint32_t t = tb - base_tb;
    return t >> rbits ? (k + 1u) << rbits : (k << rbits) + t;
}

// The segments of a wave-block at segment offset o that lie below the best index: s < q, and
// s == q when o < r, for (q, r) = the best's local index relative to wb_begin, split at a
// segment's size.
struct SegLimit {
    uint32_t q, r;
};
DPOW_DEV SegLimit seg_limit_of(const Launch &L, unsigned long long best) {
    const uint32_t segbits = 24u + L.rbits;
    const uint64_t ib = local_ceil_of_global(best, L.rbits, L.base_tb);
    const uint64_t rel = ib > L.wb_begin ? ib - L.wb_begin : 0ull;
    const uint64_t q = rel >> segbits;
    SegLimit l;
    l.q = q >= (uint64_t)kSegLimitNone ? kSegLimitNone - 1u : (uint32_t)q;
    l.r = (uint32_t)(rel - (q << segbits));
    return l;
}
DPOW_DEV uint32_t seg_limit_at(const SegLimit &l, uint32_t o) { return l.q + (o < l.r ? 1u : 0u); }

// The lane invariants of one wave-block: the state after step W0 and step W0 + 1's a + F.
template <int NBLK, int W0, int SH>
DPOW_DEV void seg_invariants(uint32_t (&x)[4][kNC], uint32_t (&p)[kNC], const Launch &L, VarWords<true> &v) {
#pragma unroll
    for (int j = 0; j < kNC; ++j) {
        x[0][j] = L.iv[0]; x[1][j] = L.iv[1]; x[2][j] = L.iv[2]; x[3][j] = L.iv[3];
    }
    md5_steps<NBLK, W0, SH, 0, 0, W0 + 1, kNC>(x, L, v);
    using R = Roles<W0 + 1>;
#pragma unroll
    for (int j = 0; j < kNC; ++j) {
        p[j] = x[R::a][j] + md5_fn<W0 + 1>(x[R::b][j], x[R::c][j], x[R::d][j]);
        // held in VGPRs across the segment loop, not recomputed in it
        asm volatile("" : "+v"(p[j]), "+v"(x[Roles<W0>::a][j]));
        asm volatile("" : "+v"(v.w0km[1][j]), "+v"(v.w0km[2][j]), "+v"(v.w0km[3][j]));
    }
}

// One wave-block of segment s (v.seg_d[0] = s: the addition to word W0 + 1): steps W0 + 1 .. 61
// from the invariants, the D-equality test and the hit path of hash_wave_block.
template <int NBLK, int W0, int SH>
DPOW_DEV uint64_t hash_wave_block_si(const Launch &L, const KConst &kc, const uint32_t (&xin)[4][kNC],
                                     const uint32_t (&p)[kNC], const VarWords<true> &v, const uint32_t (&vs)[kNC],
                                     uint32_t s, uint32_t o, uint32_t lane, uint32_t loff) {
    using K = VgprK<NBLK, W0, SH, true>;
    static_assert(K::Tune::kLead >= 2, "steps W0 and W0 + 1 precede the hand-ordered pipeline");
    uint32_t x[4][kNC];
#pragma unroll
    for (int j = 0; j < kNC; ++j)
#pragma unroll
        for (int w = 0; w < 4; ++w) x[w][j] = xin[w][j];
    {
        using R = Roles<W0 + 1>;
        const uint32_t km = L.KT[W0 + 1] + v.seg_d[0];
#pragma unroll
        for (int j = 0; j < kNC; ++j) x[R::a][j] = x[R::b][j] + __builtin_rotateleft32(p[j] + km, md5_shift(W0 + 1));
    }
    md5_steps<NBLK, W0, SH, 0, W0 + 2, K::kI0, kNC>(x, L, v);
    pipe::steps<NBLK, W0, SH, 0, K::kI0, K::kEnd0>(x, L, v);

    uint64_t bal[kNC];
    uint64_t any = 0;
#pragma unroll
    for (int j = 0; j < kNC; ++j) {
        bal[j] = __ballot(x[3][j] == L.deq);
        any |= bal[j];
    }
    // The hit path is hash_wave_block's, written out again on purpose: shared through one helper
    // (lambda or template flag) it changed all 11 search units (the header split's commit message).
    if (any != 0) {  // rare: lowest valid slot, then lowest lane
        const uint64_t i0 = L.wb_begin + ((uint64_t)s << (24u + L.rbits)) + o;
#pragma unroll
        for (int j = 0; j < kNC; ++j) {
            const uint64_t ij = i0 + 64u * j;
            uint64_t m = bal[j] & lane_range_mask((int64_t)(L.i_begin - ij), (int64_t)(L.i_end - ij));
            if (m != 0 && L.ntz > 8u) {
                const uint32_t sd[3] = {v.seg_d[0], 0u, 0u};
                const bool ok = ((m >> lane) & 1ull) && full_check<NBLK, W0, SH, true>(L, kc, vs[j], loff, sd);
                m = __ballot(ok);
            }
            if (m != 0) {
                const uint64_t g = global_of_local(ij + (uint64_t)__builtin_ctzll(m), L.rbits, L.base_tb);
                if (lane == 0) {
                    // (a returning atomic whose result is consumed: hash_wave_block)
                    const unsigned long long prev = __hip_atomic_fetch_min(
                        &L.ctrl->best, (unsigned long long)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("; dpow: atomicMin performed (%0)" ::"v"(prev));
                }
                return g;
            }
        }
    }
    return kNoHitG;
}

template <int NBLK, int W0, int SH, bool EQ>
DPOW_DEV void search_body_si(const Launch &L) {
    static_assert(NBLK == 1 && SH == 0 && EQ && W0 + 1 != 16 * NBLK - 2,
                  "segment-inner: one final block, SH = 0, D-equality, W0 + 1 not the bit-length word");
    if (blockIdx.x == 0) {  // dispatched first: the watcher
        watcher(L);
        return;
    }
    if constexpr (DPOW_SI_PAD > 0) asm volatile(".rept %0\n s_nop 0\n .endr" ::"i"(DPOW_SI_PAD));
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t loff = lane_offset(L.rbits, lane);
    KConst kc;
    kconst_init<NBLK, W0, SH, 0, 0, true>(kc, L);

    unsigned long long best = __hip_atomic_load(&L.ctrl->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    best = best < L.bound0 ? best : L.bound0;
    uint32_t stop = __hip_atomic_load(&L.ctrl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // Claims, claim-ahead, guided tail, tail priority and retirement as in search_body; a
    // claim's wave-blocks are wave-blocks of a segment's range, each hashed in every segment.
    __builtin_amdgcn_s_setprio(1);
    uint32_t x = (blockIdx.x - 1u) % kClaimCounters;
    const bool skip = stop != 0u || global_of_local(L.i_begin, L.rbits, L.base_tb) >= best;
    uint64_t claim = skip ? L.n_chunks : claim_next(L.claim + x * kClaimStride, x, lane, 0);
    const uint32_t segbits = 24u + L.rbits;
    SegLimit lim = seg_limit_of(L, best);
    // Ctrl::best / Ctrl::stop once per poll_wb hashed wave-blocks, whichever wave-block or
    // claim they belong to: the loads are issued at one poll and consumed at the next.
    uint32_t pc = L.poll_wb;
    unsigned long long best_seen = __hip_atomic_load(&L.ctrl->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t stop_seen = __hip_atomic_load(&L.ctrl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t hops = 0;
    for (;;) {
        if (claim >= L.n_chunks) {  // this counter is drained: the next one (search_body)
            if (skip || ++hops >= kClaimCounters) break;
            x = (x + 1u) % kClaimCounters;
            const unsigned long long seen =
                __hip_atomic_load(L.claim + x * kClaimStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            claim = seen * kClaimCounters + x < L.n_chunks ? claim_next(L.claim + x * kClaimStride, x, lane, 0)
                                                           : L.n_chunks;
            continue;
        }
        unsigned long long next_v = 0;
        bool issued = false;
        // The claim's span is search_body's, written out again on purpose: moved into one helper
        // it changed units <1,3>, <2,0>, <2,3> and "_ls" (the header split's commit message).
        const bool big = claim < L.n_big;
        if (!big) __builtin_amdgcn_s_setprio(0);
        const uint64_t b_begin = big ? claim * L.chunk : L.n_big * L.chunk + (claim - L.n_big) * L.chunk_tail;
        const uint32_t csz = big ? L.chunk : L.chunk_tail;
        const uint32_t nb = (uint32_t)(b_begin + csz < L.n_wblocks ? csz : L.n_wblocks - b_begin);
        uint32_t o = (uint32_t)(b_begin * (uint64_t)kWaveBlock);  // < 2^(24 + rbits) <= 2^32
        bool over = false;  // nothing below the best is left from this wave-block on
        for (uint32_t left = nb; left != 0 && stop == 0u; --left, o += (uint32_t)kWaveBlock) {
            // the segments [s, s_hi) in which this wave-block intersects the window
            uint32_t s = L.wb_begin + o + (uint64_t)kWaveBlock <= L.i_begin ? 1u : 0u;
            const uint32_t s_hi =
                L.n_seg - (L.wb_begin + ((uint64_t)(L.n_seg - 1u) << segbits) + o >= L.i_end ? 1u : 0u);
            uint32_t s_end = seg_limit_at(lim, o);
            if (s_end == 0u) {  // the best lies in the first segment at or below o: so does it for every later o
                over = true;
                break;
            }
            s_end = s_end < s_hi ? s_end : s_hi;
            if (left == 1u) {  // the claim's last wave-block: reserve the next claim now
                next_v = claim_issue<true>(L.claim + x * kClaimStride, lane);
                issued = true;
            }
            if (s >= s_end) continue;  // no segment of this wave-block is both in the window and below the best
            uint32_t vs[kNC];
            VarWords<true> v;
            v.kc = &kc;
            v.seg_d[0] = v.seg_d[1] = v.seg_d[2] = 0u;
#pragma unroll
            for (int j = 0; j < kNC; ++j) {
                vs[j] = wave_uniform_v(L.wb_begin + o + 64u * j, L.rbits, L.base_tb);
                var_words<SH>(v, j, vs[j], loff, 0u);
                w0km_fill<W0>(v, j, L);
            }
            uint32_t xin[4][kNC], p[kNC];
            seg_invariants<NBLK, W0, SH>(xin, p, L, v);
            for (; s < s_end; ++s) {
                v.seg_d[0] = s;
                if constexpr (DPOW_SI_VSEG != 0) {
                    const uint32_t d[3] = {s, 0u, 0u};
                    kconst_seg<NBLK, W0, SH, 0, 0, true>(kc, L, d);
                }
                const uint64_t g = hash_wave_block_si<NBLK, W0, SH>(L, kc, xin, p, v, vs, s, o, lane, loff);
                if (g != kNoHitG) {  // later segments of this wave-block lie above it
                    best = g < best ? g : best;
                    lim = seg_limit_of(L, best);
                    s_end = s;
                }
                if (--pc == 0u) {
                    pc = L.poll_wb;
                    const bool lower = best_seen < best;
                    best = lower ? best_seen : best;
                    stop = stop_seen;
                    best_seen = __hip_atomic_load(&L.ctrl->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    stop_seen = __hip_atomic_load(&L.ctrl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (lower) {
                        lim = seg_limit_of(L, best);
                        const uint32_t e = seg_limit_at(lim, o);
                        s_end = e < s_end ? e : s_end;
                    }
                    if (stop != 0u) s_end = s;
                }
            }
        }
        if (stop != 0u || over || !issued) break;
        claim = claim_take(next_v, x, 0);
    }
    // (a claim atomic may still be in flight: search_body)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0)
        retire(L, __hip_atomic_fetch_add(&L.ctrl->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u, L.ctrl_next);
}

}  // namespace DPOW_KNS
}  // namespace dpow
