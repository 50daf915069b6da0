// md5_search_kernel.h -- the gfx950 proof-of-work search kernel (instantiated per message layout
// by md5_variant.hip).
//
// Replaces the reference miner's inner loop (worker.go:318-400): for every candidate
// threadByte || chunk_k of the worker partition, MD5(nonce || it) and the trailing-'0' test of
// its hex form.  Pure INT32 VALU work: each lane runs an unrolled, register-resident MD5 of the
// final message block(s) of two candidates, software-pipelined in hand-ordered asm groups (see
// pipe::), the message words being wave-uniform (kernel arguments, SGPRs) except the 4 bytes
// threadByte | k_lo << 8, and the bytes of k >> 24 (L >= 4), which change once per 2^24-k
// segment of a launch (the segment words, re-derived per wave).
//
// Work decomposition: local index i = k * R + t (the reference's order, k outer, t inner).  A
// wave-block is 64 * kNC consecutive indices (lane l, slot j -> i0 + 64 j + l).  Worker waves of
// a persistent grid claim chunks of consecutive wave-blocks from 8 per-XCD counters, each in
// increasing order; the first hit of a wave-block (lowest slot, then lowest lane) goes to
// atomicMin on the global index g = k * 256 + threadByte, which is monotone in i, so the minimum
// is the reference's first hit.  A wave stops at the first chunk, or group of DPOW_POLL_WB
// wave-blocks within one, whose first index is >= the current minimum, so every candidate below
// the answer is evaluated and the result is deterministic.
//
// Workgroup 0 of the grid is a watcher: one lane polls the pinned host cancel flag (Found/Cancel,
// worker.go:194,209) and raises Ctrl::stop, which every worker wave reads every DPOW_POLL_WB
// wave-blocks together with Ctrl::best.  The workgroup that retires last writes the launch's
// completion record (Snap) to pinned host memory, which the host polls.
//
// The parts: md5_kernel_tune.h (build knobs, KernelTune: each layout's tuning), md5_hash.h (the
// MD5 and its hand-ordered pipeline), md5_launch_ctl.h (watcher, claims, retirement, wave trace),
// this file (the index-order body and the kernels), md5_search_si.h (the segment-inner body).
#pragma once
#include "md5_kernel_tune.h"
#include "md5_hash.h"
#include "md5_launch_ctl.h"

namespace dpow {
namespace DPOW_KNS {

// Hash one wave-block (64 * kNC consecutive local indices from i0) and publish its first hit, if
// any, to Ctrl::best.  Returns the hit's global index, or kNoHitG.
//
// The per-candidate test is one compare: with EQ (one final block, ntz >= 8) the raw state word
// against -iv[3] (D == 0, no add, no mask); otherwise D <= dle, the even-nibble prefilter of the
// mask, which the rare path (a hit in the wave, 16^-(ntz & ~1) per candidate) re-tests against
// the exact mask.
constexpr uint64_t kNoHitG = ~0ull;

// KSPAN (SH = 3 only): the launch's lanes may span several k (R < 64), so word W0 + 1's
// K + M carries each lane's k offset (VarWords::lane_k, one VALU add per candidate in each
// of that word's four steps).  The SH = 3 kernels of launches with R >= 64 (workerBits <= 2:
// the offset is 0) are instantiated without it: the word's K + M stays a wave-uniform SGPR.
template <int NBLK, int W0, int SH, bool EQ, bool KSPAN>
DPOW_DEV uint64_t hash_wave_block(const Launch &L, const KConst &kc, uint64_t i0, uint32_t lane, uint32_t loff) {
    static_assert(!EQ || NBLK == 1, "the D-equality test needs one final block");
    static_assert(KSPAN || SH == 3, "only the SH = 3 kernels have a narrow (R >= 64) instantiation");
    uint32_t vs[kNC];
    VarWords<KSPAN> v;
    v.kc = &kc;
    v.seg_d[0] = v.seg_d[1] = v.seg_d[2] = 0u;  // unused: the hash loop's segment-word steps all read kc
    uint32_t d1 = 0u;               // SH != 0: the segment addition to word W0 + 1 (both slots share
    if constexpr (SH != 0) {        //  the segment: wave-blocks never straddle one)
        uint32_t d2;
        seg_deltas<W0, SH>(L, (uint32_t)((i0 >> L.rbits) >> 24), d1, d2);
    }
#pragma unroll
    for (int j = 0; j < kNC; ++j) {
        vs[j] = wave_uniform_v(i0 + 64u * j, L.rbits, L.base_tb);
        var_words<SH>(v, j, vs[j], loff, d1);
    }
    uint32_t dig[4][kNC];
    md5_tail<NBLK, W0, SH, kNC, true, EQ>(dig, L, v);  // only D is tested here

    uint64_t bal[kNC];
    uint64_t any = 0;
#pragma unroll
    for (int j = 0; j < kNC; ++j) {
        bal[j] = EQ ? __ballot(dig[3][j] == L.deq) : __ballot(dig[3][j] <= L.dle);
        any |= bal[j];
    }
    // The hit path is written out again in hash_wave_block_si on purpose: shared through one helper
    // (lambda or template flag) it changed all 11 search units (the header split's commit message).
    if (any != 0) {  // rare: lowest valid slot, then lowest lane
#pragma unroll
        for (int j = 0; j < kNC; ++j) {
            const uint64_t ij = i0 + 64u * j;
            uint64_t m = bal[j] & lane_range_mask((int64_t)(L.i_begin - ij), (int64_t)(L.i_end - ij));
            if (!EQ && m != 0) m &= __ballot((dig[3][j] & L.dmask) == 0u);
            if (m != 0 && L.ntz > 8u) {
                uint32_t d0, sd[3];
                seg_all_deltas<NBLK, W0, SH>(L, seg_id((ij < L.i_begin ? L.i_begin : ij) >> L.rbits), d0, sd);
                const bool ok = ((m >> lane) & 1ull) && full_check<NBLK, W0, SH, KSPAN>(L, kc, vs[j], loff, sd);
                m = __ballot(ok);
            }
            if (m != 0) {
                const uint64_t g = global_of_local(ij + (uint64_t)__builtin_ctzll(m), L.rbits, L.base_tb);
                if (lane == 0) {
                    // A returning atomic whose result is consumed: the wave waits (vmcnt)
                    // until the min is performed, before its retirement barrier and the
                    // Ctrl::done increment that lets publish() read Ctrl::best.
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

template <int NBLK, int W0, int SH, bool EQ, bool KSPAN>
DPOW_DEV void search_body(const Launch &L) {
    if (blockIdx.x == 0) {  // dispatched first: the watcher
        watcher(L);
        return;
    }
    constexpr bool kPoll = KernelTune<NBLK, W0, SH, KSPAN>::kPoll;
    WaveTrace wt;
    wt.start();
    // The 4-byte-nonce D-equality kernel (<1,1,0,eq>, the sweep's and N >= 8's), not the
    // chunk-length-spanning unit: kPad4B s_nop in front of the worker path put its hash
    // block at round 4's offset modulo 256 (tests/test_isa.py checks it).  Any change to the
    // watcher re-runs the whole kernel's register allocation (it is inlined: a noinline
    // watcher costs the hash block 24 VALU per wave-block), and the one-round-trip poll moved
    // the hash block by 4 bytes; a move of that kind alone cost the sweep 0.5 % in round 5
    // (profiles/r05_ab.json[r05q/ab.log]).  Padded: 218.8 vs 218.7 GH/s ([r05s/ab.log]).
    if constexpr (EQ && NBLK == 1 && W0 == 1 && SH == 0 && !DPOW_VLS)
        asm volatile(".rept %0\n s_nop 0\n .endr" ::"i"(kPad4B));
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t loff = lane_offset(L.rbits, lane);
    KConst kc;
    kconst_init<NBLK, W0, SH, 0, 0, KSPAN>(kc, L);
    // The 2^24-k segment kc's segment-word constants belong to; kept in a VGPR
    // (wave-uniform, read once per group): an SGPR live across the hash loop
    // costs spill reloads inside it under the 80-SGPR budget.
    uint32_t cur_seg_v;
    asm("v_mov_b32 %0, %1" : "=v"(cur_seg_v) : "s"(L.seg0));
    // SH = 0: the lane offset plus the current segment's addition to word W0 (the 0x80 pad
    // of chunk lengths <= 2 in launches spanning chunk lengths; 0 in the template's own
    // segment), the per-lane part of W0's K + M.
    uint32_t lov = loff;

    unsigned long long best = __hip_atomic_load(&L.ctrl->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    best = best < L.bound0 ? best : L.bound0;
    uint32_t stop = __hip_atomic_load(&L.ctrl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // Waves claim chunks of L.chunk consecutive wave-blocks from their XCD's counter, which hands
    // its chunks out in increasing index order (the early exit stays exact); neither the grid size
    // nor the residency creates a tail.  The next claim is requested while the current chunk is
    // hashed.  A launch that starts at or above the best index (queued behind a hit) or after a
    // cancel claims nothing: a contended counter serves < 90 claims/us.  Worker block b (>= 1)
    // serves counter (b - 1) % 8; the host launches at least min(n_chunks, 8) worker blocks, so
    // every counter holding a chunk has waves.  Workgroups go round-robin to XCDs, so each
    // counter's waves share one XCD.
    // Tail priority: older waves win the SIMD's issue arbitration, so the youngest waves of
    // a CU barely progress until the launch drains, and then finish chunks they claimed
    // early.  Every worker wave runs at priority 1 and drops to 0 once it holds a tail
    // claim: the waves still on earlier chunks issue first.  profiles/r01_ab_tail_prio.log:
    // sweep windows at workerBits 3 (2^29-candidate launches) 209.5 -> 212.8 GH/s,
    // workerBits 0 217.4 -> 218.3.
    __builtin_amdgcn_s_setprio(1);
    // A wave requests its next claim while it hashes the current chunk (profiles/
    // r02_ab_ahead.log: 217.6 against 215.5 GH/s for one claim in flight per wave).  With
    // kDeferClaims (one-block kernels) the claim's atomic is issued in the chunk's last poll
    // group and its result read after the chunk: a slow wave does not sit on an early chunk
    // for the whole of its current one, and the polls of the chunk's earlier groups do not
    // wait for the claim atomic (vmcnt counts in issue order; round 4, profiles/
    // r04_node_ab.log: +0.03 to +0.24 %).  The deferred read holds the claim's value in two
    // more VGPRs across the hash loop; the two-block kernels sit at 71-79 VGPRs, where that
    // costs a wave per SIMD or shifts their register assignment (-5 to -10 %,
    // profiles/r02_ab_layouts/), so they read the claim in front of the chunk.
    constexpr bool kDeferClaims = NBLK == 1;
    uint32_t x = (blockIdx.x - 1u) % kClaimCounters;
    const bool skip = stop != 0u || global_of_local(L.i_begin, L.rbits, L.base_tb) >= best;
    const uint64_t cbase = kStaticFirst ? L.n_static : 0;
    uint64_t claim;
    if constexpr (kStaticFirst) {
        const uint32_t wave_id =
            __builtin_amdgcn_readfirstlane((blockIdx.x - 1u) * (kBlockThreads / 64) + threadIdx.x / 64u);
        claim = skip ? L.n_chunks
                     : (wave_id < cbase ? (uint64_t)wave_id : claim_next(L.claim + x * kClaimStride, x, lane, cbase));
    } else {
        claim = skip ? L.n_chunks : claim_next(L.claim + x * kClaimStride, x, lane, cbase);
    }
    wt.first_claim(claim);
    uint32_t hops = 0;
    for (;;) {
        // This counter is drained: move on to the next one (its waves may sit
        // on a slower XCD).  A counter only ever drains, so after a full round
        // of drained counters every chunk has been handed out.
        if (claim >= L.n_chunks) {
            wt.left(1);
            if (skip || ++hops >= kClaimCounters) break;
            x = (x + 1u) % kClaimCounters;
            const unsigned long long seen =
                __hip_atomic_load(L.claim + x * kClaimStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            claim = seen * kClaimCounters + x + cbase < L.n_chunks
                        ? claim_next(L.claim + x * kClaimStride, x, lane, cbase)
                        : L.n_chunks;
            continue;
        }
        // kDeferClaims: the next claim's atomic is issued in the chunk's last group and its
        // result read after the chunk (claim_take); else the next claim is taken now.
        unsigned long long next_v = 0;
        uint64_t next = 0;
        bool issued = false;  // kDeferClaims: the next claim's atomic was issued (in the chunk's last group)
        if constexpr (kDeferClaims) (void)issued;
        else next = claim_next(L.claim + x * kClaimStride, x, lane, cbase);
        // Claims [0, n_big) are `chunk` wave-blocks, the rest `chunk_tail`: the
        // launch ends on small claims, so its waves run dry within a few
        // wave-blocks of each other (the tail of a 2.5 ms launch was ~3 %).
        // The claim's span is written out again in search_body_si on purpose: moved into one
        // helper it changed units <1,3>, <2,0>, <2,3> and "_ls" (the header split's commit message).
        const bool big = claim < L.n_big;
        if (!big) __builtin_amdgcn_s_setprio(0);
        const uint64_t b_begin = big ? claim * L.chunk : L.n_big * L.chunk + (claim - L.n_big) * L.chunk_tail;
        const uint32_t csz = big ? L.chunk : L.chunk_tail;
        const uint32_t nb = (uint32_t)(b_begin + csz < L.n_wblocks ? csz : L.n_wblocks - b_begin);
        const uint64_t i_first = L.wb_begin + b_begin * (uint64_t)kWaveBlock;
        // Early exit at a claim: stop on a cancel, or once this chunk starts at
        // or above the best index found so far.
        // Everything below the best has been or is being hashed by earlier claims.
        if (stop != 0u ||
            global_of_local(i_first < L.i_begin ? L.i_begin : i_first, L.rbits, L.base_tb) >= best) {
            wt.left(stop != 0u ? 3 : 2);
            break;
        }
        wt.chunk(claim);
        // The chunk runs in groups of L.poll_wb wave-blocks.  Each group's loads of Ctrl::best /
        // Ctrl::stop are issued before it and consumed after it (the latency hides behind the
        // hashing), so a hit elsewhere or a cancel ends this wave within one group, not at the
        // chunk's end.  A hit of this wave ends the chunk at once: its later wave-blocks hold larger
        // indices.  Down-counters keep the loop's live SGPRs at a plain loop's count.
        uint64_t i0 = i_first;
        uint32_t left = nb;
        // (some two-block layouts: the compile-time group, KernelTune::kPoll)
        const uint32_t poll_wb = kPoll ? L.poll_wb : (uint32_t)DPOW_POLL_WB;
        for (;;) {
            uint32_t q = left < poll_wb ? left : poll_wb;
            // A chunk never straddles a 2^24-k segment boundary (the host aligns a
            // spanning launch's chunks to them, plan.cpp size_launch), so neither does a
            // group; entering another segment re-derives the segment words' K + M
            // constants.  (Splitting groups at boundaries in the kernel instead
            // costs 4 SGPR spill reloads per wave-block: tools/isa_loop.py.)
            {
                // (from the launch's first index: a wave-block below it may hold k = 0, whose
                // lanes are masked off and whose chunk length differs from its neighbours')
                const uint32_t sg = seg_id((i0 < L.i_begin ? L.i_begin : i0) >> L.rbits);
                if (sg != __builtin_amdgcn_readfirstlane(cur_seg_v)) {
                    asm volatile("v_mov_b32 %0, %1" : "=v"(cur_seg_v) : "s"(sg));
                    uint32_t d0, d[3];
                    seg_all_deltas<NBLK, W0, SH>(L, sg, d0, d);
                    kconst_seg<NBLK, W0, SH, 0, 0, KSPAN>(kc, L, d);
                    if constexpr (SH == 0) lov = lane_offset(L.rbits, lane) + d0;
                }
            }
            left -= q;
            if constexpr (kDeferClaims) {
                if (left == 0) {  // the chunk's last group: reserve the next chunk now
                    next_v = claim_issue<true>(L.claim + x * kClaimStride, lane);
                    issued = true;
                }
            }
            const unsigned long long best_seen =
                __hip_atomic_load(&L.ctrl->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t stop_seen = __hip_atomic_load(&L.ctrl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bool hit = false;
            for (; q != 0; --q, i0 += (uint64_t)kWaveBlock) {
                wt.wave_block();
                const uint64_t g = hash_wave_block<NBLK, W0, SH, EQ, KSPAN>(L, kc, i0, lane, SH == 0 ? lov : loff);
                if (g != kNoHitG) {
                    best = g < best ? g : best;
                    hit = true;
                    break;
                }
            }
            wt.hit(hit);  // (after the loop: even an empty call inside the hit branch moved the kernels' code)
            best = best_seen < best ? best_seen : best;
            stop = stop_seen;
            if (hit || left == 0 || stop != 0u || global_of_local(i0, L.rbits, L.base_tb) >= best) break;
        }
        if constexpr (kDeferClaims) {
            // left the chunk before its last group (a hit, a bound, a stop): every later chunk
            // is at or above the best, or the launch is stopping -- nothing more to claim
            if (!issued) {
                wt.left(4);
                break;
            }
            claim = claim_take(next_v, x, cbase);
        } else {
            claim = next;
        }
    }
    // Retirement is counted per workgroup (a quarter of the atomics on the shared counter).  Each
    // wave's atomicMin has been performed already (the hit path consumes the returning atomic's
    // result, which waits on vmcnt); the barrier then covers all four waves, so the Ctrl::done
    // increment -- and publish(), which reads Ctrl::best -- come after every hit of the workgroup.
    // The workgroup whose count completes the launch publishes its completion record (retire).
    wt.store(lane);
    if constexpr (kDeferClaims) {
        // A wave that left the loop right after issuing its next claim (a hit below the
        // chunk, a bound, a cancel) still has that atomic in flight; the last retiring
        // workgroup re-zeroes the launch's claim counters in publish(), and a claim
        // landing after that would leave the slot's next user one chunk short.  Every
        // claim of the workgroup is performed before its retirement count.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    wt.claims_performed();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0) {
        wt.barrier_passed();
        if constexpr (kXcdRetire) {
            // Retirement is counted per claim counter first (worker block b serves counter
            // (b - 1) % 8, its XCD's) on a word of that counter's line, and the counter's last
            // workgroup adds the counter's count to Ctrl::done: a launch's few hundred to ~1500
            // retirements no longer queue on one line (~100 atomics per us) at its end.
            const uint32_t n_wg = gridDim.x - 1u;
            const uint32_t xr = (blockIdx.x - 1u) % kClaimCounters;
            const uint32_t nx = n_wg / kClaimCounters + (xr < n_wg % kClaimCounters ? 1u : 0u);
            unsigned long long *const xc = L.claim + xr * kClaimStride + 2;
            const unsigned long long px = __hip_atomic_fetch_add(xc, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (px + 1ull == (unsigned long long)nx) {
                // every retirement of this counter is in: zero it for the slot's next launch
                __hip_atomic_store(xc, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t prev = __hip_atomic_fetch_add(&L.ctrl->done, nx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                wt.counted(L, prev, nx);
                retire(L, prev + nx, kPoll ? L.ctrl_next : nullptr);
            }
        } else {
            const uint32_t prev = __hip_atomic_fetch_add(&L.ctrl->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            wt.counted(L, prev, 1u);
            retire(L, prev + 1u, kPoll ? L.ctrl_next : nullptr);
        }
    }
}

}  // namespace DPOW_KNS
}  // namespace dpow

#if DPOW_VSI
#include "md5_search_si.h"
#define DPOW_SEARCH_BODY(NBLK, W0, SH, EQ, KSPAN) search_body_si<NBLK, W0, SH, EQ>(L)
#else
#define DPOW_SEARCH_BODY(NBLK, W0, SH, EQ, KSPAN) search_body<NBLK, W0, SH, EQ, KSPAN>(L)
#endif

namespace dpow {
namespace DPOW_KNS {

// One kernel template per SGPR budget class (KernelTune::kSgpr; md5_variant.hip kernel_of).
#define DPOW_KERNEL(NAME, SGPRS)                                                                         \
    template <int NBLK, int W0, int SH, bool EQ, bool KSPAN>                                             \
    __global__ void __launch_bounds__(kBlockThreads) __attribute__((amdgpu_num_sgpr(SGPRS))) NAME(const Launch L) { \
        DPOW_SEARCH_BODY(NBLK, W0, SH, EQ, KSPAN);                                                       \
    }
DPOW_KERNEL(md5_search_kernel, DPOW_NUM_SGPR)
DPOW_KERNEL(md5_search_kernel_lsgpr, DPOW_NUM_SGPR_LONG)
DPOW_KERNEL(md5_search_kernel_w15sgpr, DPOW_NUM_SGPR_W15)
#undef DPOW_KERNEL

}  // namespace DPOW_KNS
}  // namespace dpow
