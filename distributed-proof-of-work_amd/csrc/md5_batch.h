// md5_batch.h -- the batched search (dpow_search_batch): definitions shared by the generic
// gfx950 kernel (md5_batch.hip), its host loop and planner (batch.cpp), the task queue that launches
// the same kernel code one descriptor per workgroup (queue.cpp) and the launch engine under both
// (batch_engine.h).
//
// One kernel hashes B independent tasks over one grid.  Unlike the specialised kernels of
// md5_search_kernel.h, whose message layout (NBLK, W0, SH) is a template parameter, a batch mixes
// layouts, so here the layout is data: a task table in device memory holds each task's midstate,
// the final-block template of its nonce tail and its byte position p = nonce_len % 64, and every
// candidate assembles threadByte || chunk_k || 0x80 at byte p itself (batch_candidate_words, the
// one piece of code behind both the kernel and dpow_batch_candidate).
#pragma once

#include <stddef.h>

#include "dpow_common.h"

namespace dpow {

// One task of the device task table (read-only while a batch runs: the kernel reads it with
// scalar loads).  The task's atomicMin target lives in a separate array (BatchLaunch::best).
struct BatchTask {
    uint32_t iv[4];     // chaining value after the whole 64-byte blocks of the nonce (md5_host)
    uint32_t T[16];     // final-block template: the nonce's last p bytes, the rest zero
    uint32_t p;         // nonce_len % 64: the byte the threadByte goes to
    uint32_t rbits;     // R = 1 << rbits threadBytes per k
    uint32_t base_tb;   // uint8(worker_byte << rbits)
    uint32_t ntz;       // requested trailing zeros
    uint32_t len_bits;  // 8 * (nonce_len + 1): the message's bit length at chunk length 0
    uint32_t dmask;     // tail_nibble_mask(min(ntz, 8)): the prefilter on the digest's D word
    uint32_t pad_[6];
};
static_assert(sizeof(BatchTask) == 128, "one task per 128-byte line");

// One live task of a launch (pinned host memory, read by the kernel): the slice of its local
// index range this launch covers.  Workgroup b of the launch hashes group b / n_live of entry
// b % n_live (chunk-major: group c of every task comes before group c + 1 of any).
struct BatchEntry {
    uint64_t i_begin, i_end;  // local indices k * R + t
    uint32_t task;            // index into the task table
    uint32_t pad_[3];
};
static_assert(sizeof(BatchEntry) == 32, "one entry per 32 bytes");

// Completion record of a launch (pinned): written by the launch's last retiring workgroup after
// the live tasks' best values (BatchLaunch::out_best); the host polls seq.
struct BatchRecord {
    uint32_t seq;  // launch number + 1 (0: never written)
    uint32_t pad_;
    unsigned long long t_start, t_end;  // s_memrealtime ticks (kRealtimeNs each)
};

struct BatchLaunch {
    unsigned long long *best;      // per task: lowest hit's global index (starts at the task's bound)
    unsigned long long *out_best;  // pinned: best of live entry j, copied out at the end of the launch
    BatchRecord *rec;              // pinned
    uint32_t *done;                // workgroups retired (zero at launch start; the last one re-zeroes it)
    unsigned long long *t0;        // device word: the launch's start tick
    uint32_t n_live;               // entries of the launch's map
    uint32_t group;                // local indices per workgroup
    uint32_t n_blocks;             // rows * n_live
    uint32_t seq;
};

// The task queue (queue.cpp) launches queue_kernel over the same table: there a BatchEntry is one
// workgroup's descriptor -- [i_begin, i_end) is the workgroup's own range, at most kBatchMaxGroup
// local indices, and `task` the table slot -- and BatchLaunch::n_live counts the launch's live-slot
// list (out_best[q] = best of slot out_slots[q]); BatchLaunch::group is unused.

// One newly filled slot of the queue's task table, in pinned memory (queue_upload).
struct QueueRow {
    BatchTask t;
    unsigned long long best;  // the task's bound
    uint32_t slot;
    uint32_t pad_;
};
static_assert(sizeof(QueueRow) == 144 && offsetof(QueueRow, best) == sizeof(BatchTask), "the best follows the row");

// Chunk length of k (nextChunk^k, worker.go:234-244): the minimal little-endian bytes of k.
DPOW_HD uint32_t batch_chunk_len(uint64_t k) {
    return k ? (uint32_t)(71 - __builtin_clzll(k)) >> 3 : 0u;
}

// The local index range of workgroup row `row` of entry e (false: nothing left in that row).
DPOW_HD bool batch_block_range(uint64_t i_begin, uint64_t i_end, uint32_t row, uint32_t group, uint64_t &lo,
                               uint64_t &hi) {
    lo = i_begin + (uint64_t)row * group;
    if (lo >= i_end) return false;
    hi = i_end - lo > group ? lo + group : i_end;
    return true;
}

// The final block(s) of local index i: M[0..16 nblk) (M[16..32) is zero when one block does).
// msg = nonce || threadByte || chunk_k, the 0x80 pad behind it and the bit length in the last
// block's word 14; two blocks when p + 1 + L > 55.  The 9 bytes threadByte || chunk (<= 7) ||
// 0x80 are one 72-bit value shifted to byte p: three words from word W0 = p / 4.
// W0C >= 0 is p / 4 as a compile-time constant: the kernel branches once per workgroup on the
// wave-uniform p / 4 (batch_with_w0), so that the 13 words without variable bytes stay the
// template's (scalar registers, folded into the step constants) and, for W0 <= 11, the second
// block is known not to exist.  Every word index is a compile-time constant: M never leaves the
// registers.
template <int W0C>
DPOW_HD uint32_t batch_candidate_words_at(const uint32_t *T, uint32_t p, uint32_t rbits, uint32_t base_tb,
                                          uint32_t len_bits, uint64_t i, uint32_t M[32]) {
    const uint64_t k = i >> rbits;
    const uint32_t tb = base_tb | (uint32_t)(i & ((1ull << rbits) - 1ull));
    const uint32_t L = batch_chunk_len(k);
    uint64_t lo = (uint64_t)tb | (k << 8);  // k < 2^55
    uint32_t hi = 0u;
    if (L < 7u) lo |= 0x80ull << (8u * (1u + L));
    else hi = 0x80u;
    static_assert(W0C >= 0 && W0C <= 15, "W0 = p / 4, p < 64");
    constexpr uint32_t w0 = (uint32_t)W0C;
    const uint32_t sh = 8u * (p & 3u);
    const uint64_t los = lo << sh;
    const uint32_t X0 = (uint32_t)los, X1 = (uint32_t)(los >> 32);
    const uint32_t X2 = (sh ? (uint32_t)(lo >> (64u - sh)) : 0u) | (hi << sh);
    // p + 1 + L <= 4 W0 + 11: one block for every W0 <= 11
    const uint32_t nblk = W0C <= 11 ? 1u : p + 1u + L > 55u ? 2u : 1u;
    const uint32_t bits = len_bits + 8u * L;
#pragma unroll
    for (uint32_t w = 0; w < 32; ++w) {
        uint32_t m = w < 16 ? T[w] : 0u;
        if (w == w0) m |= X0;
        if (w == w0 + 1u) m |= X1;
        if (w == w0 + 2u) m |= X2;
        if (w == 14) m |= nblk == 1u ? bits : 0u;
        if (w == 30) m |= nblk == 2u ? bits : 0u;
        M[w] = m;
    }
    return nblk;
}

// f.template operator()<W0>() for the wave-uniform W0 = w0 (0..15).
template <typename F>
DPOW_HD void batch_with_w0(uint32_t w0, F &&f) {
    switch (w0) {
        case 0: f.template operator()<0>(); break;
        case 1: f.template operator()<1>(); break;
        case 2: f.template operator()<2>(); break;
        case 3: f.template operator()<3>(); break;
        case 4: f.template operator()<4>(); break;
        case 5: f.template operator()<5>(); break;
        case 6: f.template operator()<6>(); break;
        case 7: f.template operator()<7>(); break;
        case 8: f.template operator()<8>(); break;
        case 9: f.template operator()<9>(); break;
        case 10: f.template operator()<10>(); break;
        case 11: f.template operator()<11>(); break;
        case 12: f.template operator()<12>(); break;
        case 13: f.template operator()<13>(); break;
        case 14: f.template operator()<14>(); break;
        default: f.template operator()<15>(); break;
    }
}

// The words of one candidate through the kernel's own path (the branch on p / 4 and the
// compile-time-W0 assembly): what dpow_batch_candidate returns.
struct BatchWordsCall {
    const uint32_t *T;
    uint32_t p, rbits, base_tb, len_bits;
    uint64_t i;
    uint32_t *M;
    uint32_t nblk;
    template <int W0>
    DPOW_HD void operator()() {
        nblk = batch_candidate_words_at<W0>(T, p, rbits, base_tb, len_bits, i, M);
    }
};
DPOW_HD uint32_t batch_candidate_words(const uint32_t *T, uint32_t p, uint32_t rbits, uint32_t base_tb,
                                       uint32_t len_bits, uint64_t i, uint32_t M[32]) {
    BatchWordsCall c{T, p, rbits, base_tb, len_bits, i, M, 0u};
    batch_with_w0(p >> 2, c);
    return c.nblk;
}

// Steps I..63 of one MD5 compression (RFC 1321 3.4), compiler-scheduled.  A template recursion, not
// a loop: the step number, its constant, rotation and message word are compile-time constants in
// every instance (a `#pragma unroll` loop here was left partly rolled by the compiler, with M
// indexed through a register index).
template <int I>
DPOW_HD void batch_md5_steps(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, const uint32_t *M) {
    if constexpr (I < 64) {
        uint32_t f;
        if constexpr (I < 16) f = (b & c) | (~b & d);
        else if constexpr (I < 32) f = (d & b) | (~d & c);
        else if constexpr (I < 48) f = b ^ c ^ d;
        else f = c ^ (b | ~d);
        constexpr uint32_t K = kMd5K[I];
        constexpr int S = md5_shift(I);
        const uint32_t x = a + f + K + M[md5_word(I)];
        a = b + ((x << S) | (x >> (32 - S)));
        batch_md5_steps<I + 1>(d, a, b, c, M);
    }
}

DPOW_HD void batch_md5_block(uint32_t st[4], const uint32_t *M) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
    batch_md5_steps<0>(a, b, c, d, M);
    st[0] += a;
    st[1] += b;
    st[2] += c;
    st[3] += d;
}

#if defined(__HIPCC__)
hipError_t batch_prepare();
hipError_t batch_launch(const BatchTask *tasks, const BatchEntry *map, const BatchLaunch &L, hipStream_t stream);
// Copy a batch's upload image (n_words 32-bit words) from pinned host memory to the device with a
// kernel on the batch's stream: a stream-ordered hipMemcpyAsync in front of the first launch cost
// every batch ~0.2 ms.
hipError_t batch_upload(uint32_t *dst, const uint32_t *src, uint32_t n_words, hipStream_t stream);
// The task queue's kernels: the rows of newly filled slots to the table (n_rows may be 0), and one
// launch of L.n_blocks descriptors with the live-slot list out_slots[0..L.n_live).
hipError_t queue_prepare();
hipError_t queue_upload(BatchTask *tasks, unsigned long long *best, const QueueRow *rows, uint32_t n_rows,
                        hipStream_t stream);
hipError_t queue_launch(const BatchTask *tasks, const BatchEntry *blocks, const uint32_t *out_slots,
                        const BatchLaunch &L, hipStream_t stream);
#endif

}  // namespace dpow
