/*
 * fast_scan.c -- TEST INFRASTRUCTURE ONLY: an AVX-512 golden-vector generator.
 *
 * Finds the reference worker's first hit (worker.go:301-400, workerBits = 0:
 * k outer, threadByte 0..255 inner, msg = nonce || threadByte || chunk_k,
 * hex(MD5(msg)) ending in >= ntz '0' characters) for cases too large for the
 * byte-wise oracle (oracle/dpow_oracle.c, ~9 M candidates/s per core), e.g.
 * N = 9 (6.9e10 candidates expected).  It is a restatement of the same
 * enumeration, vectorised 16 thread bytes per AVX-512 register (4 registers
 * interleaved), multi-threaded over k-units with a shared "best so far"; the
 * trailing-'0' test is the nibble-mask form of hasNumZeroesSuffix
 * (worker.go:246-256): the last hex characters are the low and high nibbles of
 * digest bytes 15, 14, ... (word D's top byte first).
 *
 * Trust: gen_golden.py --n9 cross-checks it against every golden the
 * byte-wise oracle and the Python restatement produced (N = 0..8) before it
 * writes any new vector.  It never ships to the GPU box and nothing in the
 * product loads it.
 *
 * Nonces of 64 bytes and more: the whole nonce-only blocks are hashed by plain
 * scalar code (md5_block) into a midstate; the vectorised final block starts
 * from it, holds the nonce's last nonce_len mod 64 bytes and carries the bit
 * length of the whole message.
 *
 * Two final blocks: with p = nonce_len mod 64, a message whose p + 1 + chunk
 * length + 9 exceeds 64 pads into a second block (RFC 1321 3.1-3.2), and the
 * chunk bytes, the 0x80 and the bit length fall wherever the byte count puts
 * them.  The padded 128 bytes are laid out per k as plain bytes; the first
 * block (which always holds the thread byte, p <= 63) runs vectorised from the
 * midstate and the second, lane-uniform in its words, from each lane's state.
 * gen_golden.py --layouts cross-checks this against the byte-wise oracle's
 * all-hits lists and every two-block golden before it writes a list.
 *
 * All-hits mode (a sixth argument "all"): no best-so-far pruning; every
 * candidate of the window whose digest ends in >= ntz '0' characters is
 * collected with its actual trailing-'0' count and printed sorted by global
 * index.  gen_golden.py --seg-inner cross-checks this mode against the byte-wise
 * oracle walked hit by hit before it writes a list.
 *
 * Build (gen_golden.py does this): gcc -O3 -mavx512f -fopenmp-free:
 *   gcc -O3 -march=native -pthread -o fast_scan fast_scan.c
 * Usage: fast_scan <nonce-hex> <ntz> <k_begin> <k_end> <threads> [all]
 *   prints "hit <global_idx>" or "none"; with "all", one "hit <global_idx> <tz>"
 *   line per hit in index order, then "end <count>".
 */
#include <immintrin.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const uint32_t T[64] = {
    0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501,
    0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
    0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8,
    0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
    0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
    0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
    0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
    0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};

#define NV 4 /* independent 16-lane vectors per step: 64 thread bytes */

typedef struct {
    uint64_t g;
    unsigned tz;
} hit_t;

typedef struct {
    uint8_t nonce[1024];
    size_t nonce_len;
    uint32_t iv[4]; /* MD5 state after the nonce's whole 64-byte blocks */
    int all;        /* all-hits mode */
    pthread_mutex_t lock;
    hit_t *hits;
    size_t nhits, cap;
    unsigned ntz;
    uint64_t k_begin, k_end, unit;
    uint32_t mask[4]; /* required-zero bits of digest words A, B, C, D */
    volatile uint64_t next_unit;
    volatile uint64_t best; /* min global index found */
} job_t;

static inline uint64_t load_best(job_t *j) { return __atomic_load_n(&j->best, __ATOMIC_RELAXED); }

static void set_best(job_t *j, uint64_t g) {
    uint64_t cur = load_best(j);
    while (g < cur && !__atomic_compare_exchange_n(&j->best, &cur, g, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
}

/* Nibble positions from the end of the hex string: digest byte 15 low/high,
 * byte 14 low/high, ...  Digest word w holds bytes 4w..4w+3 little-endian. */
static void tail_masks(unsigned ntz, uint32_t m[4]) {
    memset(m, 0, 4 * sizeof m[0]);
    for (unsigned j = 0; j < ntz && j < 32; ++j) {
        unsigned byte = 15 - j / 2, nib = j % 2; /* j even: low nibble of the byte (last hex char) */
        m[byte / 4] |= 0xFu << (8 * (byte % 4) + (nib ? 4 : 0));
    }
}

static const int S[4][4] = {{7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21}};

/* RFC 1321 compression of one 64-byte block, plain scalar code (the midstate of long nonces). */
static void md5_block(uint32_t st[4], const uint8_t *blk) {
    uint32_t M[16], a = st[0], b = st[1], c = st[2], d = st[3];
    for (int w = 0; w < 16; ++w)
        M[w] = (uint32_t)blk[4 * w] | ((uint32_t)blk[4 * w + 1] << 8) | ((uint32_t)blk[4 * w + 2] << 16) |
               ((uint32_t)blk[4 * w + 3] << 24);
    for (int i = 0; i < 64; ++i) {
        uint32_t f;
        int g;
        if (i < 16) f = (b & c) | (~b & d), g = i;
        else if (i < 32) f = (d & b) | (~d & c), g = (5 * i + 1) & 15;
        else if (i < 48) f = b ^ c ^ d, g = (3 * i + 5) & 15;
        else f = c ^ (b | ~d), g = (7 * i) & 15;
        const uint32_t t = a + f + M[g] + T[i];
        const int s = S[i / 16][i % 4];
        a = d, d = c, c = b;
        b += (t << s) | (t >> (32 - s));
    }
    st[0] += a, st[1] += b, st[2] += c, st[3] += d;
}

/* Trailing '0' characters of the hex digest: byte 15 low nibble, high nibble, byte 14 ... */
static unsigned hex_trailing_zeroes(const uint32_t w[4]) {
    unsigned n = 0;
    for (int byte = 15; byte >= 0; --byte) {
        const uint8_t v = (uint8_t)(w[byte / 4] >> (8 * (byte % 4)));
        if (v & 0x0F) return n;
        ++n;
        if (v >> 4) return n;
        ++n;
    }
    return n;
}

static void add_hit(job_t *j, uint64_t g, unsigned tz) {
    pthread_mutex_lock(&j->lock);
    if (j->nhits == j->cap) {
        j->cap = j->cap ? 2 * j->cap : 1024;
        j->hits = (hit_t *)realloc(j->hits, j->cap * sizeof *j->hits);
        if (!j->hits) abort();
    }
    j->hits[j->nhits].g = g;
    j->hits[j->nhits++].tz = tz;
    pthread_mutex_unlock(&j->lock);
}

static int cmp_hit(const void *a, const void *b) {
    const uint64_t x = ((const hit_t *)a)->g, y = ((const hit_t *)b)->g;
    return x < y ? -1 : x > y;
}

#define ROL(x, s) _mm512_rol_epi32((x), (s))
/* F, G, H, I as ternary-logic truth tables over (b, c, d) */
#define TF 0xCA
#define TG 0xE4
#define TH 0x96
#define TI 0x39

/* One MD5 step on NV vectors: a = b + rol(a + f(b,c,d) + M + K, s). */
#define STEP(a, b, c, d, tt, mw, i, s)                                                     \
    do {                                                                                   \
        for (int v = 0; v < NV; ++v) {                                                     \
            __m512i f = _mm512_ternarylogic_epi32(b[v], c[v], d[v], tt);                   \
            __m512i t = _mm512_add_epi32(_mm512_add_epi32(a[v], f), _mm512_add_epi32(mw[v], \
                                                                       _mm512_set1_epi32((int)T[i]))); \
            a[v] = _mm512_add_epi32(b[v], ROL(t, s));                                     \
        }                                                                                  \
    } while (0)

/* The 64 steps of one block on NV vectors of 16 lanes: st (A, B, C, D per lane) becomes
 * st + rounds(st, mv), RFC 1321's chaining. */
static inline __attribute__((always_inline)) void block_vec(__m512i st[4][NV], __m512i mv[16][NV]) {
    __m512i a[NV], b[NV], c[NV], d[NV];
    for (int v = 0; v < NV; ++v) a[v] = st[0][v], b[v] = st[1][v], c[v] = st[2][v], d[v] = st[3][v];
#define R4(tt, r, i0, w0, w1, w2, w3)                       \
    STEP(a, b, c, d, tt, mv[w0], i0 + 0, S[r][0]);          \
    STEP(d, a, b, c, tt, mv[w1], i0 + 1, S[r][1]);          \
    STEP(c, d, a, b, tt, mv[w2], i0 + 2, S[r][2]);          \
    STEP(b, c, d, a, tt, mv[w3], i0 + 3, S[r][3]);
    R4(TF, 0, 0, 0, 1, 2, 3) R4(TF, 0, 4, 4, 5, 6, 7) R4(TF, 0, 8, 8, 9, 10, 11)
    R4(TF, 0, 12, 12, 13, 14, 15)
    R4(TG, 1, 16, 1, 6, 11, 0) R4(TG, 1, 20, 5, 10, 15, 4) R4(TG, 1, 24, 9, 14, 3, 8)
    R4(TG, 1, 28, 13, 2, 7, 12)
    R4(TH, 2, 32, 5, 8, 11, 14) R4(TH, 2, 36, 1, 4, 7, 10) R4(TH, 2, 40, 13, 0, 3, 6)
    R4(TH, 2, 44, 9, 12, 15, 2)
    R4(TI, 3, 48, 0, 7, 14, 5) R4(TI, 3, 52, 12, 3, 10, 1) R4(TI, 3, 56, 8, 15, 6, 13)
    R4(TI, 3, 60, 4, 11, 2, 9)
#undef R4
    for (int v = 0; v < NV; ++v) {
        st[0][v] = _mm512_add_epi32(st[0][v], a[v]);
        st[1][v] = _mm512_add_epi32(st[1][v], b[v]);
        st[2][v] = _mm512_add_epi32(st[2][v], c[v]);
        st[3][v] = _mm512_add_epi32(st[3][v], d[v]);
    }
}

static void *scan_worker(void *arg) {
    job_t *j = (job_t *)arg;
    const size_t p = j->nonce_len % 64; /* byte offset of the thread byte in the first final block */
    const uint8_t *tail = j->nonce + (j->nonce_len - p);
    const __m512i lane = _mm512_set_epi32(15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0);
    for (;;) {
        const uint64_t u = __atomic_fetch_add(&j->next_unit, 1, __ATOMIC_RELAXED);
        const uint64_t k0 = j->k_begin + u * j->unit;
        if (k0 >= j->k_end || (!j->all && k0 * 256u >= load_best(j))) return NULL;
        const uint64_t k1 = k0 + j->unit < j->k_end ? k0 + j->unit : j->k_end;
        for (uint64_t k = k0; k < k1; ++k) {
            /* The padded message behind the midstate (RFC 1321 3.1-3.2): the nonce's tail, the
             * thread byte (left 0 here), the chunk, 0x80, zeroes, the bit length in the last 8
             * bytes of the first 64-byte block with room for them: one block, or two. */
            uint8_t buf[128];
            memset(buf, 0, sizeof buf);
            memcpy(buf, tail, p);
            size_t clen = 0;
            for (uint64_t x = k; x; x >>= 8) buf[p + 1 + clen++] = (uint8_t)(x & 0xFF);
            const size_t len = p + 1 + clen;
            buf[len] = 0x80;
            const int nb = len + 9 > 64 ? 2 : 1;
            const uint64_t bits = (uint64_t)(j->nonce_len - p + len) * 8u;
            for (int b = 0; b < 8; ++b) buf[64 * nb - 8 + b] = (uint8_t)(bits >> (8 * b));
            uint32_t M[32];
            for (int w = 0; w < 32; ++w)
                M[w] = (uint32_t)buf[4 * w] | ((uint32_t)buf[4 * w + 1] << 8) | ((uint32_t)buf[4 * w + 2] << 16) |
                       ((uint32_t)buf[4 * w + 3] << 24);
            __m512i mv[16][NV], mv2[16][NV];
            for (int w = 0; w < 16; ++w)
                for (int v = 0; v < NV; ++v) mv[w][v] = _mm512_set1_epi32((int)M[w]);
            if (nb == 2)
                for (int w = 0; w < 16; ++w)
                    for (int v = 0; v < NV; ++v) mv2[w][v] = _mm512_set1_epi32((int)M[16 + w]);
            const int wt = (int)(p / 4), sh = (int)(8 * (p % 4)); /* p <= 63: the thread byte is in the first block */
            for (int rep = 0; rep < 256 / (16 * NV); ++rep) {
                for (int v = 0; v < NV; ++v) {
                    __m512i tb = _mm512_add_epi32(lane, _mm512_set1_epi32(16 * (NV * rep + v)));
                    mv[wt][v] = _mm512_add_epi32(_mm512_set1_epi32((int)M[wt]), _mm512_slli_epi32(tb, (unsigned)sh));
                }
                __m512i st[4][NV];
                for (int w = 0; w < 4; ++w)
                    for (int v = 0; v < NV; ++v) st[w][v] = _mm512_set1_epi32((int)j->iv[w]);
                block_vec(st, mv);
                if (nb == 2) block_vec(st, mv2);
                for (int v = 0; v < NV; ++v) {
                    const __m512i A = st[0][v], B = st[1][v], C = st[2][v], D = st[3][v];
                    __mmask16 z = _mm512_testn_epi32_mask(D, _mm512_set1_epi32((int)j->mask[3]));
                    if (j->mask[2]) z &= _mm512_testn_epi32_mask(C, _mm512_set1_epi32((int)j->mask[2]));
                    if (j->mask[1]) z &= _mm512_testn_epi32_mask(B, _mm512_set1_epi32((int)j->mask[1]));
                    if (j->mask[0]) z &= _mm512_testn_epi32_mask(A, _mm512_set1_epi32((int)j->mask[0]));
                    if (z && j->all) {
                        uint32_t wa[16], wb[16], wc[16], wd[16];
                        _mm512_storeu_si512(wa, A);
                        _mm512_storeu_si512(wb, B);
                        _mm512_storeu_si512(wc, C);
                        _mm512_storeu_si512(wd, D);
                        for (unsigned l = 0; l < 16; ++l) {
                            if (!((z >> l) & 1)) continue;
                            const uint32_t w[4] = {wa[l], wb[l], wc[l], wd[l]};
                            add_hit(j, k * 256u + 16u * (NV * rep + v) + l, hex_trailing_zeroes(w));
                        }
                    } else if (z) {
                        const unsigned tbyte = 16u * (NV * rep + v) + (unsigned)__builtin_ctz(z);
                        set_best(j, k * 256u + tbyte);
                        goto next_unit; /* later thread bytes / k of this unit hold larger indices */
                    }
                }
            }
        }
    next_unit:;
    }
}

int main(int argc, char **argv) {
    if (argc != 6 && !(argc == 7 && !strcmp(argv[6], "all"))) {
        fprintf(stderr, "usage: %s <nonce-hex> <ntz> <k_begin> <k_end> <threads> [all]\n", argv[0]);
        return 2;
    }
    static job_t j;
    const char *hx = argv[1];
    j.nonce_len = strlen(hx) / 2;
    if (j.nonce_len > sizeof j.nonce) {
        fprintf(stderr, "fast_scan: nonce longer than %zu bytes\n", sizeof j.nonce);
        return 2;
    }
    for (size_t i = 0; i < j.nonce_len; ++i) sscanf(hx + 2 * i, "%2hhx", &j.nonce[i]);
    j.ntz = (unsigned)atoi(argv[2]);
    j.k_begin = strtoull(argv[3], NULL, 0);
    j.k_end = strtoull(argv[4], NULL, 0);
    const int nth = atoi(argv[5]);
    j.all = argc == 7;
    if (j.k_end > (1ull << 55) - 1 || j.k_begin > j.k_end) {
        fprintf(stderr, "fast_scan: bad k window (k < 2^55 - 1)\n");
        return 2;
    }
    j.iv[0] = 0x67452301, j.iv[1] = 0xefcdab89, j.iv[2] = 0x98badcfe, j.iv[3] = 0x10325476;
    for (size_t b = 0; b + 64 <= j.nonce_len; b += 64) md5_block(j.iv, j.nonce + b);
    pthread_mutex_init(&j.lock, NULL);
    tail_masks(j.ntz, j.mask);
    j.unit = 1u << 12;
    j.next_unit = 0;
    j.best = UINT64_MAX;
    pthread_t th[256];
    for (int i = 0; i < nth && i < 256; ++i) pthread_create(&th[i], NULL, scan_worker, &j);
    for (int i = 0; i < nth && i < 256; ++i) pthread_join(th[i], NULL);
    if (j.all) {
        if (j.nhits) qsort(j.hits, j.nhits, sizeof *j.hits, cmp_hit);
        for (size_t i = 0; i < j.nhits; ++i) printf("hit %llu %u\n", (unsigned long long)j.hits[i].g, j.hits[i].tz);
        printf("end %zu\n", j.nhits);
        return 0;
    }
    if (j.best == UINT64_MAX) printf("none\n");
    else printf("hit %llu\n", (unsigned long long)j.best);
    return 0;
}
