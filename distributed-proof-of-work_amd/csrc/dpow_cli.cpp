// dpow_cli.cpp -- native command-line harness over the C ABI (no Python).
//
//   dpow_cli mine  <nonce-hex> <ntz> [worker_byte worker_bits [device]]
//       the reference miner's answer for one partition (worker.go:301-400), verified on the host
//   dpow_cli sweep <log2-candidates> [device]
//       hash 2^n candidates of nonce 01020304 at N=32 (unreachable) from k = 2^24, report GH/s
//   dpow_cli latency [reps [device]]
//       time-to-secret floor: platform launch round trips (dpow_diag.h) and median dpow_search
//       latency for hits at N = 0 / 3 / 5 (in-process, warm context)
//   dpow_cli worker <nonce-hex> <ntz> [device]
//       one Mine -> result -> Found -> ACK round trip through the native worker (worker.go:169-232)
//   dpow_cli batch <ntz> <nonce-hex> [<nonce-hex> ...] [--device N]
//       mine every nonce from k = 0 in one batched search (dpow_search_batch), window by window;
//       one line per task: its global index and its secret in hex
//   dpow_cli scan <nonce-hex> <ntz> <k_begin> <k_end> [worker_byte worker_bits [device]]
//       every hit of the window (dpow_scan), one line per hit: its global index, its depth and its
//       secret in hex
//   dpow_cli scan-device <nonce-hex> <ntz> <k_begin> <k_end> [worker_byte worker_bits [device]]
//       the window's hits left in device memory (dpow_scan_device), paged; one JSON line: the
//       count, the first and the last hit (index, depth, secret) and the calls' time
//   dpow_cli census <nonce-hex> <k_begin> <k_end> [worker_byte worker_bits [device]]
//       how deep the window goes (dpow_census_window), one line per depth up to the deepest: the
//       depth, the number of candidates at least that deep, the first one's global index and its
//       secret in hex
//   dpow_cli scan-many <ntz> <k_begin> <k_end> <nonce-hex> [<nonce-hex> ...] [--device N]
//       every hit of the same window of every nonce in batched calls (dpow_scan_batch), one line
//       per hit: the nonce's number (from 0), then `scan`'s line
//   dpow_cli scan-many-device <ntz> <k_begin> <k_end> <nonce-hex> [<nonce-hex> ...] [--device N]
//       the hits of the same window of every nonce left in device memory (dpow_scan_batch_device),
//       paged; per nonce a line with its number, its count and its first and last hit (index, depth),
//       then one JSON line with the total and the calls' time
//   dpow_cli census-many <k_begin> <k_end> <nonce-hex> [<nonce-hex> ...] [--device N]
//       the census of the same window of every nonce in one batched call (dpow_census_batch): per
//       task a line "# <nonce-hex>" and then `census`'s lines
//   dpow_cli digest <nonce-hex> <idx> [idx ...] [--device N]
//       the MD5 and the depth of the listed global indices (dpow_digests), one line per entry: its
//       index, its depth, its secret in hex and its md5 in hex
//   dpow_cli digest-many <ntz> <nonce-hex>:<idx>[,<idx>...] [<nonce-hex>:<idx>,... ...] [--device N]
//       the same for lists of many nonces in one call (dpow_digests_batch; a nonce with nothing behind
//       its colon is an empty task): `digest`'s line per entry, and per task a line "# <nonce-hex>
//       <entries> <shallow>", shallow being its entries with a depth below ntz
//   dpow_cli digest-host <nonce-hex> <log2-n> [reps]
//       time dpow_digest_of_index in a loop over 2^n sequential indices from 2^32 (no GPU): what a
//       caller pays per entry on the host; one JSON line with the median of `reps` loops
// Each other command prints one JSON line.
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include <algorithm>

#include "../../include/dpow.h"
#include "../../include/dpow_diag.h"
#include "../../include/dpow_worker.h"

static std::vector<uint8_t> from_hex(const char *s) {
    std::vector<uint8_t> out;
    const size_t n = strlen(s);
    for (size_t i = 0; i + 1 < n; i += 2) {
        unsigned v = 0;
        sscanf(s + i, "%2x", &v);
        out.push_back((uint8_t)v);
    }
    return out;
}

static std::string bytes_json(const uint8_t *b, size_t n) {
    std::string s = "[";
    for (size_t i = 0; i < n; ++i) s += (i ? "," : "") + std::to_string(b[i]);
    return s + "]";
}

static double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int fail(const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, dpow_last_error());
    return 1;
}

static int cmd_mine(int argc, char **argv) {
    if (argc < 4) return 2;
    std::vector<uint8_t> nonce = from_hex(argv[2]);
    const uint32_t ntz = (uint32_t)atoi(argv[3]);
    const uint32_t wb = argc > 5 ? (uint32_t)atoi(argv[4]) : 0, wbits = argc > 5 ? (uint32_t)atoi(argv[5]) : 0;
    const int dev = argc > 6 ? atoi(argv[6]) : 0;
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    uint8_t secret[DPOW_MAX_SECRET];
    size_t slen = 0;
    uint64_t best = DPOW_NO_HIT;
    const double t0 = now_s();
    uint64_t k = 0, window = 1ull << 16;
    rc = DPOW_EXHAUSTED;
    while (rc == DPOW_EXHAUSTED && k < DPOW_K_LIMIT) {
        const uint64_t ke = k + window < DPOW_K_LIMIT ? k + window : DPOW_K_LIMIT;
        rc = dpow_search(ctx, nonce.data(), nonce.size(), ntz, wb, wbits, k, ke, &best, secret, &slen);
        k = ke;
        if (window < (1ull << 26)) window <<= 2;
    }
    const double dt = now_s() - t0;
    if (rc < 0) return fail("dpow_search", rc);
    printf("{\"status\":%d,\"global_idx\":%llu,\"secret\":%s,\"verified\":%d,\"ms\":%.3f}\n", rc,
           (unsigned long long)best, bytes_json(secret, slen).c_str(),
           rc == DPOW_FOUND ? dpow_verify(nonce.data(), nonce.size(), secret, slen, ntz) : 0, dt * 1e3);
    dpow_close(ctx);
    return 0;
}

static int cmd_sweep(int argc, char **argv) {
    const int lg = argc > 2 ? atoi(argv[2]) : 36;
    const int dev = argc > 3 ? atoi(argv[3]) : 0;
    if (lg < 8 || lg > 44) return 2;
    const uint8_t nonce[4] = {1, 2, 3, 4};
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    uint8_t secret[DPOW_MAX_SECRET];
    size_t slen;
    uint64_t best = DPOW_NO_HIT;
    const uint64_t k0 = 1ull << 24, nk = 1ull << (lg - 8);
    rc = dpow_search(ctx, nonce, 4, 32, 0, 0, k0 - (1ull << 20), k0, &best, secret, &slen);  // warm-up
    if (rc < 0) return fail("dpow_search", rc);
    dpow_reset_stats(ctx);
    const double t0 = now_s();
    rc = dpow_search(ctx, nonce, 4, 32, 0, 0, k0, k0 + nk, &best, secret, &slen);
    const double dt = now_s() - t0;
    if (rc < 0) return fail("dpow_search", rc);
    dpow_stats st;
    dpow_get_stats(ctx, &st);
    printf("{\"candidates\":%llu,\"status\":%d,\"wall_ghs\":%.3f,\"kernel_ghs\":%.3f,\"launches\":%llu}\n",
           (unsigned long long)st.candidates, rc, (double)st.candidates / dt / 1e9,
           (double)st.candidates / (st.kernel_ms * 1e-3) / 1e9, (unsigned long long)st.launches);
    dpow_close(ctx);
    return 0;
}

static int cmd_latency(int argc, char **argv) {
    const int reps = argc > 2 ? atoi(argv[2]) : 200;
    const int dev = argc > 3 ? atoi(argv[3]) : 0;
    double floor_us[3] = {0, 0, 0};
    for (int m = 0; m < 3; ++m)
        if (dpow_diag_launch_latency(dev, m, reps, &floor_us[m]) != 0) return fail("dpow_diag_launch_latency", -2);
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    const uint8_t nonce[4] = {1, 2, 3, 4};
    const uint8_t nonce5[4] = {2, 2, 2, 2};
    struct Case { const uint8_t *n; uint32_t ntz; uint64_t k_end; const char *name; int idle_us; } cases[] = {
        {nonce, 0, 1, "n0_k1", 0},           {nonce, 3, 1, "n3_k1", 0},
        {nonce, 3, 256, "n3_k256", 0},       {nonce, 3, 65536, "n3_k64k", 0},
        {nonce, 3, 1ull << 24, "n3_k16M", 0}, {nonce, 3, 1ull << 26, "n3", 0},
        {nonce, 3, 1ull << 26, "n3_idle", 3000}, {nonce5, 5, 1ull << 26, "n5_02020202", 0},
        {nonce5, 5, 1ull << 26, "n5_02020202_idle", 3000}};
    std::string out = "{\"launch_sync_us\":" + std::to_string(floor_us[0]) +
                      ",\"launch_pinned_poll_us\":" + std::to_string(floor_us[1]) +
                      ",\"memcpy16_d2h_sync_us\":" + std::to_string(floor_us[2]);
    for (const Case &c : cases) {
        std::vector<double> us;
        for (int r = 0; r < reps + 5; ++r) {
            uint64_t best = DPOW_NO_HIT;
            uint8_t secret[DPOW_MAX_SECRET];
            size_t slen = 0;
            if (c.idle_us) {  // let the previous search's queued launches drain first
                const double tw = now_s();
                while ((now_s() - tw) * 1e6 < c.idle_us) {
                }
            }
            const double t0 = now_s();
            rc = dpow_search(ctx, c.n, 4, c.ntz, 0, 0, 0, c.k_end, &best, secret, &slen);
            const double dt = (now_s() - t0) * 1e6;
            if (rc != DPOW_FOUND) return fail("dpow_search", rc);
            if (r >= 5) us.push_back(dt);
        }
        std::sort(us.begin(), us.end());
        out += std::string(",\"search_") + c.name + "_us\":" + std::to_string(us[us.size() / 2]);
    }
    dpow_close(ctx);
    printf("%s}\n", out.c_str());
    return 0;
}

static int cmd_worker(int argc, char **argv) {
    if (argc < 4) return 2;
    std::vector<uint8_t> nonce = from_hex(argv[2]);
    const uint32_t ntz = (uint32_t)atoi(argv[3]);
    const int dev = argc > 4 ? atoi(argv[4]) : 0;
    dpow_worker *w = nullptr;
    int rc = dpow_worker_new(dev, &w);
    if (rc) return fail("dpow_worker_new", rc);
    const double t0 = now_s();
    rc = dpow_worker_mine(w, nonce.data(), nonce.size(), ntz, 0, 0, 1);
    if (rc) return fail("dpow_worker_mine", rc);
    dpow_worker_result r;
    rc = dpow_worker_next_result(w, &r, 600000);
    if (rc) return fail("dpow_worker_next_result", rc);
    const double dt = now_s() - t0;
    rc = dpow_worker_found(w, nonce.data(), nonce.size(), ntz, 0, r.secret, r.secret_len, 1);
    if (rc) return fail("dpow_worker_found", rc);
    dpow_worker_result ack;
    rc = dpow_worker_next_result(w, &ack, 10000);
    if (rc) return fail("dpow_worker_next_result", rc);
    printf("{\"secret\":%s,\"ack_is_nil\":%d,\"ms_to_result\":%.3f}\n", bytes_json(r.secret, r.secret_len).c_str(),
           ack.has_secret == 0, dt * 1e3);
    dpow_worker_free(w);
    return 0;
}

static int cmd_batch(int argc, char **argv) {
    if (argc < 4) return 2;
    const uint32_t ntz = (uint32_t)atoi(argv[2]);
    int dev = 0;
    std::vector<std::vector<uint8_t>> nonces;
    for (int i = 3; i < argc; ++i) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) dev = atoi(argv[++i]);
        else nonces.push_back(from_hex(argv[i]));
    }
    if (nonces.empty() || nonces.size() > DPOW_BATCH_MAX) return 2;
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    const size_t n = nonces.size();
    std::vector<dpow_batch_task> done(n);
    std::vector<size_t> todo(n);
    for (size_t i = 0; i < n; ++i) todo[i] = i;
    uint64_t k = 0, window = 1ull << 20;
    while (!todo.empty() && k < DPOW_K_LIMIT) {
        const uint64_t ke = k + window < DPOW_K_LIMIT ? k + window : DPOW_K_LIMIT;
        std::vector<dpow_batch_task> tasks(todo.size());
        for (size_t j = 0; j < todo.size(); ++j) {
            dpow_batch_task &t = tasks[j];
            memset(&t, 0, sizeof t);
            t.nonce = nonces[todo[j]].data();
            t.nonce_len = nonces[todo[j]].size();
            t.ntz = ntz;
            t.k_begin = k;
            t.k_end = ke;
            t.best_global_idx = DPOW_NO_HIT;
        }
        rc = dpow_search_batch(ctx, tasks.data(), tasks.size(), nullptr);
        if (rc < 0) return fail("dpow_search_batch", rc);
        std::vector<size_t> left;
        for (size_t j = 0; j < todo.size(); ++j) {
            done[todo[j]] = tasks[j];
            if (tasks[j].status == DPOW_EXHAUSTED) left.push_back(todo[j]);
        }
        todo.swap(left);
        k = ke;
        if (window < (1ull << 26)) window <<= 2;
    }
    for (size_t i = 0; i < n; ++i) {
        if (done[i].status != DPOW_FOUND) {
            printf("%zu status %d\n", i, done[i].status);
            continue;
        }
        printf("%zu %llu ", i, (unsigned long long)done[i].best_global_idx);
        for (uint32_t b = 0; b < done[i].secret_len; ++b) printf("%02x", done[i].secret[b]);
        printf("\n");
    }
    dpow_close(ctx);
    return 0;
}

static int cmd_scan(int argc, char **argv) {
    if (argc < 6) return 2;
    std::vector<uint8_t> nonce = from_hex(argv[2]);
    const uint32_t ntz = (uint32_t)atoi(argv[3]);
    uint64_t k = strtoull(argv[4], nullptr, 0);
    const uint64_t k_end = strtoull(argv[5], nullptr, 0);
    const uint32_t wb = argc > 7 ? (uint32_t)atoi(argv[6]) : 0, wbits = argc > 7 ? (uint32_t)atoi(argv[7]) : 0;
    const int dev = argc > 8 ? atoi(argv[8]) : 0;
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    std::vector<dpow_scan_hit> page(1u << 16);
    do {
        size_t n = 0;
        rc = dpow_scan(ctx, nonce.data(), nonce.size(), ntz, wb, wbits, k, k_end, page.data(), page.size(), &n, &k,
                       nullptr);
        if (rc < 0) return fail("dpow_scan", rc);
        for (size_t i = 0; i < n; ++i) {
            printf("%llu %u ", (unsigned long long)page[i].global_idx, page[i].tz);
            for (uint32_t b = 0; b < page[i].secret_len; ++b) printf("%02x", page[i].secret[b]);
            printf("\n");
        }
    } while (rc == DPOW_MORE);
    dpow_close(ctx);
    return rc == DPOW_EXHAUSTED ? 0 : 1;
}

// The HIP runtime calls scan-device needs for its device buffers.  The harness is built without the
// HIP headers; libdpow.so has the runtime loaded, so the symbols are looked up in the process.
typedef int (*hip_malloc_fn)(void **, size_t);
typedef int (*hip_free_fn)(void *);
typedef int (*hip_set_device_fn)(int);
typedef int (*hip_memcpy_fn)(void *, const void *, size_t, int);
constexpr int kHipMemcpyDeviceToHost = 2;

static int cmd_scan_device(int argc, char **argv) {
    if (argc < 6) return 2;
    std::vector<uint8_t> nonce = from_hex(argv[2]);
    const uint32_t ntz = (uint32_t)atoi(argv[3]);
    uint64_t k = strtoull(argv[4], nullptr, 0);
    const uint64_t k_end = strtoull(argv[5], nullptr, 0);
    const uint32_t wb = argc > 7 ? (uint32_t)atoi(argv[6]) : 0, wbits = argc > 7 ? (uint32_t)atoi(argv[7]) : 0;
    const int dev = argc > 8 ? atoi(argv[8]) : 0;
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    const hip_malloc_fn dev_malloc = (hip_malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
    const hip_free_fn dev_free = (hip_free_fn)dlsym(RTLD_DEFAULT, "hipFree");
    const hip_memcpy_fn dev_memcpy = (hip_memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
    const hip_set_device_fn dev_set = (hip_set_device_fn)dlsym(RTLD_DEFAULT, "hipSetDevice");
    if (!dev_malloc || !dev_free || !dev_memcpy || !dev_set) {
        fprintf(stderr, "scan-device: the HIP runtime's symbols are not visible in the process\n");
        return 1;
    }
    if (dev_set(dev) != 0) {  // the buffers belong on the context's device
        fprintf(stderr, "scan-device: hipSetDevice failed\n");
        return 1;
    }
    const size_t page = 1u << 20;
    void *d_idx = nullptr, *d_tz = nullptr;
    if (dev_malloc(&d_idx, page * 8) != 0 || dev_malloc(&d_tz, page) != 0) {
        fprintf(stderr, "scan-device: hipMalloc failed\n");
        return 1;
    }
    // The first and the last entry of the window's list are the first of the first page that has
    // one and the last of the last: two 9-byte copies per such page, whatever the page holds.
    uint64_t total = 0, first = 0, last = 0;
    uint8_t first_tz = 0, last_tz = 0;
    uint32_t launches = 0, slices = 0;
    double kernel_ms = 0.0;
    const double t0 = now_s();
    do {
        size_t n = 0;
        dpow_batch_stats st;
        rc = dpow_scan_device(ctx, nonce.data(), nonce.size(), ntz, wb, wbits, k, k_end, d_idx, d_tz, page, &n, &k, &st);
        if (rc < 0) return fail("dpow_scan_device", rc);
        launches += st.launches;
        slices += st.rounds;
        kernel_ms += st.kernel_ms;
        if (n == 0) continue;
        int e = 0;
        if (total == 0) {
            e |= dev_memcpy(&first, d_idx, 8, kHipMemcpyDeviceToHost);
            e |= dev_memcpy(&first_tz, d_tz, 1, kHipMemcpyDeviceToHost);
        }
        e |= dev_memcpy(&last, (const uint8_t *)d_idx + 8 * (n - 1), 8, kHipMemcpyDeviceToHost);
        e |= dev_memcpy(&last_tz, (const uint8_t *)d_tz + (n - 1), 1, kHipMemcpyDeviceToHost);
        if (e != 0) {
            fprintf(stderr, "scan-device: hipMemcpy failed\n");
            return 1;
        }
        total += n;
    } while (rc == DPOW_MORE);
    const double dt = now_s() - t0;
    const auto hit_json = [](uint64_t g, uint8_t tz) {
        uint8_t sec[DPOW_MAX_SECRET];
        size_t len = 0;
        dpow_secret_from_index(g, sec, &len);
        return "{\"global_idx\":" + std::to_string(g) + ",\"tz\":" + std::to_string(tz) +
               ",\"secret\":" + bytes_json(sec, len) + "}";
    };
    printf("{\"status\":%d,\"k_done\":%llu,\"hits\":%llu,\"first\":%s,\"last\":%s,\"slices\":%u,\"launches\":%u,"
           "\"kernel_ms\":%.3f,\"ms\":%.3f}\n",
           rc, (unsigned long long)k, (unsigned long long)total, total ? hit_json(first, first_tz).c_str() : "null",
           total ? hit_json(last, last_tz).c_str() : "null", slices, launches, kernel_ms, dt * 1e3);
    dev_free(d_idx);
    dev_free(d_tz);
    dpow_close(ctx);
    return rc == DPOW_EXHAUSTED ? 0 : 1;
}

// One line per depth up to the deepest: the depth, its count, its first index and that secret in hex.
static void print_census(const dpow_census &c) {
    for (uint32_t d = 0; d <= c.deepest && c.count_ge[d] > 0; ++d) {
        uint8_t sec[DPOW_MAX_SECRET];
        size_t len = 0;
        dpow_secret_from_index(c.first_ge[d], sec, &len);
        printf("%u %llu %llu ", d, (unsigned long long)c.count_ge[d], (unsigned long long)c.first_ge[d]);
        for (size_t b = 0; b < len; ++b) printf("%02x", sec[b]);
        printf("\n");
    }
}

static int cmd_census(int argc, char **argv) {
    if (argc < 5) return 2;
    std::vector<uint8_t> nonce = from_hex(argv[2]);
    const uint64_t k_begin = strtoull(argv[3], nullptr, 0), k_end = strtoull(argv[4], nullptr, 0);
    const uint32_t wb = argc > 6 ? (uint32_t)atoi(argv[5]) : 0, wbits = argc > 6 ? (uint32_t)atoi(argv[6]) : 0;
    const int dev = argc > 7 ? atoi(argv[7]) : 0;
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    dpow_census c;
    uint64_t k_done = 0;
    rc = dpow_census_window(ctx, nonce.data(), nonce.size(), wb, wbits, k_begin, k_end, &c, &k_done, nullptr);
    if (rc < 0) return fail("dpow_census_window", rc);
    print_census(c);
    dpow_close(ctx);
    return rc == DPOW_EXHAUSTED ? 0 : 1;
}

static int cmd_census_many(int argc, char **argv) {
    if (argc < 5) return 2;
    const uint64_t k_begin = strtoull(argv[2], nullptr, 0), k_end = strtoull(argv[3], nullptr, 0);
    int dev = 0;
    std::vector<std::vector<uint8_t>> nonces;
    std::vector<const char *> names;
    for (int i = 4; i < argc; ++i) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) {
            dev = atoi(argv[++i]);
        } else {
            nonces.push_back(from_hex(argv[i]));
            names.push_back(argv[i]);
        }
    }
    if (nonces.empty()) return 2;
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    std::vector<dpow_census_task> tasks(nonces.size());
    for (size_t i = 0; i < tasks.size(); ++i) {
        memset(&tasks[i], 0, sizeof tasks[i]);
        tasks[i].nonce = nonces[i].data();
        tasks[i].nonce_len = nonces[i].size();
        tasks[i].k_begin = k_begin;
        tasks[i].k_end = k_end;
    }
    rc = dpow_census_batch(ctx, tasks.data(), tasks.size(), nullptr);
    if (rc < 0) return fail("dpow_census_batch", rc);
    bool all = true;
    for (size_t i = 0; i < tasks.size(); ++i) {
        printf("# %s\n", names[i]);
        print_census(tasks[i].census);
        all = all && tasks[i].status == DPOW_EXHAUSTED;
    }
    dpow_close(ctx);
    return all ? 0 : 1;
}

// One line per hit: the task's number, then dpow_cli scan's line.  The unfinished tasks go in again
// from their k_done until every one is exhausted.
static int cmd_scan_many(int argc, char **argv) {
    if (argc < 6) return 2;
    const uint32_t ntz = (uint32_t)atoi(argv[2]);
    const uint64_t k_begin = strtoull(argv[3], nullptr, 0), k_end = strtoull(argv[4], nullptr, 0);
    int dev = 0;
    std::vector<std::vector<uint8_t>> nonces;
    for (int i = 5; i < argc; ++i) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) dev = atoi(argv[++i]);
        else nonces.push_back(from_hex(argv[i]));
    }
    if (nonces.empty()) return 2;
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    std::vector<uint64_t> k(nonces.size(), k_begin);
    std::vector<size_t> todo(nonces.size());
    for (size_t i = 0; i < todo.size(); ++i) todo[i] = i;
    std::vector<dpow_scan_hit> page(1u << 16);
    bool cancelled = false;
    while (!todo.empty() && !cancelled) {
        std::vector<dpow_scan_task> tasks(todo.size());
        for (size_t j = 0; j < tasks.size(); ++j) {
            memset(&tasks[j], 0, sizeof tasks[j]);
            tasks[j].nonce = nonces[todo[j]].data();
            tasks[j].nonce_len = nonces[todo[j]].size();
            tasks[j].ntz = ntz;
            tasks[j].k_begin = k[todo[j]];
            tasks[j].k_end = k_end;
        }
        size_t n = 0;
        rc = dpow_scan_batch(ctx, tasks.data(), tasks.size(), page.data(), page.size(), &n, nullptr);
        if (rc < 0) return fail("dpow_scan_batch", rc);
        std::vector<size_t> next;
        for (size_t j = 0; j < tasks.size(); ++j) {
            for (uint64_t h = tasks[j].first_hit; h < tasks[j].first_hit + tasks[j].n_hits; ++h) {
                printf("%zu %llu %u ", todo[j], (unsigned long long)page[h].global_idx, page[h].tz);
                for (uint32_t b = 0; b < page[h].secret_len; ++b) printf("%02x", page[h].secret[b]);
                printf("\n");
            }
            k[todo[j]] = tasks[j].k_done;
            if (tasks[j].status == DPOW_MORE) next.push_back(todo[j]);
            cancelled = cancelled || tasks[j].status == DPOW_CANCELLED;
        }
        todo.swap(next);
    }
    dpow_close(ctx);
    return cancelled ? 1 : 0;
}

// Per nonce its number, its count and its first and last hit; then the call's JSON line.  The
// unfinished tasks go in again from their k_done until every one is exhausted; of a page only the
// first and the last entry of each task's segment cross to the host.
static int cmd_scan_many_device(int argc, char **argv) {
    if (argc < 6) return 2;
    const uint32_t ntz = (uint32_t)atoi(argv[2]);
    const uint64_t k_begin = strtoull(argv[3], nullptr, 0), k_end = strtoull(argv[4], nullptr, 0);
    int dev = 0;
    std::vector<std::vector<uint8_t>> nonces;
    for (int i = 5; i < argc; ++i) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) dev = atoi(argv[++i]);
        else nonces.push_back(from_hex(argv[i]));
    }
    if (nonces.empty()) return 2;
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    const hip_malloc_fn dev_malloc = (hip_malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
    const hip_free_fn dev_free = (hip_free_fn)dlsym(RTLD_DEFAULT, "hipFree");
    const hip_memcpy_fn dev_memcpy = (hip_memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
    const hip_set_device_fn dev_set = (hip_set_device_fn)dlsym(RTLD_DEFAULT, "hipSetDevice");
    if (!dev_malloc || !dev_free || !dev_memcpy || !dev_set) {
        fprintf(stderr, "scan-many-device: the HIP runtime's symbols are not visible in the process\n");
        return 1;
    }
    const size_t page = 1u << 20;
    void *d_idx = nullptr, *d_tz = nullptr;
    if (dev_set(dev) != 0 || dev_malloc(&d_idx, page * 8) != 0 || dev_malloc(&d_tz, page) != 0) {
        fprintf(stderr, "scan-many-device: hipSetDevice or hipMalloc failed\n");
        return 1;
    }
    struct Seen {
        uint64_t hits = 0, first = 0, last = 0;
        uint8_t first_tz = 0, last_tz = 0;
    };
    std::vector<Seen> seen(nonces.size());
    std::vector<uint64_t> k(nonces.size(), k_begin);
    std::vector<size_t> todo(nonces.size());
    for (size_t i = 0; i < todo.size(); ++i) todo[i] = i;
    uint32_t launches = 0, rounds = 0, calls = 0;
    double kernel_ms = 0.0;
    bool cancelled = false;
    const double t0 = now_s();
    while (!todo.empty() && !cancelled) {
        const size_t n_call = std::min<size_t>(todo.size(), DPOW_BATCH_MAX);
        std::vector<dpow_scan_task> tasks(n_call);
        for (size_t j = 0; j < n_call; ++j) {
            memset(&tasks[j], 0, sizeof tasks[j]);
            tasks[j].nonce = nonces[todo[j]].data();
            tasks[j].nonce_len = nonces[todo[j]].size();
            tasks[j].ntz = ntz;
            tasks[j].k_begin = k[todo[j]];
            tasks[j].k_end = k_end;
        }
        size_t n = 0;
        dpow_batch_stats st;
        rc = dpow_scan_batch_device(ctx, tasks.data(), n_call, d_idx, d_tz, nullptr, page, &n, &st);
        if (rc < 0) return fail("dpow_scan_batch_device", rc);
        launches += st.launches;
        rounds += st.rounds;
        kernel_ms += st.kernel_ms;
        ++calls;
        std::vector<size_t> next;
        for (size_t j = 0; j < n_call; ++j) {
            Seen &s = seen[todo[j]];
            if (tasks[j].n_hits) {
                const uint64_t a = tasks[j].first_hit, b = a + tasks[j].n_hits - 1;
                int e = 0;
                if (s.hits == 0) {
                    e |= dev_memcpy(&s.first, (const uint8_t *)d_idx + 8 * a, 8, kHipMemcpyDeviceToHost);
                    e |= dev_memcpy(&s.first_tz, (const uint8_t *)d_tz + a, 1, kHipMemcpyDeviceToHost);
                }
                e |= dev_memcpy(&s.last, (const uint8_t *)d_idx + 8 * b, 8, kHipMemcpyDeviceToHost);
                e |= dev_memcpy(&s.last_tz, (const uint8_t *)d_tz + b, 1, kHipMemcpyDeviceToHost);
                if (e != 0) {
                    fprintf(stderr, "scan-many-device: hipMemcpy failed\n");
                    return 1;
                }
                s.hits += tasks[j].n_hits;
            }
            k[todo[j]] = tasks[j].k_done;
            if (tasks[j].status == DPOW_MORE) next.push_back(todo[j]);
            cancelled = cancelled || tasks[j].status == DPOW_CANCELLED;
        }
        next.insert(next.end(), todo.begin() + n_call, todo.end());
        todo.swap(next);
    }
    const double dt = now_s() - t0;
    uint64_t total = 0;
    for (size_t i = 0; i < seen.size(); ++i) {
        const Seen &s = seen[i];
        total += s.hits;
        if (s.hits)
            printf("%zu %llu %llu %u %llu %u\n", i, (unsigned long long)s.hits, (unsigned long long)s.first, s.first_tz,
                   (unsigned long long)s.last, s.last_tz);
        else
            printf("%zu 0\n", i);
    }
    printf("{\"tasks\":%zu,\"hits\":%llu,\"calls\":%u,\"mask_launches\":%u,\"launches\":%u,\"kernel_ms\":%.3f,"
           "\"ms\":%.3f}\n",
           seen.size(), (unsigned long long)total, calls, rounds, launches, kernel_ms, dt * 1e3);
    dev_free(d_idx);
    dev_free(d_tz);
    dpow_close(ctx);
    return cancelled ? 1 : 0;
}

static int cmd_digest(int argc, char **argv) {
    if (argc < 4) return 2;
    std::vector<uint8_t> nonce = from_hex(argv[2]);
    int dev = 0;
    std::vector<uint64_t> idx;
    for (int i = 3; i < argc; ++i) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) dev = atoi(argv[++i]);
        else idx.push_back(strtoull(argv[i], nullptr, 0));
    }
    if (idx.empty()) return 2;
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    std::vector<uint8_t> digest(16 * idx.size()), tz(idx.size());
    size_t n_done = 0;
    rc = dpow_digests(ctx, nonce.data(), nonce.size(), idx.data(), idx.size(), digest.data(), tz.data(), &n_done,
                      nullptr);
    if (rc < 0) return fail("dpow_digests", rc);
    for (size_t i = 0; i < n_done; ++i) {
        uint8_t sec[DPOW_MAX_SECRET];
        size_t len = 0;
        dpow_secret_from_index(idx[i], sec, &len);
        printf("%llu %u ", (unsigned long long)idx[i], tz[i]);
        for (size_t b = 0; b < len; ++b) printf("%02x", sec[b]);
        printf(" ");
        for (size_t b = 0; b < 16; ++b) printf("%02x", digest[16 * i + b]);
        printf("\n");
    }
    dpow_close(ctx);
    return rc == DPOW_EXHAUSTED ? 0 : 1;
}

static int cmd_digest_many(int argc, char **argv) {
    if (argc < 4) return 2;
    const uint32_t ntz = (uint32_t)atoi(argv[2]);
    int dev = 0;
    std::vector<std::vector<uint8_t>> nonces;
    std::vector<uint64_t> rows{0}, idx;
    for (int i = 3; i < argc; ++i) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) {
            dev = atoi(argv[++i]);
            continue;
        }
        const char *colon = strchr(argv[i], ':');
        if (!colon) return 2;
        nonces.push_back(from_hex(std::string(argv[i], (size_t)(colon - argv[i])).c_str()));
        for (const char *q = colon + 1; *q;) {
            char *end = nullptr;
            idx.push_back(strtoull(q, &end, 0));
            if (end == q) return 2;
            q = *end == ',' ? end + 1 : end;
        }
        rows.push_back(idx.size());
    }
    if (nonces.empty()) return 2;
    std::vector<dpow_digest_task> tasks(nonces.size());
    for (size_t t = 0; t < tasks.size(); ++t) {
        tasks[t] = dpow_digest_task{};
        tasks[t].nonce = nonces[t].data();
        tasks[t].nonce_len = nonces[t].size();
        tasks[t].ntz = ntz;
    }
    dpow_ctx *ctx = nullptr;
    int rc = dpow_open(dev, &ctx);
    if (rc) return fail("dpow_open", rc);
    std::vector<uint8_t> digest(16 * idx.size() + 16), tz(idx.size() + 1);
    idx.push_back(0);  // (never read: an empty list still has an address)
    size_t n_done = 0;
    rc = dpow_digests_batch(ctx, tasks.data(), tasks.size(), rows.data(), idx.data(), digest.data(), tz.data(), &n_done,
                            nullptr);
    if (rc < 0) return fail("dpow_digests_batch", rc);
    for (size_t t = 0; t < tasks.size(); ++t) {
        printf("# ");
        for (uint8_t b : nonces[t]) printf("%02x", b);
        printf(" %llu %llu\n", (unsigned long long)tasks[t].n_entries, (unsigned long long)tasks[t].n_shallow);
        for (size_t i = rows[t]; i < rows[t + 1] && i < n_done; ++i) {
            uint8_t sec[DPOW_MAX_SECRET];
            size_t len = 0;
            dpow_secret_from_index(idx[i], sec, &len);
            printf("%llu %u ", (unsigned long long)idx[i], tz[i]);
            for (size_t b = 0; b < len; ++b) printf("%02x", sec[b]);
            printf(" ");
            for (size_t b = 0; b < 16; ++b) printf("%02x", digest[16 * i + b]);
            printf("\n");
        }
    }
    dpow_close(ctx);
    return rc == DPOW_EXHAUSTED ? 0 : 1;
}

static int cmd_digest_host(int argc, char **argv) {
    if (argc < 4) return 2;
    std::vector<uint8_t> nonce = from_hex(argv[2]);
    const int lg = atoi(argv[3]);
    const int reps = argc > 4 ? atoi(argv[4]) : 5;
    if (lg < 0 || lg > 26 || reps < 1) return 2;
    const uint64_t n = 1ull << lg, g0 = 1ull << 32;
    std::vector<double> ns;
    uint32_t sink = 0;
    for (int r = 0; r < reps + 1; ++r) {  // (the first loop is the warm-up)
        const double t0 = now_s();
        for (uint64_t j = 0; j < n; ++j) {
            uint8_t d[16];
            uint32_t tz = 0;
            const int rc = dpow_digest_of_index(nonce.data(), nonce.size(), g0 + j, d, &tz);
            if (rc < 0) return fail("dpow_digest_of_index", rc);
            sink += tz + d[0];
        }
        if (r) ns.push_back((now_s() - t0) * 1e9 / (double)n);
    }
    std::sort(ns.begin(), ns.end());
    printf("{\"n\":%llu,\"ns_per_entry\":%.2f,\"call_ms\":%.4f,\"sink\":%u}\n", (unsigned long long)n,
           ns[ns.size() / 2], ns[ns.size() / 2] * (double)n * 1e-6, sink);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "digest")) return cmd_digest(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "digest-many")) return cmd_digest_many(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "digest-host")) return cmd_digest_host(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "census")) return cmd_census(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "census-many")) return cmd_census_many(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "scan")) return cmd_scan(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "scan-device")) return cmd_scan_device(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "scan-many")) return cmd_scan_many(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "scan-many-device")) return cmd_scan_many_device(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "batch")) return cmd_batch(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "mine")) return cmd_mine(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "sweep")) return cmd_sweep(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "worker")) return cmd_worker(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "latency")) return cmd_latency(argc, argv);
    fprintf(stderr,
            "usage: dpow_cli mine <nonce-hex> <ntz> [worker_byte worker_bits [device]]\n"
            "       dpow_cli sweep <log2-candidates> [device]\n"
            "       dpow_cli worker <nonce-hex> <ntz> [device]\n"
            "       dpow_cli latency [reps [device]]\n"
            "       dpow_cli batch <ntz> <nonce-hex> [<nonce-hex> ...] [--device N]\n"
            "       dpow_cli scan <nonce-hex> <ntz> <k_begin> <k_end> [worker_byte worker_bits [device]]\n"
            "       dpow_cli scan-device <nonce-hex> <ntz> <k_begin> <k_end> [worker_byte worker_bits [device]]\n"
            "       dpow_cli scan-many <ntz> <k_begin> <k_end> <nonce-hex> [<nonce-hex> ...] [--device N]\n"
            "       dpow_cli scan-many-device <ntz> <k_begin> <k_end> <nonce-hex> [<nonce-hex> ...] [--device N]\n"
            "       dpow_cli census <nonce-hex> <k_begin> <k_end> [worker_byte worker_bits [device]]\n"
            "       dpow_cli census-many <k_begin> <k_end> <nonce-hex> [<nonce-hex> ...] [--device N]\n"
            "       dpow_cli digest <nonce-hex> <idx> [idx ...] [--device N]\n"
            "       dpow_cli digest-many <ntz> <nonce-hex>:<idx>[,<idx>...] [...] [--device N]\n"
            "       dpow_cli digest-host <nonce-hex> <log2-n> [reps]\n");
    return 2;
}
