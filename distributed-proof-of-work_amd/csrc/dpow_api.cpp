// dpow_api.cpp -- the C ABI (include/dpow.h) over the gfx950 search kernels: the context's
// lifecycle (dpow_open, dpow_close), its accessors and stats, the argument-checking entry points
// of the searches (dpow_search: search.cpp; dpow_search_batch: batch.cpp; dpow_scan: scan.cpp;
// dpow_census_window: census.cpp; dpow_census_batch: census_many.cpp; dpow_scan_batch: scan_many.cpp; dpow_digests, dpow_digests_device: digests.cpp; dpow_scan_device: scan_dev.cpp; dpow_scan_batch_device: scan_many_dev.cpp; dpow_digests_batch, dpow_digests_batch_device: digests_many.cpp; dpow_search_bound) and the pure host helpers.  The three batched loops' planner and task set-up are many_plan.cpp.  The node layer is node.cpp, the dpow_diag_* entry points diag.cpp.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>

#include "../../include/dpow_diag.h"
#include "../../include/dpow_worker.h"
#include "batch.h"
#include "batch_engine.h"
#include "census.h"
#include "census_many.h"
#include "ctx.h"
#include "digests.h"
#include "digests_many.h"
#include "md5_host.h"
#include "md5_variants.h"
#include "scan.h"
#include "scan_dev.h"
#include "scan_many.h"
#include "scan_many_dev.h"

using namespace dpow;

static thread_local std::string g_last_error;

int dpow::set_error(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

namespace {

// Persistent grid: one round of resident workgroups (6 four-wave workgroups per
// CU; the kernel's <= 80 SGPRs would admit 8), work handed out by in-order
// chunk claims from 8 per-XCD counters.  A chunk is sized for >= 16 claims per
// wave (small tail) and within [kMinChunk, kMaxChunk] wave-blocks: a contended
// counter serves < 90 claims/us (MI355X_MICROARCH.md "dequeue") and a wave
// hashes one wave-block in ~6 us, so 8k waves at chunk c ask ~1300/c claims/us
// of the 8 counters.  Small launches get fewer workgroups instead of smaller
// chunks.  Why 6, not 8: the SIMD issues oldest-first, and the five oldest
// waves of a SIMD already take ~all its VALU cycles (tools/wave_trace.py); the
// youngest ones hash ~1/60 of the mean and sit on the early chunks they
// claimed, which a first hit has to wait for.  6 vs 8 (profiles/r01_ab_tail_prio.log):
// throughput equal in every layout, time-to-secret N = 7 1.49 -> 1.37 ms.
// (The grid of a short launch is smaller: plan.h launch_blocks_per_cu.)
constexpr uint64_t kBlocksPerCu = kMaxBlocksPerCu;

// Lower Ctrl::best of the running search to g (dpow_search_bound): the pinned bound
// word, which the running launch's watcher relays to Ctrl::best within its poll (about
// 1 us).  Round 2 launched a one-thread atomicMin kernel on a second stream instead,
// which took 50-160 us to start beside the running grid.  The caller holds bound_mu.
int inject_bound_locked(dpow_ctx *c, uint64_t g) {
    if (g >= c->ext_bound.load(std::memory_order_relaxed)) return 0;
    c->ext_bound.store(g, std::memory_order_release);
    __atomic_store_n(bound_word(c), g, __ATOMIC_RELEASE);
    return 0;
}

// Kernels loaded per device in this process (search_prepare): once, under a lock.
hipError_t prepare_device(int device) {
    static std::mutex mu;
    static bool prepared[kMaxDevices] = {};
    std::lock_guard<std::mutex> g(mu);
    if (device < kMaxDevices && prepared[device]) return hipSuccess;
    const hipError_t e = search_prepare();
    if (e == hipSuccess && device < kMaxDevices) prepared[device] = true;
    return e;
}

}  // namespace

extern "C" {

const char *dpow_last_error(void) { return g_last_error.c_str(); }
int dpow_abi_version(void) { return DPOW_ABI_VERSION; }

int dpow_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int dpow_open(int device, dpow_ctx **out) {
    if (!out) return set_error(DPOW_EINVAL, "dpow_open: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return set_error(DPOW_EHIP, "dpow_open: no HIP device visible");
    if (device < 0 || device >= n) return set_error(DPOW_EINVAL, "dpow_open: bad device ordinal");
    const DeviceScope on_device(device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    dpow_ctx *c = new (std::nothrow) dpow_ctx();
    if (!c) return set_error(DPOW_ENOMEM, "dpow_open: out of memory");
    c->device = device;
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) {
        delete c;
        return hip_fail(e, "hipGetDeviceProperties");
    }
    c->cus = (uint32_t)prop.multiProcessorCount;
    {   // FNV-1a of the PCI bus id: the same GPU gives the same key in every process of the host
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, (int)sizeof bus - 1, device) != hipSuccess) {
            (void)hipGetLastError();
            snprintf(bus, sizeof bus, "ordinal-%d-pid-%d", device, (int)getpid());  // never matches another process
        }
        uint64_t h = 1469598103934665603ull;
        for (const char *q = bus; *q; ++q) h = (h ^ (uint8_t)*q) * 1099511628211ull;
        c->dev_key = h | 1ull;
    }
    if (const char *pw = getenv("DPOW_DIAG_POLL_WB")) c->knobs.poll_wb = (uint32_t)std::max(0, atoi(pw));
    if (const char *pw = getenv("DPOW_DIAG_BPC")) c->knobs.bpc = (uint32_t)std::max(0, atoi(pw));
    if (const char *pw = getenv("DPOW_DIAG_CPW")) c->knobs.cpw = (uint32_t)std::max(0, atoi(pw));
    if (const char *pw = getenv("DPOW_DIAG_SHARE_LAUNCH_US")) c->knobs.share_launch_us = (uint32_t)std::max(0, atoi(pw));
    if (const char *pw = getenv("DPOW_DIAG_SHARE_MAX")) c->knobs.share_max = (uint32_t)std::max(0, atoi(pw));
    // DPOW_DIAG_SEG_INNER: 0 = no segment-inner launch, 1 = wherever the shape permits (plan.h)
    if (const char *pw = getenv("DPOW_DIAG_SEG_INNER")) c->knobs.seg_inner = atoi(pw) != 0 ? 1 : 0;
    if (const char *pw = getenv("DPOW_DIAG_MIN_CHUNK")) {
        const uint32_t v = (uint32_t)std::max(0, atoi(pw));
        if (v && !(v & (v - 1))) c->knobs.min_chunk = v;
    }
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipMalloc(&c->d_ctrl_alloc, 2 * kCtrlRing * kCtrlStride * sizeof(Ctrl))) != hipSuccess ||
        (e = hipMalloc(&c->d_claims, kClaimRing * kClaimSlot * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipHostMalloc(&c->h_snap, kRing * sizeof(Snap), hipHostMallocCoherent | hipHostMallocMapped)) !=
            hipSuccess ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void **>(&c->d_snap), c->h_snap, 0)) != hipSuccess ||
        (e = hipHostMalloc(&c->h_cancel, kCancelPage, hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void **>(&c->d_cancel), c->h_cancel, 0)) != hipSuccess) {
        dpow_close(c);
        return hip_fail(e, "dpow_open: allocation");
    }
    {   // the control-block ring, aligned to its size (publish() derives the next block's address)
        const uintptr_t rb = kCtrlRing * kCtrlStride * sizeof(Ctrl);
        c->d_ctrl = reinterpret_cast<Ctrl *>((reinterpret_cast<uintptr_t>(c->d_ctrl_alloc) + rb - 1) & ~(rb - 1));
    }
    memset(c->h_snap, 0, kRing * sizeof(Snap));
    memset(c->h_cancel, 0, kCancelPage);
    *bound_word(c) = DPOW_NO_HIT;
    // Clean control blocks and zero claim counters (the launches keep them so): a kernel on
    // the context's own stream, which stays the only device queue a context uses (no null-
    // stream copy: with 8 processes sharing one GPU, every extra queue a process keeps busy
    // pushed the device into queue oversubscription, whose time slices held each search
    // ~10 ms, profiles/r03_rehearsal_queues.json).
    if ((e = context_init(c->d_ctrl, kCtrlRing * kCtrlStride, c->d_claims, (uint32_t)(kClaimRing * kClaimSlot),
                          c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        dpow_close(c);
        return hip_fail(e, "dpow_open: control state");
    }
    // Every search kernel resolved on this device before the first search (once per device and
    // process): a translation unit's code object loads on its first use, which cost round 3's
    // first search ~1 ms (the k = 0 kernel, then a 972.8 us gap before the "_ls" md5 launch).
    if ((e = prepare_device(device)) != hipSuccess) {
        dpow_close(c);
        return hip_fail(e, "dpow_open: loading the search kernels");
    }
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        g_ctxs.push_back(c);
        c->counted = true;
    }
    *out = c;
    return 0;
}

void dpow_close(dpow_ctx *c) {
    if (!c) return;
    if (c->counted) {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), c), g_ctxs.end());
    }
    const DeviceScope on_device(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    // Drained: no watcher of ours reads the node pages any more.  Leave the page registry
    // before the stream is destroyed (dpow_node_release synchronizes every holder's stream).
    c->node = c->d_node = nullptr;
    pages_release_ctx(c);
    batch_free(c->batch);
    scan_free(c->scan);
    census_free(c->census);
    census_many_free(c->census_many);
    scan_many_free(c->scan_many);
    digests_free(c->digests);
    scan_dev_free(c->scan_dev);
    scan_many_dev_free(c->scan_many_dev);
    digests_many_free(c->digests_many);
    if (c->d_ctrl_alloc) (void)hipFree(c->d_ctrl_alloc);
    if (c->d_claims) (void)hipFree(c->d_claims);
    if (c->h_snap) (void)hipHostFree(c->h_snap);
    if (c->h_cancel) (void)hipHostFree(c->h_cancel);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

volatile uint32_t *dpow_cancel_flag(dpow_ctx *c) { return c ? c->h_cancel : nullptr; }
void *dpow_stream(dpow_ctx *c) { return c ? (void *)c->stream : nullptr; }
int dpow_device(dpow_ctx *c) { return c ? c->device : -1; }

int dpow_geometry(dpow_ctx *c, uint32_t *cus, uint32_t *blocks_per_cu, uint32_t *threads_per_block) {
    if (!c) return set_error(DPOW_EINVAL, "dpow_geometry: ctx is NULL");
    if (cus) *cus = c->cus;
    if (blocks_per_cu) *blocks_per_cu = (uint32_t)kBlocksPerCu;
    if (threads_per_block) *threads_per_block = kBlockThreads;
    return 0;
}

int dpow_get_stats(dpow_ctx *c, dpow_stats *out) {
    if (!c || !out) return set_error(DPOW_EINVAL, "dpow_get_stats: NULL argument");
    *out = c->stats;
    return 0;
}

void dpow_reset_stats(dpow_ctx *c) {
    if (!c) return;
    c->stats = dpow_stats{};
}

int dpow_search_bound(dpow_ctx *c, uint64_t global_idx) {
    if (!c) return set_error(DPOW_EINVAL, "dpow_search_bound: ctx is NULL");
    std::lock_guard<std::mutex> g(c->bound_mu);
    if (!c->searching) return 0;  // no search in flight: the caller passes its bound to the next one
    return inject_bound_locked(c, global_idx);
}

int dpow_secret_from_index(uint64_t g, uint8_t secret_out[DPOW_MAX_SECRET], size_t *secret_len) {
    if (!secret_out || !secret_len) return set_error(DPOW_EINVAL, "dpow_secret_from_index: NULL argument");
    if (g == DPOW_NO_HIT) return set_error(DPOW_EINVAL, "dpow_secret_from_index: no hit");
    size_t n = 0;
    secret_out[n++] = (uint8_t)(g & 0xFF);
    for (uint64_t k = g >> 8; k; k >>= 8) secret_out[n++] = (uint8_t)(k & 0xFF);
    *secret_len = n;
    return 0;
}

void dpow_md5(const uint8_t *msg, size_t len, uint8_t digest_out[16]) { md5_digest(msg, len, digest_out); }

uint32_t dpow_trailing_zero_nibbles(const uint8_t digest[16]) { return digest_trailing_zero_nibbles(digest); }

int dpow_verify(const uint8_t *nonce, size_t nonce_len, const uint8_t *secret, size_t secret_len, uint32_t ntz) {
    std::vector<uint8_t> msg(nonce_len + secret_len);
    if (nonce_len) memcpy(msg.data(), nonce, nonce_len);
    if (secret_len) memcpy(msg.data() + nonce_len, secret, secret_len);
    uint8_t d[16];
    md5_digest(msg.data(), msg.size(), d);
    return digest_trailing_zero_nibbles(d) >= ntz ? 1 : 0;
}

int dpow_plan_window(const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                     uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, dpow_plan_launch *out,
                     size_t max_launches) {
    std::vector<PlannedLaunch> plan;
    int n = plan_window(nonce, nonce_len, ntz, worker_byte, worker_bits, k_begin, k_end, plan);
    if (n < 0) return set_error(n, "dpow_plan_window: bad arguments");
    for (size_t i = 0; i < plan.size() && i < max_launches && out; ++i) out[i] = plan[i].info;
    return n;
}

int dpow_plan_candidate(const uint8_t *nonce, size_t nonce_len, uint32_t worker_byte, uint32_t worker_bits,
                        uint64_t local_idx, uint32_t iv_out[4], uint32_t words_out[32], uint32_t *nblk_out) {
    if (!iv_out || !words_out || !nblk_out) return set_error(DPOW_EINVAL, "dpow_plan_candidate: NULL argument");
    const uint64_t k = local_idx >> remainder_bits(worker_bits);
    // The launch a search from the start of k's chunk-length segment would use
    // (it spans the 2^24-k segments up to k: the segment-word path of the kernel).
    const uint32_t clen = chunk_len_of(k);
    uint64_t k_first = clen == 0 ? k : 1ull << (8 * (clen - 1));
    if (const uint64_t w2 = word2_period((uint32_t)(nonce_len % 64) % 4))  // the planner's W0 + 2 split
        if (k_first < k / w2 * w2) k_first = k / w2 * w2;
    std::vector<PlannedLaunch> plan;
    int n = plan_window(nonce, nonce_len, 0, worker_byte, worker_bits, k_first, k + 1, plan);
    if (n != 1) return set_error(n < 0 ? n : DPOW_EINVAL, "dpow_plan_candidate: bad arguments");
    for (int w = 0; w < 4; ++w) iv_out[w] = plan[0].L.iv[w];
    memset(words_out, 0, 32 * sizeof(uint32_t));
    candidate_words(plan[0], local_idx, words_out);
    *nblk_out = plan[0].info.nblk;
    return 0;
}

int dpow_search_batch(dpow_ctx *c, dpow_batch_task *tasks, size_t n_tasks, dpow_batch_stats *stats) {
    const int rc = batch_check(tasks, n_tasks);  // the tasks' own errors first: they need no context
    if (rc < 0) return rc;
    if (!c) return set_error(DPOW_EINVAL, "dpow_search_batch: ctx is NULL");
    if (c->node) return set_error(DPOW_EINVAL, "dpow_search_batch: a node slot is attached to the context");
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return batch_run(&c->batch, c->stream, c->h_cancel, tasks, n_tasks, stats);
}

int dpow_scan(dpow_ctx *c, const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
              uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, dpow_scan_hit *out, size_t max_hits,
              size_t *n_hits, uint64_t *k_done, dpow_batch_stats *stats) {
    if (!out || !n_hits || !k_done) return set_error(DPOW_EINVAL, "dpow_scan: NULL argument");
    if (max_hits < 256) return set_error(DPOW_EINVAL, "dpow_scan: max_hits below 256 (one k's candidates)");
    dpow_batch_task t{};  // the window's own errors first: they need no context
    t.nonce = nonce;
    t.nonce_len = nonce_len;
    t.worker_byte = worker_byte;
    t.k_begin = k_begin;
    t.k_end = k_end;
    const int rc = batch_check_task(t, "dpow_scan");
    if (rc < 0) return rc;
    if (!c) return set_error(DPOW_EINVAL, "dpow_scan: ctx is NULL");
    if (c->node) return set_error(DPOW_EINVAL, "dpow_scan: a node slot is attached to the context");
    *n_hits = 0;
    *k_done = k_begin;
    if (stats) *stats = dpow_batch_stats{};
    if (k_begin == k_end) return DPOW_EXHAUSTED;  // (*k_done = k_end)
    if (__atomic_load_n(c->h_cancel, __ATOMIC_ACQUIRE) != 0u) return DPOW_CANCELLED;  // raised on entry: no launch
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return scan_run(&c->scan, c->stream, c->h_cancel, nonce, nonce_len, ntz, worker_byte, worker_bits, k_begin, k_end,
                    out, max_hits, n_hits, k_done, stats);
}

int dpow_scan_device(dpow_ctx *c, const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                     uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, void *d_idx_out, void *d_tz_out,
                     size_t max_hits, size_t *n_hits, uint64_t *k_done, dpow_batch_stats *stats) {
    if (!d_idx_out || !n_hits || !k_done) return set_error(DPOW_EINVAL, "dpow_scan_device: NULL argument");
    if ((reinterpret_cast<uintptr_t>(d_idx_out) & 7u) != 0u)
        return set_error(DPOW_EINVAL, "dpow_scan_device: indices not 8-byte aligned");
    if (max_hits < DPOW_SCAN_DEVICE_MIN_HITS)
        return set_error(DPOW_EINVAL, "dpow_scan_device: max_hits below 16384 (one workgroup's candidates)");
    dpow_batch_task t{};  // the window's own errors first: they need no context
    t.nonce = nonce;
    t.nonce_len = nonce_len;
    t.worker_byte = worker_byte;
    t.k_begin = k_begin;
    t.k_end = k_end;
    const int rc = batch_check_task(t, "dpow_scan_device");
    if (rc < 0) return rc;
    if (!c) return set_error(DPOW_EINVAL, "dpow_scan_device: ctx is NULL");
    if (c->node) return set_error(DPOW_EINVAL, "dpow_scan_device: a node slot is attached to the context");
    *n_hits = 0;
    *k_done = k_begin;
    if (stats) *stats = dpow_batch_stats{};
    if (k_begin == k_end) return DPOW_EXHAUSTED;  // (*k_done = k_end)
    if (__atomic_load_n(c->h_cancel, __ATOMIC_ACQUIRE) != 0u) return DPOW_CANCELLED;  // raised on entry: no launch
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return scan_dev_run(&c->scan_dev, c->stream, c->h_cancel, nonce, nonce_len, ntz, worker_byte, worker_bits, k_begin,
                        k_end, d_idx_out, d_tz_out, max_hits, n_hits, k_done, stats);
}

int dpow_diag_scan_device_times(dpow_ctx *c, double *mask_ms, double *place_ms, double *depth_ms) {
    if (!c || !mask_ms || !place_ms || !depth_ms)
        return set_error(DPOW_EINVAL, "dpow_diag_scan_device_times: NULL argument");
    scan_dev_times(c->scan_dev, mask_ms, place_ms, depth_ms);
    return 0;
}

int dpow_scan_batch(dpow_ctx *c, dpow_scan_task *tasks, size_t n_tasks, dpow_scan_hit *out, size_t max_hits,
                    size_t *n_out, dpow_batch_stats *stats) {
    const int rc = scan_many_check(tasks, n_tasks, out, max_hits, n_out);  // the call's own errors first: they need no context
    if (rc < 0) return rc;
    if (!c) return set_error(DPOW_EINVAL, "dpow_scan_batch: ctx is NULL");
    if (c->node) return set_error(DPOW_EINVAL, "dpow_scan_batch: a node slot is attached to the context");
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return scan_many_run(&c->scan_many, c->stream, c->h_cancel, tasks, n_tasks, out, max_hits, n_out, stats);
}

int dpow_scan_batch_device(dpow_ctx *c, dpow_scan_task *tasks, size_t n_tasks, void *d_idx_out, void *d_tz_out,
                           void *d_row_out, size_t max_hits, size_t *n_out, dpow_batch_stats *stats) {
    const int rc = scan_many_dev_check(tasks, n_tasks, d_idx_out, d_row_out, max_hits, n_out);  // the call's own errors first: they need no context
    if (rc < 0) return rc;
    if (!c) return set_error(DPOW_EINVAL, "dpow_scan_batch_device: ctx is NULL");
    if (c->node) return set_error(DPOW_EINVAL, "dpow_scan_batch_device: a node slot is attached to the context");
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return scan_many_dev_run(&c->scan_many_dev, c->stream, c->h_cancel, tasks, n_tasks, d_idx_out, d_tz_out, d_row_out,
                             max_hits, n_out, stats);
}

int dpow_census_window(dpow_ctx *c, const uint8_t *nonce, size_t nonce_len, uint32_t worker_byte,
                       uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, dpow_census *out, uint64_t *k_done,
                       dpow_batch_stats *stats) {
    if (!out || !k_done) return set_error(DPOW_EINVAL, "dpow_census_window: NULL argument");
    dpow_batch_task t{};  // the window's own errors first: they need no context
    t.nonce = nonce;
    t.nonce_len = nonce_len;
    t.worker_byte = worker_byte;
    t.k_begin = k_begin;
    t.k_end = k_end;
    const int rc = batch_check_task(t, "dpow_census_window");
    if (rc < 0) return rc;
    if (!c) return set_error(DPOW_EINVAL, "dpow_census_window: ctx is NULL");
    if (c->node) return set_error(DPOW_EINVAL, "dpow_census_window: a node slot is attached to the context");
    census_clear(*out);
    *k_done = k_begin;
    if (stats) *stats = dpow_batch_stats{};
    if (k_begin == k_end) return DPOW_EXHAUSTED;  // (*k_done = k_end)
    if (__atomic_load_n(c->h_cancel, __ATOMIC_ACQUIRE) != 0u) return DPOW_CANCELLED;  // raised on entry: no launch
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return census_run(&c->census, c->stream, c->h_cancel, nonce, nonce_len, worker_byte, worker_bits, k_begin, k_end,
                      out, k_done, stats);
}

int dpow_census_batch(dpow_ctx *c, dpow_census_task *tasks, size_t n_tasks, dpow_batch_stats *stats) {
    const int rc = census_many_check(tasks, n_tasks);  // the tasks' own errors first: they need no context
    if (rc < 0) return rc;
    if (!c) return set_error(DPOW_EINVAL, "dpow_census_batch: ctx is NULL");
    if (c->node) return set_error(DPOW_EINVAL, "dpow_census_batch: a node slot is attached to the context");
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return census_many_run(&c->census_many, c->stream, c->h_cancel, tasks, n_tasks, stats);
}

// The argument errors dpow_digests and dpow_digests_device share (`who`: the entry point named in the message).
static int digests_check(dpow_ctx *c, const uint8_t *nonce, size_t nonce_len, const void *idx, const void *digest_out,
                         const void *tz_out, const char *who) {
    const std::string w(who);
    if (!c || !idx) return set_error(DPOW_EINVAL, w + ": NULL argument");
    if (!digest_out && !tz_out) return set_error(DPOW_EINVAL, w + ": both outputs are NULL");
    if (nonce_len && !nonce) return set_error(DPOW_EINVAL, w + ": nonce is NULL");
    if (nonce_len > DPOW_MAX_NONCE) return set_error(DPOW_EINVAL, w + ": nonce longer than DPOW_MAX_NONCE");
    if (c->node) return set_error(DPOW_EINVAL, w + ": a node slot is attached to the context");
    return 0;
}

int dpow_digests(dpow_ctx *c, const uint8_t *nonce, size_t nonce_len, const uint64_t *global_idx, size_t n,
                 uint8_t *digest_out, uint8_t *tz_out, size_t *n_done, dpow_batch_stats *stats) {
    if (!n_done) return set_error(DPOW_EINVAL, "dpow_digests: NULL argument");
    const int rc = digests_check(c, nonce, nonce_len, global_idx, digest_out, tz_out, "dpow_digests");
    if (rc < 0) return rc;
    for (size_t j = 0; j < n; ++j)
        if ((global_idx[j] >> 8) >= DPOW_K_LIMIT)
            return set_error(DPOW_ERANGE, "dpow_digests: an entry beyond DPOW_K_LIMIT");
    *n_done = 0;
    if (stats) *stats = dpow_batch_stats{};
    if (n == 0) return DPOW_EXHAUSTED;
    if (__atomic_load_n(c->h_cancel, __ATOMIC_ACQUIRE) != 0u) return DPOW_CANCELLED;  // raised on entry: no launch
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return digests_run(&c->digests, c->stream, c->h_cancel, nonce, nonce_len, global_idx, n, digest_out, tz_out, n_done,
                       stats);
}

int dpow_digests_device(dpow_ctx *c, const uint8_t *nonce, size_t nonce_len, const void *d_global_idx, size_t n,
                        void *d_digest_out, void *d_tz_out, dpow_batch_stats *stats) {
    const int rc = digests_check(c, nonce, nonce_len, d_global_idx, d_digest_out, d_tz_out, "dpow_digests_device");
    if (rc < 0) return rc;
    if ((reinterpret_cast<uintptr_t>(d_global_idx) & 7u) != 0u || (reinterpret_cast<uintptr_t>(d_digest_out) & 15u) != 0u)
        return set_error(DPOW_EINVAL, "dpow_digests_device: indices not 8-byte or digests not 16-byte aligned");
    if (stats) *stats = dpow_batch_stats{};
    if (n == 0) return DPOW_EXHAUSTED;
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return digests_run_device(&c->digests, c->stream, nonce, nonce_len, d_global_idx, n, d_digest_out, d_tz_out, stats);
}

int dpow_digests_batch(dpow_ctx *c, dpow_digest_task *tasks, size_t n_tasks, const uint64_t *rows,
                       const uint64_t *global_idx, uint8_t *digest_out, uint8_t *tz_out, size_t *n_done,
                       dpow_batch_stats *stats) {
    const int rc = digests_many_check(tasks, n_tasks, rows, global_idx, n_done);  // the call's own errors first: they need no context
    if (rc < 0) return rc;
    if (!c) return set_error(DPOW_EINVAL, "dpow_digests_batch: ctx is NULL");
    if (c->node) return set_error(DPOW_EINVAL, "dpow_digests_batch: a node slot is attached to the context");
    for (size_t i = 0; i < n_tasks; ++i) {
        tasks[i].n_entries = rows[i + 1] - rows[i];
        tasks[i].n_shallow = 0;
    }
    *n_done = 0;
    if (stats) *stats = dpow_batch_stats{};
    if (rows[n_tasks] == 0) return DPOW_EXHAUSTED;
    if (__atomic_load_n(c->h_cancel, __ATOMIC_ACQUIRE) != 0u) return DPOW_CANCELLED;  // raised on entry: no launch
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return digests_many_run(&c->digests_many, &c->digests, c->stream, c->h_cancel, tasks, n_tasks, rows, global_idx,
                            digest_out, tz_out, n_done, stats);
}

int dpow_digests_batch_device(dpow_ctx *c, dpow_digest_task *tasks, size_t n_tasks, const void *d_rows,
                              const void *d_global_idx, size_t n, void *d_digest_out, void *d_tz_out,
                              dpow_batch_stats *stats) {
    const int rc = digests_many_check_device(tasks, n_tasks, d_rows, d_global_idx, d_digest_out);  // the call's own errors first: they need no context
    if (rc < 0) return rc;
    if (!c) return set_error(DPOW_EINVAL, "dpow_digests_batch_device: ctx is NULL");
    if (c->node) return set_error(DPOW_EINVAL, "dpow_digests_batch_device: a node slot is attached to the context");
    if (stats) *stats = dpow_batch_stats{};
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    return digests_many_run_device(&c->digests_many, c->stream, tasks, n_tasks, d_rows, d_global_idx, n, d_digest_out,
                                   d_tz_out, stats);
}

int dpow_search(dpow_ctx *c, const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, uint64_t *best_global_idx,
                uint8_t secret_out[DPOW_MAX_SECRET], size_t *secret_len) {
    if (!c || !best_global_idx || !secret_out || !secret_len)
        return set_error(DPOW_EINVAL, "dpow_search: NULL argument");
    if (nonce_len && !nonce) return set_error(DPOW_EINVAL, "dpow_search: nonce is NULL");
    if (worker_byte > 255u) return set_error(DPOW_EINVAL, "dpow_search: worker_byte > 255");
    if (k_end > DPOW_K_LIMIT) return set_error(DPOW_ERANGE, "dpow_search: k_end beyond DPOW_K_LIMIT");
    *secret_len = 0;
    c->stats.searches++;
    c->last_use.store(now_ns(), std::memory_order_relaxed);
    if (k_begin >= k_end) return DPOW_EXHAUSTED;
    // A node slot whose stop is raised (another rank was cancelled or failed), or a
    // raised cancel flag: nothing to do.  A node slot's stop is raised by every
    // attached rank that returns DPOW_CANCELLED or an error, so the other ranks end
    // their searches too (node_stop below).
    dpow_node_slot *const node = c->node;
    if (node && __atomic_load_n(&node->stop, __ATOMIC_ACQUIRE) != 0u) return DPOW_CANCELLED;
    if (__atomic_load_n(c->h_cancel, __ATOMIC_ACQUIRE) != 0u) {
        dpow_node_stop(node);
        return DPOW_CANCELLED;
    }
    const int status = search_window(c, nonce, nonce_len, ntz, worker_byte, worker_bits, k_begin, k_end,
                                     best_global_idx, secret_out, secret_len);
    if (node) {
        if (status == DPOW_FOUND) dpow_node_post(node, *best_global_idx);
        else if (status != DPOW_EXHAUSTED) dpow_node_stop(node);
    }
    return status;
}

}  // extern "C"
