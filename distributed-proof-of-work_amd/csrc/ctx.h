// ctx.h -- what the host units of the library share: the context (struct dpow_ctx), its ring and
// pinned-page constants, and the small helpers every unit needs (errors, the current device, the
// clock, the timer slack, the stream-liveness check).  Internal: not part of the C ABI, and
// nothing declared here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <sys/prctl.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dpow.h"
#include "dpow_common.h"
#include "plan.h"

#pragma GCC visibility push(hidden)

namespace dpow {

// Sets dpow_last_error for the calling thread and returns code (dpow_api.cpp).
int set_error(int code, const std::string &msg);

inline int hip_fail(hipError_t e, const char *what) {
    return set_error(DPOW_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define DPOW_HIP(call)                                    \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

// The calling thread's current device (HIP per-thread state) for the duration of an
// entry point, restored on return: a host thread that drives several GPUs -- one rank's
// coordinator mirror with a worker per GPU, torch's current device -- keeps its own.
struct DeviceScope {
    int prev = -1;
    hipError_t e = hipSuccess;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) e = hipSetDevice(dev);
        if (prev == dev) prev = -1;  // nothing to restore
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

inline int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// The calling thread's timer slack, lowered for sleeping polls and restored when the wait is
// over -- the thread is the caller's own, e.g. a cgo goroutine's.
struct TimerSlack {
    long old_slack = -1;
    void lower() {
        if (old_slack >= 0) return;
        // Linux pads a normal thread's nanosleep by its 50 us default timer slack,
        // which a hit's record would wait out; 1 us keeps the poll at ~kPollNs.
        const int r = prctl(PR_GET_TIMERSLACK, 0UL, 0UL, 0UL, 0UL);
        if (r <= 0) return;
        old_slack = r;
        (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL);
    }
    ~TimerSlack() {
        if (old_slack >= 0) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)old_slack, 0UL, 0UL, 0UL);
    }
};

// A wait for a completion record queries its stream now and then, so a failed launch, or a
// stream that went idle without writing the record, ends the wait with an error: 1 when the
// record word holds `want` after all, 0 while the stream is busy (go on waiting), < 0 on error
// (`idle_msg`: the caller's "stream idle without ... completion record").
inline int stream_liveness(hipStream_t stream, const uint32_t *record, uint32_t want, const char *idle_msg) {
    const hipError_t q = hipStreamQuery(stream);
    if (q == hipSuccess) {
        if (__atomic_load_n(record, __ATOMIC_ACQUIRE) == want) return 1;
        return set_error(DPOW_EHIP, idle_msg);
    }
    if (q != hipErrorNotReady) return hip_fail(q, "hipStreamQuery");
    return 0;
}

// Claim-counter slots (kClaimSlot counters each) used round-robin by the launches
// of a search: zeroed at search start, re-zeroed by each launch's last workgroup.
constexpr size_t kClaimRing = 64;
// Launches kept in flight: launch j is queued only after the completion record
// of launch j - kDepth shows no hit and no cancel, so a hit or a cancel leaves
// at most kDepth launches to retire (each exits at its first check).
constexpr size_t kDepth = 3;
static_assert(kDepth < kClaimRing, "a claim slot is reused only after its launch completed");
constexpr size_t kRing = 8;  // completion records and event pairs, indexed by launch seq (>= kDepth + 1)
// Words of the pinned cancel page: the stale launch sequence (Launch::stale) and the
// 64-bit bound injected by dpow_search_bound (Launch::ext_bound, relayed by the watcher).
constexpr size_t kStaleWord = 8;
constexpr size_t kBoundWord = 16;  // uint32 index of an 8-byte-aligned 64-bit word
constexpr size_t kEarlyWord = 20;  // uint32 index of kCtrlRing 64-bit early-hit words (Launch::early)
constexpr size_t kCancelPage = 128;
static_assert(kEarlyWord * 4 + kCtrlRing * 8 <= kCancelPage, "the early-hit words fit the pinned page");

// Searches in flight per device in this process.  Several logical workers may
// share one GPU (the coordinator mirror places W workers round-robin on the
// node's devices; BASELINE config 4 runs 8 on one in the 1-GPU bench): each
// search then sizes its persistent grids to its share of the device and keeps its
// launches short (plan.h grid_share, cap_shared_launch), so the device stays full and
// every search's grid follows the others that start or end beside it.
constexpr int kMaxDevices = 64;
extern std::atomic<int> g_active[kMaxDevices];  // search.cpp
// Contexts open per device in this process, each with the time it was last used (opened, or a
// search started): several used recently means other searches may start beside this one at any
// moment (the coordinator mirror's logical workers); contexts idle in a pool do not count.
extern std::mutex g_ctx_mu;  // search.cpp
extern std::vector<dpow_ctx *> g_ctxs;

// One queued launch: its completion record slot (seq % kRing) and what its record adds
// to dpow_stats once consumed (launches, candidates, and the kernel time the launch
// stamps into the record itself).
struct LaunchSlot {
    uint64_t seq = 0;       // launch sequence number of the slot's last user
    bool in_flight = false; // its record was not consumed: it may still be running
    uint64_t candidates = 0;
    uint64_t g_end = 0;    // global indices of this launch are below g_end = k_end * 256
    hipStream_t stream = nullptr;  // the stream it was queued on (the k = 0 kernel: the second one)
};

struct BatchState;  // batch.h
struct ScanState;   // scan.h
struct CensusState;  // census.h
struct CensusManyState;  // census_many.h
struct ScanManyState;  // scan_many.h
struct DigestState;  // digests.h
struct ScanDevState;  // scan_dev.h
struct ScanManyDevState;  // scan_many_dev.h
struct DigestManyState;  // digests_many.h

// The body of dpow_search (arguments checked): search.cpp.
int search_window(dpow_ctx *c, const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                  uint32_t worker_bits, uint64_t k_begin, uint64_t k_end, uint64_t *best_global_idx,
                  uint8_t secret_out[DPOW_MAX_SECRET], size_t *secret_len);

// dpow_close: ctx's references go (its stream has drained); pages without holders are
// unregistered (node.cpp).
void pages_release_ctx(dpow_ctx *c);

}  // namespace dpow

// (Default visibility, as before the split: the type names the std::vector<dpow_ctx *> instantiation.)
struct __attribute__((visibility("default"))) dpow_ctx {
    int device = 0;
    bool counted = false;  // in g_ctxs
    hipStream_t stream = nullptr;
    dpow::Ctrl *d_ctrl = nullptr;  // kCtrlRing control blocks (kCtrlStride apart, aligned to the ring's size);
                                   //  ctrl_idx's is clean
    dpow::Ctrl *d_ctrl_alloc = nullptr;
    uint32_t ctrl_idx = 0;
    unsigned long long *d_claims = nullptr;  // kClaimRing slots of kClaimSlot claim counters
    dpow::Snap *h_snap = nullptr;  // kRing completion records: pinned, host-coherent, mapped
    dpow::Snap *d_snap = nullptr;  // device alias
    uint32_t *h_cancel = nullptr;  // pinned, host-coherent, mapped: [0] the cancel flag, [kStaleWord] stale seq,
                                   //  [kBoundWord] the injected bound (64-bit)
    uint32_t *d_cancel = nullptr;  // device alias
    uint32_t cus = 0;
    uint64_t seq = 0;  // launches ever queued on this context (record/slot index = seq % kRing)
    dpow::LaunchSlot slots[dpow::kRing];
    dpow_stats stats{};
    // External bound (dpow_search_bound): lowered from another thread while a
    // search runs, written to the pinned bound word, which the running launch's
    // watcher relays to Ctrl::best (as it relays the node slot's best).
    std::mutex bound_mu;
    bool searching = false;                      // under bound_mu
    std::atomic<uint64_t> ext_bound{DPOW_NO_HIT};  // the lowest bound injected into the running search
    // Node slot (dpow_node_attach): shared by the ranks of one node, polled while a
    // search waits for its records.
    dpow_node_slot *node = nullptr;
    dpow_node_slot *d_node = nullptr;  // its device alias (the watcher polls it)
    // A/B overrides of the launch policy (dpow_diag.h): DPOW_DIAG_POLL_WB (wave-blocks per poll
    // group), DPOW_DIAG_BPC (worker workgroups per CU), DPOW_DIAG_MIN_CHUNK (minimum wave-blocks
    // per claim, a power of two), DPOW_DIAG_CPW (big claims per wave), DPOW_DIAG_SHARE_LAUNCH_US
    // (launch length on a shared device), DPOW_DIAG_SHARE_MAX (grid share cap); 0 = the policy.
    dpow::LaunchKnobs knobs;
    int64_t diag_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the last search's host timeline (dpow_diag_search_times)
    // The last search's launches, in launch order (dpow_diag_search_launches): host times of
    // each queueing and record consumption (absolute now_ns), the search's start.
    struct DiagLaunch {
        uint64_t seq = 0, candidates = 0, g_end = 0;
        int32_t kind = 0;  // 0: the k = 0 kernel, 1: an md5 launch
        int64_t queued = -1, seen = -1;
    };
    static constexpr size_t kDiagLaunches = 32;
    DiagLaunch diag_l[kDiagLaunches];
    size_t diag_nl = 0;
    int64_t diag_t0 = 0;
    uint64_t dev_key = 0;  // the GPU's identity across processes: a hash of its PCI bus id, never 0 (board.cpp)
    std::atomic<int64_t> last_use{0};  // now_ns() of dpow_open / the last search start (recent_contexts)
    // The context searches every partition of a node whose ranks share its GPU (dpow_board_search):
    // the young-search rule (plan.h kYoungNs) does not share the device with the idle ranks.
    bool solo = false;
    dpow::BatchState *batch = nullptr;  // buffers of dpow_search_batch: allocated by the first batch (batch.cpp)
    dpow::ScanState *scan = nullptr;    // buffers of dpow_scan: allocated by the first scan (scan.cpp)
    dpow::CensusState *census = nullptr;  // buffers of dpow_census_window: allocated by the first census (census.cpp)
    dpow::CensusManyState *census_many = nullptr;  // buffers of dpow_census_batch: allocated by the first call (census_many.cpp)
    dpow::ScanManyState *scan_many = nullptr;  // buffers of dpow_scan_batch: allocated by the first call (scan_many.cpp)
    dpow::DigestState *digests = nullptr;  // buffers of dpow_digests: allocated by the first call (digests.cpp)
    dpow::ScanDevState *scan_dev = nullptr;  // buffers of dpow_scan_device: allocated by the first call (scan_dev.cpp)
    dpow::ScanManyDevState *scan_many_dev = nullptr;  // buffers of dpow_scan_batch_device: allocated by the first call (scan_many_dev.cpp)
    dpow::DigestManyState *digests_many = nullptr;  // buffers of dpow_digests_batch and dpow_digests_batch_device: allocated by the first call (digests_many.cpp)
};

namespace dpow {

inline uint64_t *bound_word(dpow_ctx *c) { return reinterpret_cast<uint64_t *>(c->h_cancel + kBoundWord); }

}  // namespace dpow

#pragma GCC visibility pop
