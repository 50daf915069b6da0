// node.cpp -- the node layer: the registry of host pages that hold node slots, the slot's
// attach / release / post / stop, the node vote and the node search (dpow_node_mine).
#include <string.h>
#include <time.h>

#include <algorithm>

#include "../../include/dpow_worker.h"
#include "ctx.h"
#include "node.h"

using namespace dpow;

namespace {

// Host pages registered for node slots (hipHostRegister: process-wide, not per context).  A
// context that attaches a slot holds its pages until dpow_close (detaching keeps them, so
// node_mine's attach / detach per node search costs no registration); a page is registered by
// its first holder and unregistered when its last holder closes, so two contexts of one
// process attached to one slot (one per GPU, or the 2-rank rehearsal) never see the page
// unregistered under a running watcher.  Memory about to be unmapped is released explicitly
// (dpow_node_release: NodeBoard.close), so a new mapping at the same address is registered
// afresh instead of reusing the old registration's device alias.
// The registration is portable (every device of the process may map the page) and the device
// alias is looked up per device, under that device, the first time a context of that device
// holds the page: a process whose contexts on several GPUs share one slot (a node scheduler with
// a context per GPU, the board's workers) never hands one GPU's alias to another's watcher
// (VERDICT r05 item 2(i)).
struct PageEntry {
    void *page;
    bool foreign;                    // registered outside this library: never unregistered here
    std::vector<dpow_ctx *> holders;
    char *dev[kMaxDevices] = {};     // the page's alias on each device (hipHostGetDevicePointer, once per device)
};
std::mutex g_page_mu;
std::vector<PageEntry> g_pages;

// Drop entry i (every holder's streams drained by the caller).  g_page_mu held.
void page_drop_locked(size_t i) {
    if (!g_pages[i].foreign) (void)hipHostUnregister(g_pages[i].page);
    g_pages.erase(g_pages.begin() + (long)i);
}

// A reference of ctx on `page` (registering it if no context holds it).  g_page_mu held, the
// calling thread on ctx's device.  *dev: the page's alias on ctx's device.
hipError_t page_hold_locked(dpow_ctx *c, void *page, char **dev) {
    PageEntry *pe = nullptr;
    for (PageEntry &x : g_pages)
        if (x.page == page) {
            pe = &x;
            break;
        }
    if (!pe) {
        hipError_t e = hipHostRegister(page, 4096, hipHostRegisterMapped | hipHostRegisterPortable);
        bool foreign = false;
        if (e == hipErrorHostMemoryAlreadyRegistered) {
            (void)hipGetLastError();
            e = hipSuccess;
            foreign = true;
        }
        if (e != hipSuccess) return e;
        g_pages.push_back(PageEntry{page, foreign, {}, {}});
        pe = &g_pages.back();
    }
    if (!pe->dev[c->device]) {
        void *d = nullptr;
        const hipError_t e = hipHostGetDevicePointer(&d, page, 0);
        if (e != hipSuccess) {
            if (pe->holders.empty()) page_drop_locked((size_t)(pe - g_pages.data()));
            return e;
        }
        pe->dev[c->device] = static_cast<char *>(d);
    }
    if (std::find(pe->holders.begin(), pe->holders.end(), c) == pe->holders.end()) pe->holders.push_back(c);
    *dev = pe->dev[c->device];
    return hipSuccess;
}

}  // namespace

// dpow_close: ctx's references go (its stream has drained); pages without holders are unregistered.
void dpow::pages_release_ctx(dpow_ctx *c) {
    std::lock_guard<std::mutex> g(g_page_mu);
    for (size_t i = g_pages.size(); i-- > 0;) {
        auto &h = g_pages[i].holders;
        h.erase(std::remove(h.begin(), h.end(), c), h.end());
        if (h.empty()) page_drop_locked(i);
    }
}

extern "C" {

int dpow_node_attach(dpow_ctx *c, dpow_node_slot *slot) {
    if (!c) return set_error(DPOW_EINVAL, "dpow_node_attach: ctx is NULL");
    if (!slot) {  // detach: the pages stay held (registered) until dpow_close or dpow_node_release
        c->node = c->d_node = nullptr;
        return 0;
    }
    if (((uintptr_t)slot & 7u) != 0u) return set_error(DPOW_EINVAL, "dpow_node_attach: slot not 8-byte aligned");
    if (c->device >= kMaxDevices) return set_error(DPOW_EINVAL, "dpow_node_attach: device ordinal too large");
    // Map the slot's host page(s) for the watcher (fine-grained: hipHostRegister's default).
    const DeviceScope on_device(c->device);
    if (on_device.e != hipSuccess) return hip_fail(on_device.e, "hipSetDevice");
    // The device alias of a slot within one page comes from its page's, looked up once when the
    // page is registered: a node search attaches once per call, and hipHostGetDevicePointer per
    // attach cost every node search its call (a board's slots are 64-byte aligned; a slot
    // across two pages still asks the runtime).
    const uintptr_t pg = 4096;
    const bool one_page = (((uintptr_t)slot & (pg - 1)) + sizeof(dpow_node_slot)) <= pg;
    char *dev = nullptr;
    {
        std::lock_guard<std::mutex> g(g_page_mu);
        for (uintptr_t a = (uintptr_t)slot & ~(pg - 1); a < (uintptr_t)slot + sizeof(dpow_node_slot); a += pg) {
            char *d = nullptr;
            const hipError_t e = page_hold_locked(c, (void *)a, &d);
            if (e != hipSuccess) return hip_fail(e, "dpow_node_attach: hipHostRegister");
            if (!dev) dev = d;
        }
    }
    void *d = dev + ((uintptr_t)slot & (pg - 1));
    if (!one_page) DPOW_HIP(hipHostGetDevicePointer(&d, slot, 0));
    c->node = slot;
    c->d_node = (dpow_node_slot *)d;
    return 0;
}

int dpow_node_release(void *mem, size_t len) {
    if (!mem || !len) return 0;
    const uintptr_t pg = 4096;
    const uintptr_t lo = (uintptr_t)mem & ~(pg - 1), hi = (uintptr_t)mem + len;
    std::lock_guard<std::mutex> g(g_page_mu);
    for (const PageEntry &pe : g_pages) {
        const uintptr_t p = (uintptr_t)pe.page;
        if (p < lo || p >= hi) continue;
        for (dpow_ctx *h : pe.holders)
            if (h->node && (uintptr_t)h->node < p + pg && (uintptr_t)h->node + sizeof(dpow_node_slot) > p)
                return set_error(DPOW_EINVAL, "dpow_node_release: a context is still attached to a slot in the range");
    }
    for (size_t i = g_pages.size(); i-- > 0;) {
        const uintptr_t p = (uintptr_t)g_pages[i].page;
        if (p < lo || p >= hi) continue;
        // launches a holder left queued behind its last search may still read the page
        for (dpow_ctx *h : g_pages[i].holders) {
            const DeviceScope on_device(h->device);
            const hipError_t e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) return hip_fail(e, "dpow_node_release: hipStreamSynchronize");
        }
        page_drop_locked(i);
    }
    return 0;
}

void dpow_node_slot_reset(dpow_node_slot *slot) {
    if (!slot) return;
    __atomic_store_n(&slot->stop, 0u, __ATOMIC_RELAXED);
    __atomic_store_n(&slot->best, DPOW_NO_HIT, __ATOMIC_RELEASE);
}

void dpow_node_post(dpow_node_slot *slot, uint64_t global_idx) {
    if (!slot) return;
    uint64_t cur = __atomic_load_n(&slot->best, __ATOMIC_RELAXED);
    while (global_idx < cur &&
           !__atomic_compare_exchange_n(&slot->best, &cur, global_idx, true, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED)) {
    }
}

int dpow_node_vote(dpow_node_vote_entry *votes, uint32_t rank, uint32_t world, uint64_t epoch, const int64_t in[3],
                   int64_t out[3], int64_t timeout_ns) {
    return dpow::node_vote(votes, rank, world, epoch, in, out, timeout_ns, nullptr);
}

void dpow_node_stop(dpow_node_slot *slot) {
    if (slot) __atomic_store_n(&slot->stop, 1u, __ATOMIC_RELEASE);
}

}  // extern "C"

// dpow_node_vote, and the wait of a board search (dpow_board_search): `abort_flag` non-NULL and
// raised (the rank's cancel flag: its task was killed) ends the wait with DPOW_CANCELLED, the
// vote left behind -- every rank of a board task is killed by the same Found / Cancel fan-out
// (coordinator.go:210-230), so none is left waiting for it.
int dpow::node_vote(dpow_node_vote_entry *votes, uint32_t rank, uint32_t world, uint64_t epoch, const int64_t in[3],
                    int64_t out[3], int64_t timeout_ns, const uint32_t *abort_flag) {
    if (!votes || !in || !out || world == 0 || rank >= world || epoch == 0)
        return set_error(DPOW_EINVAL, "dpow_node_vote: bad argument");
    dpow_node_vote_entry &mine = votes[2 * rank + (epoch & 1)];
    for (int i = 0; i < 3; ++i) __atomic_store_n(&mine.v[i], in[i], __ATOMIC_RELAXED);
    __atomic_store_n(&mine.epoch, epoch, __ATOMIC_RELEASE);
    int64_t acc[3] = {in[0], in[1], in[2]};
    const int64_t t0 = now_ns();
    // Spin while the other ranks are expected soon (a node's ranks end a search within tens of
    // microseconds of each other), then poll every 2 us with the thread's timer slack lowered
    // (a 2 us nanosleep under Linux's default 50 us slack wakes ~50 us late).
    constexpr int64_t kVoteSpinNs = 500000;
    TimerSlack slack;
    for (uint32_t r = 0; r < world; ++r) {
        if (r == rank) continue;
        const dpow_node_vote_entry &e = votes[2 * r + (epoch & 1)];
        for (uint64_t it = 0; __atomic_load_n(&e.epoch, __ATOMIC_ACQUIRE) != epoch; ++it) {
            if (abort_flag && it % 64 == 0 && __atomic_load_n(abort_flag, __ATOMIC_ACQUIRE) != 0u) return DPOW_CANCELLED;
            if (it % 64 != 0 || now_ns() - t0 < std::min(kVoteSpinNs, timeout_ns)) {
                __builtin_ia32_pause();
                continue;
            }
            if (now_ns() - t0 > timeout_ns)
                return set_error(DPOW_EPROTO, "dpow_node_vote: rank " + std::to_string(r) + " did not vote at epoch " +
                                                  std::to_string(epoch));
            slack.lower();
            const struct timespec d = {0, 2000};
            nanosleep(&d, nullptr);
        }
        for (int i = 0; i < 3; ++i) {
            const int64_t v = __atomic_load_n(&e.v[i], __ATOMIC_RELAXED);
            if (v < acc[i]) acc[i] = v;
        }
    }
    for (int i = 0; i < 3; ++i) out[i] = acc[i];
    return 0;
}

extern "C" int dpow_node_mine(dpow_ctx *c, dpow_node_slot *slot, dpow_node_vote_entry *votes, uint32_t rank,
                              uint32_t world, uint64_t *epoch, int64_t vote_timeout_ns, const uint8_t *nonce,
                              size_t nonce_len, uint32_t ntz, uint64_t k_begin, uint64_t k_limit, uint64_t first_k,
                              uint64_t batch_k, uint64_t *best_global_idx, uint8_t secret_out[DPOW_MAX_SECRET],
                              size_t *secret_len, uint32_t *batches) {
    return dpow::node_mine(c, slot, votes, rank, world, epoch, vote_timeout_ns, nonce, nonce_len, ntz, k_begin, k_limit,
                           first_k, batch_k, best_global_idx, secret_out, secret_len, batches, false, 0);
}

// dpow_node_mine; `abandon_on_cancel` (a board search, dpow_board_search): a rank whose cancel flag
// is raised -- its task was killed by Found or Cancel -- stops the slot and returns DPOW_CANCELLED
// at once instead of voting running = 0 and waiting for the other ranks' votes.  The fan-out kills
// every rank of the task, so each leaves on its own kill, also when some rank never joined (a
// worker that answered from its cache, worker.go:261-299).
int dpow::node_mine(dpow_ctx *c, dpow_node_slot *slot, dpow_node_vote_entry *votes, uint32_t rank, uint32_t world,
                    uint64_t *epoch, int64_t vote_timeout_ns, const uint8_t *nonce, size_t nonce_len, uint32_t ntz,
                    uint64_t k_begin, uint64_t k_limit, uint64_t first_k, uint64_t batch_k, uint64_t *best_global_idx,
                    uint8_t secret_out[DPOW_MAX_SECRET], size_t *secret_len, uint32_t *batches, bool abandon_on_cancel,
                    int role) {
    if (!c || !slot || !epoch || !best_global_idx || !secret_out || !secret_len || !batches)
        return set_error(DPOW_EINVAL, "dpow_node_mine: NULL argument");
    if (world == 0 || (world & (world - 1)) != 0 || world > 256 || rank >= world)
        return set_error(DPOW_EINVAL, "dpow_node_mine: world must be a power of two <= 256, rank < world");
    if (batch_k == 0 || k_limit > DPOW_K_LIMIT) return set_error(DPOW_EINVAL, "dpow_node_mine: bad window");
    // The partition of rank r of world 2^b: worker_byte = r, worker_bits = b (coordinator.go:127,326).
    const uint32_t wbits = (uint32_t)__builtin_ctz(world);
    *batches = 0;
    *secret_len = 0;
    // A rank that cannot attach the slot fails its first batch: it stops the slot (the other
    // ranks' searches end at once) and votes healthy = 0 at the first boundary.
    int err = dpow_node_attach(c, slot);
    if (err < 0) dpow_node_stop(slot);
    uint64_t k = k_begin, window = first_k ? first_k : batch_k;
    uint8_t sec[DPOW_MAX_SECRET];
    size_t slen = 0;
    uint64_t own = DPOW_NO_HIT;  // this rank's verified hit (the secret bytes are ours)
    int status = DPOW_EXHAUSTED;
    while (k < k_limit) {
        const uint64_t ke = k_limit - k > window ? k + window : k_limit;
        window = batch_k;
        int rc = DPOW_EXHAUSTED;
        if (err == 0) {
            uint64_t best = DPOW_NO_HIT;
            // role 0: this rank's partition; 1: every partition of the node (the ranks share this
            // GPU, dpow_board_search); 2: none (the role-1 rank covers this one's window)
            if (role == 2) rc = DPOW_EXHAUSTED;
            else rc = dpow_search(c, nonce, nonce_len, ntz, role == 1 ? 0 : rank, role == 1 ? 0 : wbits, k, ke, &best,
                                  sec, &slen);
            if (rc < 0) {
                err = rc;
                dpow_node_stop(slot);
            } else if (rc == DPOW_FOUND && best < own) {
                own = best;
                memcpy(secret_out, sec, slen);
                *secret_len = slen;
            }
        }
        const int64_t running =
            (err != 0 || rc == DPOW_CANCELLED || __atomic_load_n(c->h_cancel, __ATOMIC_ACQUIRE) != 0u) ? 0 : 1;
        const uint64_t posted = __atomic_load_n(&slot->best, __ATOMIC_ACQUIRE);
        const int64_t in[3] = {(int64_t)(own < posted ? own : posted), running, err != 0 ? 0 : 1};
        int64_t out[3] = {in[0], in[1], in[2]};
        if (abandon_on_cancel && err == 0 && __atomic_load_n(c->h_cancel, __ATOMIC_ACQUIRE) != 0u) {
            // this rank was killed: leave without the vote
            dpow_node_stop(slot);
            status = DPOW_CANCELLED;
            break;
        }
        if (votes) {
            const int vr = node_vote(votes, rank, world, ++*epoch, in, out, vote_timeout_ns,
                                     abandon_on_cancel ? c->h_cancel : nullptr);
            if (vr == DPOW_CANCELLED) {
                dpow_node_stop(slot);
                status = DPOW_CANCELLED;
                break;
            }
            if (vr < 0) {
                err = err ? err : vr;
                out[2] = 0;
            }
        }
        ++*batches;
        if (out[2] == 0) {  // a rank failed: the node's search is lost (coordinator.go:202-206)
            status = err ? err : set_error(DPOW_EPROTO, "dpow_node_mine: another rank's search failed");
            break;
        }
        if ((uint64_t)out[0] != DPOW_NO_HIT) {
            *best_global_idx = (uint64_t)out[0];
            if ((uint64_t)out[0] != own) dpow_secret_from_index((uint64_t)out[0], secret_out, secret_len);
            status = DPOW_FOUND;
            break;
        }
        if (out[1] == 0) {
            status = DPOW_CANCELLED;
            break;
        }
        k = ke;
    }
    if (c->node == slot) c->node = c->d_node = nullptr;  // detach (the pages stay held: dpow_node_attach)
    if (status != DPOW_FOUND) *secret_len = 0;
    return status;
}
