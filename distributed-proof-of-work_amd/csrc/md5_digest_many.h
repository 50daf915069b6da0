// md5_digest_many.h -- the digests of many nonces (dpow_digests_batch, dpow_digests_batch_device):
// MD5 and depth of a list in CSR order -- entry e with rows[i] <= e < rows[i + 1] is a global index
// of task i's nonce -- in one pass.  Definitions shared by the gfx950 kernel (md5_digest_many.hip),
// its host loops (digests_many.cpp) and the host helper dpow_digests_batch_walk.
//
// The kernel is digest_kernel's (md5_digest.h) with the task found on the device: the rows stay
// where dpow_scan_batch_device left them, and nothing per entry says which task it belongs to.  A
// wave finds the task of its first entry by bisecting the rows and walks forward from there, one
// pass per non-empty task that overlaps its 64 entries (digest_many_walk below, the one piece of
// code behind the kernel and dpow_digests_batch_walk).
#pragma once

#include "md5_batch.h"
#include "md5_digest.h"

namespace dpow {

// One launch, passed by value.  The task table holds batch_fill_task rows with worker_bits = 0, row
// i task i's, with the task's own ntz.  Workgroup b takes the launch's entries
// [b * group, min(n, (b + 1) * group)); entry e of the launch is entry e_base + e of the list the
// rows describe, so one rows array serves every chunk and launch of a call, while idx, digest and tz
// are the launch's own (a staging set, or the caller's arrays from e_base on).
struct DigestManyLaunch {
    const unsigned long long *rows;  // n_tasks + 1 row pointers (8-byte aligned), whatever they hold; the kernel
                                     //  takes them as a __restrict__ argument of its own (scalar loads)
    const unsigned long long *idx;   // n global indices
    uint4 *digest;                   // n digests, or null
    uint8_t *tz;                     // n depth bytes, or null
    unsigned long long *shallow;     // per task: entries with depth < the task's ntz, added to
    uint32_t *ctl;                   // device words, added to: [0] entries out of range, [1] entries no task covers
    unsigned long long e_base;       // the list position of the launch's entry 0
    uint32_t n;                      // entries of this launch (<= kDigestDeviceSlice)
    uint32_t group;                  // entries per workgroup, a multiple of 256
    uint32_t n_tasks;                // 1 .. DPOW_BATCH_MAX
};

// The last task t >= hint with rows[t] <= e, given rows[hint] <= e; `hint` itself when no row above
// it is at most e.  Reads rows[hint + 1 .. n_tasks) only, and ends within log2(n_tasks) + 1 steps
// whatever the rows hold.  (The first test spares a wave that is still in the task of its last step
// the bisection.)
DPOW_HD uint32_t digest_many_find(const unsigned long long *rows, uint32_t n_tasks, uint32_t hint, uint64_t e) {
    uint32_t a = hint, b = n_tasks;  // rows[b] > e, or b == n_tasks
    if (a + 1u < n_tasks && rows[a + 1u] > e) return a;
    while (b - a > 1u) {
        const uint32_t mid = a + (b - a) / 2u;
        if (rows[mid] <= e) a = mid;
        else b = mid;
    }
    return a;
}

// The passes of one wave over the list positions [e_first, e_end), e_end - e_first <= 64:
// pass(t, lo, hi) for every task t, in ascending order, whose segment [rows[t], rows[t + 1]) meets
// the wave's positions in the non-empty [lo, hi).  Returns the task the walk began at, the hint of
// the wave's next step (a wave's positions only ascend).
//
// With rows that begin at or below e_first's task and do not descend, the passes are disjoint and
// cover exactly the wave's positions within [rows[0], rows[n_tasks]).  Whatever the rows hold --
// descending ones included -- the walk reads rows[0 .. n_tasks] only, names no task >= n_tasks,
// keeps every [lo, hi) within [e_first, e_end) and ends within n_tasks steps: t only grows.
template <typename Pass>
DPOW_HD uint32_t digest_many_walk(const unsigned long long *rows, uint32_t n_tasks, uint32_t hint, uint64_t e_first,
                                  uint64_t e_end, Pass &&pass) {
    const uint32_t t0 = digest_many_find(rows, n_tasks, hint, e_first);
    uint64_t r0 = rows[t0];
    for (uint32_t t = t0; t < n_tasks; ++t) {
        if (r0 >= e_end) break;
        const uint64_t r1 = rows[t + 1u];
        const uint64_t lo = r0 > e_first ? r0 : e_first, hi = r1 < e_end ? r1 : e_end;
        if (lo < hi) pass(t, lo, hi);
        if (r1 >= e_end) break;
        r0 = r1;
    }
    return t0;
}

#if defined(__HIPCC__)
hipError_t digest_many_prepare();
hipError_t digest_many_launch(const BatchTask *tasks, const DigestManyLaunch &D, uint32_t n_blocks, hipStream_t stream);
#endif

}  // namespace dpow
