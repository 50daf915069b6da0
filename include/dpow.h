/*
 * dpow.h -- C ABI of the MI355X proof-of-work search (libdpow.so).
 *
 * The drop-in boundary for philipjesic/Distributed-Proof-Of-Work's hot path:
 * the worker's brute-force search, `miner` (worker.go:258-401), whose search
 * loop (worker.go:301-400) is replaced by GPU dispatch.  The reference has no
 * FFI of its own; these entry points are what its Go worker would bind through
 * cgo (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Plain C types only (pointers + sizes); no HIP / torch types cross the ABI.
 * Ownership: the caller owns every host buffer passed in or out; the library
 * owns all device memory and the pinned cancel flag of a context.
 * Threading: one search in flight per context (the caller serialises); the
 * cancel flag may be written from any thread while a search runs.  An entry point
 * that works on a context's GPU makes it the calling thread's current HIP device
 * for the call and restores the caller's device on return.
 * Errors are returned as negative codes; nothing longjmps, throws or aborts.
 */
#ifndef DPOW_H
#define DPOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: dpow_worker_result gained `error` (dpow_worker.h), DPOW_K_LIMIT = 2^55 - 1 and
 * 7-byte chunks (round 2); dpow_node_* (round 3).
 * 3 (round 4): dpow_diag_launch_geometry takes ntz (dpow_diag.h); dpow_node_release.
 * 4 (round 5): dpow_node_mine.
 * 5 (round 6): the node board, dpow_board_* (the node scheduler under the coordinator protocol).
 * The batch entry points (dpow_search_batch, dpow_batch_candidate, dpow_batch_plan,
 * dpow_batch_plan_block) were added within ABI 5: nothing older changed, and the Python binding
 * refuses a library that lacks a prototype it lists, or one built from another tree.
 * The task queue (dpow_queue_*, DPOW_EAGAIN) and dpow_worker_set_queue were added the same way,
 * and so were the scan (dpow_scan, dpow_scan_slice, DPOW_MORE) and the census
 * (dpow_census_window, dpow_census_merge) and the digests (dpow_digests, dpow_digests_device,
 * dpow_digest_of_index) and the batched census (dpow_census_batch, dpow_census_plan) and the
 * batched scan (dpow_scan_batch, dpow_scan_plan, dpow_scan_plan_halve) and the device scan
 * (dpow_scan_device, dpow_scan_device_cut, DPOW_SCAN_DEVICE_MIN_HITS) and the batched device
 * scan (dpow_scan_batch_device, dpow_scan_batch_device_settle) and the digests of many nonces
 * (dpow_digests_batch, dpow_digests_batch_device, dpow_digests_batch_walk).
 * A consumer built against another version must refuse the library before any
 * other call (distpow/_lib.py check_abi, tests/c/abi_harness.c). */
#define DPOW_ABI_VERSION 5

/* "no hit" sentinel for global indices: INT64_MAX, so that signed (RCCL/gloo
 * int64 MIN) and unsigned (device atomicMin u64) reductions agree. */
#define DPOW_NO_HIT 0x7FFFFFFFFFFFFFFFull

/* Longest secret the search can return: 1 thread byte + 7 chunk bytes
 * (k < DPOW_K_LIMIT).  Buffers are sized 16 for headroom. */
#define DPOW_MAX_SECRET 16

/* k (the number of nextChunk applications, worker.go:234-244/399) is limited to
 * k < DPOW_K_LIMIT = 2^55 - 1: chunks of at most 7 bytes, and every global index
 * k * 256 + threadByte stays below DPOW_NO_HIT (about 2^63 candidates: decades of
 * a GPU node, so the reference's unbounded loop is never cut short in practice). */
#define DPOW_K_LIMIT ((1ull << 55) - 1)

/* dpow_search return codes */
#define DPOW_EXHAUSTED 0   /* window searched, no hit (the reference keeps looping) */
#define DPOW_FOUND 1       /* hit; *best_global_idx / secret filled, MD5 re-verified on host */
#define DPOW_CANCELLED 2   /* the cancel flag was raised (Found/Cancel RPC, worker.go:194,209) */
#define DPOW_EINVAL (-1)   /* bad argument */
#define DPOW_EHIP (-2)     /* HIP runtime error (see dpow_last_error) */
#define DPOW_EVERIFY (-3)  /* kernel hit failed host MD5 re-verification (never expected) */
#define DPOW_ERANGE (-4)   /* k window beyond DPOW_K_LIMIT */
#define DPOW_ENOMEM (-5)

typedef struct dpow_ctx dpow_ctx;

/* ---------------------------------------------------------------------------
 * Context: one per GPU.  Owns persistent device buffers (control block), the
 * HIP stream the kernels run on, and a pinned host-coherent cancel flag.
 * Replaces the per-task setup of worker.go:301-316 (buffers + threadBytes).
 * ------------------------------------------------------------------------- */
int dpow_open(int device, dpow_ctx **out);
void dpow_close(dpow_ctx *ctx);

/* Pinned, host-coherent cancel flag polled by the running kernel.  Writing a
 * non-zero value stops the search mid-launch (dpow_search returns
 * DPOW_CANCELLED).  Replaces the per-candidate `select` on killChan
 * (worker.go:320-345) and the writes at worker.go:194 (Cancel) / 209 (Found).
 * The caller clears it (writes 0) before the next task. */
volatile uint32_t *dpow_cancel_flag(dpow_ctx *ctx);

/* ---------------------------------------------------------------------------
 * The hot path.  Replaces worker.go:301-400 (the miner's enumeration loop).
 *
 * Searches the worker partition (worker_byte, worker_bits) -- threadBytes
 * uint8((worker_byte << R_bits) | t), R_bits = 8 - worker_bits % 9
 * (worker.go:302-316) -- over chunks k in [k_begin, k_end) (chunk_k = the
 * minimal little-endian bytes of k, i.e. nextChunk applied k times), in the
 * reference's order (k outer, t inner), for the first candidate whose
 * hex(MD5(nonce || threadByte || chunk_k)) ends in `ntz` '0' characters
 * (worker.go:353-356, hasNumZeroesSuffix worker.go:246-256).
 *
 * best_global_idx (in/out): on input an upper bound (DPOW_NO_HIT = none); only
 * hits with global index below it are reported.  Global index
 * g = k * 256 + threadByte; it is monotone in the worker's local order, so the
 * minimum over partitions equals the worker_bits = 0 answer.
 * On DPOW_FOUND, secret_out[0..*secret_len) = threadByte || chunk_k (the
 * `Secret` of WorkerResult, worker.go:357-362), recomputed and verified with
 * a host MD5 before returning.
 * ------------------------------------------------------------------------- */
int dpow_search(dpow_ctx *ctx, const uint8_t *nonce, size_t nonce_len, uint32_t ntz,
                uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin, uint64_t k_end,
                uint64_t *best_global_idx, uint8_t secret_out[DPOW_MAX_SECRET],
                size_t *secret_len);

/* Lower the bound of the search running on ctx, from any thread: candidates at
 * or above global_idx are no longer wanted (another partition -- another GPU of
 * the node -- has a hit there).  The running kernel stops claiming work at or
 * above it within one group of wave-blocks, and dpow_search returns
 * DPOW_EXHAUSTED unless it finds a hit below the bound (then DPOW_FOUND with
 * that hit).  Used by the multi-GPU node (distpow.node.node_mine_async) to stop
 * every rank at the node's best hit without waiting for batch boundaries; the
 * reference has no counterpart (its coordinator's Found fan-out,
 * coordinator.go:210-230, cancels instead).  No effect when no search runs.
 * Returns 0 or a negative error code. */
int dpow_search_bound(dpow_ctx *ctx, uint64_t global_idx);

/* ---------------------------------------------------------------------------
 * Batched search (added within ABI 5): B independent tasks in one pass over the GPU.
 *
 * The reference coordinator takes any number of concurrent Mine requests
 * (coordinator.go:139-199); a caller holding B small tasks (a node scheduler, a
 * worker, a benchmarking client) pays the launch and completion round trip once
 * per round here instead of once per task.  Each task is a dpow_search argument
 * tuple and gets the answer dpow_search gives for it on an idle context: the first
 * hit below its bound in the reference's order (worker.go:318-400), re-verified
 * with the host MD5 before DPOW_FOUND is written.  Tasks are independent (a task's
 * result does not depend on the others of its batch; duplicates are legal).
 *
 * One generic kernel (csrc/md5_batch.hip) hashes the tasks in rounds: round r
 * covers the next slice of every undecided task's window, slices growing 4x per
 * round up to a cap of a few milliseconds of hashing.
 *
 * Returns 0, or a negative code with no task written: DPOW_EINVAL for a NULL
 * pointer, n_tasks of 0 or above DPOW_BATCH_MAX, k_begin > k_end, worker_byte >
 * 255, a nonce longer than DPOW_MAX_NONCE (dpow_worker.h) or a context with a
 * node slot attached; DPOW_ERANGE for k_end > DPOW_K_LIMIT; all of these before any
 * GPU work.  The context's cancel flag ends the call: undecided tasks get
 * DPOW_CANCELLED, decided ones keep their answer; a flag raised on entry cancels
 * every task without a launch.  dpow_search_bound has no effect on a batch, and a
 * batch does not touch dpow_stats: its counts go to *stats.  One batch or search
 * is in flight per context.
 * ------------------------------------------------------------------------- */
#define DPOW_BATCH_MAX 4096
typedef struct dpow_batch_task {
    const uint8_t *nonce;         /* in */
    size_t nonce_len;             /* in */
    uint32_t ntz, worker_byte, worker_bits;  /* in */
    uint64_t k_begin, k_end;      /* in */
    uint64_t best_global_idx;     /* in: bound (DPOW_NO_HIT = none); out: the hit */
    int32_t status;               /* out: DPOW_FOUND / DPOW_EXHAUSTED / DPOW_CANCELLED */
    uint32_t secret_len;          /* out on DPOW_FOUND */
    uint8_t secret[DPOW_MAX_SECRET];
} dpow_batch_task;
typedef struct dpow_batch_stats {
    uint32_t launches, rounds;    /* kernel launches; rounds of the schedule (one launch each) */
    uint64_t candidates;          /* candidates covered by the launches' slices */
    double kernel_ms;             /* sum of the launches' durations, as they stamp them */
} dpow_batch_stats;
int dpow_search_batch(dpow_ctx *ctx, dpow_batch_task *tasks, size_t n_tasks, dpow_batch_stats *stats);

/* ---------------------------------------------------------------------------
 * Scan (added within ABI 5): every hit of a window in one pass.
 *
 * Every search above answers "the first hit of a window".  dpow_scan reports every candidate
 * of partition (worker_byte, worker_bits) over k in [k_begin, k_end) whose digest ends in at
 * least ntz '0' characters, in increasing global index -- the reference's order, so dpow_search
 * started at a hit's k returns that hit -- each with its depth.  It is what a cache that keeps a
 * nonce's dominant secret (more zeros, else the greater bytes: worker.go's cache rule), a
 * difficulty calibration or an audit asks.  Every entry is recomputed with the host MD5 before it
 * is written (tz is the host's value; the device reports indices only); a device entry that fails
 * verification is DPOW_EVERIFY.
 *
 * One generic kernel (csrc/md5_scan.hip) appends the hits of one bounded launch per slice of the
 * window to a list.
 *
 * Returns DPOW_EXHAUSTED (0): the window is done, *k_done = k_end.  DPOW_MORE: `out` could not
 * take the next k's hits; out[0..*n_hits) holds all hits of [k_begin, *k_done) and the caller
 * continues with k_begin = *k_done.  A k's hits are never split over two calls, and max_hits
 * < 256 is DPOW_EINVAL, so one k (at most 256 candidates) always fits and every call makes
 * progress.  DPOW_CANCELLED: the context's cancel flag is raised (checked on entry, where it
 * costs no launch, and between launches); the hits of [k_begin, *k_done) are complete.
 * The argument errors are those of dpow_search_batch, returned before any GPU work: DPOW_EINVAL
 * for a NULL pointer (stats may be NULL), worker_byte > 255, k_begin > k_end, a nonce longer than
 * DPOW_MAX_NONCE or a context with a node slot attached; DPOW_ERANGE for k_end > DPOW_K_LIMIT.
 * ntz = 0 is legal and makes every candidate a hit; ntz > 32 scans and finds nothing; an empty
 * window is DPOW_EXHAUSTED without a launch.  One scan, search or batch is in flight per
 * context.  dpow_search_bound has no effect on a scan, and a scan does not touch dpow_stats:
 * its counts go to *stats.
 * ------------------------------------------------------------------------- */
#define DPOW_MORE 3            /* dpow_scan: `out` is full; call again from *k_done */
typedef struct dpow_scan_hit {
    uint64_t global_idx;       /* k * 256 + threadByte */
    uint32_t tz;               /* trailing '0' characters of its digest (>= ntz), from the host MD5 */
    uint32_t secret_len;
    uint8_t secret[DPOW_MAX_SECRET];
} dpow_scan_hit;
int dpow_scan(dpow_ctx *ctx, const uint8_t *nonce, size_t nonce_len, uint32_t ntz,
              uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin, uint64_t k_end,
              dpow_scan_hit *out, size_t max_hits, size_t *n_hits, uint64_t *k_done,
              dpow_batch_stats *stats /* may be NULL */);
/* (dpow_scan_slice, the scan's slice rule, is with the host helpers below.) */

/* ---------------------------------------------------------------------------
 * Batched scan (added within ABI 5): every hit of many windows in one pass.
 *
 * A scan of a small window is a launch and a host round trip, not hashing, as a small search or
 * census is (dpow_search_batch, dpow_census_batch): a caller that wants the hit lists of B
 * windows -- a cache refreshing its dominant secrets, a difficulty calibration over fresh nonces,
 * an audit of what a batch returned -- pays them once per launch here instead of once per task.
 * Each task is a dpow_scan argument tuple, and its hits are exactly what dpow_scan writes for it on
 * an idle context: every candidate of its partition over [k_begin, k_done) with depth >= its ntz,
 * in increasing global index, tz and secret from the host MD5.  Tasks are independent; duplicates
 * are legal and each gets its own copy; ntz = 0 makes every candidate a hit and ntz > 32 finds
 * nothing.
 *
 * One generic kernel (csrc/md5_scan_many.hip) hashes the tasks in array order, one bounded launch
 * per 2^28 local indices or a quarter of its hit list's worth of expected hits, whichever is less,
 * of the tasks taken together: a launch holds as many whole tasks as fit and at most one task cut
 * at its end (dpow_scan_plan below).  The hits go to `out`, each task's
 * contiguous and the tasks' in array order: task i's are out[first_hit .. first_hit + n_hits),
 * and *n_out is the total.
 *
 * Returns 0 with every task's status set, or a negative code with no task and nothing of `out`
 * written: dpow_census_batch's argument errors, and DPOW_EINVAL for max_hits < 256 or a NULL `out`
 * or `n_out`; all of these before any GPU work (stats may be NULL); DPOW_EVERIFY for a device
 * entry that fails the host's checks.  On 0 a finished task is DPOW_EXHAUSTED with k_done = k_end;
 * a task with k_begin == k_end is DPOW_EXHAUSTED without GPU work whenever the call gets past its
 * entry check, and a call whose tasks are all empty makes no launch and allocates nothing.
 * Paging: when `out` cannot take the next whole k of the task being written the call stops; that
 * task is DPOW_MORE with k_done at that k and the complete hits of [k_begin, k_done), every task
 * after it is DPOW_MORE with k_done = k_begin and no hits, and the caller submits the unfinished
 * tasks again from their k_done.  A k's hits are never split, and max_hits >= 256 lets the first
 * unfinished task make progress in every call.  The context's cancel flag is checked on entry and
 * between launches.  Raised on entry: every task is DPOW_CANCELLED with k_done = k_begin, without
 * a launch.  Raised between launches: the tasks finished by then are DPOW_EXHAUSTED, the task a
 * launch boundary cut is DPOW_CANCELLED at a whole k with its hits so far complete, the tasks not
 * begun are DPOW_CANCELLED with k_done = k_begin.  One search, batch, scan, census or digest call
 * is in flight per context.  dpow_search_bound has no effect on the call, and it does not touch
 * dpow_stats: its counts go to *stats as dpow_census_batch's do (an overflowed launch, which is
 * discarded and re-planned, counts as well).
 * ------------------------------------------------------------------------- */
typedef struct dpow_scan_task {
    const uint8_t *nonce; size_t nonce_len;        /* in */
    uint32_t ntz, worker_byte, worker_bits;        /* in */
    uint64_t k_begin, k_end;                       /* in */
    uint64_t k_done;                               /* out */
    int32_t  status;                               /* out: DPOW_EXHAUSTED / DPOW_MORE / DPOW_CANCELLED */
    uint64_t first_hit, n_hits;                    /* out: out[first_hit .. first_hit + n_hits) */
} dpow_scan_task;
int dpow_scan_batch(dpow_ctx *ctx, dpow_scan_task *tasks, size_t n_tasks,
                    dpow_scan_hit *out, size_t max_hits, size_t *n_out,
                    dpow_batch_stats *stats /* may be NULL */);
/* (dpow_scan_plan, the call's launch planner, is with the host helpers below.) */

/* ---------------------------------------------------------------------------
 * Device scan (added within ABI 5): a window's hits in index order, left in device memory.
 *
 * dpow_scan's kernel appends hits in no order and its host sorts, re-hashes and copies every one,
 * so a dense scan is host work (DESIGN.md sections 13 and 17).  dpow_scan_device answers the same
 * question into caller-owned device memory: d_idx_out receives the global indices of the window's
 * hits as uint64, in increasing order, and d_tz_out (may be NULL) the depth byte of each.  A
 * caller goes on with dpow_digests_device, or with its own kernels, without the hits crossing to
 * the host; the secret of an index is dpow_secret_from_index's.
 *
 * The order comes from the kernel's geometry, not from a sort (csrc/md5_scan_dev.hip, DESIGN.md
 * section 18): one launch writes a slice's hit bitmap and per-workgroup hit totals, a second turns
 * bitmap and prefix into the list, and the digest kernel (csrc/md5_digest.hip) computes the depths
 * of the entries placed, which re-checks every verdict.  A slice is 2^28 candidates whatever ntz;
 * the host reads one total per slice and no hit.  A last launch counts, over the whole list, the
 * entries shallower than ntz or not above their predecessor, and the host recomputes 16 sampled
 * entries with its own MD5: DPOW_EVERIFY if either fails.
 *
 * Returns DPOW_EXHAUSTED (0): the window is done, *k_done = k_end.  DPOW_MORE: the list is as full
 * as whole workgroups' hits allow; it holds every hit of [k_begin, *k_done), and the caller goes on
 * from *k_done.  A k's hits are never split, and a call that starts at k_begin always advances:
 * a workgroup's range holds at most DPOW_SCAN_DEVICE_MIN_HITS hits, which is why max_hits below
 * that is DPOW_EINVAL.  DPOW_CANCELLED: the context's cancel flag is raised (checked on entry,
 * where it costs no launch, and between slices); the list holds every hit of [k_begin, *k_done).
 * Argument errors are dpow_scan's, returned before any GPU work, plus DPOW_EINVAL for a NULL
 * d_idx_out or one that is not 8-byte aligned; a context with a node slot attached is refused.
 * ntz = 0 lists every candidate; ntz > 32 scans and lists none; an empty window is DPOW_EXHAUSTED
 * without a launch.  The function returns after the context's stream has drained, so the outputs
 * are complete on return.  It does not touch dpow_stats: stats->rounds = the slices (mask
 * launches), stats->launches = every kernel launch of the call, stats->kernel_ms their durations.
 * ------------------------------------------------------------------------- */
#define DPOW_SCAN_DEVICE_MIN_HITS 16384
int dpow_scan_device(dpow_ctx *ctx, const uint8_t *nonce, size_t nonce_len, uint32_t ntz,
                     uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin, uint64_t k_end,
                     void *d_idx_out /* max_hits uint64, 8-byte aligned */,
                     void *d_tz_out  /* max_hits bytes, or NULL */,
                     size_t max_hits, size_t *n_hits, uint64_t *k_done,
                     dpow_batch_stats *stats /* may be NULL */);
/* (dpow_scan_device_cut, the call's cut of a slice, is with the host helpers below.) */

/* ---------------------------------------------------------------------------
 * Batched device scan (added within ABI 5): the hits of many windows left in device memory, in
 * CSR order.
 *
 * dpow_scan_batch's task array in, dpow_scan_device's output form out.  Each task is a
 * dpow_scan_task as dpow_scan_batch takes it, and the tasks are worked in array order.  Task i's
 * hits are d_idx_out[first_hit .. first_hit + n_hits): uint64 global indices in strictly increasing
 * order, exactly the indices dpow_scan_device writes for that task on an idle context; d_tz_out (may
 * be NULL) holds the depth byte of each.  The tasks' segments are contiguous and in array order and
 * *n_out is the total.  d_row_out (may be NULL: a context-owned array serves) receives the n_tasks
 * + 1 row pointers: d_row_out[i] is task i's first_hit and d_row_out[n_tasks] is *n_out; the array
 * does not descend, and an empty task, or one not begun, has the row of the next one.  The task
 * structs' first_hit and n_hits come from the same array, copied out once per call: the host's work
 * is O(tasks), never O(hits).
 *
 * The launches are dpow_census_batch's (2^28 local indices of the tasks taken together, whatever
 * ntz: the list has no capacity of its own), each a mask launch whose total the host reads and,
 * behind it without a wait, a rows, a place and a depth launch (csrc/md5_scan_many_dev.hip,
 * DESIGN.md section 20).  The depth launch re-checks every entry placed -- a candidate of its
 * workgroup descriptor, above its predecessor within the task, and, when depths are asked for, as
 * deep as its task's ntz by an independent hash -- and the host recomputes 16 sampled entries with
 * its own MD5 and their task's nonce: DPOW_EVERIFY if either fails.
 *
 * Returns 0 with every task's status set, or a negative code with no task written: dpow_scan_batch's
 * argument errors, and DPOW_EINVAL for a NULL d_idx_out or n_out, a d_idx_out or d_row_out that is
 * not 8-byte aligned, or max_hits < DPOW_SCAN_DEVICE_MIN_HITS; all of these before any GPU work
 * (stats may be NULL); a context with a node slot attached is refused.  On 0 a finished task is
 * DPOW_EXHAUSTED with k_done = k_end.  Paging: when the room ends the list is cut at a whole
 * workgroup descriptor, a multiple of 256 local indices from the task's begin and hence a k boundary
 * in every partition, so a k's hits are never split.  The task the cut falls in is DPOW_MORE at that k
 * with its hits so far complete, every later task is DPOW_MORE with k_done = k_begin and no hits,
 * and a cut that falls exactly on a task's first descriptor leaves the task before it
 * DPOW_EXHAUSTED.  A descriptor holds at most DPOW_SCAN_DEVICE_MIN_HITS hits, so the first
 * unfinished task advances in every call.  The cancel flag follows dpow_scan_batch: raised on entry,
 * every task is DPOW_CANCELLED with k_done = k_begin without a launch; between launches, the tasks
 * finished by then are DPOW_EXHAUSTED, the task a launch boundary cut is DPOW_CANCELLED at a whole k
 * with its hits so far complete, the tasks not begun are DPOW_CANCELLED with k_done = k_begin.
 * ntz = 0 lists every candidate and ntz > 32 none; a call whose tasks are all empty makes no launch
 * and allocates nothing, but still writes the rows.  The function returns after the context's stream
 * has drained.  It does not touch dpow_stats: stats->rounds = the mask launches, stats->launches =
 * every kernel launch of the call, stats->kernel_ms their durations.
 * ------------------------------------------------------------------------- */
int dpow_scan_batch_device(dpow_ctx *ctx, dpow_scan_task *tasks, size_t n_tasks,
                           void *d_idx_out  /* max_hits uint64, 8-byte aligned */,
                           void *d_tz_out   /* max_hits bytes, or NULL */,
                           void *d_row_out  /* n_tasks + 1 uint64, 8-byte aligned, or NULL */,
                           size_t max_hits, size_t *n_out,
                           dpow_batch_stats *stats /* may be NULL */);
/* (dpow_scan_batch_device_settle, what a launch means for the tasks, is with the host helpers below.) */

/* ---------------------------------------------------------------------------
 * Census (added within ABI 5): depth counts and per-depth first hits of a window in one pass.
 *
 * A search answers "the first hit at depth N", a scan "which candidates reach depth N".  A census
 * answers "how deep does this window go": over partition (worker_byte, worker_bits) and k in
 * [k_begin, k_end), a candidate's depth being the trailing '0' characters of its digest (0..32),
 * for every d in 0..32
 *   count_ge[d]  the number of candidates with depth >= d (count_ge[0]: the window's size);
 *   first_ge[d]  the lowest global index with depth >= d, or DPOW_NONE: what dpow_search with
 *                ntz = d returns for the window (first_ge[0]: the window's first candidate);
 *   first_tz[d]  that candidate's depth by the host MD5 (0 where first_ge[d] is DPOW_NONE);
 * and deepest, the largest d with count_ge[d] > 0: first_ge[deepest] is the deepest candidate,
 * ties going to the lowest index.  Of an empty window count_ge is all 0, first_ge all DPOW_NONE
 * and deepest 0.  It is what a cache that keeps a nonce's dominant secret, a difficulty
 * calibration, an audit or best-share mining under a hash budget asks, without an ntz chosen up
 * front and without a list: the answer is 33 counts and 33 indices whatever the density.
 *
 * One generic kernel (csrc/md5_census.hip) counts one bounded launch per 2^28 local indices of
 * the window; the host checks each launch's table, recomputes every first
 * index with the host MD5 (a failure is DPOW_EVERIFY) and folds it with dpow_census_merge's code.
 *
 * dpow_census_window returns DPOW_EXHAUSTED (0): the window is done, *k_done = k_end.
 * DPOW_CANCELLED: the context's cancel flag is raised (checked on entry, where it costs no launch
 * and leaves *k_done = k_begin, and between launches); *out is the complete census of
 * [k_begin, *k_done), and the caller continues from *k_done and merges.  The argument errors are
 * dpow_scan's, returned before any GPU work: DPOW_EINVAL for a NULL pointer (stats may be NULL),
 * worker_byte > 255, k_begin > k_end, a nonce longer than DPOW_MAX_NONCE or a context with a node
 * slot attached; DPOW_ERANGE for k_end > DPOW_K_LIMIT.  An empty window is DPOW_EXHAUSTED without
 * a launch.  One search, batch, scan or census is in flight per context.  dpow_search_bound has
 * no effect on a census, and a census does not touch dpow_stats: its counts go to *stats.
 *
 * dpow_census_merge is a pure host function (no context, no GPU): it folds into `into` the census
 * `next` of a window that lies wholly above into's.  Counts add; for each depth first_ge and
 * first_tz keep into's entry unless it is DPOW_NONE; deepest is the maximum.  Returns 0, or
 * DPOW_EINVAL with `into` unchanged when an argument is NULL or not self-consistent -- count_ge
 * does not increase with d, count_ge[d] > 0 exactly where first_ge[d] is set, the set first_ge do
 * not decrease with d, first_tz[d] >= d where set, deepest as defined above -- or when a set
 * first_ge of next is not above every set first_ge of into.
 * ------------------------------------------------------------------------- */
#define DPOW_CENSUS_DEPTHS 33
#define DPOW_NONE DPOW_NO_HIT   /* an absent index of a census */
typedef struct dpow_census {
    uint64_t count_ge[DPOW_CENSUS_DEPTHS];
    uint64_t first_ge[DPOW_CENSUS_DEPTHS];
    uint32_t first_tz[DPOW_CENSUS_DEPTHS];
    uint32_t deepest;
} dpow_census;
int dpow_census_window(dpow_ctx *ctx, const uint8_t *nonce, size_t nonce_len,
                       uint32_t worker_byte, uint32_t worker_bits,
                       uint64_t k_begin, uint64_t k_end,
                       dpow_census *out, uint64_t *k_done,
                       dpow_batch_stats *stats /* may be NULL */);
int dpow_census_merge(dpow_census *into, const dpow_census *next);

/* ---------------------------------------------------------------------------
 * Batched census (added within ABI 5): the census of many tasks in one pass.
 *
 * A census of a small window is a launch and a host round trip, not hashing, as a small search is
 * (dpow_search_batch above): a caller that wants the depth profile of B nonces -- a cache
 * refreshing its dominant secrets, a difficulty calibration over fresh nonces, an audit of what a
 * batch returned -- pays them once per launch here instead of once per task.  Each task is a
 * dpow_census_window argument tuple, and tasks[i].census is exactly what dpow_census_window writes
 * for it on an idle context, first_tz included.  Tasks are independent; duplicates are legal and
 * each gets its own full answer.
 *
 * One generic kernel (csrc/md5_census_many.hip) hashes the tasks in array order, one bounded launch
 * per 2^28 local indices of the tasks taken together: a launch holds as many whole tasks as fit and
 * at most one task cut at its end, which goes on in the next launch (DESIGN.md section 16;
 * dpow_census_plan below).  After each launch the host checks every task's table, recomputes
 * every first index with the host MD5 (a failure is DPOW_EVERIFY) and folds it as
 * dpow_census_window does.
 *
 * Returns 0, or a negative code with no task written: DPOW_EINVAL for a NULL ctx or tasks, n_tasks
 * of 0 or above DPOW_BATCH_MAX, worker_byte > 255, k_begin > k_end, a NULL nonce with a non-zero
 * nonce_len, a nonce longer than DPOW_MAX_NONCE or a context with a node slot attached; DPOW_ERANGE
 * for k_end > DPOW_K_LIMIT; all of these before any GPU work (stats may be NULL).  On 0 every task
 * has its status: DPOW_EXHAUSTED, k_done = k_end and the census of its window; a task with
 * k_begin == k_end is DPOW_EXHAUSTED with the empty census and takes no GPU work, and a call whose
 * tasks are all empty makes no launch.  The context's cancel flag is checked on entry and between
 * launches.  Raised on entry: every task is DPOW_CANCELLED with k_done = k_begin and the empty
 * census, without a launch.  Raised between launches: the tasks finished by then are
 * DPOW_EXHAUSTED; the task a launch boundary cut is DPOW_CANCELLED with k_done at the cut and the
 * complete census of [k_begin, k_done), so the caller continues from k_done and merges
 * (dpow_census_merge); the tasks not begun are DPOW_CANCELLED with k_done = k_begin and the empty
 * census (an empty task among them is DPOW_EXHAUSTED all the same).  One search, batch, scan,
 * census or digest call is in flight per context.  dpow_search_bound has no effect on the call,
 * and it does not touch dpow_stats: stats->launches = stats->rounds = its launches,
 * stats->candidates = the local indices they covered, stats->kernel_ms = their durations.
 * ------------------------------------------------------------------------- */
typedef struct dpow_census_task {
    const uint8_t *nonce; size_t nonce_len;      /* in */
    uint32_t worker_byte, worker_bits;           /* in */
    uint64_t k_begin, k_end;                     /* in */
    uint64_t k_done;                             /* out */
    int32_t status;                              /* out: DPOW_EXHAUSTED / DPOW_CANCELLED */
    dpow_census census;                          /* out: the complete census of [k_begin, k_done) */
} dpow_census_task;
int dpow_census_batch(dpow_ctx *ctx, dpow_census_task *tasks, size_t n_tasks,
                      dpow_batch_stats *stats /* may be NULL */);
/* (dpow_census_plan, the call's launch planner, is with the host helpers below.) */

/* ---------------------------------------------------------------------------
 * Digests (added within ABI 5): MD5 and depth of any listed candidates in one pass.
 *
 * Every call above walks a contiguous window and reports the candidates whose digest ends in
 * zeros.  dpow_digests takes a list of global indices of one nonce and returns what the GPU
 * computes for each: entry j of digest_out is the 16-byte MD5 of
 * nonce || dpow_secret_from_index(global_idx[j]) and entry j of tz_out its depth, the trailing '0'
 * characters of its hex form (0..32).  A global index fixes the secret, so there is no partition
 * argument.  The list may be in any order and duplicates are legal; outputs are positional; either
 * output may be NULL, not both.  It is what a pool checking the shares a scan produced, a cache
 * audit, or a client re-checking a census's first_ge asks, instead of one host MD5 per entry.
 *
 * One generic kernel (csrc/md5_digest.hip) hashes the list in chunks of 2^18 entries, one launch
 * each, staged through two buffer sets so that chunk i + 1's indices move while chunk i hashes
 * (DESIGN.md section 15); device memory does not grow with n.
 *
 * Verification is sampled: re-hashing every entry on the host would cost what the call saves.  Of
 * each chunk the host recomputes the first entry, the last entry and 14 evenly spaced ones
 * (dpow_digest_of_index) and compares every output asked for; a mismatch is DPOW_EVERIFY.  A
 * caller that needs every entry host-verified calls dpow_digest_of_index itself.
 *
 * Returns DPOW_EXHAUSTED (0): the list is done, *n_done = n.  DPOW_CANCELLED: the context's cancel
 * flag is raised (checked on entry, where it costs no launch, and between chunks); entries
 * [0, *n_done) of the outputs are complete.  Argument errors are returned before any GPU work
 * with the outputs untouched: DPOW_EINVAL for a NULL ctx, global_idx or n_done (stats may be
 * NULL), both outputs NULL, a NULL nonce with a non-zero nonce_len, a nonce longer than
 * DPOW_MAX_NONCE or a context with a node slot attached; DPOW_ERANGE for any entry g with
 * (g >> 8) >= DPOW_K_LIMIT.  n = 0 returns 0 without a launch.  One search, batch, scan, census
 * or digest call is in flight per context.  The call does not touch dpow_stats: stats->candidates
 * = the entries done, stats->launches = the chunks, stats->kernel_ms = the launches' durations.
 *
 * dpow_digests_device is the same kernel on lists already in device memory: d_global_idx holds n
 * uint64 (8-byte aligned), d_digest_out 16 n bytes (16-byte aligned), d_tz_out n bytes; either
 * output may be NULL, not both.  The caller guarantees the inputs are ready (the work that
 * produced them has completed); the function returns after the context's stream has drained, so
 * the outputs are complete on return.  It cannot pre-check the list: the kernel writes the depth
 * byte 0xFF and a zero digest for an entry with (g >> 8) >= DPOW_K_LIMIT and counts such entries
 * in a device word, and the function returns DPOW_ERANGE if that count is not zero -- the valid
 * entries are written all the same.  It verifies nothing, because the data never reaches the
 * host, and it does not look at the cancel flag (one bounded launch per 2^24 entries).  The other
 * argument errors are dpow_digests', plus DPOW_EINVAL for a misaligned pointer.
 *
 * dpow_digest_of_index is the pure host counterpart (no context, no GPU): dpow_secret_from_index
 * plus the host MD5.  Either output may be NULL, not both (DPOW_EINVAL); DPOW_EINVAL for a NULL
 * nonce with a non-zero nonce_len, DPOW_ERANGE for (global_idx >> 8) >= DPOW_K_LIMIT.
 * ------------------------------------------------------------------------- */
int dpow_digests(dpow_ctx *ctx, const uint8_t *nonce, size_t nonce_len,
                 const uint64_t *global_idx, size_t n,
                 uint8_t *digest_out /* 16 n bytes, may be NULL */,
                 uint8_t *tz_out     /* n bytes, may be NULL */,
                 size_t *n_done, dpow_batch_stats *stats /* may be NULL */);
int dpow_digests_device(dpow_ctx *ctx, const uint8_t *nonce, size_t nonce_len,
                        const void *d_global_idx, size_t n,
                        void *d_digest_out, void *d_tz_out,
                        dpow_batch_stats *stats /* may be NULL */);
int dpow_digest_of_index(const uint8_t *nonce, size_t nonce_len, uint64_t global_idx,
                         uint8_t digest_out[16], uint32_t *tz_out);   /* pure host */

/* ---------------------------------------------------------------------------
 * Digests of many nonces (added within ABI 5): dpow_digests for a list that mixes nonces.
 *
 * The list is in CSR order, as dpow_scan_batch_device leaves its hits: entry e with
 * rows[i] <= e < rows[i + 1] is a global index of tasks[i].nonce, and its outputs are exactly what
 * dpow_digests writes for (tasks[i].nonce, global_idx[e]), 16 bytes and a depth byte at position
 * e.  Empty tasks are legal anywhere.  Both outputs may be NULL, unlike dpow_digests: the call is
 * then a pure check that moves 8 bytes per entry in and returns, per task, n_shallow -- how many of
 * its entries done by the call have a depth below the task's ntz (0: none can).  One generic kernel
 * (csrc/md5_digest_many.hip) finds each entry's task on the device; DESIGN.md section 21.
 *
 * dpow_digests_batch returns, before any GPU work, DPOW_EINVAL for a NULL tasks, rows, global_idx
 * or n_done, n_tasks of 0 or above DPOW_BATCH_MAX, a NULL nonce with a non-zero nonce_len, a nonce
 * longer than DPOW_MAX_NONCE, rows[0] != 0 or a descending row, DPOW_ERANGE for an entry with
 * (g >> 8) >= DPOW_K_LIMIT -- these need no context -- and DPOW_EINVAL for a NULL ctx or a context
 * with a node slot attached; nothing is written then.  Otherwise it sets every n_entries, and works
 * the list in dpow_digests' chunks and staging (DPOW_DIAG_DIGEST_CHUNK, DPOW_DIAG_DIGEST_STAGING).
 * The cancel flag is checked on entry and between chunks: DPOW_CANCELLED with *n_done entries
 * complete and n_shallow covering those; DPOW_EXHAUSTED with *n_done = rows[n_tasks] otherwise.  Per
 * chunk the host recomputes 16 samples, each with its own task's nonce, and compares every output
 * asked for; a mismatch is DPOW_EVERIFY.
 *
 * dpow_digests_batch_device is the same kernel on lists already in device memory: d_rows holds
 * n_tasks + 1 uint64 (8-byte aligned), which the host does not read before the launches; n is the
 * caller's count of entries in d_global_idx (8-byte aligned), d_digest_out (16-byte aligned) and
 * d_tz_out, either or both of which may be NULL.  It makes one bounded launch per 2^24 entries
 * and drains the stream once; behind the last launch it copies out the rows (n_entries), the
 * shallow counts and two count words.  An entry outside [rows[0], rows[n_tasks]) gets the depth
 * byte 0xFF and a zero digest, and the call returns DPOW_EINVAL; an entry beyond DPOW_K_LIMIT
 * likewise, and the call returns DPOW_ERANGE; the other entries are written all the same.  It
 * verifies nothing on the host and does not look at the cancel flag.  Rows that descend cost wrong
 * outputs, never an access outside the arrays as described.  DPOW_EINVAL up front for a NULL
 * tasks, d_rows or d_global_idx, a misaligned pointer, a bad n_tasks or nonce, a NULL ctx or an
 * attached node slot.
 *
 * One search, batch, scan, census or digest call is in flight per context.
 * ------------------------------------------------------------------------- */
typedef struct dpow_digest_task {
    const uint8_t *nonce; size_t nonce_len;   /* in */
    uint32_t ntz;                             /* in: the depth this task's entries are held against (0: none) */
    uint64_t n_entries;                       /* out: rows[i + 1] - rows[i] */
    uint64_t n_shallow;                       /* out: entries of the task done by this call with depth < ntz */
} dpow_digest_task;

int dpow_digests_batch(dpow_ctx *ctx, dpow_digest_task *tasks, size_t n_tasks,
                       const uint64_t *rows /* n_tasks + 1 */, const uint64_t *global_idx /* rows[n_tasks] */,
                       uint8_t *digest_out /* 16 per entry, may be NULL */, uint8_t *tz_out /* may be NULL */,
                       size_t *n_done, dpow_batch_stats *stats /* may be NULL */);
int dpow_digests_batch_device(dpow_ctx *ctx, dpow_digest_task *tasks, size_t n_tasks,
                              const void *d_rows /* n_tasks + 1 uint64 in device memory */,
                              const void *d_global_idx, size_t n,
                              void *d_digest_out, void *d_tz_out,
                              dpow_batch_stats *stats /* may be NULL */);
/* (dpow_digests_batch_walk, a wave's passes over the rows, is with the host helpers below.) */

/* ---------------------------------------------------------------------------
 * Task queue (added within ABI 5): the batched search as a service on one GPU.
 *
 * dpow_search_batch wants its tasks at once and returns when the slowest is decided; the
 * reference's Mine requests arrive one at a time, each wants its answer as soon as it exists,
 * and each is killed on its own (worker.go:169-232).  A queue takes tasks one by one from any
 * thread while its pump thread keeps launching the generic kernel over whatever is live: a
 * task is a dpow_search argument tuple and gets the answer dpow_search gives for it (the first
 * hit below its bound in the reference's order, re-verified with the host MD5), as soon as the
 * launch that decides it has retired.  One launch is in flight per queue and every launch is
 * bounded; how a launch is shared among tasks of different ages is DESIGN.md section 12
 * (dpow_queue_plan below).  An idle queue issues no GPU work and does not poll.
 *
 * A queue owns a private context on its device, DPOW_BATCH_MAX task slots and its pump thread.
 * Every entry point may be called from any thread between open and close; close is called
 * once, with no other call in flight.
 * ------------------------------------------------------------------------- */
#define DPOW_EAGAIN (-8)   /* dpow_queue_submit: DPOW_BATCH_MAX tickets are out; nothing queued */
typedef struct dpow_queue dpow_queue;
typedef struct dpow_queue_result {
    uint64_t ticket, user;        /* ticket: never 0, never reused in a queue's life */
    int32_t status;               /* DPOW_FOUND / EXHAUSTED / CANCELLED, or a negative code */
    uint32_t secret_len;
    uint64_t global_idx;          /* on DPOW_FOUND */
    uint8_t secret[DPOW_MAX_SECRET];
    uint32_t launches;            /* launches the task took part in */
    uint32_t pad;
    double queued_ms;             /* submit to decided, on the host clock */
} dpow_queue_result;

/* DPOW_EINVAL for out = NULL or a bad ordinal, DPOW_EHIP without a visible device (as dpow_open). */
int dpow_queue_open(int device, dpow_queue **out);
/* Cancels what is undecided, lets the launch in flight retire, joins the pump, closes the context. */
void dpow_queue_close(dpow_queue *q);
/* Queue one task (the nonce is copied) and return its ticket.  The argument errors of
 * dpow_search_batch (DPOW_EINVAL, DPOW_ERANGE) are returned before any GPU work; DPOW_EAGAIN
 * with DPOW_BATCH_MAX tickets out (tasks undecided, or decided and not yet collected: collecting
 * one makes room); the queue's failure code once a launch has failed.  A
 * window that is empty or starts at or above `bound` is DPOW_EXHAUSTED without a launch. */
int dpow_queue_submit(dpow_queue *q, const uint8_t *nonce, size_t nonce_len, uint32_t ntz,
                      uint32_t worker_byte, uint32_t worker_bits, uint64_t k_begin, uint64_t k_end,
                      uint64_t bound, uint64_t user, uint64_t *ticket);
/* 1: the task was undecided and is DPOW_CANCELLED now -- its result is available at once, before
 * the launch in flight ends, and wins over a hit that launch may still find (worker.go:320-342);
 * 0: it was decided already (its result stands) or the ticket is unknown. */
int dpow_queue_cancel(dpow_queue *q, uint64_t ticket);
/* Collect a result: dpow_queue_next any decided task, in the order they were decided;
 * dpow_queue_wait the given one.  1 with *out filled, 0 on time-out (timeout_ms < 0 blocks), or a
 * negative code (DPOW_EINVAL: a NULL argument, or a ticket that is neither undecided nor waiting to
 * be collected; the queue's failure code when it has failed and nothing is left to collect).
 * Each result is handed out exactly once, to whichever of the two asks first.  After a failed
 * launch (a HIP error, DPOW_EVERIFY, a stream idle without its record) every undecided task's
 * result carries that negative code as its status; nothing is retried. */
int dpow_queue_next(dpow_queue *q, dpow_queue_result *out, int timeout_ms);
int dpow_queue_wait(dpow_queue *q, uint64_t ticket, dpow_queue_result *out, int timeout_ms);
/* Totals since open (launches = rounds; candidates of the launches' slices; kernel ms from the
 * records' ticks), tasks undecided, results not yet collected.  Any pointer may be NULL. */
int dpow_queue_stats(dpow_queue *q, dpow_batch_stats *out, uint32_t *live, uint32_t *uncollected);
/* (dpow_queue_plan, the queue's launch planner, is with the host helpers below.) */

/* ---------------------------------------------------------------------------
 * Node slot (round 3): the Found fan-out of one node's ranks, in shared memory.
 *
 * The reference coordinator fans Found out to every worker once the first
 * result arrives (coordinator.go:210-230).  Here the G GPUs of one node search
 * the prefix partitions of the same k-window, one process each, and share a
 * dpow_node_slot (e.g. a POSIX shared-memory page mapped by every rank).  A
 * search on a context attached to a slot
 *   - takes the slot's best as a bound from its start and whenever it drops
 *     while the search waits for its launches (as dpow_search_bound), so every
 *     rank stops at the node's lowest hit without waiting for a batch boundary;
 *   - posts its own verified hit to the slot (atomic min) before it returns
 *     DPOW_FOUND;
 *   - returns DPOW_CANCELLED when the slot's stop is raised, and raises it when
 *     it returns DPOW_CANCELLED or an error itself, so a cancelled or failed rank
 *     ends the node's search on every GPU at once.
 * The node's answer is still the minimum over the ranks' results, taken once per
 * batch (distpow.node.node_mine): through dpow_node_vote below when every rank
 * shares the host, else one RCCL MIN all-reduce.  It equals the workerBits = 0
 * first hit.
 * ------------------------------------------------------------------------- */
typedef struct dpow_node_slot {
    uint64_t best;     /* lowest verified hit of any rank; DPOW_NO_HIT = none */
    uint32_t stop;     /* non-zero: every attached search ends (DPOW_CANCELLED) */
    uint32_t pad[13];  /* one 64-byte line per slot */
} dpow_node_slot;
/* Attach a slot to ctx for its next searches (NULL detaches).  Not thread-safe
 * against a running search on ctx.  The slot's host page is registered with HIP once
 * per process and stays registered while any context that attached it is open, so
 * detaching and re-attaching costs nothing and several contexts may share a slot. */
int dpow_node_attach(dpow_ctx *ctx, dpow_node_slot *slot);
/* Memory holding slots is about to be unmapped or freed: waits for the launches of every
 * context that attached a slot in [mem, mem + len), then drops the library's HIP
 * registration of those pages (so a later mapping at the same address is registered
 * afresh).  DPOW_EINVAL if a context is still attached to a slot there (ABI 3).
 * Mandatory before any memory that held an attached slot is unmapped or freed, whoever
 * owns it (a shared mapping, a heap buffer, a Go or Python array): the library keys its
 * registrations on the page address, so a later slot at the same address would otherwise
 * be matched to the old registration and its stale device alias. */
int dpow_node_release(void *mem, size_t len);
/* best = DPOW_NO_HIT, stop = 0 (before the node's search that uses the slot). */
void dpow_node_slot_reset(dpow_node_slot *slot);
/* Atomic min of a verified hit into the slot. */
void dpow_node_post(dpow_node_slot *slot, uint64_t global_idx);
/* Raise the slot's stop. */
void dpow_node_stop(dpow_node_slot *slot);

/* Node vote (round 3): node_mine's batch boundary among the G ranks of one host, through
 * the same shared memory instead of a collective -- MIN over the ranks of three int64
 * values ([best index, running, healthy]); every rank gets the same result.  `votes` is
 * an array of world * 2 dpow_node_vote_entry (zeroed before the first vote), shared by the
 * ranks; each rank votes once per boundary with the same increasing epoch (1, 2, ...),
 * into entry [rank][epoch % 2] (a rank is at most one boundary ahead of the slowest),
 * then waits for every rank's entry of that epoch.  An RCCL all-reduce of the same 24
 * bytes costs 33 us at world 1 on an MI355X (tests/test_gpu_rccl.py); this costs the
 * slowest rank's arrival plus a cache-line transfer.  Returns 0, or DPOW_EPROTO (dpow_worker.h) when some
 * rank's vote has not arrived within timeout_ns (a dead rank; the node's search is lost). */
typedef struct dpow_node_vote_entry {
    uint64_t epoch;
    int64_t v[3];
    uint64_t pad[4];   /* one 64-byte line per entry */
} dpow_node_vote_entry;
int dpow_node_vote(dpow_node_vote_entry *votes, uint32_t rank, uint32_t world, uint64_t epoch,
                   const int64_t in[3], int64_t out[3], int64_t timeout_ns);

/* One node search of this rank, natively (ABI 4): distpow.node.node_mine's batch loop over a
 * shared board, without a Python round per batch -- what a Go node scheduler would call.
 * Rank `rank` of `world` (a power of two <= 256) searches its partition (worker_byte = rank,
 * worker_bits = log2 world; coordinator.go:127,326) window by window from k_begin: the first
 * window first_k chunks (0: batch_k), every later one batch_k, up to k_limit.  The context is
 * attached to `slot` for the call (the Found fan-out, dpow_node_attach) and detached after it.
 * Each window ends in the node vote through `votes` (dpow_node_vote, epoch advanced from
 * *epoch, which the caller keeps across calls), a MIN of [the lower of its own hit and the
 * slot's posted best, running, healthy]; votes = NULL takes this rank's values alone (one rank,
 * or the one-GPU emulation of tools/node_probe.py).  Returns DPOW_FOUND with *best_global_idx =
 * the node's first hit (the workerBits = 0 answer) and its secret (this rank's verified bytes,
 * or dpow_secret_from_index of another rank's hit), DPOW_CANCELLED when some rank was
 * cancelled (the context's cancel flag, the slot's stop), DPOW_EXHAUSTED at k_limit; this
 * rank's error code when its own search failed (it stopped the slot and voted healthy = 0),
 * DPOW_EPROTO when another rank's did or a vote timed out.  *batches = windows voted. */
int dpow_node_mine(dpow_ctx *ctx, dpow_node_slot *slot, dpow_node_vote_entry *votes, uint32_t rank,
                   uint32_t world, uint64_t *epoch, int64_t vote_timeout_ns, const uint8_t *nonce,
                   size_t nonce_len, uint32_t ntz, uint64_t k_begin, uint64_t k_limit, uint64_t first_k,
                   uint64_t batch_k, uint64_t *best_global_idx, uint8_t secret_out[DPOW_MAX_SECRET],
                   size_t *secret_len, uint32_t *batches);

/* ---------------------------------------------------------------------------
 * Node board (ABI 5): the node scheduler under the reference coordinator's unchanged protocol.
 *
 * The coordinator fans a task out to W workers, worker i searching prefix partition i
 * (coordinator.go:122-129,179-199,326), and answers with the first result to arrive
 * (coordinator.go:202).  When the W workers of a coordinator share one host (one worker per GPU
 * of the node), they open one board, and each miner runs its partition's node search there
 * (dpow_board_search): the task's entry -- keyed by (nonce, ntz, W), created by the first rank
 * to arrive -- carries its node slot and votes, and every rank gets the node's first hit, the
 * minimum global index over the partitions (the workerBits = 0 answer).  Only its owner reports
 * it; the other workers wait for their kill (worker.go:320-342).  So the coordinator's first
 * result is the deterministic answer, with the reference's messages unchanged: 2 per worker.
 *
 * Requirements: W a power of two in [2, DPOW_BOARD_MAX_WORLD]; all W workers of the
 * coordinator on this host, sharing one board; one live task per (nonce, ntz) at a time (the
 * reference's task maps, worker.go:173 and coordinator.go:175, key on the same).  A worker with
 * W = 1 or a non-power-of-two W (coordinator.go:326 floor(log2 W) leaves partitions that
 * overlap) searches alone with dpow_search, and the first result wins as in the reference.
 * ------------------------------------------------------------------------- */
#define DPOW_BOARD_MAX_WORLD 64
#define DPOW_BOARD_TASKS 64      /* tasks in flight on one board at once */
typedef struct dpow_board dpow_board;
/* name NULL: a board private to this process (workers of one process, the coordinator mirror);
 * else a POSIX shared-memory object "/name", created by the first worker process that opens it
 * (zero-filled: an empty board) and mapped by every other. */
int dpow_board_open(const char *name, dpow_board **out);
/* Unmaps the board (no search may run on it); the shared object stays (dpow_board_unlink). */
void dpow_board_close(dpow_board *b);
int dpow_board_unlink(const char *name);
/* Rank `rank` of `world` joins the task (nonce, ntz, world): its entry's slot and 2 * world vote
 * entries (zeroed by the rank that created the entry).  dpow_board_leave: the last rank out
 * frees the entry.  dpow_board_search does both; they are exposed for node schedulers that call
 * dpow_node_mine themselves, and for tests. */
int dpow_board_join(dpow_board *b, const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t world,
                    uint32_t rank, dpow_node_slot **slot, dpow_node_vote_entry **votes);
int dpow_board_leave(dpow_board *b, dpow_node_slot *slot);
/* Task entries in use (0 once every joined rank has left). */
int dpow_board_tasks(dpow_board *b);
/* Task entries created over the board's life, and of those the tasks whose W ranks all ran on one
 * GPU (dpow_board_search then searched the node's windows once, on rank 0, instead of W ways). */
int dpow_board_counters(dpow_board *b, uint64_t *tasks, uint64_t *shared_gpu);
/* One worker's search of a task on the board: replaces the miner's loop (worker.go:301-400) when
 * the node's W = 2^worker_bits workers share the board.  Joins the task's entry, runs
 * dpow_node_mine for partition worker_byte (rank = worker_byte, world = 2^worker_bits) from k = 0,
 * and leaves.  Returns DPOW_FOUND with *best_global_idx = the node's first hit and its secret;
 * *owner = 1 when the hit lies in this worker's partition (this worker sends WorkerResult),
 * 0 when another worker owns it (this worker waits for its kill, then sends the two nil
 * messages of the cancel path).  DPOW_CANCELLED when the context's cancel flag is raised (the
 * task's kill: Found or Cancel; the rank leaves at once, without waiting for the others' votes),
 * or another rank's cancel stopped the task; a negative code when a search failed or another
 * rank's did, or a vote timed out (120 s: a rank that never joined).  DPOW_EINVAL unless
 * 1 <= worker_bits <= 6 and worker_byte < 2^worker_bits.
 * A rank first waits until the task's other ranks have joined or one of them is seen on another
 * GPU (microseconds: the Mine fan-out's skew).  When all W ranks share one GPU (more workers than
 * GPUs), rank 0 searches every partition of each window (worker_bits 0) and the others only
 * vote: the same answer, without splitting one device W ways. */
int dpow_board_search(dpow_board *b, dpow_ctx *ctx, const uint8_t *nonce, size_t nonce_len, uint32_t ntz,
                      uint32_t worker_byte, uint32_t worker_bits, uint64_t *best_global_idx,
                      uint8_t secret_out[DPOW_MAX_SECRET], size_t *secret_len, uint32_t *owner);

/* ---------------------------------------------------------------------------
 * Host helpers (no GPU needed).
 * ------------------------------------------------------------------------- */
/* Secret bytes of a global index: threadByte = g & 255, chunk = minimal LE bytes of g >> 8. */
int dpow_secret_from_index(uint64_t global_idx, uint8_t secret_out[DPOW_MAX_SECRET],
                           size_t *secret_len);
/* Host MD5 (RFC 1321) of msg -> 16-byte digest. */
void dpow_md5(const uint8_t *msg, size_t len, uint8_t digest_out[16]);
/* Number of trailing '0' characters of the 32-char hex form of a digest. */
uint32_t dpow_trailing_zero_nibbles(const uint8_t digest[16]);
/* 1 if hex(MD5(nonce || secret)) ends in >= ntz '0' characters, else 0. */
int dpow_verify(const uint8_t *nonce, size_t nonce_len, const uint8_t *secret,
                size_t secret_len, uint32_t ntz);

/* Launch plan of a window (host logic of dpow_search, exposed for testing):
 * one entry per kernel launch, as dpow_search with these arguments would queue them
 * (ntz matters: chunk lengths 1..3 share a launch only when a hit is expected early).  Returns the number of launches (may exceed
 * max_launches, in which case only the first max_launches are written), or a
 * negative error code. */
typedef struct dpow_plan_launch {
    uint64_t k_begin, k_end;   /* chunk range of this launch */
    uint64_t i_begin, i_end;   /* local index range (k * R + t) */
    uint32_t nblk;             /* final MD5 blocks computed per candidate (1 or 2) */
    uint32_t w0, sh;           /* variable bytes start at word w0, byte shift sh */
    uint32_t chunk_len;        /* L: chunk bytes of k_begin ... */
    uint32_t chunk_len_last;   /* ... and of k_end - 1 (one launch may span chunk lengths 1..3) */
    uint32_t start_kernel;     /* 1: k = 0, hashed by the search's k = 0 kernel, not an md5 launch */
} dpow_plan_launch;
int dpow_plan_window(const uint8_t *nonce, size_t nonce_len, uint32_t ntz, uint32_t worker_byte,
                     uint32_t worker_bits, uint64_t k_begin, uint64_t k_end,
                     dpow_plan_launch *out, size_t max_launches);

/* Final-block message words and chaining value the kernel hashes for local
 * index `local_idx` of a partition, assembled with the same template + lane
 * arithmetic the kernel uses.  words_out: 16 * (*nblk_out) words. */
int dpow_plan_candidate(const uint8_t *nonce, size_t nonce_len, uint32_t worker_byte,
                        uint32_t worker_bits, uint64_t local_idx, uint32_t iv_out[4],
                        uint32_t words_out[32], uint32_t *nblk_out);

/* Final-block words and chaining value the batch kernel hashes for local index `local_idx`
 * of a partition, assembled by the code the kernel itself calls (csrc/md5_batch.h
 * batch_candidate_words).  words_out: 16 * (*nblk_out) words (the rest zero). */
int dpow_batch_candidate(const uint8_t *nonce, size_t nonce_len, uint32_t worker_byte,
                         uint32_t worker_bits, uint64_t local_idx, uint32_t iv_out[4],
                         uint32_t words_out[32], uint32_t *nblk_out);

/* Round plan of a batch (host logic of dpow_search_batch, exposed for testing): the
 * launches the host loop queues for tasks with windows [k_begin[i], k_end[i]) and
 * partitions worker_bits[i] when no task hits.  One entry per (launch, live task), in
 * launch order and, within a launch, in the order of the launch's block map: the
 * slice [i_begin, i_end) of the task's local indices (k * R + t) the launch covers,
 * cut into `rows` workgroup groups of `group` local indices.  Workgroup b of a launch
 * with n live entries hashes row b / n of entry b % n (dpow_batch_plan_block).
 * Returns the number of entries (may exceed max_entries, in which case only the first
 * max_entries are written) or a negative error code; *launches_out = launches. */
typedef struct dpow_batch_range {
    uint32_t launch, task;     /* launch number (= round), task index */
    uint64_t i_begin, i_end;   /* local index slice of this launch */
    uint32_t group, rows;      /* the launch's workgroup size in local indices, rows per entry */
} dpow_batch_range;
int dpow_batch_plan(const uint64_t *k_begin, const uint64_t *k_end, const uint32_t *worker_bits,
                    size_t n_tasks, dpow_batch_range *out, size_t max_entries, uint64_t *launches_out);
/* The local index range workgroup `block` of a launch hashes, by the kernel's own block
 * map arithmetic: entries = the launch's n_live entries of dpow_batch_plan.  Returns 1
 * with *task, *lo, *hi, 0 when the workgroup has nothing to hash (its entry's slice ended
 * in an earlier row), or a negative error code. */
int dpow_batch_plan_block(const dpow_batch_range *entries, uint32_t n_live, uint32_t block,
                          uint32_t *task, uint64_t *lo, uint64_t *hi);

/* The task queue's planner for one launch (host logic of dpow_queue_*, exposed for testing;
 * DESIGN.md section 12): live task i has left[i] > 0 local indices to go and has taken part in
 * age[i] launches.  One entry per workgroup, in descriptor order (by the block's ordinal within
 * its task, then by task): task = index into the inputs, [i_begin, i_end) relative to the task's
 * current position, group = the launch's block size, rows = the task's block count, launch = 0.
 * When every task has the same age the slices and the group are those of dpow_batch_plan's round
 * of that age.  Returns the block count (may exceed max_blocks, in which case only the first
 * max_blocks are written) or a negative code (DPOW_EINVAL: a NULL argument, n_tasks of 0 or above
 * DPOW_BATCH_MAX, a left[i] of 0); *budget_out = the launch's candidate budget. */
int dpow_queue_plan(const uint64_t *left, const uint32_t *age, size_t n_tasks,
                    dpow_batch_range *out, size_t max_blocks, uint64_t *budget_out);

/* The batched census's launch planner (host logic of dpow_census_batch, exposed for testing;
 * DESIGN.md section 16) for tasks with windows [k_begin[i], k_end[i]) and partitions
 * worker_bits[i].  A launch takes tasks in array order until it holds `cap` local indices (0: the
 * call's own 2^28; else 256..2^28, rounded down to a multiple of 256); only its last task can be
 * cut, at a multiple of 256 local indices from the task's begin, and goes on in the next launch.
 * One entry per workgroup descriptor, in launch order and within a launch in task order: launch =
 * the launch number, task = the task index, [i_begin, i_end) the descriptor's absolute local index
 * range (k * R + t), group = the launch's block size -- the descriptors of a task's part are that
 * long, the last one possibly shorter, none above 16384 -- and rows = the task's descriptor count
 * in that launch.  An empty task has no entry; no launch has more than 20480.  Returns the number
 * of entries (may exceed max_entries, in which case only the first max_entries are written) or a
 * negative code (DPOW_EINVAL: a NULL argument, n_tasks of 0 or above DPOW_BATCH_MAX, k_begin >
 * k_end, a cap outside its range; DPOW_ERANGE: k_end > DPOW_K_LIMIT, more than INT32_MAX entries);
 * *launches_out = launches. */
int dpow_census_plan(const uint64_t *k_begin, const uint64_t *k_end, const uint32_t *worker_bits,
                     size_t n_tasks, uint64_t cap, dpow_batch_range *out, size_t max_entries,
                     uint64_t *launches_out);

/* The scan's slice rule (host logic of dpow_scan, exposed for testing):
 * the local indices one launch of a scan for `ntz` covers when its hit list holds `capacity`
 * entries (clamped to [256, 65536]; dpow_scan's own is 65536).  A multiple of 256 in
 * [256, 2^28]; its expected hits, slice / 16^min(ntz, 32), are at most capacity / 4 wherever
 * the slice is above 256. */
uint64_t dpow_scan_slice(uint32_t ntz, uint32_t capacity);

/* The batched scan's launch planner (host logic of dpow_scan_batch, exposed for testing; DESIGN.md
 * section 17) for tasks with local index ranges [i_begin[i], i_end[i]) (k * R + t, R = 256 >>
 * worker_bits % 9 candidates per k) and depths ntz[i].  A launch takes tasks in array order under
 * two budgets: its local indices total at most `cap` (0: the call's own 2^28; else 256..2^28,
 * rounded down to a multiple of 256), and its hit weight at most capacity / 4, where `capacity`
 * is the hit list's (0: the call's own 65536; else 1024..65536, rounded down to a multiple of
 * 1024) and a part of n indices at depth N weighs ceil(n / 16^min(N, 7)).  Only its last task
 * can be cut, at a multiple of 256 local indices from the task's begin, and goes on in the next
 * launch; a launch takes at least 256 indices or what is left of a task.  For one task the launches
 * are dpow_scan's (dpow_scan_slice).  The entries are dpow_census_plan's: one per workgroup
 * descriptor, in launch order and within a launch in task order, none above 16384 indices, no
 * launch with more than 20480, no entry for an empty task.  Returns the number of entries (may
 * exceed max_entries, in which case only the first max_entries are written) or a negative code
 * (DPOW_EINVAL: a NULL argument, n_tasks of 0 or above DPOW_BATCH_MAX, i_begin > i_end, a budget
 * outside its range; DPOW_ERANGE: i_end > DPOW_K_LIMIT * 256, more than INT32_MAX entries);
 * *launches_out = launches. */
int dpow_scan_plan(const uint64_t *i_begin, const uint64_t *i_end, const uint32_t *ntz,
                   size_t n_tasks, uint64_t cap, uint32_t capacity, dpow_batch_range *out,
                   size_t max_entries, uint64_t *launches_out);
/* What dpow_scan_batch does when a launch of `total` local indices and hit weight `weight`
 * overflowed its list: the budgets (*cap_out local indices, *capacity_out / 4 hit weight, both
 * arguments of dpow_scan_plan) it plans the same parts with again, each half of what the launch
 * held, rounded up to a multiple of 256 (1024 for the capacity) and at least that.  A launch of
 * 256 indices cannot overflow a list of at least 256 entries, and repeated halving gets there. */
void dpow_scan_plan_halve(uint64_t total, uint64_t weight, uint64_t *cap_out, uint32_t *capacity_out);

/* The device scan's cut (host logic of dpow_scan_device, exposed for testing; DESIGN.md section
 * 18): given the inclusive prefix of a slice's per-workgroup hit totals (non-decreasing, n_groups
 * entries) and the room left in the caller's list, the largest number of leading workgroups whose
 * hits fit: n_groups when the slice's total fits, 0 when not even the first does (or for a NULL
 * prefix). */
size_t dpow_scan_device_cut(const uint32_t *inclusive_prefix, size_t n_groups, size_t room);

/* The passes of one wave of the digests of many nonces (device logic of csrc/md5_digest_many.hip,
 * the same code compiled for the host, exposed for testing): the wave holds
 * the list positions [e_first, e_end), at most 64, and makes one pass per task whose segment
 * [rows[t], rows[t + 1]) meets them in a non-empty [lo, hi), in ascending task order.  Returns the
 * number of passes and writes the first max_passes of them.  Whatever the rows hold it reads
 * rows[0 .. n_tasks] only, makes at most n_tasks passes, and every pass has task < n_tasks and
 * e_first <= lo < hi <= e_end; with rows that do not descend the passes are disjoint and cover
 * exactly the wave's positions within [rows[0], rows[n_tasks]).  DPOW_EINVAL for a NULL rows (or
 * out with max_passes > 0), n_tasks of 0 or above DPOW_BATCH_MAX, e_end < e_first or more than 64
 * positions. */
typedef struct dpow_digest_pass {
    uint64_t lo, hi;
    uint32_t task;
    uint32_t pad_;
} dpow_digest_pass;
int dpow_digests_batch_walk(const uint64_t *rows, size_t n_tasks, uint64_t e_first, uint64_t e_end,
                            dpow_digest_pass *out, size_t max_passes);

/* What a launch means for the tasks (host logic of dpow_scan_batch_device, exposed for testing;
 * DESIGN.md section 20): the first n_fit workgroup descriptors of a launch (entries of
 * dpow_census_plan, local indices; only task, i_begin and i_end are read) have been placed.  The
 * tasks have local index ranges [i_begin[i], i_end[i]) and progress i_done[i] (in: before the launch;
 * out: after it): each placed descriptor must begin where its task's progress stands and moves it
 * to its own end.  *next_row (in/out) is the first task whose row pointer no earlier launch has
 * settled.  A placed descriptor that begins its task settles that task's row and those of the
 * (empty) tasks from *next_row up to it: row_block[j] = that descriptor's index in the launch, the
 * row being the list's length before the launch plus the launch's hits before that descriptor;
 * row_block[j] = 0xFFFFFFFF for every task this launch does not settle.  status[i] =
 * DPOW_EXHAUSTED where i_done[i] == i_end[i] (an empty task is), else `unfinished` (DPOW_MORE or
 * DPOW_CANCELLED when the call ends with this launch).  Returns the number of rows settled, or
 * DPOW_EINVAL (nothing written) for a NULL argument, n_tasks of 0 or above DPOW_BATCH_MAX, n_fit
 * above 20480, progress outside its task, or a descriptor that names no task, reaches beyond its
 * task or does not begin at its task's progress. */
int dpow_scan_batch_device_settle(const dpow_batch_range *blocks, size_t n_fit,
                                  const uint64_t *i_begin, const uint64_t *i_end, size_t n_tasks,
                                  uint64_t *i_done, uint32_t *next_row, uint32_t *row_block,
                                  int32_t unfinished, int32_t *status);

/* ---------------------------------------------------------------------------
 * Introspection / measurement.
 * ------------------------------------------------------------------------- */
typedef struct dpow_stats {
    uint64_t searches;     /* dpow_search calls */
    uint64_t launches;     /* kernel launches whose completion record a search consumed */
    uint64_t candidates;   /* candidates covered by those launches' windows */
    double kernel_ms;      /* sum of their durations, as each launch stamps them into its
                              completion record (s_memrealtime at its start and at the record) */
} dpow_stats;
int dpow_get_stats(dpow_ctx *ctx, dpow_stats *out);
void dpow_reset_stats(dpow_ctx *ctx);
/* The hipStream_t the context's kernels run on (as void*, for event timing). */
void *dpow_stream(dpow_ctx *ctx);
/* Device ordinal of the context. */
int dpow_device(dpow_ctx *ctx);
/* Worker waves per launch and CUs used (for reporting). */
int dpow_geometry(dpow_ctx *ctx, uint32_t *cus, uint32_t *blocks_per_cu, uint32_t *threads_per_block);
/* Thread-local description of the last error. */
const char *dpow_last_error(void);
int dpow_abi_version(void);
/* Source hash the library was built from: 16 hex digits of sha256 over the
 * kernel/host sources, the Makefile, these headers and the build flags.  The
 * Python host (distpow/_lib.py) refuses a library whose id does not match the
 * tree it runs in, so a stale build is never tested or benched. */
const char *dpow_build_id(void);
/* Number of visible HIP devices (0 when none; never an error). */
int dpow_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* DPOW_H */
