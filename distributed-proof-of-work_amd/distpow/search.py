"""Host-side mirror of the reference worker's search (worker.go:258-401) over libdpow.

`Miner` is one GPU's search engine.  `Miner.mine` reproduces the reference
miner's loop (worker.go:318-400: k = 0, 1, 2, ... until a hit or a kill) as a
sequence of GPU windows; `Miner.search` is one window (the C ABI dpow_search).
Names and argument meaning follow the reference: nonce, num_trailing_zeros
(NumTrailingZeros), worker_byte (WorkerByte), worker_bits (WorkerBits).
"""
import array
import ctypes
import struct
from dataclasses import dataclass
from typing import List, Optional, Sequence

from . import _lib
from ._lib import (CANCELLED, DPOW_K_LIMIT, DPOW_MAX_SECRET, DPOW_NO_HIT, EXHAUSTED, FOUND, DpowError,
                   PlanLaunch, Stats, check, lib)

__all__ = ["Miner", "SearchResult", "BatchTask", "batch_candidate", "batch_plan", "batch_plan_block",
           "TaskQueue", "QueueResult", "queue_plan", "ScanHit", "scan_slice", "ScanTask", "scan_plan", "scan_plan_halve", "Census",
           "scan_device_cut", "scan_batch_device_settle", "CensusTask", "census_plan", "digest_of_index", "secret_from_index", "md5", "verify", "trailing_zero_nibbles",
           "thread_bytes", "remainder_bits", "global_index", "plan_window", "plan_candidate",
           "device_count", "DPOW_NO_HIT", "FOUND", "EXHAUSTED", "CANCELLED"]


@dataclass
class SearchResult:
    status: int                   # FOUND / EXHAUSTED / CANCELLED
    global_idx: int = DPOW_NO_HIT  # k * 256 + threadByte of the hit
    secret: Optional[bytes] = None  # threadByte || chunk_k  (WorkerResult.Secret, worker.go:361)

    @property
    def found(self):
        return self.status == FOUND


def _b(x) -> bytes:
    return bytes(x)


def remainder_bits(worker_bits: int) -> int:
    """worker.go:302: remainderBits := 8 - (args.WorkerBits % 9)."""
    return 8 - (worker_bits % 9)


def thread_bytes(worker_byte: int, worker_bits: int) -> List[int]:
    """worker.go:312-316: threadBytes[i] = uint8((WorkerByte << remainderBits) | i)."""
    rb = remainder_bits(worker_bits)
    return [((worker_byte << rb) | i) & 0xFF for i in range(1 << rb)]


def global_index(k: int, thread_byte: int) -> int:
    return k * 256 + thread_byte


def secret_from_index(g: int) -> bytes:
    buf = (ctypes.c_uint8 * DPOW_MAX_SECRET)()
    n = ctypes.c_size_t()
    check(lib().dpow_secret_from_index(g, buf, ctypes.byref(n)), "dpow_secret_from_index")
    return bytes(buf[:n.value])


def md5(msg) -> bytes:
    out = (ctypes.c_uint8 * 16)()
    m = _b(msg)
    lib().dpow_md5(m, len(m), out)
    return bytes(out)


def digest_of_index(nonce, global_idx: int):
    """(digest, depth) of one candidate on the host (dpow_digest_of_index): the 16-byte MD5 of
    nonce || secret_from_index(global_idx) and its trailing '0' characters."""
    n = _b(nonce)
    out, tz = (ctypes.c_uint8 * 16)(), ctypes.c_uint32()
    check(lib().dpow_digest_of_index(n, len(n), global_idx, out, ctypes.byref(tz)), "dpow_digest_of_index")
    return bytes(out), tz.value


def trailing_zero_nibbles(digest: bytes) -> int:
    assert len(digest) == 16
    return lib().dpow_trailing_zero_nibbles(digest)


def verify(nonce, secret, num_trailing_zeros: int) -> bool:
    n, s = _b(nonce), _b(secret)
    return lib().dpow_verify(n, len(n), s, len(s), num_trailing_zeros) == 1


def plan_window(nonce, worker_byte, worker_bits, k_begin, k_end, num_trailing_zeros: int = 0) -> List[PlanLaunch]:
    """The launches dpow_search would queue for this window (dpow_plan_window)."""
    n = _b(nonce)
    cnt = check(lib().dpow_plan_window(n, len(n), num_trailing_zeros, worker_byte, worker_bits, k_begin, k_end,
                                       None, 0), "dpow_plan_window")
    arr = (PlanLaunch * max(cnt, 1))()
    check(lib().dpow_plan_window(n, len(n), num_trailing_zeros, worker_byte, worker_bits, k_begin, k_end, arr, cnt),
          "dpow_plan_window")
    return list(arr[:cnt])


def plan_candidate(nonce, worker_byte, worker_bits, local_idx):
    """(iv[4], words[16*nblk], nblk) the kernel hashes for one candidate."""
    n = _b(nonce)
    iv = (ctypes.c_uint32 * 4)()
    words = (ctypes.c_uint32 * 32)()
    nblk = ctypes.c_uint32()
    check(lib().dpow_plan_candidate(n, len(n), worker_byte, worker_bits, local_idx, iv, words,
                                    ctypes.byref(nblk)), "dpow_plan_candidate")
    return list(iv), list(words[:16 * nblk.value]), nblk.value


@dataclass
class BatchTask:
    """One task of Miner.search_batch: the arguments of Miner.search (dpow_batch_task)."""
    nonce: Sequence[int]
    num_trailing_zeros: int
    worker_byte: int = 0
    worker_bits: int = 0
    k_begin: int = 0
    k_end: int = 1
    bound: int = DPOW_NO_HIT


def batch_candidate(nonce, worker_byte, worker_bits, local_idx):
    """(iv[4], words[16*nblk], nblk) the batch kernel hashes for one candidate (dpow_batch_candidate)."""
    n = _b(nonce)
    iv = (ctypes.c_uint32 * 4)()
    words = (ctypes.c_uint32 * 32)()
    nblk = ctypes.c_uint32()
    check(lib().dpow_batch_candidate(n, len(n), worker_byte, worker_bits, local_idx, iv, words,
                                     ctypes.byref(nblk)), "dpow_batch_candidate")
    return list(iv), list(words[:16 * nblk.value]), nblk.value


def batch_plan(windows):
    """The launches dpow_search_batch queues for windows [(k_begin, k_end, worker_bits), ...] when no
    task hits (dpow_batch_plan): (entries, launches), entries a ctypes array of BatchRange, one per
    (launch, live task) in block-map order."""
    n = len(windows)
    kb = (ctypes.c_uint64 * max(n, 1))(*[w[0] for w in windows])
    ke = (ctypes.c_uint64 * max(n, 1))(*[w[1] for w in windows])
    wb = (ctypes.c_uint32 * max(n, 1))(*[w[2] for w in windows])
    launches = ctypes.c_uint64()
    cnt = check(lib().dpow_batch_plan(kb, ke, wb, n, None, 0, ctypes.byref(launches)), "dpow_batch_plan")
    arr = (_lib.BatchRange * max(cnt, 1))()
    check(lib().dpow_batch_plan(kb, ke, wb, n, arr, cnt, ctypes.byref(launches)), "dpow_batch_plan")
    return (_lib.BatchRange * cnt).from_buffer(arr), launches.value


def batch_plan_block(entries, n_live, block):
    """(task, lo, hi) of workgroup `block` of a launch whose n_live entries start at entries[0], or
    None when the workgroup has nothing to hash (dpow_batch_plan_block: the kernel's block map)."""
    task, lo, hi = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
    r = check(lib().dpow_batch_plan_block(entries, n_live, block, ctypes.byref(task), ctypes.byref(lo),
                                          ctypes.byref(hi)), "dpow_batch_plan_block")
    return (task.value, lo.value, hi.value) if r else None


def queue_plan(left: Sequence[int], age: Sequence[int]):
    """One launch of the task queue for live tasks with left[i] local indices to go and age[i]
    launches behind them (dpow_queue_plan): (blocks, budget), blocks a ctypes array of BatchRange,
    one per workgroup in descriptor order, ranges relative to each task's current position."""
    n = len(left)
    if len(age) != n:
        raise ValueError("queue_plan: left and age differ in length")
    la = (ctypes.c_uint64 * max(n, 1))(*left)
    aa = (ctypes.c_uint32 * max(n, 1))(*age)
    budget = ctypes.c_uint64()
    cnt = check(lib().dpow_queue_plan(la, aa, n, None, 0, ctypes.byref(budget)), "dpow_queue_plan")
    arr = (_lib.BatchRange * max(cnt, 1))()
    check(lib().dpow_queue_plan(la, aa, n, arr, cnt, ctypes.byref(budget)), "dpow_queue_plan")
    return (_lib.BatchRange * cnt).from_buffer(arr), budget.value


_SCAN_HIT = struct.Struct(f"<QII{DPOW_MAX_SECRET}s")  # dpow_scan_hit
assert _SCAN_HIT.size == ctypes.sizeof(_lib.ScanHitC)


@dataclass(frozen=True)
class ScanHit:
    """One hit of Miner.scan (dpow_scan_hit)."""
    global_idx: int  # k * 256 + threadByte
    tz: int          # trailing '0' characters of its digest, from the host MD5
    secret: bytes    # threadByte || chunk_k


def scan_slice(num_trailing_zeros: int, capacity: int = _lib.SCAN_CAP) -> int:
    """Local indices per launch of a scan whose hit list holds `capacity` entries (dpow_scan_slice)."""
    return lib().dpow_scan_slice(num_trailing_zeros, capacity)


def scan_device_cut(inclusive_prefix: Sequence[int], room: int) -> int:
    """Leading workgroups of a slice whose hits fit `room`, given the inclusive prefix of the slice's
    per-workgroup hit totals (dpow_scan_device_cut, the cut dpow_scan_device makes)."""
    n = len(inclusive_prefix)
    arr = (ctypes.c_uint32 * max(n, 1))(*inclusive_prefix)
    return lib().dpow_scan_device_cut(arr, n, room)


def digests_batch_walk(rows: Sequence[int], e_first: int, e_end: int):
    """The passes [(task, lo, hi), ...] of one wave of the digests of many nonces over the list
    positions [e_first, e_end) (dpow_digests_batch_walk, the walk digest_many_kernel makes): `rows`
    holds the n_tasks + 1 row pointers, whatever they are."""
    n = len(rows) - 1
    arr = (ctypes.c_uint64 * (n + 1))(*rows)
    out = (_lib.DigestPassC * max(n, 1))()
    cnt = check(lib().dpow_digests_batch_walk(arr, n, e_first, e_end, out, n), "dpow_digests_batch_walk")
    return [(p.task, p.lo, p.hi) for p in out[:min(cnt, n)]]


def scan_batch_device_settle(blocks, n_fit: int, i_begin: Sequence[int], i_end: Sequence[int], i_done: Sequence[int],
                             next_row: int = 0, unfinished: int = _lib.MORE):
    """What the first `n_fit` workgroup descriptors of a launch having been placed means for the tasks
    of a dpow_scan_batch_device call (dpow_scan_batch_device_settle): (i_done, next_row, row_block,
    status).  `blocks` is the launch's descriptors (BatchRange entries, as census_plan returns them);
    the tasks have local index ranges [i_begin[i], i_end[i]) and progress i_done[i] before the launch.
    row_block[j] is the descriptor whose place in the list is task j's row pointer, None for a task
    this launch does not settle."""
    n = len(i_begin)
    arr = (_lib.BatchRange * max(n_fit, 1))(*blocks[:n_fit])
    ib, ie, idn = ((ctypes.c_uint64 * max(n, 1))(*v) for v in (i_begin, i_end, i_done))
    nr = ctypes.c_uint32(next_row)
    rb = (ctypes.c_uint32 * max(n, 1))()
    st = (ctypes.c_int32 * max(n, 1))()
    check(lib().dpow_scan_batch_device_settle(arr, n_fit, ib, ie, n, idn, ctypes.byref(nr), rb, unfinished, st),
          "dpow_scan_batch_device_settle")
    return (list(idn)[:n], nr.value, [None if b == 0xFFFFFFFF else b for b in list(rb)[:n]], list(st)[:n])


_SCAN_TASK_IN = struct.Struct("@PNIIIQQ")  # dpow_scan_task: the input fields
_SCAN_TASK = struct.Struct("@PNIIIQQQiQQ")
assert _SCAN_TASK.size == ctypes.sizeof(_lib.ScanTaskC) and _SCAN_TASK_IN.size == _lib.ScanTaskC.k_done.offset


@dataclass
class ScanTask:
    """One task of Miner.scan_many: the arguments of Miner.scan (dpow_scan_task)."""
    nonce: Sequence[int]
    num_trailing_zeros: int
    worker_byte: int = 0
    worker_bits: int = 0
    k_begin: int = 0
    k_end: int = 1


_DIGEST_TASK_IN = struct.Struct("@PNI")  # dpow_digest_task: the input fields
_DIGEST_TASK = struct.Struct("@PNIQQ")
assert _DIGEST_TASK.size == ctypes.sizeof(_lib.DigestTaskC) and _lib.DigestTaskC.n_entries.offset == 24


@dataclass
class DigestTask:
    """One task of Miner.digests_many: the arguments of Miner.digests (dpow_digest_task), and the depth
    its entries are held against (0: none)."""
    nonce: Sequence[int]
    indices: Sequence[int]
    num_trailing_zeros: int = 0


def scan_plan(windows, cap: int = 0, capacity: int = 0):
    """The launches dpow_scan_batch makes for windows [(i_begin, i_end, num_trailing_zeros), ...] of
    local indices (dpow_scan_plan): (blocks, launches), blocks a ctypes array of BatchRange, one per
    workgroup descriptor in launch order, ranges in absolute local indices.  `cap` is a launch's
    budget of local indices (0: the call's own 2^28), `capacity` the hit list's, a quarter of which
    is a launch's budget of hit weight (0: the call's own 65536)."""
    n = len(windows)
    ib = (ctypes.c_uint64 * max(n, 1))(*[w[0] for w in windows])
    ie = (ctypes.c_uint64 * max(n, 1))(*[w[1] for w in windows])
    nz = (ctypes.c_uint32 * max(n, 1))(*[w[2] for w in windows])
    launches = ctypes.c_uint64()
    cnt = check(lib().dpow_scan_plan(ib, ie, nz, n, cap, capacity, None, 0, ctypes.byref(launches)), "dpow_scan_plan")
    arr = (_lib.BatchRange * max(cnt, 1))()
    check(lib().dpow_scan_plan(ib, ie, nz, n, cap, capacity, arr, cnt, ctypes.byref(launches)), "dpow_scan_plan")
    return (_lib.BatchRange * cnt).from_buffer(arr), launches.value


def scan_plan_halve(total: int, weight: int):
    """(cap, capacity) dpow_scan_batch plans a launch's parts with again after the launch, of `total`
    local indices and hit weight `weight`, overflowed its list (dpow_scan_plan_halve)."""
    cap, capacity = ctypes.c_uint64(), ctypes.c_uint32()
    lib().dpow_scan_plan_halve(total, weight, ctypes.byref(cap), ctypes.byref(capacity))
    return cap.value, capacity.value


@dataclass(frozen=True)
class Census:
    """Depth counts and per-depth first hits of a window (dpow_census, Miner.census).  A candidate's
    depth is the number of trailing '0' characters of its digest; every tuple has 33 entries, d = 0..32."""
    count_ge: tuple  # candidates with depth >= d (count_ge[0]: the window's size)
    first_ge: tuple  # lowest global index with depth >= d (Miner.search's answer at d), None where absent
    first_tz: tuple  # that candidate's depth, from the host MD5 (0 where absent)
    deepest: int     # the largest d with count_ge[d] > 0 (0 of an empty window)

    @classmethod
    def empty(cls) -> "Census":
        return cls((0,) * _lib.CENSUS_DEPTHS, (None,) * _lib.CENSUS_DEPTHS, (0,) * _lib.CENSUS_DEPTHS, 0)

    @classmethod
    def _from_c(cls, c) -> "Census":
        return cls(tuple(c.count_ge), tuple(None if g == DPOW_NO_HIT else g for g in c.first_ge),
                   tuple(c.first_tz), c.deepest)

    def _to_c(self):
        c = _lib.CensusC()
        for d in range(_lib.CENSUS_DEPTHS):
            c.count_ge[d] = self.count_ge[d]
            c.first_ge[d] = DPOW_NO_HIT if self.first_ge[d] is None else self.first_ge[d]
            c.first_tz[d] = self.first_tz[d]
        c.deepest = self.deepest
        return c

    def exact(self, d: int) -> int:
        """Candidates of depth exactly d."""
        return self.count_ge[d] - (self.count_ge[d + 1] if d + 1 < _lib.CENSUS_DEPTHS else 0)

    def secret(self, d: int) -> Optional[bytes]:
        """The secret of first_ge[d] (threadByte || chunk_k), None where absent."""
        return None if self.first_ge[d] is None else secret_from_index(self.first_ge[d])

    def merged(self, other: "Census") -> "Census":
        """This census followed by the census of a window that lies wholly above it
        (dpow_census_merge); DpowError with code EINVAL when it does not, or either is not
        self-consistent."""
        into, nxt = self._to_c(), other._to_c()
        check(lib().dpow_census_merge(ctypes.byref(into), ctypes.byref(nxt)), "dpow_census_merge")
        return Census._from_c(into)


_CENSUS_TASK_IN = struct.Struct("@PNIIQQ")  # dpow_census_task: the input fields
_CENSUS_TASK = struct.Struct(f"@PNIIQQQi{_lib.CENSUS_DEPTHS}Q{_lib.CENSUS_DEPTHS}Q{_lib.CENSUS_DEPTHS}II")
assert _CENSUS_TASK.size == ctypes.sizeof(_lib.CensusTaskC) and _CENSUS_TASK_IN.size == _lib.CensusTaskC.k_done.offset


@dataclass
class CensusTask:
    """One task of Miner.census_many: the arguments of Miner.census (dpow_census_task)."""
    nonce: Sequence[int]
    worker_byte: int = 0
    worker_bits: int = 0
    k_begin: int = 0
    k_end: int = 1


def census_plan(windows, cap: int = 0):
    """The launches dpow_census_batch makes for windows [(k_begin, k_end, worker_bits), ...]
    (dpow_census_plan): (blocks, launches), blocks a ctypes array of BatchRange, one per workgroup
    descriptor in launch order, ranges in absolute local indices.  `cap` is a launch's budget of
    local indices (0: the call's own 2^28)."""
    n = len(windows)
    kb = (ctypes.c_uint64 * max(n, 1))(*[w[0] for w in windows])
    ke = (ctypes.c_uint64 * max(n, 1))(*[w[1] for w in windows])
    wb = (ctypes.c_uint32 * max(n, 1))(*[w[2] for w in windows])
    launches = ctypes.c_uint64()
    cnt = check(lib().dpow_census_plan(kb, ke, wb, n, cap, None, 0, ctypes.byref(launches)), "dpow_census_plan")
    arr = (_lib.BatchRange * max(cnt, 1))()
    check(lib().dpow_census_plan(kb, ke, wb, n, cap, arr, cnt, ctypes.byref(launches)), "dpow_census_plan")
    return (_lib.BatchRange * cnt).from_buffer(arr), launches.value


@dataclass
class QueueResult:
    """One decided task of a TaskQueue (dpow_queue_result)."""
    result: SearchResult
    ticket: int
    user: int = 0
    launches: int = 0        # launches the task took part in
    queued_ms: float = 0.0   # submit to decided, on the host clock

    @property
    def status(self):
        return self.result.status


class TaskQueue:
    """The batched search as a service on one GPU (dpow_queue_*): tasks are submitted, cancelled and
    collected one by one, from any thread, while the queue's launches keep running over whatever
    is live.  A task's answer is what Miner.search returns for it."""

    def __init__(self, device: int = 0):
        self._q = ctypes.c_void_p()
        check(lib().dpow_queue_open(device, ctypes.byref(self._q)), "dpow_queue_open")
        self.device = device

    def close(self):
        """Cancels what is undecided and ends the queue (no other call may be in flight)."""
        if self._q:
            lib().dpow_queue_close(self._q)
            self._q = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, task: BatchTask, user: int = 0) -> int:
        """Queue one task; returns its ticket.  DpowError with code EAGAIN when DPOW_BATCH_MAX tasks
        are undecided."""
        n = _b(task.nonce)
        ticket = ctypes.c_uint64()
        check(lib().dpow_queue_submit(self._q, n, len(n), task.num_trailing_zeros, task.worker_byte,
                                      task.worker_bits, task.k_begin, task.k_end, task.bound, user,
                                      ctypes.byref(ticket)), "dpow_queue_submit")
        return ticket.value

    def cancel(self, ticket: int) -> bool:
        """True when the task was undecided and is CANCELLED now; False when it was decided already."""
        return check(lib().dpow_queue_cancel(self._q, ticket), "dpow_queue_cancel") == 1

    @staticmethod
    def _result(c) -> QueueResult:
        res = (SearchResult(FOUND, c.global_idx, bytes(c.secret[:c.secret_len])) if c.status == FOUND
               else SearchResult(c.status))
        return QueueResult(res, c.ticket, c.user, c.launches, c.queued_ms)

    def next(self, timeout_ms: int = -1) -> Optional[QueueResult]:
        """Any decided task, in the order they were decided; None on time-out (timeout_ms < 0 blocks).
        A task the queue's failure ended carries the negative code as its status."""
        c = _lib.QueueResultC()
        r = check(lib().dpow_queue_next(self._q, ctypes.byref(c), timeout_ms), "dpow_queue_next")
        return self._result(c) if r else None

    def wait(self, ticket: int, timeout_ms: int = -1) -> Optional[QueueResult]:
        """The given task's result; None on time-out.  Each result is handed out once, by next or wait."""
        c = _lib.QueueResultC()
        r = check(lib().dpow_queue_wait(self._q, ticket, ctypes.byref(c), timeout_ms), "dpow_queue_wait")
        return self._result(c) if r else None

    def stats(self):
        """(BatchStats totals since open, tasks undecided, results not yet collected)."""
        st = _lib.BatchStats()
        live, unc = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().dpow_queue_stats(self._q, ctypes.byref(st), ctypes.byref(live), ctypes.byref(unc)),
              "dpow_queue_stats")
        return st, live.value, unc.value


def device_count() -> int:
    return lib().dpow_device_count()


class Miner:
    """One GPU's search context (dpow_ctx): persistent device buffers, a HIP stream
    and the pinned cancel flag that Found/Cancel raise (worker.go:194,209)."""

    # k-window per dpow_search call.  Launches inside a window are queued
    # back-to-back (split where the chunk length changes); a call returns
    # at the first window holding a hit.
    DEFAULT_WINDOW = 1 << 26

    def __init__(self, device: int = 0):
        self._ctx = ctypes.c_void_p()
        check(lib().dpow_open(device, ctypes.byref(self._ctx)), "dpow_open")
        self.device = device
        self._cancel = lib().dpow_cancel_flag(self._ctx)

    def close(self):
        if self._ctx:
            lib().dpow_close(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- cancellation (killChan) ------------------------------------------------
    def cancel(self):
        """Raise the pinned cancel flag: a running search stops mid-launch."""
        self._cancel[0] = 1

    def clear_cancel(self):
        self._cancel[0] = 0

    def bound(self, global_idx: int):
        """Lower the bound of the search running on this context (from another thread):
        it stops at global_idx and returns EXHAUSTED unless it has a hit below it
        (dpow_search_bound).  No effect when no search runs."""
        check(lib().dpow_search_bound(self._ctx, global_idx), "dpow_search_bound")

    def attach_node(self, slot: Optional[int]):
        """Attach a node slot (NodeBoard.begin(): the address of a dpow_node_slot in the
        node's shared memory) to this context's searches, or detach it (None)
        (dpow_node_attach)."""
        check(lib().dpow_node_attach(self._ctx, slot or None), "dpow_node_attach")

    @property
    def cancelled(self) -> bool:
        return self._cancel[0] != 0

    # -- the hot path -----------------------------------------------------------
    def search(self, nonce: Sequence[int], num_trailing_zeros: int, worker_byte: int = 0,
               worker_bits: int = 0, k_begin: int = 0, k_end: int = 1, bound: int = DPOW_NO_HIT) -> SearchResult:
        n = _b(nonce)
        best = ctypes.c_uint64(bound)
        sec = (ctypes.c_uint8 * DPOW_MAX_SECRET)()
        slen = ctypes.c_size_t()
        r = check(lib().dpow_search(self._ctx, n, len(n), num_trailing_zeros, worker_byte, worker_bits,
                                    k_begin, k_end, ctypes.byref(best), sec, ctypes.byref(slen)), "dpow_search")
        if r == FOUND:
            return SearchResult(FOUND, best.value, bytes(sec[:slen.value]))
        return SearchResult(r)

    def mine(self, nonce: Sequence[int], num_trailing_zeros: int, worker_byte: int = 0, worker_bits: int = 0,
             k_start: int = 0, k_limit: int = DPOW_K_LIMIT, window: int = DEFAULT_WINDOW) -> SearchResult:
        """worker.go:318-400: search k = k_start, k_start + 1, ... until a hit, the
        cancel flag, or k_limit (the reference has no limit; DPOW_K_LIMIT = 2^55 - 1 k)."""
        k = k_start
        while k < k_limit:
            ke = min(k_limit, k + window)
            res = self.search(nonce, num_trailing_zeros, worker_byte, worker_bits, k, ke)
            if res.status != EXHAUSTED:
                return res
            k = ke
        return SearchResult(EXHAUSTED)

    # -- batched search ---------------------------------------------------------
    def search_batch(self, tasks: Sequence[BatchTask]) -> List[SearchResult]:
        """B independent windows in one pass over the GPU (dpow_search_batch): result i is what
        `search` returns for tasks[i].  The call's launch counts are kept in last_batch_stats."""
        n = len(tasks)
        arr = (_lib.BatchTaskC * max(n, 1))()
        nonces = [_b(t.nonce) for t in tasks]
        buf = ctypes.create_string_buffer(b"".join(nonces), max(sum(map(len, nonces)), 1))  # alive for the call
        addr = ctypes.addressof(buf)
        for t, nb, c in zip(tasks, nonces, arr):
            c.nonce, c.nonce_len = addr, len(nb)
            addr += len(nb)
            c.ntz, c.worker_byte, c.worker_bits = t.num_trailing_zeros, t.worker_byte, t.worker_bits
            c.k_begin, c.k_end, c.best_global_idx = t.k_begin, t.k_end, t.bound
        st = _lib.BatchStats()
        check(lib().dpow_search_batch(self._ctx, arr, n, ctypes.byref(st)), "dpow_search_batch")
        self.last_batch_stats = st
        return [SearchResult(FOUND, c.best_global_idx, bytes(c.secret[:c.secret_len])) if c.status == FOUND
                else SearchResult(c.status) for c in arr[:n]]

    def mine_many(self, requests: Sequence[BatchTask], k_limit: int = DPOW_K_LIMIT,
                  window: int = DEFAULT_WINDOW) -> List[SearchResult]:
        """`mine` for many requests at once: every unfinished request advances window by window
        from its k_begin (its k_end is ignored) through search_batch, until each has a hit, the
        cancel flag is raised, or k_limit is reached."""
        out: List[Optional[SearchResult]] = [None] * len(requests)
        k = [r.k_begin for r in requests]
        todo = [i for i in range(len(requests))]
        while todo:
            for i in [i for i in todo if k[i] >= k_limit]:
                out[i] = SearchResult(EXHAUSTED)
            todo = [i for i in todo if out[i] is None]
            if not todo:
                break
            batch = [BatchTask(requests[i].nonce, requests[i].num_trailing_zeros, requests[i].worker_byte,
                               requests[i].worker_bits, k[i], min(k_limit, k[i] + window), requests[i].bound)
                     for i in todo]
            results = []
            for off in range(0, len(batch), _lib.DPOW_BATCH_MAX):  # at most DPOW_BATCH_MAX tasks per call
                results += self.search_batch(batch[off:off + _lib.DPOW_BATCH_MAX])
            for i, t, res in zip(todo, batch, results):
                if res.status != EXHAUSTED:
                    out[i] = res
                k[i] = t.k_end
            todo = [i for i in todo if out[i] is None]
        return out

    # -- scan -------------------------------------------------------------------
    def scan_page(self, nonce: Sequence[int], num_trailing_zeros: int, worker_byte: int = 0, worker_bits: int = 0,
                  k_begin: int = 0, k_end: int = 1, max_hits: int = _lib.SCAN_CAP):
        """One dpow_scan call: (status, hits, k_done).  EXHAUSTED: the window is done; MORE: `hits`
        are all hits of [k_begin, k_done) and the caller continues from k_done; CANCELLED likewise.
        The call's launch counts are kept in last_scan_stats."""
        n = _b(nonce)
        arr = (_lib.ScanHitC * max(max_hits, 1))()
        cnt, k_done, st = ctypes.c_size_t(), ctypes.c_uint64(), _lib.BatchStats()
        r = check(lib().dpow_scan(self._ctx, n, len(n), num_trailing_zeros, worker_byte, worker_bits, k_begin, k_end,
                                  arr, max_hits, ctypes.byref(cnt), ctypes.byref(k_done), ctypes.byref(st)),
                  "dpow_scan")
        self.last_scan_stats = st
        raw = ctypes.string_at(arr, cnt.value * _SCAN_HIT.size)
        hits = [ScanHit(g, tz, sec[:slen]) for g, tz, slen, sec in _SCAN_HIT.iter_unpack(raw)]
        return r, hits, k_done.value

    def scan(self, nonce: Sequence[int], num_trailing_zeros: int, worker_byte: int = 0, worker_bits: int = 0,
             k_begin: int = 0, k_end: int = 1, max_hits: int = _lib.SCAN_CAP) -> List[ScanHit]:
        """Every candidate of the partition over k in [k_begin, k_end) whose digest ends in at least
        num_trailing_zeros '0' characters, in increasing global index, each with its depth
        (dpow_scan, paged over MORE; max_hits is the page size).  A raised cancel flag ends the scan
        early with the hits found so far (see `cancelled`; scan_page tells how far it got)."""
        out: List[ScanHit] = []
        k = k_begin
        while True:
            r, hits, k = self.scan_page(nonce, num_trailing_zeros, worker_byte, worker_bits, k, k_end, max_hits)
            out += hits
            if r != _lib.MORE:
                return out

    def scan_batch(self, tasks: Sequence[ScanTask], max_hits: int = _lib.SCAN_CAP):
        """Every hit of many windows in one pass over the GPU (dpow_scan_batch): one
        (status, hits, k_done) per task, what scan_page returns for it while `max_hits` hits of the
        tasks together have room.  The task that does not fit is MORE from its k_done, the tasks
        behind it MORE from their k_begin; a raised cancel flag leaves the tasks not finished
        CANCELLED likewise.  The call's launch counts are kept in last_scan_many_stats."""
        n = len(tasks)
        arr = (_lib.ScanTaskC * max(n, 1))()
        nonces = [_b(t.nonce) for t in tasks]
        buf = ctypes.create_string_buffer(b"".join(nonces), max(sum(map(len, nonces)), 1))  # alive for the call
        addr = ctypes.addressof(buf)
        raw = (ctypes.c_ubyte * ctypes.sizeof(arr)).from_buffer(arr)
        for j, (t, nb) in enumerate(zip(tasks, nonces)):  # (packed: a field at a time costs 4096 tasks milliseconds)
            _SCAN_TASK_IN.pack_into(raw, j * _SCAN_TASK.size, addr, len(nb), t.num_trailing_zeros, t.worker_byte,
                                    t.worker_bits, t.k_begin, t.k_end)
            addr += len(nb)
        hits_c = (_lib.ScanHitC * max(max_hits, 1))()
        cnt, st = ctypes.c_size_t(), _lib.BatchStats()
        check(lib().dpow_scan_batch(self._ctx, arr, n, hits_c, max_hits, ctypes.byref(cnt), ctypes.byref(st)),
              "dpow_scan_batch")
        self.last_scan_many_stats = st
        hits = [ScanHit(g, tz, sec[:slen])
                for g, tz, slen, sec in _SCAN_HIT.iter_unpack(ctypes.string_at(hits_c, cnt.value * _SCAN_HIT.size))]
        return [(f[8], hits[f[9]:f[9] + f[10]], f[7])
                for f in _SCAN_TASK.iter_unpack(ctypes.string_at(arr, n * _SCAN_TASK.size))]

    def scan_many(self, tasks: Sequence[ScanTask], max_hits: int = _lib.SCAN_CAP) -> List[List[ScanHit]]:
        """`scan` for many windows at once (dpow_scan_batch, the unfinished tasks submitted again
        over MORE; max_hits is the page size): result i is what `scan` returns for tasks[i].  A
        raised cancel flag ends it early with the hits found so far (see `cancelled`)."""
        out: List[List[ScanHit]] = [[] for _ in tasks]
        todo = list(range(len(tasks)))
        k = [t.k_begin for t in tasks]
        while todo:
            batch = todo[:_lib.DPOW_BATCH_MAX]  # at most DPOW_BATCH_MAX tasks per call
            res = self.scan_batch([ScanTask(tasks[i].nonce, tasks[i].num_trailing_zeros, tasks[i].worker_byte,
                                            tasks[i].worker_bits, k[i], tasks[i].k_end) for i in batch], max_hits)
            for i, (r, hits, k_done) in zip(batch, res):
                out[i] += hits
                k[i] = k_done
            if any(r == CANCELLED for r, _, _ in res):
                break
            todo = [i for i, (r, _, _) in zip(batch, res) if r == _lib.MORE] + todo[len(batch):]
        return out

    # -- census -----------------------------------------------------------------
    def census_page(self, nonce: Sequence[int], worker_byte: int = 0, worker_bits: int = 0, k_begin: int = 0,
                    k_end: int = 1):
        """One dpow_census_window call: (status, census, k_done).  EXHAUSTED: the window is done;
        CANCELLED: `census` is the complete census of [k_begin, k_done) and the caller continues from
        k_done and merges.  The call's launch counts are kept in last_census_stats."""
        n = _b(nonce)
        c, k_done, st = _lib.CensusC(), ctypes.c_uint64(), _lib.BatchStats()
        r = check(lib().dpow_census_window(self._ctx, n, len(n), worker_byte, worker_bits, k_begin, k_end,
                                           ctypes.byref(c), ctypes.byref(k_done), ctypes.byref(st)),
                  "dpow_census_window")
        self.last_census_stats = st
        return r, Census._from_c(c), k_done.value

    def census(self, nonce: Sequence[int], worker_byte: int = 0, worker_bits: int = 0, k_begin: int = 0,
               k_end: int = 1) -> Census:
        """How deep the partition's window k in [k_begin, k_end) goes: for every depth d the number of
        candidates whose digest ends in at least d '0' characters and the first of them
        (dpow_census_window).  A raised cancel flag ends it early with the census of the part done
        (see `cancelled`; census_page tells how far it got)."""
        return self.census_page(nonce, worker_byte, worker_bits, k_begin, k_end)[1]

    def census_batch(self, tasks: Sequence[CensusTask]):
        """The census of many windows in one pass over the GPU (dpow_census_batch): one
        (status, census, k_done) per task, what census_page returns for it.  A raised cancel flag
        leaves the tasks not finished CANCELLED, each with the complete census of
        [k_begin, k_done).  The call's launch counts are kept in last_census_many_stats."""
        n = len(tasks)
        arr = (_lib.CensusTaskC * max(n, 1))()
        nonces = [_b(t.nonce) for t in tasks]
        buf = ctypes.create_string_buffer(b"".join(nonces), max(sum(map(len, nonces)), 1))  # alive for the call
        addr = ctypes.addressof(buf)
        raw = (ctypes.c_ubyte * ctypes.sizeof(arr)).from_buffer(arr)
        for j, (t, nb) in enumerate(zip(tasks, nonces)):  # (packed: a field at a time costs 4096 tasks milliseconds)
            _CENSUS_TASK_IN.pack_into(raw, j * _CENSUS_TASK.size, addr, len(nb), t.worker_byte, t.worker_bits,
                                      t.k_begin, t.k_end)
            addr += len(nb)
        st = _lib.BatchStats()
        check(lib().dpow_census_batch(self._ctx, arr, n, ctypes.byref(st)), "dpow_census_batch")
        self.last_census_many_stats = st
        D, out = _lib.CENSUS_DEPTHS, []
        for f in _CENSUS_TASK.iter_unpack(ctypes.string_at(arr, n * _CENSUS_TASK.size)):
            # (a census the library returns is self-consistent: its set firsts are depths 0..deepest)
            n_set = f[8 + 3 * D] + 1 if f[8] else 0
            out.append((f[7], Census(f[8:8 + D], f[8 + D:8 + D + n_set] + (None,) * (D - n_set),
                                     f[8 + 2 * D:8 + 3 * D], f[8 + 3 * D]), f[6]))
        return out

    def census_many(self, tasks: Sequence[CensusTask]) -> List[Census]:
        """`census` for many windows at once (dpow_census_batch): result i is what `census` returns
        for tasks[i]."""
        return [c for _, c, _ in self.census_batch(tasks)]

    # -- digests ----------------------------------------------------------------
    @staticmethod
    def _u64_list(indices):
        """(keep-alive object, address, n) of a list of global indices: a sequence of ints, or any
        contiguous buffer of 8-byte items (array('Q'), a uint64 array, packed little-endian bytes)."""
        try:
            mv = memoryview(indices)
        except TypeError:
            mv = memoryview(array.array("Q", indices))
        if not mv.contiguous or (mv.itemsize != 8 and (mv.itemsize != 1 or mv.nbytes % 8)):
            raise ValueError("digests: indices must be ints or a contiguous buffer of uint64")
        n = mv.nbytes // 8
        if n == 0:
            return None, None, 0
        raw = mv.cast("B")
        buf = (ctypes.c_uint8 * raw.nbytes).from_buffer_copy(raw) if raw.readonly else \
            (ctypes.c_uint8 * raw.nbytes).from_buffer(raw)
        return buf, ctypes.addressof(buf), n

    def digests(self, nonce: Sequence[int], indices, want_digests: bool = True, want_depths: bool = True):
        """(digests, depths) of the listed candidates of one nonce (dpow_digests): 16 bytes and one
        byte per entry, in the list's order -- the MD5 of nonce || secret_from_index(g) and its
        trailing '0' characters.  `indices` is a sequence of ints or any buffer of uint64, in any
        order, duplicates included.  An output not wanted is None.  A raised cancel flag ends the call
        early with the entries done so far (shorter outputs; last_digest_status is CANCELLED).  The
        call's launch counts are kept in last_digest_stats."""
        nb = _b(nonce)
        keep, addr, n = self._u64_list(indices)
        dig = ctypes.create_string_buffer(16 * n) if want_digests else None
        dep = ctypes.create_string_buffer(max(n, 1)) if want_depths else None
        done, st = ctypes.c_size_t(), _lib.BatchStats()
        if n == 0:  # (an empty list still goes through the call's argument checks)
            keep = ctypes.c_uint64()
            addr = ctypes.addressof(keep)
        r = check(lib().dpow_digests(self._ctx, nb, len(nb), addr, n, dig, dep, ctypes.byref(done), ctypes.byref(st)),
                  "dpow_digests")
        del keep
        self.last_digest_stats, self.last_digest_status = st, r
        m = done.value
        return (dig.raw[:16 * m] if want_digests else None, dep.raw[:m] if want_depths else None)

    def digests_cuda(self, nonce: Sequence[int], idx, strict: bool = True):
        """`digests` for a CUDA torch.int64 tensor of global indices on this context's device
        (dpow_digests_device): uint8 tensors of shape [n, 16] and [n] on the same device, nothing
        crossing to the host.  torch's current stream is synchronised before the call, and the outputs
        are complete on return.  The device cannot refuse a list up front: an entry beyond DPOW_K_LIMIT
        (a negative one included) reads depth 255 and a zero digest, and the call raises DpowError with
        code ERANGE -- or, with strict=False, returns the outputs so marked."""
        import torch
        if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 1):
            raise ValueError("digests_cuda: idx must be a one-dimensional CUDA torch.int64 tensor")
        if idx.device.index != self.device:
            raise ValueError(f"digests_cuda: idx is on {idx.device}, the context on device {self.device}")
        nb = _b(nonce)
        idx = idx.contiguous()
        n = idx.numel()
        dig = torch.empty((n, 16), dtype=torch.uint8, device=idx.device)
        dep = torch.empty((n,), dtype=torch.uint8, device=idx.device)
        st = _lib.BatchStats()
        self.last_digest_stats, self.last_digest_status = st, EXHAUSTED
        if n == 0:
            return dig, dep
        torch.cuda.current_stream(idx.device).synchronize()
        r = lib().dpow_digests_device(self._ctx, nb, len(nb), idx.data_ptr(), n, dig.data_ptr(), dep.data_ptr(),
                                      ctypes.byref(st))
        self.last_digest_status = r
        if not (r == _lib.ERANGE and not strict):
            check(r, "dpow_digests_device")
        return dig, dep

    # -- digests of many nonces -------------------------------------------------
    @staticmethod
    def _digest_tasks(tasks):
        """(array, keep-alive) of dpow_digest_task for anything with .nonce and .num_trailing_zeros."""
        n = len(tasks)
        arr = (_lib.DigestTaskC * max(n, 1))()
        nonces = [_b(t.nonce) for t in tasks]
        buf = ctypes.create_string_buffer(b"".join(nonces), max(sum(map(len, nonces)), 1))  # alive for the call
        addr = ctypes.addressof(buf)
        raw = (ctypes.c_ubyte * ctypes.sizeof(arr)).from_buffer(arr)
        for j, (t, nb) in enumerate(zip(tasks, nonces)):
            _DIGEST_TASK_IN.pack_into(raw, j * _DIGEST_TASK.size, addr, len(nb), t.num_trailing_zeros)
            addr += len(nb)
        return arr, buf

    @staticmethod
    def _digest_task_outs(arr, n):
        """([n_entries], [n_shallow]) of the first n task structs."""
        fields = list(_DIGEST_TASK.iter_unpack(ctypes.string_at(arr, n * _DIGEST_TASK.size)))
        return [f[3] for f in fields], [f[4] for f in fields]

    _DIGESTS_MANY_KEEP = 1 << 21  # entries: 50 MB of buffers at the most stay with the Miner

    def _digests_many_buffers(self, n):
        """(indices, digests, depths) for a dpow_digests_batch call of n entries.  Lists of up to
        _DIGESTS_MANY_KEEP entries reuse buffers kept with the Miner: the first touch of fresh pages
        cost a call of 2^20 entries more than its GPU work.  (The outputs are copied out per task.)"""
        kept = getattr(self, "_digests_many_kept", None)
        if kept is not None and kept[0] >= n:
            return kept[1:]
        cap = max(n, 1)
        made = (cap, (ctypes.c_uint64 * cap)(), ctypes.create_string_buffer(16 * cap), ctypes.create_string_buffer(cap))
        if cap <= self._DIGESTS_MANY_KEEP:
            self._digests_many_kept = made
        return made[1:]

    def digests_many(self, tasks: Sequence[DigestTask], want_digests: bool = True, want_depths: bool = True):
        """[(digests, depths), ...], one per task, each what Miner.digests returns for the task's nonce
        and indices (dpow_digests_batch: every task's list in one pass, more than DPOW_BATCH_MAX tasks
        split across calls).  With neither output wanted the call is a pure check.
        last_digest_many_shallow[i] is the number of task i's entries with a depth below its
        num_trailing_zeros, last_digest_many_stats the sums over the calls, last_digest_many_status the
        last call's status: a raised cancel flag ends it early (CANCELLED) with shorter or empty
        outputs for the tasks not done."""
        out, shallow, total = [], [], _lib.BatchStats()
        status = EXHAUSTED
        for at in range(0, len(tasks), _lib.DPOW_BATCH_MAX):
            part = tasks[at:at + _lib.DPOW_BATCH_MAX]
            if status != EXHAUSTED:  # cancelled: the tasks behind are not begun
                out += [(b"" if want_digests else None, b"" if want_depths else None) for _ in part]
                shallow += [0] * len(part)
                continue
            arr, keep = self._digest_tasks(part)
            lists = [self._u64_list(t.indices) for t in part]
            rows = (ctypes.c_uint64 * (len(part) + 1))()
            for j, (_, _, cnt) in enumerate(lists):
                rows[j + 1] = rows[j] + cnt
            n = rows[len(part)]
            idx, dig, dep = self._digests_many_buffers(n)
            for j, (_, addr, cnt) in enumerate(lists):
                if cnt:
                    ctypes.memmove(ctypes.addressof(idx) + 8 * rows[j], addr, 8 * cnt)
            dig, dep = dig if want_digests else None, dep if want_depths else None
            done, st = ctypes.c_size_t(), _lib.BatchStats()
            status = check(lib().dpow_digests_batch(self._ctx, arr, len(part), rows, idx, dig, dep, ctypes.byref(done),
                                                    ctypes.byref(st)), "dpow_digests_batch")
            del keep, lists
            total.launches += st.launches
            total.rounds += st.rounds
            total.candidates += st.candidates
            total.kernel_ms += st.kernel_ms
            m = done.value
            shallow += self._digest_task_outs(arr, len(part))[1]
            for j in range(len(part)):
                lo, hi = min(rows[j], m), min(rows[j + 1], m)
                out.append((ctypes.string_at(ctypes.addressof(dig) + 16 * lo, 16 * (hi - lo)) if want_digests else None,
                            ctypes.string_at(ctypes.addressof(dep) + lo, hi - lo) if want_depths else None))
        self.last_digest_many_shallow, self.last_digest_many_stats, self.last_digest_many_status = shallow, total, status
        return out

    def digests_many_cuda(self, tasks, idx, rows, want_digests: bool = True, want_depths: bool = True,
                          strict: bool = True):
        """(digests [n, 16], depths [n], shallow) of a CSR list on this context's device
        (dpow_digests_batch_device): `idx` is a CUDA torch.int64 tensor of n global indices and `rows` one
        of len(tasks) + 1 row pointers, entry e with rows[i] <= e < rows[i + 1] being a candidate of
        tasks[i].nonce -- what scan_many_cuda returns; `tasks` is any sequence with .nonce and
        .num_trailing_zeros, so scan_many_cuda's own ScanTask list passes straight through.  The
        outputs are uint8 tensors on the same device (None where not wanted), nothing crossing to the
        host but len(tasks) + 1 rows and `shallow`, the per-task counts of entries with a depth below
        the task's num_trailing_zeros.  An entry beyond DPOW_K_LIMIT reads depth 255 and a zero digest,
        and the call raises DpowError with code ERANGE -- or, with strict=False, returns the outputs so
        marked; an entry no row covers reads the same and always raises (EINVAL).  torch's current
        stream is synchronised before the call, and the outputs are complete on return."""
        import torch
        for name, t in (("idx", idx), ("rows", rows)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 1):
                raise ValueError(f"digests_many_cuda: {name} must be a one-dimensional CUDA torch.int64 tensor")
            if t.device.index != self.device:
                raise ValueError(f"digests_many_cuda: {name} is on {t.device}, the context on device {self.device}")
        if rows.numel() != len(tasks) + 1:
            raise ValueError("digests_many_cuda: rows must hold len(tasks) + 1 row pointers")
        if len(tasks) > _lib.DPOW_BATCH_MAX:
            raise ValueError("digests_many_cuda: more than DPOW_BATCH_MAX tasks")
        idx, rows = idx.contiguous(), rows.contiguous()
        n = idx.numel()
        dig = torch.empty((n, 16), dtype=torch.uint8, device=idx.device) if want_digests else None
        dep = torch.empty((n,), dtype=torch.uint8, device=idx.device) if want_depths else None
        arr, keep = self._digest_tasks(tasks)
        st = _lib.BatchStats()
        pad = idx if n else rows  # (an empty list still goes through the call's argument checks)
        torch.cuda.current_stream(idx.device).synchronize()
        r = lib().dpow_digests_batch_device(self._ctx, arr, len(tasks), rows.data_ptr(), pad.data_ptr(), n,
                                            dig.data_ptr() if want_digests and n else None,
                                            dep.data_ptr() if want_depths and n else None, ctypes.byref(st))
        del keep
        self.last_digest_many_stats, self.last_digest_many_status = st, r
        self.last_digest_many_entries, shallow = self._digest_task_outs(arr, len(tasks))
        self.last_digest_many_shallow = shallow
        if not (r == _lib.ERANGE and not strict):
            check(r, "dpow_digests_batch_device")
        return dig, dep, shallow

    # -- device scan ------------------------------------------------------------
    def scan_cuda_page(self, nonce: Sequence[int], num_trailing_zeros: int, worker_byte: int = 0,
                       worker_bits: int = 0, k_begin: int = 0, k_end: int = 1, max_hits: int = 1 << 20,
                       want_depths: bool = True):
        """One dpow_scan_device call: (status, idx, depths, k_done).  `idx` is a CUDA torch.int64
        tensor of the hits' global indices in increasing order and `depths` a torch.uint8 tensor of
        their depths (None unless want_depths), both on the context's device and of shape [n]: views
        of the filled part of the call's max_hits-entry buffers, nothing crossing to the host.
        EXHAUSTED: the window is done; MORE: these are all hits of [k_begin, k_done) and the caller
        continues from k_done; CANCELLED likewise.  torch's current stream is synchronised before the
        call, and the outputs are complete on return.  The call's launch counts are kept in
        last_scan_device_stats (rounds: the slices; launches: every kernel launch)."""
        import torch
        nb = _b(nonce)
        dev = torch.device("cuda", self.device)
        idx = torch.empty((max(max_hits, 1),), dtype=torch.int64, device=dev)
        dep = torch.empty((max(max_hits, 1),), dtype=torch.uint8, device=dev) if want_depths else None
        cnt, k_done, st = ctypes.c_size_t(), ctypes.c_uint64(), _lib.BatchStats()
        torch.cuda.current_stream(dev).synchronize()
        r = check(lib().dpow_scan_device(self._ctx, nb, len(nb), num_trailing_zeros, worker_byte, worker_bits,
                                         k_begin, k_end, idx.data_ptr(), dep.data_ptr() if want_depths else None,
                                         max_hits, ctypes.byref(cnt), ctypes.byref(k_done), ctypes.byref(st)),
                  "dpow_scan_device")
        self.last_scan_device_stats = st
        n = cnt.value
        return r, idx[:n], dep[:n] if want_depths else None, k_done.value

    def scan_cuda(self, nonce: Sequence[int], num_trailing_zeros: int, worker_byte: int = 0, worker_bits: int = 0,
                  k_begin: int = 0, k_end: int = 1, max_hits: int = 1 << 20, want_depths: bool = True):
        """(idx, depths) of every candidate of the partition over k in [k_begin, k_end) whose digest
        ends in at least num_trailing_zeros '0' characters, in increasing global index, as CUDA
        tensors (dpow_scan_device, paged over MORE and concatenated; max_hits is the page size).
        `depths` is None unless want_depths.  A raised cancel flag ends the scan early with the hits
        found so far (see `cancelled`; scan_cuda_page tells how far it got).  last_scan_device_stats
        holds the sums over the pages."""
        import torch
        idxs, deps, total = [], [], _lib.BatchStats()
        k = k_begin
        while True:
            r, idx, dep, k = self.scan_cuda_page(nonce, num_trailing_zeros, worker_byte, worker_bits, k, k_end,
                                                 max_hits, want_depths)
            st = self.last_scan_device_stats
            total.launches += st.launches
            total.rounds += st.rounds
            total.candidates += st.candidates
            total.kernel_ms += st.kernel_ms
            idxs.append(idx)
            deps.append(dep)
            if r != _lib.MORE:
                break
        self.last_scan_device_stats = total
        if len(idxs) == 1:
            return idxs[0], deps[0]
        return torch.cat(idxs), torch.cat(deps) if want_depths else None

    def scan_device_times(self):
        """(mask_ms, place_ms, depth_ms): the kernel time of the last dpow_scan_device call by kind
        (dpow_diag_scan_device_times)."""
        m, p, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(lib().dpow_diag_scan_device_times(self._ctx, ctypes.byref(m), ctypes.byref(p), ctypes.byref(d)),
              "dpow_diag_scan_device_times")
        return m.value, p.value, d.value

    # -- batched device scan ----------------------------------------------------
    def scan_batch_cuda(self, tasks: Sequence[ScanTask], max_hits: int = 1 << 20, want_depths: bool = True,
                        want_rows: bool = True):
        """One dpow_scan_batch_device call: (results, idx, depths, rows).  `results` is one
        (status, k_done) per task, as scan_batch's.  `idx` is a CUDA torch.int64 tensor of the hits'
        global indices, task after task and within a task in increasing order, `depths` a torch.uint8
        tensor of their depths (None unless want_depths) and `rows` a torch.int64 tensor of
        len(tasks) + 1 row pointers (None unless want_rows): task i's hits are
        idx[rows[i]:rows[i + 1]].  All are on the context's device, views of the call's buffers, no
        hit crossing to the host; last_scan_many_device_rows holds the rows as a host list, from the
        task structs.  The task that does not fit `max_hits` is MORE from its k_done, the tasks behind
        it MORE from their k_begin.  torch's current stream is synchronised before the call, and the
        outputs are complete on return.  The call's launch counts are kept in
        last_scan_many_device_stats (rounds: the mask launches; launches: every kernel launch)."""
        import torch
        n = len(tasks)
        arr = (_lib.ScanTaskC * max(n, 1))()
        nonces = [_b(t.nonce) for t in tasks]
        buf = ctypes.create_string_buffer(b"".join(nonces), max(sum(map(len, nonces)), 1))  # alive for the call
        addr = ctypes.addressof(buf)
        raw = (ctypes.c_ubyte * ctypes.sizeof(arr)).from_buffer(arr)
        for j, (t, nb) in enumerate(zip(tasks, nonces)):
            _SCAN_TASK_IN.pack_into(raw, j * _SCAN_TASK.size, addr, len(nb), t.num_trailing_zeros, t.worker_byte,
                                    t.worker_bits, t.k_begin, t.k_end)
            addr += len(nb)
        dev = torch.device("cuda", self.device)
        idx = torch.empty((max(max_hits, 1),), dtype=torch.int64, device=dev)
        dep = torch.empty((max(max_hits, 1),), dtype=torch.uint8, device=dev) if want_depths else None
        rows = torch.empty((n + 1,), dtype=torch.int64, device=dev) if want_rows else None
        cnt, st = ctypes.c_size_t(), _lib.BatchStats()
        torch.cuda.current_stream(dev).synchronize()
        check(lib().dpow_scan_batch_device(self._ctx, arr, n, idx.data_ptr(), dep.data_ptr() if want_depths else None,
                                           rows.data_ptr() if want_rows else None, max_hits, ctypes.byref(cnt),
                                           ctypes.byref(st)), "dpow_scan_batch_device")
        self.last_scan_many_device_stats = st
        fields = list(_SCAN_TASK.iter_unpack(ctypes.string_at(arr, n * _SCAN_TASK.size)))
        self.last_scan_many_device_rows = [f[9] for f in fields] + [cnt.value]
        return ([(f[8], f[7]) for f in fields], idx[:cnt.value], dep[:cnt.value] if want_depths else None, rows)

    def scan_many_cuda(self, tasks: Sequence[ScanTask], max_hits: int = 1 << 20, want_depths: bool = True):
        """(idx, depths, rows) of every hit of many windows as CUDA tensors (dpow_scan_batch_device,
        the unfinished tasks submitted again from their k_done over MORE and the pages concatenated
        per task; max_hits is the page size): idx[rows[i]:rows[i + 1]] and the same slice of `depths`
        (None unless want_depths) are what scan_cuda returns for tasks[i].  A raised cancel flag ends
        it early with the hits found so far (see `cancelled`).  last_scan_many_device_stats holds the
        sums over the calls."""
        import torch
        dev = torch.device("cuda", self.device)
        total = _lib.BatchStats()
        todo = list(range(len(tasks)))
        k = [t.k_begin for t in tasks]
        pages = []  # (the call's tasks, its idx, its depths, its rows on the host)
        first = None
        while todo:
            batch = todo[:_lib.DPOW_BATCH_MAX]  # at most DPOW_BATCH_MAX tasks per call
            out = self.scan_batch_cuda(
                [ScanTask(tasks[i].nonce, tasks[i].num_trailing_zeros, tasks[i].worker_byte, tasks[i].worker_bits,
                          k[i], tasks[i].k_end) for i in batch], max_hits, want_depths)
            res, idx, dep, rows = out
            first = first or out
            st = self.last_scan_many_device_stats
            total.launches += st.launches
            total.rounds += st.rounds
            total.candidates += st.candidates
            total.kernel_ms += st.kernel_ms
            pages.append((batch, idx, dep, self.last_scan_many_device_rows))
            for j, i in enumerate(batch):
                k[i] = res[j][1]
            if any(r == CANCELLED for r, _ in res):
                break
            todo = [i for i, (r, _) in zip(batch, res) if r == _lib.MORE] + todo[len(batch):]
        self.last_scan_many_device_stats = total
        if len(pages) == 1 and len(pages[0][0]) == len(tasks):  # one call did everything: its own outputs
            return first[1], first[2], first[3]
        seg_idx: List[list] = [[] for _ in tasks]
        seg_dep: List[list] = [[] for _ in tasks]
        counts = [0] * len(tasks)
        for batch, idx, dep, r_host in pages:
            for j, i in enumerate(batch):
                if r_host[j + 1] > r_host[j]:
                    seg_idx[i].append(idx[r_host[j]:r_host[j + 1]])
                    if want_depths:
                        seg_dep[i].append(dep[r_host[j]:r_host[j + 1]])
                    counts[i] += r_host[j + 1] - r_host[j]
        row_list = [0]
        for c in counts:
            row_list.append(row_list[-1] + c)
        flat_idx = [s for segs in seg_idx for s in segs]
        flat_dep = [s for segs in seg_dep for s in segs]
        idx_all = torch.cat(flat_idx) if flat_idx else torch.empty((0,), dtype=torch.int64, device=dev)
        dep_all = None
        if want_depths:
            dep_all = torch.cat(flat_dep) if flat_dep else torch.empty((0,), dtype=torch.uint8, device=dev)
        return idx_all, dep_all, torch.tensor(row_list, dtype=torch.int64, device=dev)

    # -- measurement ------------------------------------------------------------
    def stats(self) -> Stats:
        s = Stats()
        check(lib().dpow_get_stats(self._ctx, ctypes.byref(s)), "dpow_get_stats")
        return s

    def reset_stats(self):
        lib().dpow_reset_stats(self._ctx)

    def stream_handle(self) -> int:
        return lib().dpow_stream(self._ctx) or 0

    def geometry(self):
        cus, bpc, tpb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().dpow_geometry(self._ctx, ctypes.byref(cus), ctypes.byref(bpc), ctypes.byref(tpb)),
              "dpow_geometry")
        return cus.value, bpc.value, tpb.value
