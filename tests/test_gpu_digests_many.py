"""GPU: the digests of many nonces (dpow_digests_batch, dpow_digests_batch_device, Miner.digests_many,
Miner.digests_many_cuda) -- the MD5 and the depth of a list in CSR order over many tasks.

Every assertion is equality with something that does not come from digest_many_kernel: hashlib over
all 16 bytes of the seam list (tests/_digests_many_cases.py: seams after lane 0, 62 and 63 of a wave,
on step and workgroup boundaries, runs of empty tasks, 130 tasks of one entry), Miner.digests and
Miner.digests_cuda per task, the committed fixtures, and the batched device scan whose rows and hits
the call takes over without their leaving the GPU.

Each test prints its time (pytest -s).
"""
import ctypes
import hashlib
import json
import os
import time

import pytest

import distpow
from distpow import CANCELLED, DPOW_K_LIMIT, EINVAL, ERANGE, EXHAUSTED, DigestTask, ScanTask
from distpow import _lib

from _digests_many_cases import E, hashlib_of, nonce_of, rows_of, seam_list, secret_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_SEAM = {}


def _seam():
    """The seam list, its rows and hashlib's answer per task, computed once."""
    if not _SEAM:
        nonces, lists = seam_list()
        _SEAM.update(nonces=nonces, lists=lists, rows=rows_of([len(x) for x in lists]),
                     ref=[hashlib_of(n, x) for n, x in zip(nonces, lists)])
    return _SEAM


def _shallow(ref, ntz):
    return [sum(1 for d in dep if d < ntz) for _, dep in ref]


def _bytes(t):
    return bytes(t.cpu().flatten().tolist())


def _cuda(miner, values):
    import torch
    return torch.tensor(values, dtype=torch.int64, device=torch.device("cuda", miner.device))


class _T:
    """A task as digests_many_cuda takes it: anything with .nonce and .num_trailing_zeros."""

    def __init__(self, nonce, ntz=0):
        self.nonce, self.num_trailing_zeros = nonce, ntz


def test_seam_list_equals_hashlib_host_and_device_forms(miner):
    s = _seam()
    assert 180 <= len(s["lists"]) <= 200 and s["lists"][0] == [] and s["lists"][60] == [] and s["lists"][59] == []
    tasks = [DigestTask(n, x, 1) for n, x in zip(s["nonces"], s["lists"])]
    t = time.perf_counter()
    got = miner.digests_many(tasks)
    t_host = time.perf_counter() - t
    assert got == s["ref"]
    assert miner.last_digest_many_shallow == _shallow(s["ref"], 1)
    st = miner.last_digest_many_stats
    assert (st.launches, st.candidates, miner.last_digest_many_status) == (1, s["rows"][-1], EXHAUSTED)
    # each task's slice is what Miner.digests returns for it
    for task, g in zip(tasks[:64:3], got[:64:3]):
        assert miner.digests(task.nonce, task.indices) == g
    # either output alone
    assert miner.digests_many(tasks, want_depths=False) == [(d, None) for d, _ in s["ref"]]
    assert miner.digests_many(tasks, want_digests=False) == [(None, z) for _, z in s["ref"]]
    # the same list uploaded, through the device form
    idx = _cuda(miner, [g for x in s["lists"] for g in x])
    rows = _cuda(miner, s["rows"])
    t = time.perf_counter()
    dig, dep, shallow = miner.digests_many_cuda(tasks, idx, rows)
    t_dev = time.perf_counter() - t
    assert _bytes(dig) == b"".join(d for d, _ in s["ref"]) and _bytes(dep) == b"".join(z for _, z in s["ref"])
    assert shallow == _shallow(s["ref"], 1)
    assert miner.last_digest_many_entries == [len(x) for x in s["lists"]]
    assert (miner.last_digest_many_stats.launches, miner.last_digest_many_stats.candidates) == (1, s["rows"][-1])
    print(f"{len(tasks)} tasks, {s['rows'][-1]} entries: host form {t_host * 1e3:.2f} ms, device form {t_dev * 1e3:.2f} ms")


def test_chunk_seams_change_nothing(miner, monkeypatch):
    """DPOW_DIAG_DIGEST_CHUNK=256: chunk seams inside tasks and on task boundaries, both buffer sets
    reused; outputs and n_shallow are the single-chunk run's."""
    s = _seam()
    tasks = [DigestTask(n, x, 1) for n, x in zip(s["nonces"], s["lists"])]
    monkeypatch.delenv("DPOW_DIAG_DIGEST_CHUNK", raising=False)
    one = miner.digests_many(tasks)
    one_shallow = miner.last_digest_many_shallow
    monkeypatch.setenv("DPOW_DIAG_DIGEST_CHUNK", "256")
    t = time.perf_counter()
    cut = miner.digests_many(tasks)
    dt = time.perf_counter() - t
    assert cut == one == s["ref"] and miner.last_digest_many_shallow == one_shallow == _shallow(s["ref"], 1)
    assert miner.last_digest_many_stats.launches == -(-s["rows"][-1] // 256)
    monkeypatch.setenv("DPOW_DIAG_DIGEST_STAGING", "copy")
    assert miner.digests_many(tasks) == one and miner.last_digest_many_shallow == one_shallow
    print(f"{miner.last_digest_many_stats.launches} chunks of 256 in {dt * 1e3:.2f} ms")


def test_check_only_mode(miner):
    """Both outputs NULL: n_shallow equals the count from a run with depths."""
    s = _seam()
    for ntz in (1, 2):
        tasks = [DigestTask(n, x, ntz) for n, x in zip(s["nonces"], s["lists"])]
        assert miner.digests_many(tasks, want_digests=False, want_depths=False) == [(None, None)] * len(tasks)
        assert miner.last_digest_many_shallow == _shallow(s["ref"], ntz), ntz
        assert miner.last_digest_many_stats.candidates == s["rows"][-1]
    idx, rows = _cuda(miner, [g for x in s["lists"] for g in x]), _cuda(miner, s["rows"])
    dig, dep, shallow = miner.digests_many_cuda(tasks, idx, rows, want_digests=False, want_depths=False)
    assert (dig, dep, shallow) == (None, None, _shallow(s["ref"], 2))


def test_golden_fixture_entries_in_one_call(miner, golden):
    """Every entry of tests/golden/pow_golden.json with an index, grouped by nonce, in one call."""
    entries = [e for key in ("first_hits", "partitions", "windows", "nonce_lengths", "deep_hits")
               for e in golden[key]]
    by_nonce = {}
    for e in entries:
        assert bytes(e["secret"]) == secret_of(e["global_idx"])
        by_nonce.setdefault(tuple(e["nonce"]), []).append(e)
    t = time.perf_counter()
    got = miner.digests_many([DigestTask(n, [e["global_idx"] for e in es]) for n, es in by_nonce.items()])
    dt = time.perf_counter() - t
    assert miner.last_digest_many_stats.launches == 1
    for (nonce, es), (dig, dep) in zip(by_nonce.items(), got):
        for j, e in enumerate(es):
            md5 = e.get("md5") or hashlib.md5(bytes(nonce) + bytes(e["secret"])).hexdigest()
            assert dig[16 * j:16 * j + 16].hex() == md5, e
            assert dep[j] >= e["ntz"] and dep[j] == 32 - len(md5.rstrip("0")), e
    print(f"{len(entries)} entries of {len(by_nonce)} nonces in {dt * 1e3:.2f} ms")


def test_layout_deep_hits_in_one_call(miner):
    """Every layout of tests/golden/layout_deep_hits.json as one task each, in one call: mixed layouts
    at every seam; the depths are the CPU-scanned list's, each held against its own N."""
    with open(os.path.join(GOLDEN, "layout_deep_hits.json")) as f:
        cases = json.load(f)["cases"]
    tasks = [DigestTask(c["nonce"], [g for g, _ in c["hits"]], min(tz for _, tz in c["hits"]) if c["hits"] else 0)
             for c in cases]
    t = time.perf_counter()
    got = miner.digests_many(tasks)
    dt = time.perf_counter() - t
    assert len(tasks) >= 72 and miner.last_digest_many_stats.launches == 1
    assert miner.last_digest_many_shallow == [0] * len(tasks)
    for c, (dig, dep) in zip(cases, got):
        assert list(dep) == [tz for _, tz in c["hits"]], c["name"]
        assert (dig, dep) == hashlib_of(c["nonce"], [g for g, _ in c["hits"]]), c["name"]
    print(f"{sum(len(c['hits']) for c in cases)} hits of {len(cases)} layouts in {dt * 1e3:.2f} ms")


def _chain_tasks():
    readme = [ScanTask([1, 2, 3, 4], 6, k_end=1 << 16), ScanTask([5, 6, 7, 8], 2, 5, 3, 0, 100)]
    dozen = [ScanTask(nonce_of(n, salt=90 + j), 2, k_end=16)
             for j, n in enumerate([0, 3, 4, 7, 47, 48, 55, 56, 59, 63, 64, 130])]
    none = lambda j: ScanTask(nonce_of(5, salt=j), 33, k_end=16)  # N = 33: no candidate can hit
    return readme, [none(0)] + dozen[:6] + [none(1), none(2)] + dozen[6:] + [none(3)]


@pytest.mark.parametrize("which", ["readme", "dozen"])
def test_chaining_behind_the_batched_device_scan(miner, which):
    """scan_many_cuda, then digests_many_cuda(tasks, idx, rows) with the rows never leaving the device:
    the depths are the scan's, the digests hashlib's, nothing is shallow; with every ntz raised by one,
    shallow[i] counts task i's entries whose depth is exactly the old ntz."""
    tasks = _chain_tasks()[which == "dozen"]
    t = time.perf_counter()
    idx, dep_scan, rows = miner.scan_many_cuda(tasks)
    dig, dep, shallow = miner.digests_many_cuda(tasks, idx, rows)
    dt = time.perf_counter() - t
    import torch
    assert torch.equal(dep, dep_scan) and shallow == [0] * len(tasks)
    h_idx, h_rows, h_dep = idx.tolist(), rows.tolist(), dep.tolist()
    assert h_rows[-1] == len(h_idx) > 0 and miner.last_digest_many_entries == [b - a for a, b in zip(h_rows, h_rows[1:])]
    if which == "dozen":
        assert [miner.last_digest_many_entries[j] for j in (0, 7, 8, 15)] == [0, 0, 0, 0]
        assert all(miner.last_digest_many_entries[j] > 0 for j in (1, 6, 9, 14))
    want = b"".join(hashlib_of(t_.nonce, h_idx[a:b])[0] for t_, a, b in zip(tasks, h_rows, h_rows[1:]))
    assert _bytes(dig) == want
    raised = [_T(t_.nonce, t_.num_trailing_zeros + 1) for t_ in tasks]
    dig2, dep2, shallow2 = miner.digests_many_cuda(raised, idx, rows, want_digests=False)
    assert dig2 is None and torch.equal(dep2, dep)
    assert shallow2 == [sum(1 for d in h_dep[a:b] if d == t_.num_trailing_zeros)
                        for t_, a, b in zip(tasks, h_rows, h_rows[1:])]
    assert sum(shallow2) > 0
    print(f"{which}: {len(h_idx)} hits of {len(tasks)} tasks scanned and hashed again in {dt * 1e3:.2f} ms")


@pytest.mark.parametrize("lengths", [(2**20 + 300, 0, 2**20 + 400, 77), (2**24 - 5, 1005)])
def test_multi_step_workgroups_and_launch_seams(miner, lengths):
    """Sequential indices, device form, against digests_cuda per segment: workgroups of more than one
    step with seams in the middle of a step; and two launches, a non-zero e_base, the seam five
    entries before the launch boundary."""
    import torch
    dev = torch.device("cuda", miner.device)
    rows_h = rows_of(lengths)
    n = rows_h[-1]
    idx = torch.arange(n, dtype=torch.int64, device=dev) * 3 + 1
    tasks = [_T(nonce_of(nl, salt=j), 1) for j, nl in zip(range(len(lengths)), (60, 4, 55, 130))]
    t = time.perf_counter()
    dig, dep, shallow = miner.digests_many_cuda(tasks, idx, _cuda(miner, rows_h))
    dt = time.perf_counter() - t
    assert miner.last_digest_many_stats.launches == -(-n // 2**24)
    for j, (a, b) in enumerate(zip(rows_h, rows_h[1:])):
        want_dig, want_dep = miner.digests_cuda(tasks[j].nonce, idx[a:b])
        assert torch.equal(dig[a:b], want_dig) and torch.equal(dep[a:b], want_dep), j
        assert shallow[j] == int((want_dep < 1).sum().item()), j
    print(f"{lengths}: {n} entries in {dt * 1e3:.2f} ms, {miner.last_digest_many_stats.launches} launches")


def _raw_device(miner, tasks, idx, rows, n=None):
    """dpow_digests_batch_device on pre-filled outputs: (code, digests, depths, the task structs)."""
    import torch
    n = idx.numel() if n is None else n
    dig = torch.full((idx.numel(), 16), 0xA5, dtype=torch.uint8, device=idx.device)
    dep = torch.full((idx.numel(),), 0xA5, dtype=torch.uint8, device=idx.device)
    arr, keep = miner._digest_tasks(tasks)
    torch.cuda.current_stream(idx.device).synchronize()
    rc = distpow.lib().dpow_digests_batch_device(miner._ctx, arr, len(tasks), rows.data_ptr(), idx.data_ptr(), n,
                                                 dig.data_ptr(), dep.data_ptr(), None)
    return rc, _bytes(dig), _bytes(dep), arr


def test_uncovered_entries_are_marked_and_refused(miner):
    """rows[n_tasks] < n, and rows[0] > 0: the call returns EINVAL, the entries no row covers read
    0xFF and a zero digest, the covered ones are right.  (In-bounds cases only.)"""
    s = _seam()
    nonces, lists = s["nonces"][1:20], s["lists"][1:20]
    tasks = [_T(n) for n in nonces]
    flat = [g for x in lists for g in x]
    ref_dig = b"".join(hashlib_of(n, x)[0] for n, x in zip(nonces, lists))
    ref_dep = b"".join(hashlib_of(n, x)[1] for n, x in zip(nonces, lists))
    rows_h = rows_of([len(x) for x in lists])
    total = rows_h[-1]
    # 70 entries behind the last row
    idx = _cuda(miner, flat + E[:25] + E)
    rc, dig, dep, arr = _raw_device(miner, tasks, idx, _cuda(miner, rows_h))
    assert rc == EINVAL and "outside" in _lib.last_error()
    assert (dig[:16 * total], dep[:total]) == (ref_dig, ref_dep)
    assert dep[total:] == b"\xff" * 70 and dig[16 * total:] == bytes(16 * 70)
    # 70 entries below the first row, and 3 behind the last
    idx = _cuda(miner, E[:25] + E + flat + E[:3])
    rc, dig, dep, arr = _raw_device(miner, tasks, idx, _cuda(miner, [r + 70 for r in rows_h]))
    assert rc == EINVAL
    assert (dig[16 * 70:16 * (70 + total)], dep[70:70 + total]) == (ref_dig, ref_dep)
    assert dep[:70] + dep[70 + total:] == b"\xff" * 73 and dig[:16 * 70] + dig[16 * (70 + total):] == bytes(16 * 73)
    assert [arr[j].n_entries for j in range(len(tasks))] == [len(x) for x in lists]
    # the counts are per call: the covered list alone is good
    rc, dig, dep, arr = _raw_device(miner, tasks, _cuda(miner, flat), _cuda(miner, rows_h))
    assert (rc, dig, dep) == (EXHAUSTED, ref_dig, ref_dep)
    # n below rows[n_tasks]: the caller's n bounds the call
    rc, dig, dep, arr = _raw_device(miner, tasks, _cuda(miner, flat), _cuda(miner, rows_h), n=100)
    assert (rc, dig[:1600], dep[:100]) == (EXHAUSTED, ref_dig[:1600], ref_dep[:100])
    assert dep[100:] == b"\xa5" * (total - 100)


def test_errors_cancel_and_ordering(miner):
    import torch
    s = _seam()
    nonces, lists = s["nonces"][1:9], s["lists"][1:9]
    ref = [hashlib_of(n, x) for n, x in zip(nonces, lists)]
    rows_h = rows_of([len(x) for x in lists])
    flat = [g for x in lists for g in x]
    tasks = [DigestTask(n, x) for n, x in zip(nonces, lists)]
    # an out-of-range index in the middle: the host form refuses the list, the device form marks the entry
    at = rows_h[4] + 3
    bad_lists = [list(x) for x in lists]
    bad_lists[4][3] = DPOW_K_LIMIT << 8
    with pytest.raises(distpow.DpowError) as e:
        miner.digests_many([DigestTask(n, x) for n, x in zip(nonces, bad_lists)])
    assert e.value.code == ERANGE
    idx, rows = _cuda(miner, flat[:at] + [-1] + flat[at + 1:]), _cuda(miner, rows_h)
    with pytest.raises(distpow.DpowError) as e:
        miner.digests_many_cuda(tasks, idx, rows)
    assert e.value.code == ERANGE
    dig, dep, _ = miner.digests_many_cuda(tasks, idx, rows, strict=False)
    assert miner.last_digest_many_status == ERANGE
    dig, dep = _bytes(dig), _bytes(dep)
    want_dig, want_dep = b"".join(d for d, _ in ref), b"".join(z for _, z in ref)
    assert dep[at] == 255 and dig[16 * at:16 * at + 16] == bytes(16)
    assert dep[:at] + dep[at + 1:] == want_dep[:at] + want_dep[at + 1:]
    assert dig[:16 * at] + dig[16 * at + 16:] == want_dig[:16 * at] + want_dig[16 * at + 16:]
    # a context with a node slot attached is refused
    class Slot(ctypes.Structure):
        """dpow_node_slot (include/dpow.h)."""
        _fields_ = [("best", ctypes.c_uint64), ("stop", ctypes.c_uint32), ("pad", ctypes.c_uint32 * 13)]

    slot = Slot()
    distpow.lib().dpow_node_slot_reset(ctypes.addressof(slot))
    miner.attach_node(ctypes.addressof(slot))
    try:
        with pytest.raises(distpow.DpowError) as e:
            miner.digests_many(tasks)
        assert e.value.code == EINVAL
    finally:
        miner.attach_node(None)
    # a cancel flag raised on entry: no launch, nothing done; cleared, the same call succeeds
    miner.cancel()
    try:
        assert miner.digests_many(tasks) == [(b"", b"")] * len(tasks)
        assert miner.last_digest_many_status == CANCELLED and miner.last_digest_many_stats.launches == 0
    finally:
        miner.clear_cancel()
    # digests before and after digests_many on one context, and the device forms likewise
    assert miner.digests(nonces[2], lists[2]) == ref[2]
    assert miner.digests_many(tasks) == ref and miner.last_digest_many_status == EXHAUSTED
    assert miner.digests(nonces[5], lists[5]) == ref[5]
    good = _cuda(miner, flat)
    a, b = rows_h[2], rows_h[3]
    d1, z1 = miner.digests_cuda(nonces[2], good[a:b].clone())
    dig, dep, _ = miner.digests_many_cuda(tasks, good, rows)
    d2, z2 = miner.digests_cuda(nonces[2], good[a:b].clone())
    assert torch.equal(d1, d2) and torch.equal(z1, z2) and torch.equal(dig[a:b], d1) and torch.equal(dep[a:b], z1)
    assert (_bytes(dig), _bytes(dep)) == (want_dig, want_dep)
    # only empty tasks: no launch
    assert miner.digests_many([DigestTask(b"", []), DigestTask([1], [])]) == [(b"", b""), (b"", b"")]
    assert miner.last_digest_many_stats.launches == 0 and miner.last_digest_many_shallow == [0, 0]
