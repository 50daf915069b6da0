"""Host side of the digests of many nonces (dpow_digests_batch, dpow_digests_batch_device,
dpow_digests_batch_walk), no GPU needed: the entry points exist in the header, the library and the
binding within ABI 5, the argument errors that need no context come back as codes with the outputs
untouched, and the walk a wave of digest_many_kernel makes over the rows -- the same code compiled
for the host -- is the specification's for every wave of the seam list and stays in bounds and
finite for arbitrary rows, descending ones included (the only place those are exercised)."""
import ctypes
import os
import random
import re
import subprocess

import distpow
from distpow import EINVAL, ERANGE, _lib

from _digests_many_cases import rows_of, seam_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_have_the_entry_points():
    header = open(os.path.join(ROOT, "include", "dpow.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = set(re.findall(r"\b(dpow_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", distpow.LIB_PATH]).decode()
    exported = set(re.findall(r"\s[TW]\s+(dpow_[a-z0-9_]+)$", out, flags=re.M))
    L = distpow.lib()
    for sym in ("dpow_digests_batch", "dpow_digests_batch_device", "dpow_digests_batch_walk"):
        assert sym in names and sym in exported, sym
        assert getattr(L, sym).argtypes is not None
    assert L.dpow_abi_version() == 5 and re.search(r"#define\s+DPOW_ABI_VERSION\s+5\b", header)
    assert "DigestTask" in distpow.__all__ and "digests_batch_walk" in distpow.__all__
    assert callable(distpow.Miner.digests_many) and callable(distpow.Miner.digests_many_cuda)
    t = distpow.DigestTask([1, 2, 3, 4], [5, 6])
    assert (t.nonce, t.indices, t.num_trailing_zeros) == ([1, 2, 3, 4], [5, 6], 0)
    # the struct as the header lays it out
    assert ctypes.sizeof(_lib.DigestTaskC) == 40 and _lib.DigestTaskC.n_shallow.offset == 32
    assert ctypes.sizeof(_lib.DigestPassC) == 24


def _tasks(nonces):
    arr = (_lib.DigestTaskC * max(len(nonces), 1))()
    keep = [ctypes.create_string_buffer(bytes(n), max(len(n), 1)) for n in nonces]
    for j, (n, k) in enumerate(zip(nonces, keep)):
        arr[j].nonce, arr[j].nonce_len, arr[j].ntz = ctypes.addressof(k), len(n), 1
        arr[j].n_entries = arr[j].n_shallow = 0xA5A5
    return arr, keep


def test_argument_errors_before_any_context_is_used():
    """Every call passes a NULL context: what comes back is the call's own error, decided first."""
    L = distpow.lib()
    arr, keep = _tasks([b"\x01\x02", b"", b"\x03"])
    rows = (ctypes.c_uint64 * 4)(0, 2, 2, 4)
    idx = (ctypes.c_uint64 * 4)(0, 1, 2, 3)
    dig, dep = ctypes.create_string_buffer(b"\xa5" * 64), ctypes.create_string_buffer(b"\xa5" * 4)
    done = ctypes.c_size_t(12345)

    def call(tasks=arr, n=3, rows=rows, idx=idx, done=ctypes.byref(done)):
        return L.dpow_digests_batch(None, tasks, n, rows, idx, dig, dep, done, None)

    def untouched():
        return (dig.raw[:64] == b"\xa5" * 64 and dep.raw[:4] == b"\xa5" * 4 and done.value == 12345 and
                all(arr[j].n_entries == 0xA5A5 and arr[j].n_shallow == 0xA5A5 for j in range(3)))

    for kw in (dict(tasks=None), dict(rows=None), dict(idx=None), dict(done=None)):
        assert call(**kw) == EINVAL and "NULL argument" in _lib.last_error(), kw
    for n in (0, _lib.DPOW_BATCH_MAX + 1):
        assert call(n=n) == EINVAL and "n_tasks" in _lib.last_error(), n
    assert call(rows=(ctypes.c_uint64 * 4)(1, 2, 2, 4)) == EINVAL and "rows[0]" in _lib.last_error()
    assert call(rows=(ctypes.c_uint64 * 4)(0, 3, 2, 4)) == EINVAL and "descending" in _lib.last_error()
    for at in range(4):
        bad = (ctypes.c_uint64 * 4)(0, 1, 2, 3)
        bad[at] = distpow.DPOW_K_LIMIT << 8
        assert call(idx=bad) == ERANGE and "DPOW_K_LIMIT" in _lib.last_error(), at
    # an entry behind rows[n_tasks] is not the call's
    tail = (ctypes.c_uint64 * 4)(0, 1, 2, 2**64 - 1)
    assert call(rows=(ctypes.c_uint64 * 4)(0, 2, 2, 3), idx=tail) == EINVAL and "ctx is NULL" in _lib.last_error()
    # a nonce: NULL with a length, and one too long
    arr[1].nonce, arr[1].nonce_len = None, 4
    assert call() == EINVAL and "nonce is NULL" in _lib.last_error()
    arr[1].nonce_len = 0
    arr[2].nonce_len = _lib.DPOW_MAX_NONCE + 1
    assert call() == EINVAL and "DPOW_MAX_NONCE" in _lib.last_error()
    arr[2].nonce_len = 1
    # the call itself is sound: only the context is missing
    assert call() == EINVAL and "ctx is NULL" in _lib.last_error()
    assert untouched()

    # the device form: NULLs, the misaligned pointers of dpow_digests_device (and the rows'), n_tasks
    def dev(tasks=arr, n=3, d_rows=4096, d_idx=8192, d_dig=16384):
        return L.dpow_digests_batch_device(None, tasks, n, d_rows, d_idx, 4, d_dig, None, None)

    for kw in (dict(tasks=None), dict(d_rows=None), dict(d_idx=None)):
        assert dev(**kw) == EINVAL and "NULL argument" in _lib.last_error(), kw
    for kw in (dict(d_rows=4100), dict(d_idx=8196), dict(d_dig=16392)):
        assert dev(**kw) == EINVAL and "aligned" in _lib.last_error(), kw
    for n in (0, _lib.DPOW_BATCH_MAX + 1):
        assert dev(n=n) == EINVAL and "n_tasks" in _lib.last_error(), n
    assert dev(d_dig=None) == EINVAL and "ctx is NULL" in _lib.last_error()  # (both outputs may be NULL)
    assert "dpow_digests_batch_device" in _lib.last_error()
    assert untouched()


def _spec(rows, e_first, e_end):
    """The passes of a wave by the specification, for rows that do not descend: every task whose
    segment meets the wave's positions, in order."""
    out = []
    for t in range(len(rows) - 1):
        lo, hi = max(rows[t], e_first), min(rows[t + 1], e_end)
        if lo < hi:
            out.append((t, lo, hi))
    return out


def _restated(rows, e_first, e_end):
    """The walk restated: the task of the first position by bisection (a first look at the next row
    spares it), then forward while rows begin below the wave's end."""
    n = len(rows) - 1
    a, b = 0, n
    if not (a + 1 < n and rows[a + 1] > e_first):
        while b - a > 1:
            mid = a + (b - a) // 2
            if rows[mid] <= e_first:
                a = mid
            else:
                b = mid
    out, r0 = [], rows[a]
    for t in range(a, n):
        if r0 >= e_end:
            break
        r1 = rows[t + 1]
        lo, hi = max(r0, e_first), min(r1, e_end)
        if lo < hi:
            out.append((t, lo, hi))
        if r1 >= e_end:
            break
        r0 = r1
    return out


def test_walk_of_the_seam_list_at_every_wave_offset():
    """A wave of 64 (and a ragged one of 17) placed at every position of the seam list, and beyond
    both ends of lists that begin above 0: the passes are the specification's."""
    rows = rows_of(seam_lengths())
    n = rows[-1]
    assert len(rows) - 1 >= 180 and rows[1] == 0 and rows[-3] == rows[-2] - 1
    most = 0
    for e in range(0, n + 70):
        for width in (64, 17):
            got = distpow.digests_batch_walk(rows, e, e + width)
            assert got == _spec(rows, e, e + width) == _restated(rows, e, e + width), (e, width)
            most = max(most, len(got))
    assert most == 64  # the worst case is there: 64 tasks of one entry in one wave
    shifted = [r + 100 for r in rows]  # rows[0] > 0: the positions below it are nobody's
    for e in list(range(0, 300)) + list(range(n, n + 200)):
        assert distpow.digests_batch_walk(shifted, e, e + 64) == _spec(shifted, e, e + 64), e
    assert distpow.digests_batch_walk(shifted, 0, 64) == []
    assert distpow.digests_batch_walk(shifted, 90, 154) == [(1, 100, 101), (5, 101, 154)]
    # a workgroup's launch cut: the wave ends where the launch does
    assert distpow.digests_batch_walk(rows, 60, 63) == [(5, 60, 63)]
    # one task and 4096 tasks
    assert distpow.digests_batch_walk([0, 1000], 128, 192) == [(0, 128, 192)]
    many = list(range(4097))
    assert distpow.digests_batch_walk(many, 4000, 4064) == [(t, t, t + 1) for t in range(4000, 4064)]
    assert distpow.digests_batch_walk(many, 4090, 4154) == [(t, t, t + 1) for t in range(4090, 4096)]


def test_walk_with_arbitrary_rows_stays_in_bounds():
    """Rows as device memory may hold them -- random, descending, huge: at most n_tasks + 1 passes,
    every (task, lo, hi) in bounds, the restated walk's passes; and with rows that do not descend the
    passes are disjoint and cover exactly the wave's positions within [rows[0], rows[n_tasks])."""
    rnd = random.Random(2121)
    L = distpow.lib()
    for case in range(600):
        n = rnd.choice([1, 2, 3, 7, 64, 65, 200])
        kind = case % 4
        if kind == 0:
            rows = [rnd.randrange(0, 400) for _ in range(n + 1)]
        elif kind == 1:
            rows = sorted((rnd.randrange(0, 400) for _ in range(n + 1)), reverse=True)
        elif kind == 2:
            rows = [rnd.choice([0, 1, 63, 64, 2**63, 2**64 - 1, rnd.randrange(0, 400)]) for _ in range(n + 1)]
        else:
            rows = sorted(rnd.randrange(0, 400) for _ in range(n + 1))
        arr = (ctypes.c_uint64 * (n + 1))(*rows)
        out = (_lib.DigestPassC * (n + 1))()
        for e_first in (0, 1, 37, 64, 128, 256, 399, 2**63 - 5):
            for width in (64, 1, 0):
                e_end = e_first + width
                cnt = L.dpow_digests_batch_walk(arr, n, e_first, e_end, out, n + 1)
                assert 0 <= cnt <= n + 1, (rows, e_first)
                got = [(p.task, p.lo, p.hi) for p in out[:cnt]]
                assert got == _restated(rows, e_first, e_end), (rows, e_first, e_end)
                assert all(t < n and e_first <= lo < hi <= e_end for t, lo, hi in got), (rows, got)
                assert [t for t, _, _ in got] == sorted({t for t, _, _ in got})  # the task number only grows
                if kind == 3:
                    covered = [e for _, lo, hi in got for e in range(lo, hi)]
                    want = [e for e in range(e_first, e_end) if rows[0] <= e < rows[n]]
                    assert covered == want and got == _spec(rows, e_first, e_end), (rows, e_first)
    # the helper's own argument errors
    arr = (ctypes.c_uint64 * 2)(0, 5)
    out = (_lib.DigestPassC * 2)()
    assert L.dpow_digests_batch_walk(None, 1, 0, 64, out, 2) == EINVAL
    assert L.dpow_digests_batch_walk(arr, 1, 0, 64, None, 2) == EINVAL
    assert L.dpow_digests_batch_walk(arr, 1, 0, 64, None, 0) == 1  # a count alone
    assert L.dpow_digests_batch_walk(arr, 0, 0, 64, out, 2) == EINVAL
    assert L.dpow_digests_batch_walk(arr, _lib.DPOW_BATCH_MAX + 1, 0, 64, out, 2) == EINVAL
    assert L.dpow_digests_batch_walk(arr, 1, 0, 65, out, 2) == EINVAL
    assert L.dpow_digests_batch_walk(arr, 1, 5, 4, out, 2) == EINVAL
