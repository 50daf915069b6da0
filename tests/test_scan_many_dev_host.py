"""Host side of the batched device scan (dpow_scan_batch_device, dpow_scan_batch_device_settle), no
GPU needed: what a launch's placed descriptors mean for the tasks against a Python restatement
(_scan_many_dev_model.settle_model), the argument errors that come back as codes before any GPU
work, and the entry points in the header, the library and the binding."""
import ctypes
import os
import re
import subprocess

import pytest

import distpow
from distpow import _lib
from _scan_many_dev_model import launches_of, settle_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_HITS = 16384


def _ranges(blocks):
    return [_lib.BatchRange(0, task, lo, hi, 0, 0) for task, lo, hi in blocks]


def _i_ranges(windows):
    rb = [distpow.remainder_bits(w[2]) for w in windows]
    return [w[0] << r for w, r in zip(windows, rb)], [w[1] << r for w, r in zip(windows, rb)]


# (windows, cap): one launch of ten descriptors with empty tasks first, between and last; the same
# tasks in launches of four descriptors, so tasks continue from earlier launches; partitions of 32
# and 1 candidates per k with a ragged last descriptor; one task only.
LAYOUTS = [
    ([(5, 5, 0), (0, 3, 0), (7, 7, 0), (10, 15, 0), (2, 2, 0), (1, 3, 0), (9, 9, 0)], 0),
    ([(5, 5, 0), (0, 3, 0), (7, 7, 0), (10, 15, 0), (2, 2, 0), (1, 3, 0), (9, 9, 0)], 1024),
    ([(0, 0, 3), (0, 100, 3), (3, 3, 8), (1, 700, 8), (0, 9, 3), (4, 4, 0)], 512),
    ([(0, 40, 0)], 2048),
    ([(0, 1, 0), (0, 1, 0), (0, 0, 0), (0, 1, 0)], 256),
]


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_settle_against_the_restatement_at_every_cut(layout):
    """Every launch of the layout, reached through its earlier launches placed whole, cut after every
    number of descriptors: at descriptor 0, inside a task, exactly at a task's first descriptor, with
    empty tasks before, at and behind the cut."""
    windows, cap = LAYOUTS[layout]
    i_begin, i_end = _i_ranges(windows)
    launches = launches_of(windows, cap)
    assert launches
    done, next_row = list(i_begin), 0
    seen_first, seen_mid, seen_continued = False, False, False
    for blocks in launches:
        seen_continued = seen_continued or blocks[0][1] != i_begin[blocks[0][0]]
        for n_fit in range(len(blocks) + 1):
            unfinished = distpow.MORE if n_fit < len(blocks) else distpow.CANCELLED
            want = settle_model(blocks, n_fit, i_begin, i_end, done, next_row, unfinished)
            got = distpow.scan_batch_device_settle(_ranges(blocks), n_fit, i_begin, i_end, done, next_row, unfinished)
            assert got == want, (layout, n_fit, got, want)
            if 0 < n_fit < len(blocks):
                first = blocks[n_fit][1] == i_begin[blocks[n_fit][0]]
                seen_first, seen_mid = seen_first or first, seen_mid or not first
                if first:  # the cut on a task's first descriptor leaves the task before it done, this one not begun
                    assert got[3][blocks[n_fit - 1][0]] == distpow.EXHAUSTED
                    assert got[0][blocks[n_fit][0]] == i_begin[blocks[n_fit][0]] and got[2][blocks[n_fit][0]] is None
        done, next_row, _, _ = settle_model(blocks, len(blocks), i_begin, i_end, done, next_row, distpow.MORE)
    assert done == i_end and next_row == max(t for b in launches for t, _, _ in b) + 1
    if layout in (1, 2):
        assert seen_first and seen_mid and seen_continued


def test_settle_hand_checked():
    """Tasks: empty, 3 descriptors, empty, 2 descriptors, empty; two of five descriptors placed."""
    i_begin, i_end = [9, 0, 5, 1024, 7], [9, 768, 5, 1536, 7]
    blocks = [(1, 0, 256), (1, 256, 512), (1, 512, 768), (3, 1024, 1280), (3, 1280, 1536)]
    done, nxt, rows, st = distpow.scan_batch_device_settle(_ranges(blocks), 2, i_begin, i_end, i_begin, 0, distpow.MORE)
    assert (done, nxt, rows) == ([9, 512, 5, 1024, 7], 2, [0, 0, None, None, None])
    assert st == [distpow.EXHAUSTED, distpow.MORE, distpow.EXHAUSTED, distpow.MORE, distpow.EXHAUSTED]
    done, nxt, rows, st = distpow.scan_batch_device_settle(_ranges(blocks), 3, i_begin, i_end, i_begin, 0, distpow.MORE)
    assert (done, nxt, rows) == ([9, 768, 5, 1024, 7], 2, [0, 0, None, None, None])   # cut on task 3's first descriptor
    assert st[1] == distpow.EXHAUSTED and st[3] == distpow.MORE
    done, nxt, rows, st = distpow.scan_batch_device_settle(_ranges(blocks), 5, i_begin, i_end, i_begin, 0, distpow.MORE)
    assert (done, nxt, rows) == (i_end, 4, [0, 0, 3, 3, None]) and set(st) == {distpow.EXHAUSTED}
    done, nxt, rows, st = distpow.scan_batch_device_settle(_ranges(blocks), 0, i_begin, i_end, i_begin, 0, distpow.CANCELLED)
    assert (done, nxt, rows) == (i_begin, 0, [None] * 5) and st[1] == st[3] == distpow.CANCELLED
    # task 3 continued from an earlier launch: its row is not settled again
    done, nxt, rows, st = distpow.scan_batch_device_settle(_ranges(blocks[4:]), 1, i_begin, i_end,
                                                           [9, 768, 5, 1280, 7], 4, distpow.MORE)
    assert (done, nxt, rows) == (i_end, 4, [None] * 5)


def test_settle_argument_errors():
    L = distpow.lib()
    i_begin, i_end = [0, 0], [512, 256]
    ok = [(0, 0, 256), (0, 256, 512), (1, 0, 256)]

    def call(blocks=ok, n_fit=3, done=None, next_row=0, n=2):
        arr = (_lib.BatchRange * max(len(blocks), 1))(*_ranges(blocks))
        ib, ie = (ctypes.c_uint64 * 2)(*i_begin), (ctypes.c_uint64 * 2)(*i_end)
        dn = (ctypes.c_uint64 * 2)(*(done or i_begin))
        nr, rb, st = ctypes.c_uint32(next_row), (ctypes.c_uint32 * 2)(7, 7), (ctypes.c_int32 * 2)(7, 7)
        rc = L.dpow_scan_batch_device_settle(arr, n_fit, ib, ie, n, dn, ctypes.byref(nr), rb, distpow.MORE, st)
        if rc < 0:  # nothing written
            assert list(dn) == list(done or i_begin) and list(rb) == [7, 7] and list(st) == [7, 7] and nr.value == next_row
        return rc

    assert call() == 2
    assert call(n=0) == distpow.EINVAL and call(n=4097) == distpow.EINVAL
    assert call(n_fit=20481) == distpow.EINVAL
    assert call(blocks=[(2, 0, 256)], n_fit=1) == distpow.EINVAL          # names no task
    assert call(blocks=[(0, 256, 512)], n_fit=1) == distpow.EINVAL        # does not begin at the task's progress
    assert call(blocks=[(1, 0, 512)], n_fit=1) == distpow.EINVAL          # reaches beyond its task
    assert call(blocks=[(1, 0, 256), (0, 0, 256)], n_fit=2) == distpow.EINVAL   # out of task order: row 0 behind row 1
    assert call(done=[513, 0]) == distpow.EINVAL and call(next_row=3) == distpow.EINVAL
    nr = ctypes.c_uint32(0)
    assert L.dpow_scan_batch_device_settle(None, 1, None, None, 2, None, ctypes.byref(nr), None, 3, None) == distpow.EINVAL
    assert "NULL argument" in _lib.last_error()


def test_header_library_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "dpow.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", distpow.LIB_PATH]).decode()
    exported = set(re.findall(r"\s[TW]\s+(dpow_[a-z0-9_]+)$", out, flags=re.M))
    L = distpow.lib()
    for sym in ("dpow_scan_batch_device", "dpow_scan_batch_device_settle"):
        m = re.search(r"\bint\s+" + sym + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert m and sym in exported, sym
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        fn = getattr(L, sym)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), (sym, params)
        for p, a in zip(params, fn.argtypes):
            if "*" in p:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (sym, p, a)
            elif p.startswith("size_t"):
                assert a is ctypes.c_size_t, (sym, p, a)
            else:
                assert p.startswith("int32_t") and a is ctypes.c_int32, (sym, p, a)
    assert re.search(r"#define\s+DPOW_ABI_VERSION\s+5\b", text)
    assert "scan_batch_device_settle" in distpow.__all__
    assert callable(distpow.Miner.scan_batch_cuda) and callable(distpow.Miner.scan_many_cuda)


def test_argument_errors_before_any_gpu_work():
    """The call's own errors come first: they show without a context, no pointer is followed (the
    "device" pointers here are plain integers) and no task is written."""
    L = distpow.lib()
    nonce = ctypes.create_string_buffer(b"\x01\x02\x03\x04")
    n_out = ctypes.c_size_t(77)

    def call(n=2, idx=0x1000, tz=0x2000, rows=0x3000, max_hits=MIN_HITS, out=n_out, nonce_ptr=ctypes.addressof(nonce),
             nlen=4, wb=0, k0=0, k1=4, tasks=True):
        arr = (_lib.ScanTaskC * 2)()
        for t in arr:
            t.nonce, t.nonce_len, t.ntz, t.worker_byte, t.k_begin, t.k_end = ctypes.addressof(nonce), 4, 1, 0, 0, 4
            t.status, t.k_done, t.first_hit, t.n_hits = 55, 66, 77, 88
        t = arr[1]
        t.nonce, t.nonce_len, t.worker_byte, t.k_begin, t.k_end = nonce_ptr, nlen, wb, k0, k1
        rc = L.dpow_scan_batch_device(None, arr if tasks else None, n, idx, tz, rows, max_hits,
                                      ctypes.byref(out) if out is not None else None, None)
        assert rc < 0 and n_out.value == 77
        assert all((t.status, t.k_done, t.first_hit, t.n_hits) == (55, 66, 77, 88) for t in arr)
        return rc

    assert call(idx=None) == call(out=None) == call(tasks=False) == distpow.EINVAL
    assert "NULL argument" in _lib.last_error()
    assert call(idx=0x1004) == distpow.EINVAL and "indices not 8-byte aligned" in _lib.last_error()
    assert call(rows=0x3004) == distpow.EINVAL and "rows not 8-byte aligned" in _lib.last_error()
    assert call(n=0) == distpow.EINVAL and call(n=4097) == distpow.EINVAL and "n_tasks" in _lib.last_error()
    assert call(max_hits=MIN_HITS - 1) == distpow.EINVAL and "max_hits" in _lib.last_error()
    assert call(nonce_ptr=None) == distpow.EINVAL and "nonce is NULL" in _lib.last_error()
    assert call(wb=256) == distpow.EINVAL and "worker_byte" in _lib.last_error()
    assert call(k0=5) == distpow.EINVAL and "k_begin > k_end" in _lib.last_error()
    assert "dpow_scan_batch_device" in _lib.last_error()
    assert call(nlen=1025) == distpow.EINVAL and "DPOW_MAX_NONCE" in _lib.last_error()
    assert call(k1=distpow.DPOW_K_LIMIT + 1) == distpow.ERANGE
    assert call() == distpow.EINVAL and "ctx is NULL" in _lib.last_error()              # good tasks, no context
    assert call(tz=None, rows=None) == distpow.EINVAL and "ctx is NULL" in _lib.last_error()   # both are optional
