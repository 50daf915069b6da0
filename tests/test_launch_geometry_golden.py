"""The launch records of the two geometry diagnostics, pinned field by field (host logic; no GPU).

tests/golden/launch_geometry.json holds every dpow_diag_launch record that
dpow_diag_launch_geometry (share 1, 2, 8) and dpow_diag_seg_inner_geometry (mode -1, 0, 1)
returned for a small fixed table of windows, recorded before the sizing sequence of dpow_search
(plan.h size_window_launch) was shared between the search and the diagnostics.  The table holds
a chunk-length-spanning launch (N <= 7 from below k = 2^24), capped shared launches (share 2
and 8), segment-inner launches that were cut (N = 10: 4 segments each) and windows that a
2^24-k segment boundary straddles.

Regenerate (only when the launch policy changes on purpose):
    python tests/test_launch_geometry_golden.py
"""
import ctypes
import itertools
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "launch_geometry.json")
FIELDS = ["k_begin", "k_end", "i_begin", "i_end", "wb_begin", "n_wblocks", "n_big", "n_chunks", "worker_blocks",
          "chunk", "chunk_tail", "rbits", "wave_block", "n_static", "poll_wb", "n_seg"]
SEG = 1 << 24
NONCES = ([1, 2, 3, 4], [9, 8, 7, 6, 5, 4, 3, 2, 1])
WINDOWS = ((0, 1 << 20), (SEG - (1 << 10), SEG + (1 << 26)), (SEG, SEG + (1 << 28)))
ENTRIES = (("dpow_diag_launch_geometry", (1, 2, 8)), ("dpow_diag_seg_inner_geometry", (-1, 0, 1)))


class DiagLaunch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in FIELDS[:9]] + [(n, ctypes.c_uint32) for n in FIELDS[9:13]] + \
               [("n_static", ctypes.c_uint64), ("poll_wb", ctypes.c_uint32), ("n_seg", ctypes.c_uint32)]


def keep(fn, nonce, ntz, wbits, k0, k1, cus, extra):
    """The table is thinned to keep the file small; every axis value and every kind of launch stays."""
    four = len(nonce) == 4
    if extra in (1, -1):  # the policy alone: the 9-byte nonce at N = 7 and 32, one CU at worker_bits 0
        return (cus == 256 or wbits == 0) if four else (ntz in (7, 32) and cus == 256)
    if fn == "dpow_diag_seg_inner_geometry":  # modes 0 and 1: where a launch can be segment-inner
        return four and cus == 256 and k1 > 1 << 20 and ntz in (8, 10, 32)
    # a shared device's ~8 ms launches (up to 300 a window): a rank's partition, the longest window at share 2
    return four and cus == 256 and wbits == 3 and ntz in (7, 8, 32) and (k1 - k0 < 1 << 28 or extra == 2)


def table():
    """(entry point, nonce, ntz, worker_bits, k_begin, k_end, cus, share or mode)."""
    for (fn, extras), nonce, ntz, wbits, (k0, k1), cus in itertools.product(
            ENTRIES, NONCES, (5, 7, 8, 10, 32), (0, 3), WINDOWS, (1, 256)):
        for extra in extras:
            if keep(fn, nonce, ntz, wbits, k0, k1, cus, extra):
                yield fn, nonce, ntz, wbits, k0, k1, cus, extra


def records(case):
    import distpow
    name, nonce, ntz, wbits, k0, k1, cus, extra = case
    fn = getattr(distpow.lib(), name)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                   ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                   ctypes.c_uint32 if name == "dpow_diag_launch_geometry" else ctypes.c_int32,
                   ctypes.POINTER(DiagLaunch), ctypes.c_size_t]
    n = bytes(nonce)
    wb = 5 if wbits else 0
    cnt = fn(n, len(n), ntz, wb, wbits, k0, k1, cus, extra, None, 0)
    assert cnt >= 0, distpow._lib.last_error()
    arr = (DiagLaunch * max(cnt, 1))()
    assert fn(n, len(n), ntz, wb, wbits, k0, k1, cus, extra, arr, cnt) == cnt
    return [[getattr(d, f) for f in FIELDS] for d in arr[:cnt]]


@pytest.fixture(scope="module")
def golden_doc():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(golden_doc):
    assert golden_doc["fields"] == FIELDS
    assert [c[:8] for c in golden_doc["cases"]] == [list(c) for c in table()]
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_every_field_of_every_launch(golden_doc):
    for c in golden_doc["cases"]:
        assert records(tuple(c[:8])) == c[8], c[:8]


def test_the_table_holds_each_kind_of_launch(golden_doc):
    f = {n: i for i, n in enumerate(FIELDS)}
    lspan = capped = cut = straddled = 0
    for name, nonce, ntz, wbits, k0, k1, cus, extra, launches in golden_doc["cases"]:
        for d in launches:
            kb, ke = d[f["k_begin"]], d[f["k_end"]]
            lspan += kb < 256 and ke > 65536          # chunk lengths 1..3 in one launch
            cut += d[f["n_seg"]] >= 2 and extra == -1 and ke - kb < k1 - max(k0, SEG)
            straddled += kb >= SEG and kb >> 24 != (ke - 1) >> 24
        if name == "dpow_diag_launch_geometry" and extra > 1:
            alone = next(c[8] for c in golden_doc["cases"] if c[:7] == [name, nonce, ntz, wbits, k0, k1, cus])
            capped += len(launches) > len(alone)
        if k0 < SEG < k1:                              # the window itself straddles k = 2^24
            assert any(d[f["k_end"]] == SEG for d in launches) and launches[-1][f["k_end"]] == k1
    assert lspan and capped and cut and straddled, (lspan, capped, cut, straddled)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "distributed-proof-of-work_amd"))
    rows = [json.dumps(list(c) + [records(c)], separators=(",", ":")) for c in table()]
    with open(GOLDEN, "w") as out:  # one case per line
        out.write('{"fields":%s,"cases":[\n%s\n]}\n' % (json.dumps(FIELDS, separators=(",", ":")), ",\n".join(rows)))
    print(len(rows), "cases,", os.path.getsize(GOLDEN), "bytes")
