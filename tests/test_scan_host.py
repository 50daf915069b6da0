"""Host side of the scan (dpow_scan, dpow_scan_slice), no GPU needed: the slice rule keeps its
bounds (DESIGN.md "Scan"), dpow_scan_hit is the header's struct in the binding, the entry points
exist, and the argument errors come back as codes before any GPU work."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import distpow
from distpow import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP, BATCH_CAP = 1 << 16, 1 << 28   # csrc/md5_scan.h kScanCap, csrc/batch.h kBatchCap


def test_slice_rule():
    slices = [distpow.scan_slice(ntz) for ntz in range(34)]
    for ntz, s in enumerate(slices):
        assert s % 256 == 0 and 256 <= s <= BATCH_CAP, (ntz, s)
        if s > 256:   # expected hits s / 16^min(ntz, 32) at most a quarter of the list
            assert 4 * s <= CAP * 16 ** min(ntz, 32), (ntz, s)
    assert slices == sorted(slices)
    assert slices[0] == CAP // 4 and slices[3] == (CAP // 4) << 12 and slices[4] == BATCH_CAP == slices[33]
    # the rule for another capacity (what the tests' small lists would ask for, were the rule to follow them)
    for cap in (256, 1024, 4096, CAP):
        ss = [distpow.scan_slice(ntz, cap) for ntz in range(34)]
        assert ss == sorted(ss) and ss[0] == max(cap // 4, 256) and ss[-1] == BATCH_CAP
        assert all(s % 256 == 0 and (s == 256 or 4 * s <= cap * 16 ** min(n, 32)) for n, s in enumerate(ss))
    # capacities outside [256, 65536] are clamped
    assert distpow.scan_slice(0, 1) == distpow.scan_slice(0, 256) == 256
    assert distpow.scan_slice(0, 1 << 20) == CAP // 4


@pytest.mark.skipif(not shutil.which("gcc"), reason="gcc not available")
def test_scan_hit_layout_against_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dpow.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(dpow_scan_hit), '
                   'offsetof(dpow_scan_hit, global_idx), offsetof(dpow_scan_hit, tz), '
                   'offsetof(dpow_scan_hit, secret_len), offsetof(dpow_scan_hit, secret), DPOW_MORE); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_g, o_tz, o_len, o_sec, more = map(int, subprocess.check_output([str(exe)]).split())
    H = _lib.ScanHitC
    assert (size, o_g, o_tz, o_len, o_sec) == (ctypes.sizeof(H), H.global_idx.offset, H.tz.offset,
                                              H.secret_len.offset, H.secret.offset) == (32, 0, 8, 12, 16)
    assert more == _lib.MORE == distpow.MORE == 3


def test_scan_hit_is_32_bytes():
    H = _lib.ScanHitC
    assert ctypes.sizeof(H) == 32
    assert (H.global_idx.offset, H.tz.offset, H.secret_len.offset, H.secret.offset) == (0, 8, 12, 16)
    assert H.secret.size == _lib.DPOW_MAX_SECRET


def test_header_library_and_binding_have_the_scan_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpow.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(dpow_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", distpow.LIB_PATH]).decode()
    exported = set(re.findall(r"\s[TW]\s+(dpow_[a-z0-9_]+)$", out, flags=re.M))
    L = distpow.lib()
    for sym in ("dpow_scan", "dpow_scan_slice"):
        assert sym in names and sym in exported, sym
        assert getattr(L, sym).argtypes is not None
    assert re.search(r"#define\s+DPOW_MORE\s+3\b", open(os.path.join(ROOT, "include", "dpow.h")).read())
    assert {"ScanHit", "scan_slice", "MORE"} <= set(distpow.__all__)
    assert callable(distpow.Miner.scan) and callable(distpow.Miner.scan_page)


def test_argument_errors_before_any_gpu_work():
    """The window's own errors come first: they show without a context."""
    L = distpow.lib()
    arr = (_lib.ScanHitC * 256)()
    n, kd = ctypes.c_size_t(), ctypes.c_uint64()
    pn, pk = ctypes.byref(n), ctypes.byref(kd)
    nonce = b"\x01\x02\x03\x04"

    def call(nonce=nonce, nlen=4, wb=0, k0=0, k1=4, out=arr, max_hits=256, n_hits=pn, k_done=pk):
        return L.dpow_scan(None, nonce, nlen, 1, wb, 0, k0, k1, out, max_hits, n_hits, k_done, None)

    assert call(out=None) == call(n_hits=None) == call(k_done=None) == distpow.EINVAL
    assert "NULL argument" in _lib.last_error()
    assert call(max_hits=255) == distpow.EINVAL and "max_hits" in _lib.last_error()
    assert call(nonce=None) == distpow.EINVAL and "nonce is NULL" in _lib.last_error()
    assert call(wb=256) == distpow.EINVAL and "worker_byte" in _lib.last_error()
    assert call(k0=5) == distpow.EINVAL and "k_begin > k_end" in _lib.last_error()
    assert "dpow_scan" in _lib.last_error()
    assert call(nonce=bytes(1025), nlen=1025) == distpow.EINVAL and "DPOW_MAX_NONCE" in _lib.last_error()
    assert call(k1=distpow.DPOW_K_LIMIT + 1) == distpow.ERANGE
    assert call() == distpow.EINVAL and "ctx is NULL" in _lib.last_error()   # a good window, no context
