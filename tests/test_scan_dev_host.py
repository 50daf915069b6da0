"""Host side of the device scan (dpow_scan_device, dpow_scan_device_cut), no GPU needed: the cut of
a slice against a brute-force loop, the entry points in the header, the library and the binding, and
the argument errors that come back as codes before any GPU work."""
import ctypes
import os
import random
import re
import subprocess

import distpow
from distpow import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAX_GROUPS, GROUP_HITS = 16384, 16384  # csrc/md5_scan_dev.h kScanDevMaxBlocks, kScanDevMaxGroup


def _brute(prefix, room):
    """The largest number of leading groups whose inclusive prefix fits `room`."""
    n = 0
    for g, p in enumerate(prefix):
        if p > room:
            break
        n = g + 1
    return n


def _prefix(totals):
    out, s = [], 0
    for t in totals:
        s += t
        out.append(s)
    return out


def test_cut_against_brute_force_random():
    rnd = random.Random(18)
    for _ in range(300):
        n = rnd.choice([1, 2, 3, 17, 256, 1000])
        hi = rnd.choice([0, 1, 3, 64, GROUP_HITS])
        prefix = _prefix([rnd.randint(0, hi) if rnd.random() < 0.7 else 0 for _ in range(n)])
        for room in {0, 1, prefix[0], prefix[-1], max(prefix[-1] - 1, 0), prefix[-1] + 1, prefix[n // 2],
                     max(prefix[n // 2] - 1, 0), rnd.randint(0, prefix[-1] + 2)}:
            assert distpow.scan_device_cut(prefix, room) == _brute(prefix, room), (prefix, room)


def test_cut_adversarial():
    cut = distpow.scan_device_cut
    zeros = [0] * 1000
    assert cut(zeros, 0) == 1000 and cut(zeros, 5) == 1000            # all zero: everything fits any room
    assert cut([GROUP_HITS], GROUP_HITS - 1) == 0                       # one group over the room
    assert cut([3, 7, 7, 7, 12], 7) == 4 and cut([3, 7, 7, 7, 12], 6) == 1   # an exact fit takes the empty groups behind it
    assert cut([3, 7, 12], 12) == 3 and cut([3, 7, 12], 11) == 2
    assert cut([1, 2, 3], 0) == 0 and cut([0, 0, 3], 0) == 2           # a room of 0 takes leading empty groups only
    assert cut([], 100) == 0
    assert distpow.lib().dpow_scan_device_cut(None, 5, 100) == 0
    # 16384 groups: every group full (a dense slice), and sparse
    full = _prefix([GROUP_HITS] * MAX_GROUPS)
    assert full[-1] == 1 << 28
    for room in (0, GROUP_HITS - 1, GROUP_HITS, 1 << 20, (1 << 20) + 5, (1 << 28) - 1, 1 << 28, 1 << 40):
        assert cut(full, room) == _brute(full, room) == min(room // GROUP_HITS, MAX_GROUPS)
    rnd = random.Random(7)
    sparse = _prefix([rnd.choice([0, 0, 0, 1, 2, 900]) for _ in range(MAX_GROUPS)])
    for room in [0, 1, 899, 900, sparse[-1] - 1, sparse[-1], sparse[-1] + 1] + [rnd.randint(0, sparse[-1]) for _ in range(50)]:
        assert cut(sparse, room) == _brute(sparse, room)
    # a room above 2^32 is not truncated
    assert cut([0xFFFFFFFF], (1 << 32) + 1) == 1 and cut([0xFFFFFFFF], 0xFFFFFFFE) == 0


def test_header_library_and_binding_have_the_entry_points():
    text = open(os.path.join(ROOT, "include", "dpow.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(dpow_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", distpow.LIB_PATH]).decode()
    exported = set(re.findall(r"\s[TW]\s+(dpow_[a-z0-9_]+)$", out, flags=re.M))
    L = distpow.lib()
    for sym in ("dpow_scan_device", "dpow_scan_device_cut"):
        assert sym in names and sym in exported, sym
        assert getattr(L, sym).argtypes is not None
    assert re.search(r"#define\s+DPOW_SCAN_DEVICE_MIN_HITS\s+16384\b", text)
    assert distpow.SCAN_DEVICE_MIN_HITS == _lib.SCAN_DEVICE_MIN_HITS == GROUP_HITS
    assert {"scan_device_cut", "SCAN_DEVICE_MIN_HITS"} <= set(distpow.__all__)
    assert callable(distpow.Miner.scan_cuda) and callable(distpow.Miner.scan_cuda_page)


def test_argument_errors_before_any_gpu_work():
    """The window's own errors come first: they show without a context, and no pointer is followed
    (the "device" pointers here are plain integers)."""
    L = distpow.lib()
    n, kd = ctypes.c_size_t(), ctypes.c_uint64()
    pn, pk = ctypes.byref(n), ctypes.byref(kd)
    nonce = b"\x01\x02\x03\x04"

    def call(nonce=nonce, nlen=4, wb=0, k0=0, k1=4, idx=0x1000, tz=0x2000, max_hits=GROUP_HITS, n_hits=pn,
             k_done=pk):
        return L.dpow_scan_device(None, nonce, nlen, 1, wb, 0, k0, k1, idx, tz, max_hits, n_hits, k_done, None)

    assert call(idx=None) == call(n_hits=None) == call(k_done=None) == distpow.EINVAL
    assert "NULL argument" in _lib.last_error()
    assert call(idx=0x1004) == distpow.EINVAL and "aligned" in _lib.last_error()
    assert call(max_hits=GROUP_HITS - 1) == distpow.EINVAL and "max_hits" in _lib.last_error()
    assert call(nonce=None) == distpow.EINVAL and "nonce is NULL" in _lib.last_error()
    assert call(wb=256) == distpow.EINVAL and "worker_byte" in _lib.last_error()
    assert call(k0=5) == distpow.EINVAL and "k_begin > k_end" in _lib.last_error()
    assert "dpow_scan_device" in _lib.last_error()
    assert call(nonce=bytes(1025), nlen=1025) == distpow.EINVAL and "DPOW_MAX_NONCE" in _lib.last_error()
    assert call(k1=distpow.DPOW_K_LIMIT + 1) == distpow.ERANGE
    assert call() == distpow.EINVAL and "ctx is NULL" in _lib.last_error()   # a good window, no context
    assert call(tz=None) == distpow.EINVAL and "ctx is NULL" in _lib.last_error()   # depths are optional
