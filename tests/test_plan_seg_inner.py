"""Which launches dpow_search runs segment-inner, and what their kernel hashes (host logic; no GPU).

plan.h seg_inner_select / seg_inner_size through dpow_diag_seg_inner_geometry and
dpow_diag_seg_inner_candidate.  A launch is segment-inner when its layout has such a kernel
(one final block, SH = 0, W0 <= 3), ntz >= 8, k >= 2^24, it spans at least 2 * 2^24 k, and it
is at most 1/64 of the partition's expected first hit (16^N R / 256 candidates): N >= 14 and
the sweep's N = 32 unlimited, N = 10 cut to 4 segments, N <= 9 never.  Its claims cover ONE
segment's wave-blocks, each hashed in every segment of the launch.
"""
import ctypes
import random
import struct

import pytest

import distpow

SEG = 1 << 24
CLAIM_COUNTERS = 8
WPB = 4
MD5_IV = [0x67452301, 0xefcdab89, 0x98badcfe, 0x10325476]


class DiagLaunch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("k_begin", "k_end", "i_begin", "i_end", "wb_begin", "n_wblocks",
                                                "n_big", "n_chunks", "worker_blocks")] + \
               [(n, ctypes.c_uint32) for n in ("chunk", "chunk_tail", "rbits", "wave_block")] + \
               [("n_static", ctypes.c_uint64), ("poll_wb", ctypes.c_uint32), ("n_seg", ctypes.c_uint32)]


def _geometry(fn_name, nonce, ntz, wb, wbits, k0, k1, extra, cus=256):
    fn = getattr(distpow.lib(), fn_name)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                   ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.POINTER(DiagLaunch),
                   ctypes.c_size_t]
    n = bytes(nonce)
    cnt = fn(n, len(n), ntz, wb, wbits, k0, k1, cus, extra, None, 0)
    assert cnt >= 0, distpow._lib.last_error()
    arr = (DiagLaunch * max(cnt, 1))()
    assert fn(n, len(n), ntz, wb, wbits, k0, k1, cus, extra, arr, cnt) == cnt
    return list(arr[:cnt])


def si_geometry(nonce, ntz, wb, wbits, k0, k1, mode=-1, cus=256):
    """The launches of the window as their kernels get them (segment-inner ones re-cut)."""
    return _geometry("dpow_diag_seg_inner_geometry", nonce, ntz, wb, wbits, k0, k1, mode, cus)


def check_si(d):
    """The claim geometry of a segment-inner launch (md5_search_si.h search_body_si)."""
    W = d.wave_block
    segbits = 24 + d.rbits
    assert d.k_begin >= SEG and d.k_end - d.k_begin >= 2 * SEG
    assert d.n_seg == ((d.k_end - 1) >> 24) - (d.k_begin >> 24) + 1 >= 2
    assert d.wb_begin == (d.k_begin >> 24) << segbits and d.n_wblocks * W == 1 << segbits
    assert d.wb_begin <= d.i_begin < d.i_end <= d.wb_begin + (d.n_seg << segbits)
    assert d.i_end > d.wb_begin + ((d.n_seg - 1) << segbits)  # the last segment holds part of the window
    assert d.chunk >= 1 and d.chunk & (d.chunk - 1) == 0 and 1 <= d.chunk_tail <= d.chunk
    assert d.chunk * d.n_seg <= 32 or d.chunk == 1  # a claim's work: about the index-ordered claim's 32 wave-blocks
    tails = d.n_chunks - d.n_big
    covered = d.n_big * d.chunk + tails * d.chunk_tail
    assert covered >= d.n_wblocks > covered - d.chunk_tail
    assert min(d.n_chunks, CLAIM_COUNTERS) <= d.worker_blocks <= max(-(-d.n_chunks // WPB), CLAIM_COUNTERS)
    assert d.n_static == 0 and d.poll_wb >= 1


@pytest.mark.parametrize("ntz", [32, 14])
@pytest.mark.parametrize("wb,wbits", [(0, 0), (5, 3), (77, 8)])
def test_sweep_windows_are_one_segment_inner_launch(ntz, wb, wbits):
    for k0, k1 in ((SEG, SEG + (1 << 28)),                      # the bench step: 16 whole segments
                   (SEG + 12345, 13 * SEG + 12345),             # unaligned at both ends
                   (3 * SEG, 5 * SEG),                          # exactly 2 segments
                   (7 * SEG - 1, 10 * SEG + 1),                 # one k in the first and the last segment
                   ((1 << 32) + 254 * SEG, (1 << 32) + 257 * SEG)):  # L = 5, k >> 24 carries across a byte
        ds = si_geometry([1, 2, 3, 4], ntz, wb, wbits, k0, k1)
        assert len(ds) == 1 and (ds[0].k_begin, ds[0].k_end) == (k0, k1)
        check_si(ds[0])
    d, = si_geometry([1, 2, 3, 4], ntz, 0, 0, SEG, SEG + (1 << 28))
    assert (d.n_seg, d.chunk, d.chunk_tail, d.worker_blocks, d.poll_wb) == (16, 2, 1, 1536, 16)
    d, = si_geometry([1, 2, 3, 4], ntz, 5, 3, SEG, SEG + (1 << 31))  # an 8-GPU rank's step
    assert (d.n_seg, d.chunk, d.worker_blocks) == (128, 1, 1536)


def test_search_geometry_diagnostic_flags_the_launch():
    """dpow_diag_launch_geometry keeps reporting the claims as sized in index order, and says in
    n_seg that the search re-cuts them."""
    fn = "dpow_diag_launch_geometry"
    d, = _geometry(fn, [1, 2, 3, 4], 32, 0, 0, SEG, SEG + (1 << 28), 1)
    assert d.n_seg == 16 and d.chunk == 32 and d.n_wblocks * d.wave_block == (1 << 28) << 8
    d, = _geometry(fn, [1, 2, 3, 4], 9, 0, 0, SEG, SEG + (1 << 28), 1)
    assert d.n_seg == 0


@pytest.mark.parametrize("ntz", [0, 3, 7, 8, 9])
def test_short_searches_never(ntz):
    for wb, wbits in ((0, 0), (5, 3), (1, 1)):
        for d in si_geometry([1, 2, 3, 4], ntz, wb, wbits, SEG, 41 * SEG):
            assert d.n_seg == 0
    if ntz < 8:  # no D-equality kernel below 8: not even when forced
        assert all(d.n_seg == 0 for d in si_geometry([1, 2, 3, 4], ntz, 0, 0, SEG, 9 * SEG, mode=1))


@pytest.mark.parametrize("wb,wbits", [(0, 0), (5, 3)])
def test_n10_launches_are_capped_to_four_segments(wb, wbits):
    """16^10 R / 256 expected candidates; 1/64 of them is 4 segments of 2^24 R candidates."""
    ds = si_geometry([1, 2, 3, 4], 10, wb, wbits, SEG, 19 * SEG)
    assert [(d.k_begin // SEG, d.k_end // SEG) for d in ds] == [(1, 5), (5, 9), (9, 13), (13, 17), (17, 19)]
    for d in ds:
        check_si(d)
    assert [d.n_seg for d in ds] == [4, 4, 4, 4, 2]
    # unaligned: launches of 4 * 2^24 k lie in 5 segments; a remainder below 2 segments is index-ordered
    ds = si_geometry([1, 2, 3, 4], 10, wb, wbits, SEG + 999, 10 * SEG + 999 + SEG // 2)
    assert all(d.k_end - d.k_begin <= 4 * SEG for d in ds) and ds[-1].k_end == 10 * SEG + 999 + SEG // 2
    assert [d.n_seg for d in ds] == [5, 5, 0]
    for d in ds[:2]:
        check_si(d)
    # N = 11: 64 segments; N = 13 on a rank: 2^14
    assert [d.n_seg for d in si_geometry([1, 2, 3, 4], 11, wb, wbits, SEG, 101 * SEG)] == [64, 36]
    assert [d.n_seg for d in si_geometry([1, 2, 3, 4], 13, wb, wbits, SEG, 101 * SEG)] == [100]


def test_windows_below_two_segments_never():
    for mode in (-1, 1):
        for k0, k1 in ((SEG, 3 * SEG - 1), (SEG + 5, 2 * SEG + 5), (1, SEG), (1 << 16, SEG)):
            assert all(d.n_seg == 0 for d in si_geometry([1, 2, 3, 4], 32, 0, 0, k0, k1, mode=mode))
    # a window from below 2^24: only its launches from 2^24 on qualify
    ds = si_geometry([1, 2, 3, 4], 32, 0, 0, 1 << 20, 4 * SEG)
    assert [d.n_seg for d in ds] == [0, 3] and ds[1].k_begin == SEG


def test_uncovered_layouts_and_the_knob():
    for nonce in ([1, 2, 3], [1] * 16, [1] * 52, [1] * 56, [9] * 60):  # SH = 3; W0 = 4, 13, 14; two final blocks
        assert all(d.n_seg == 0 for d in si_geometry(nonce, 32, 0, 0, SEG, 9 * SEG, mode=1))
    for nonce in ([], [1, 2, 3, 4], [7] * 8, [7] * 12):  # W0 = 0 .. 3
        d, = si_geometry(nonce, 32, 0, 0, SEG, 9 * SEG)
        check_si(d)
        assert all(x.n_seg == 0 for x in si_geometry(nonce, 32, 0, 0, SEG, 9 * SEG, mode=0))
    d, = si_geometry([1, 2, 3, 4], 8, 0, 0, SEG, 9 * SEG, mode=1)  # forced: no expected-first-hit cap
    check_si(d)


def _expected_words(nonce, secret):
    msg = bytes(nonce) + bytes(secret)
    pad = msg + b"\x80" + b"\x00" * ((55 - len(msg)) % 64) + struct.pack("<Q", 8 * len(msg))
    assert len(pad) == 64  # nonces of at most 12 bytes: one final block from the MD5 IV
    return list(struct.unpack("<16I", pad))


@pytest.mark.parametrize("nonce,wb,wbits,k0,k1", [
    ([1, 2, 3, 4], 0, 0, SEG + 12345, 13 * SEG + 12345),
    ([1, 2, 3, 4], 5, 3, 2 * SEG + 1, 42 * SEG + 7),
    ([1, 2, 3, 4], 200, 8, SEG, 401 * SEG),
    ([1, 2, 3, 4], 0, 0, (1 << 32) + 254 * SEG, (1 << 32) + 257 * SEG),
    ([9, 8, 7, 6, 5, 4, 3, 2], 1, 1, (1 << 40) - 3 * SEG + 5, 1 << 40),
    ([], 3, 2, 0xFFFD * SEG + 1, (1 << 40)),
])
def test_candidate_words_equal_the_oracles_message(oracle, nonce, wb, wbits, k0, k1):
    fn = distpow.lib().dpow_diag_seg_inner_candidate
    u32p = ctypes.POINTER(ctypes.c_uint32)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                   ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint64, u32p, u32p, u32p]
    rb = 8 - wbits % 9
    tbs = oracle.thread_bytes(wb, wbits)
    rnd = random.Random(len(nonce) * 1000 + wbits)
    i_lo, i_hi = k0 << rb, k1 << rb
    seg_i = SEG << rb
    idxs = [i_lo, i_lo + 1, i_hi - 1, i_lo + 127, (i_lo // seg_i + 1) * seg_i - 1, (i_lo // seg_i + 1) * seg_i]
    idxs += [rnd.randrange(i_lo, i_hi) for _ in range(200)]
    n = bytes(nonce)
    for i in idxs:
        iv, words, nblk = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 32)(), ctypes.c_uint32()
        rc = fn(n, len(n), 32, wb, wbits, k0, k1, -1, i, iv, words, ctypes.byref(nblk))
        assert rc == 1, (rc, distpow._lib.last_error())  # the launch is segment-inner
        k, t = i >> rb, i & ((1 << rb) - 1)
        secret = [tbs[t]] + oracle.chunk_of(k)
        assert nblk.value == 1 and list(iv) == MD5_IV
        assert list(words[:16]) == _expected_words(nonce, secret), (i, k, t)
