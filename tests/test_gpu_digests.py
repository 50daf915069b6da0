"""GPU: the digests (dpow_digests, Miner.digests, Miner.digests_cuda) -- the MD5 and the depth of any
listed candidates of one nonce.

Every assertion is equality with something that does not come from the digest kernel: hashlib over
all 16 bytes (the edge list E below: every chunk length next to its neighbour, three thread bytes,
at every byte position of the message), the committed fixtures, and the census and the scan of the
same candidates.  E has 45 entries in a fixed shuffled order, so one wave mixes every chunk length,
and for nonce lengths with p = len % 64 >= 48 both block counts.

Each test prints its time (pytest -s).
"""
import array
import ctypes
import hashlib
import json
import os
import random
import time

import pytest

import distpow
from distpow import CANCELLED, DPOW_K_LIMIT, EINVAL, ERANGE, EXHAUSTED
from distpow import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

KS = [0, 1, 255, 256, 65535, 65536, 2**24 - 1, 2**24, 2**32 - 1, 2**32, 2**40 - 1, 2**40, 2**48 - 1, 2**48,
      2**55 - 2]
E = [k << 8 | tb for k in KS for tb in (0, 1, 255)]
random.Random(20240).shuffle(E)
assert len(E) == 45 and max(E) >> 8 == DPOW_K_LIMIT - 1


def _secret_of(g):
    out, k = [g & 0xFF], g >> 8
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return bytes(out)


def _nonce(n, salt=0):
    rnd = random.Random(7000 * n + salt)
    return bytes(rnd.randrange(256) for _ in range(n))


def _hashlib(nonce, indices):
    """(digests, depths) as Miner.digests returns them, from hashlib."""
    base, dig, dep = hashlib.md5(bytes(nonce)), bytearray(), bytearray()
    for g in indices:
        h = base.copy()
        h.update(_secret_of(g))
        dig += h.digest()
        hx = h.hexdigest()
        dep.append(32 - len(hx.rstrip("0")))
    return bytes(dig), bytes(dep)


_REF = {}


def _ref_e(nlen):
    """hashlib's answer for E under the test nonce of that length, computed once."""
    if nlen not in _REF:
        _REF[nlen] = _hashlib(_nonce(nlen), E)
    return _REF[nlen]


def _ref_of(nlen, indices):
    """hashlib's answer for a list made of E's entries."""
    dig, dep = _ref_e(nlen)
    at = {g: j for j, g in enumerate(E)}
    return (b"".join(dig[16 * at[g]:16 * at[g] + 16] for g in indices), bytes(dep[at[g]] for g in indices))


LENGTHS = list(range(131)) + [1024]


def test_edges_equal_hashlib_at_every_nonce_length(miner):
    """One call per nonce length 0..130 and 1024: every p twice, one and two final blocks, midstates of
    one, two and sixteen blocks; all 16 bytes and the depth of each of E's 45 entries."""
    t = time.perf_counter()
    for nlen in LENGTHS:
        got = miner.digests(_nonce(nlen), E)
        assert got == _ref_e(nlen), nlen
        st = miner.last_digest_stats
        assert (st.launches, st.candidates, miner.last_digest_status) == (1, 45, EXHAUSTED)
    print(f"{len(LENGTHS)} nonce lengths x {len(E)} entries: {time.perf_counter() - t:.3f} s")


@pytest.mark.parametrize("nlen", [4, 60])
@pytest.mark.parametrize("n,chunk", [(1, None), (63, None), (64, None), (65, None), (255, None), (256, None),
                                     (257, 256), (1000, 256)])
def test_shapes(miner, monkeypatch, n, chunk, nlen):
    """Partial waves, partial workgroups, chunk seams and the reuse of both buffer sets: E repeated,
    in descending order, duplicates included; outputs are positional."""
    indices = sorted((E * (n // len(E) + 1))[:n], reverse=True)
    want = _ref_of(nlen, indices)
    if chunk:
        monkeypatch.setenv("DPOW_DIAG_DIGEST_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("DPOW_DIAG_DIGEST_CHUNK", raising=False)
    nonce = _nonce(nlen)
    t = time.perf_counter()
    got = miner.digests(nonce, indices)
    st = miner.last_digest_stats
    assert got == want
    assert (st.launches, st.candidates) == (-(-n // (chunk or n)), n)
    # the same list as a buffer of uint64, and either output alone
    assert miner.digests(nonce, array.array("Q", indices)) == want
    assert miner.digests(nonce, indices, want_depths=False) == (want[0], None)
    assert miner.digests(nonce, bytes(array.array("Q", indices)), want_digests=False) == (None, want[1])
    print(f"n {n} chunk {chunk} len {nlen}: {st.launches} launches, four calls in {time.perf_counter() - t:.3f} s")


def test_golden_fixture_entries(miner, golden):
    """Every entry of tests/golden/pow_golden.json with an index: its digest is the fixture's md5 (the
    hashlib MD5 of its nonce and secret where the fixture lists no md5), its depth at least its N."""
    entries = [e for key in ("first_hits", "partitions", "windows", "nonce_lengths", "deep_hits")
               for e in golden[key]]
    by_nonce = {}
    for e in entries:
        assert bytes(e["secret"]) == _secret_of(e["global_idx"])
        by_nonce.setdefault(tuple(e["nonce"]), []).append(e)
    t = time.perf_counter()
    for nonce, es in by_nonce.items():
        dig, dep = miner.digests(nonce, [e["global_idx"] for e in es])
        for j, e in enumerate(es):
            md5 = e.get("md5") or hashlib.md5(bytes(nonce) + bytes(e["secret"])).hexdigest()
            assert dig[16 * j:16 * j + 16].hex() == md5, e
            assert dep[j] >= e["ntz"] and dep[j] == 32 - len(md5.rstrip("0")), e
    print(f"{len(entries)} entries of {len(by_nonce)} nonces in {time.perf_counter() - t:.3f} s")


def test_layout_deep_hits(miner):
    """Every hit of every layout in tests/golden/layout_deep_hits.json, one call per layout: the depth
    is what the CPU-scanned list says."""
    with open(os.path.join(GOLDEN, "layout_deep_hits.json")) as f:
        cases = json.load(f)["cases"]
    t = time.perf_counter()
    total = 0
    for c in cases:
        if not c["hits"]:
            continue
        dig, dep = miner.digests(c["nonce"], [g for g, _ in c["hits"]])
        assert list(dep) == [tz for _, tz in c["hits"]], c["name"]
        assert (dig, dep) == _hashlib(c["nonce"], [g for g, _ in c["hits"]]), c["name"]
        total += len(c["hits"])
    assert total >= 200
    print(f"{total} hits of {len(cases)} layouts in {time.perf_counter() - t:.3f} s")


def test_census_and_scan_of_the_same_candidates(miner):
    """Indices 0..2^16-1 of one nonce in one call: the cumulated depth histogram is the census's
    count_ge, the entries of depth >= 2 are the scan's, index by index and depth by depth."""
    nonce, n = [1, 2, 3, 4], 1 << 16
    t = time.perf_counter()
    dig, dep = miner.digests(nonce, range(n))
    t_call = time.perf_counter() - t
    assert (miner.last_digest_stats.launches, miner.last_digest_stats.candidates) == (1, n)
    hist = [0] * 34
    for d in dep:
        hist[d] += 1
    count_ge = [sum(hist[d:]) for d in range(33)]
    assert tuple(count_ge) == miner.census(nonce, k_end=256).count_ge
    assert [(g, d) for g, d in enumerate(dep) if d >= 2] == [(h.global_idx, h.tz)
                                                           for h in miner.scan(nonce, 2, k_end=256)]
    for g in (0, 255, 256, 65535):
        assert dig[16 * g:16 * g + 16] == hashlib.md5(bytes(nonce) + _secret_of(g)).digest()
    print(f"{n} entries in {t_call * 1e3:.2f} ms; depths {[c for c in count_ge if c]}")


def _raw_call(miner, indices, nonce=b"\x01\x02\x03\x04", nlen=None, dig=True, dep=True, fill=0xA5, n_done=True):
    """dpow_digests on pre-filled outputs: (code, digests, depths, n_done, stats)."""
    n = len(indices)
    idx = (ctypes.c_uint64 * max(n, 1))(*indices)
    d = ctypes.create_string_buffer(bytes([fill]) * (16 * max(n, 1)))
    z = ctypes.create_string_buffer(bytes([fill]) * max(n, 1))
    done, st = ctypes.c_size_t(12345), _lib.BatchStats()
    rc = distpow.lib().dpow_digests(miner._ctx, nonce, len(nonce) if nlen is None else nlen, idx, n,
                                    d if dig else None, z if dep else None,
                                    ctypes.byref(done) if n_done else None, ctypes.byref(st))
    return rc, d.raw[:16 * n], z.raw[:n], done.value, st


def test_errors_and_cancel(miner):
    bad = DPOW_K_LIMIT << 8
    untouched = (b"\xa5" * (16 * 45), b"\xa5" * 45)
    for at in (0, 22, 44):  # an entry with k = DPOW_K_LIMIT anywhere in the list
        rc, d, z, done, st = _raw_call(miner, E[:at] + [bad] + E[at + 1:])
        assert (rc, d, z, st.launches) == (ERANGE, *untouched, 0), at
    rc, d, z, done, st = _raw_call(miner, E[:44] + [2**64 - 1])
    assert (rc, d, z, st.launches) == (ERANGE, *untouched, 0)
    assert _raw_call(miner, E, dig=False, dep=False)[0] == EINVAL
    assert _raw_call(miner, E, n_done=False)[0] == EINVAL
    rc, d, z, done, st = _raw_call(miner, E, nonce=bytes(_lib.DPOW_MAX_NONCE + 1))
    assert (rc, d, z, st.launches) == (EINVAL, *untouched, 0)
    assert _raw_call(miner, E, nonce=None, nlen=4)[0] == EINVAL
    L = distpow.lib()
    done = ctypes.c_size_t()
    assert L.dpow_digests(miner._ctx, b"", 0, None, 4, ctypes.create_string_buffer(64), None, ctypes.byref(done),
                          None) == EINVAL
    # n = 0 is done without a launch
    rc, d, z, done, st = _raw_call(miner, [])
    assert (rc, done, st.launches, st.candidates) == (EXHAUSTED, 0, 0, 0)
    assert miner.digests([1, 2, 3, 4], []) == (b"", b"")
    # a cancel flag raised on entry: no launch, nothing written; cleared, the same call succeeds
    miner.cancel()
    try:
        rc, d, z, done, st = _raw_call(miner, E)
        assert miner.digests([1, 2, 3, 4], E) == (b"", b"") and miner.last_digest_status == CANCELLED
    finally:
        miner.clear_cancel()
    assert (rc, d, z, done, st.launches) == (CANCELLED, *untouched, 0, 0)
    miner.reset_stats()
    rc, d, z, done, st = _raw_call(miner, E)
    assert (rc, done, st.launches, st.candidates) == (EXHAUSTED, 45, 1, 45)
    assert (d, z) == _hashlib([1, 2, 3, 4], E)
    # a digest call leaves dpow_stats alone
    s = miner.stats()
    assert (s.searches, s.launches, s.candidates) == (0, 0, 0)


def test_node_slot_attached_is_refused(miner):
    class Slot(ctypes.Structure):
        """dpow_node_slot (include/dpow.h)."""
        _fields_ = [("best", ctypes.c_uint64), ("stop", ctypes.c_uint32), ("pad", ctypes.c_uint32 * 13)]

    slot = Slot()
    addr = ctypes.addressof(slot)
    distpow.lib().dpow_node_slot_reset(addr)
    miner.attach_node(addr)
    try:
        with pytest.raises(distpow.DpowError) as e:
            miner.digests([1, 2, 3, 4], E)
        assert e.value.code == EINVAL
    finally:
        miner.attach_node(None)
    assert miner.digests([1, 2, 3, 4], [0]) == _hashlib([1, 2, 3, 4], [0])


def _bytes(t):
    return bytes(t.cpu().flatten().tolist())


@pytest.mark.parametrize("nlen", [4, 55, 60])
def test_device_variant(miner, nlen):
    """E as a CUDA tensor: byte-identical to Miner.digests; then one out-of-range entry in the middle."""
    import torch
    nonce = _nonce(nlen)
    dev = torch.device("cuda", miner.device)
    idx = torch.tensor(E, dtype=torch.int64, device=dev)
    t = time.perf_counter()
    dig, dep = miner.digests_cuda(nonce, idx)
    assert (dig.shape, dig.dtype, dep.shape, dep.dtype) == ((45, 16), torch.uint8, (45,), torch.uint8)
    host = miner.digests(nonce, E)
    assert (_bytes(dig), _bytes(dep)) == host == _ref_e(nlen)
    assert (miner.last_digest_stats.launches, miner.last_digest_stats.candidates) == (1, 45)
    bad = E[:22] + [DPOW_K_LIMIT << 8] + E[23:]
    idx = torch.tensor(bad, dtype=torch.int64, device=dev)
    with pytest.raises(distpow.DpowError) as e:
        miner.digests_cuda(nonce, idx)
    assert e.value.code == ERANGE
    dig, dep = miner.digests_cuda(nonce, idx, strict=False)
    assert miner.last_digest_status == ERANGE
    dig, dep = _bytes(dig), _bytes(dep)
    assert dep[22] == 255 and dig[16 * 22:16 * 23] == bytes(16)
    assert dep[:22] + dep[23:] == host[1][:22] + host[1][23:]
    assert dig[:16 * 22] + dig[16 * 23:] == host[0][:16 * 22] + host[0][16 * 23:]
    # the count is per call: a good list after a bad one is good
    dig, dep = miner.digests_cuda(nonce, torch.tensor(E, dtype=torch.int64, device=dev))
    assert miner.last_digest_status == EXHAUSTED and _bytes(dep) == host[1]
    print(f"len {nlen}: {time.perf_counter() - t:.3f} s")
