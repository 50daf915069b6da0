"""GPU: the device scan (dpow_scan_device, Miner.scan_cuda) -- a window's hits in index order with
their depths, left in device memory.

Every assertion is equality with something the device scan did not produce: a Python loop over
hashlib (test_gpu_scan.py's, shared with it), the committed CPU-scanned hit lists
(tests/golden/layout_deep_hits.json), Miner.scan (another kernel, a host sort and a host MD5 per
hit), and for a list too long for hashlib the digest kernel and the census kernel together.  The
N = 0 tests are the test of the order: a lost, duplicated, misplaced or stale entry shows as a wrong
index.

Each test prints its time (pytest -s).
"""
import ctypes
import hashlib
import threading
import time

import pytest
import torch

import _batch_walk_cases as W
import distpow
from distpow import CANCELLED, DPOW_K_LIMIT, EINVAL, ERANGE, EXHAUSTED, FOUND, MORE
from test_gpu_scan import CASES, _nonce, _ref_cached, _reference, _secret_of, _thread_bytes

pytestmark = pytest.mark.gpu

MIN_HITS = 16384  # include/dpow.h DPOW_SCAN_DEVICE_MIN_HITS


def _lists(idx, dep):
    assert idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 1
    assert dep.is_cuda and dep.dtype == torch.uint8 and dep.shape == idx.shape
    return idx.tolist(), dep.tolist()


def _ref_lists(hits, ntz=0):
    return [h.global_idx for h in hits if h.tz >= ntz], [h.tz for h in hits if h.tz >= ntz]


@pytest.mark.parametrize("window", [(0, 300), (65536 - 40, 65536 + 40)], ids=["k0", "k64k"])
@pytest.mark.parametrize("part", [(0, 0), (5, 3)], ids=["all", "wb5of8"])
@pytest.mark.parametrize("nlen", [0, 4, 47, 48, 55, 56, 63, 64, 119])
def test_dense_equals_hashlib(miner, nlen, part, window):
    """One and two final blocks, a midstate, the 55/56 edge; k = 0 and the chunk lengths 1 -> 2 -> 3."""
    (wb, wbits), (k0, k1) = part, window
    every = _ref_cached(nlen, wb, wbits, k0, k1)
    assert len(every) == (k1 - k0) * (256 >> wbits) <= 76800
    t = time.perf_counter()
    for ntz in (1, 2):
        got = _lists(*miner.scan_cuda(_nonce(nlen), ntz, wb, wbits, k0, k1))
        assert got == _ref_lists(every, ntz)
        assert got[0] or ntz > 1
    print(f"len {nlen} part {part} k {window}: {time.perf_counter() - t:.3f} s")


@pytest.mark.parametrize("wb,wbits,k1", [(0, 0, 512), (167, 8, 4096)], ids=["wbits0", "wbits8"])
def test_every_candidate(miner, wb, wbits, k1):
    """N = 0: the answer is every index of the partition once, in order, each depth hashlib's."""
    nonce = _nonce(4, 1)
    t = time.perf_counter()
    idx, dep = _lists(*miner.scan_cuda(nonce, 0, wb, wbits, 0, k1))
    t_scan = time.perf_counter() - t
    tbs = _thread_bytes(wb, wbits)
    assert idx == [k << 8 | tb for k in range(k1) for tb in tbs]
    assert len(idx) == (131072 if wbits == 0 else 4096)
    assert (idx, dep) == _ref_lists(_reference(nonce, 0, wb, wbits, 0, k1))
    print(f"{len(idx)} candidates listed in {t_scan:.3f} s")


def test_stale_mask_words(miner):
    """The bitmap is never zeroed: a dense slice, then a sparse, shorter, ragged one on the same
    context (R = 32 and an odd number of k: the last wave is half full), then one k."""
    nonce = _nonce(4, 3)
    assert _lists(*miner.scan_cuda(nonce, 0, 0, 0, 0, 512)) == _ref_lists(_reference(nonce, 0, 0, 0, 0, 512))
    k0, k1 = 1000, 1333
    assert ((k1 - k0) * 32) % 64 == 32
    sparse = _reference(nonce, 0, 5, 3, k0, k1)
    got = _lists(*miner.scan_cuda(nonce, 3, 5, 3, k0, k1))
    assert got == _ref_lists(sparse, 3)
    print(f"{len(got[0])} hits at N = 3 behind a dense slice")
    assert _lists(*miner.scan_cuda(nonce, 2, 0, 0, 7, 8)) == _ref_lists(_reference(nonce, 2, 0, 0, 7, 8))
    # and the dense list again behind the sparse ones
    assert _lists(*miner.scan_cuda(nonce, 1, 0, 0, 0, 512)) == _ref_lists(_reference(nonce, 1, 0, 0, 0, 512))


def test_paging_dense(miner):
    nonce = _nonce(4, 2)
    ref = _ref_lists(_reference(nonce, 0, 0, 0, 0, 256))
    idxs, deps, k = [], [], 0
    for want_k in (64, 128, 192):
        r, idx, dep, k = miner.scan_cuda_page(nonce, 0, 0, 0, k, 256, max_hits=MIN_HITS)
        assert (r, k, idx.numel(), dep.numel()) == (MORE, want_k, MIN_HITS, MIN_HITS)
        idxs += idx.tolist()
        deps += dep.tolist()
    r, idx, dep, k = miner.scan_cuda_page(nonce, 0, 0, 0, k, 256, max_hits=MIN_HITS)
    assert (r, k, idx.numel()) == (EXHAUSTED, 256, MIN_HITS)
    assert (idxs + idx.tolist(), deps + dep.tolist()) == ref
    assert _lists(*miner.scan_cuda(nonce, 0, 0, 0, 0, 256, max_hits=MIN_HITS)) == ref
    assert miner.last_scan_device_stats.rounds == 4
    with pytest.raises(distpow.DpowError) as e:
        miner.scan_cuda_page(nonce, 0, 0, 0, 0, 256, max_hits=MIN_HITS - 1)
    assert e.value.code == EINVAL


def test_paging_long_list_against_digests_and_census(miner):
    """N = 1 over 2^26 candidates, pages of 2^20: a list too long for hashlib, pinned by two
    independent kernels -- the digest kernel gives every entry's depth, the census the count."""
    nonce, wb, wbits, k1, page = _nonce(4, 5), 5, 3, 1 << 21, 1 << 20   # R = 32 candidates per k
    t = time.perf_counter()
    idxs, deps, k, n_more = [], [], 0, 0
    while True:
        r, idx, dep, k_next = miner.scan_cuda_page(nonce, 1, wb, wbits, k, k1, max_hits=page)
        idxs.append(idx)
        deps.append(dep)
        if r != MORE:
            break
        n_more += 1
        assert k < k_next < k1 and ((k_next - k) * 32) % 256 == 0   # a whole number of workgroup ranges
        # the cut is greedy and a group holds at most 16384 hits
        assert page - MIN_HITS < idx.numel() <= page
        k = k_next
    assert (r, k_next) == (EXHAUSTED, k1) and n_more >= 3
    idx, dep = torch.cat(idxs), torch.cat(deps)
    t_scan = time.perf_counter() - t
    assert bool((idx[1:] > idx[:-1]).all()) and int(idx[0]) >= 0 and int(idx[-1]) < k1 << 8
    assert torch.equal(miner.digests_cuda(nonce, idx)[1], dep) and int(dep.min()) >= 1
    assert bool(((idx & 255) >> 5 == wb).all())
    assert idx.numel() == miner.census(nonce, wb, wbits, 0, k1).count_ge[1]
    # The depths above are the digest kernel's over the call's own entries, so they cannot see a hit at
    # a wrong index.  This can: the digest kernel over every candidate of the window, listed
    # arithmetically, and the entries are those of depth >= 1.
    t = time.perf_counter()
    every = W.window_depths_cuda(miner, nonce, wb, wbits, 0, k1)
    assert every.numel() == k1 << 5
    assert torch.equal(idx, W.window_indices_cuda(wb, wbits, 0, every.numel(), idx.device)[every >= 1])
    print(f"{idx.numel()} hits in {n_more + 1} pages, {t_scan:.3f} s; the reference {time.perf_counter() - t:.3f} s")


def test_slice_seams(miner):
    """2.5 slices of 2^28 candidates at N = 5: the list is Miner.scan's of the same window."""
    nonce, k1 = _nonce(4, 6), 5 << 19
    t = time.perf_counter()
    got = _lists(*miner.scan_cuda(nonce, 5, 0, 0, 0, k1))
    t_scan = time.perf_counter() - t
    st = miner.last_scan_device_stats
    assert (st.rounds, st.candidates) == (3, k1 << 8)
    assert got == _ref_lists(miner.scan(nonce, 5, 0, 0, 0, k1)) and len(got[0]) > 300
    print(f"{len(got[0])} hits over {k1 << 8} candidates in {t_scan:.3f} s, {st.launches} launches, "
          f"kernel {st.kernel_ms:.2f} ms")


@pytest.mark.parametrize("name", ["len04", "len56", "mid115"])
def test_committed_lists(miner, name):
    """One final block, two final blocks and a midstate: the CPU-scanned lists at N = 8 and N = 9."""
    c = CASES[name]
    t = time.perf_counter()
    for ntz in (8, 9):
        idx, dep = _lists(*miner.scan_cuda(c["nonce"], ntz, 0, 0, c["k_begin"], c["k_end"]))
        assert list(zip(idx, dep)) == [(g, tz) for g, tz in c["hits"] if tz >= ntz]
    print(f"{name}: {len(c['hits'])} hits, two scans in {time.perf_counter() - t:.2f} s")


def test_composes_with_digests_cuda(miner):
    nonce = _nonce(56, 4)
    idx, dep = miner.scan_cuda(nonce, 2, 3, 2, 100, 400)
    dig, dep2 = miner.digests_cuda(nonce, idx)
    assert torch.equal(dep, dep2) and idx.numel() > 20
    for g, d, row in zip(idx.tolist(), dep.tolist(), dig.cpu().tolist()):
        hx = bytes(row).hex()
        assert d >= 2 and hx.endswith("0" * d) and not hx.endswith("0" * (d + 1))
        assert hx == hashlib.md5(nonce + _secret_of(g)).hexdigest()


def test_want_depths_false(miner):
    nonce = _nonce(4, 7)
    idx, dep = miner.scan_cuda(nonce, 1, 0, 0, 0, 300)
    idx2, none = miner.scan_cuda(nonce, 1, 0, 0, 0, 300, want_depths=False)
    assert none is None and torch.equal(idx, idx2) and idx.numel() > 0
    r, idx3, none, k_done = miner.scan_cuda_page(nonce, 1, 0, 0, 0, 300, want_depths=False)
    assert (r, none, k_done) == (EXHAUSTED, None, 300) and torch.equal(idx, idx3)


def test_cancel_raised_on_entry(miner):
    miner.cancel()
    try:
        r, idx, dep, k_done = miner.scan_cuda_page([1, 2, 3, 4], 2, 0, 0, 7, 64)
    finally:
        miner.clear_cancel()
    assert (r, idx.numel(), dep.numel(), k_done) == (CANCELLED, 0, 0, 7)
    assert miner.last_scan_device_stats.launches == 0


def test_cancel_mid_call(miner, golden):
    k_end, out = 1 << 30, {}

    def run():
        out["r"] = miner.scan_cuda_page([1, 2, 3, 4], 32, 0, 0, 0, k_end)
        out["t_end"] = time.perf_counter()

    th = threading.Thread(target=run)
    th.start()
    time.sleep(0.05)
    t_cancel = time.perf_counter()
    miner.cancel()
    th.join(timeout=30)
    miner.clear_cancel()
    assert not th.is_alive()
    r, idx, dep, k_done = out["r"]
    st = miner.last_scan_device_stats
    print(f"device scan cancel latency {(out['t_end'] - t_cancel) * 1e3:.2f} ms at k {k_done}, {st.rounds} slices")
    assert r == CANCELLED and idx.numel() == 0 and 0 <= k_done < k_end
    assert k_done == st.rounds << 20 and st.launches == st.rounds   # whole slices of 2^28, nothing placed
    e = next(e for e in golden["first_hits"] if e["nonce"] == [1, 2, 3, 4] and e["ntz"] == 6)
    res = miner.mine([1, 2, 3, 4], 6)
    assert (res.status, res.global_idx, list(res.secret)) == (FOUND, e["global_idx"], e["secret"])


def test_argument_errors(miner):
    L = distpow.lib()
    dev = torch.device("cuda", miner.device)
    idx = torch.empty(MIN_HITS + 1, dtype=torch.int64, device=dev)
    dep = torch.empty(MIN_HITS, dtype=torch.uint8, device=dev)
    n, kd = ctypes.c_size_t(), ctypes.c_uint64()
    pn, pk = ctypes.byref(n), ctypes.byref(kd)
    nonce = b"\x01\x02\x03\x04"

    def call(nonce=nonce, nlen=4, ntz=1, wb=0, k0=0, k1=4, out=idx.data_ptr(), tz=dep.data_ptr(), max_hits=MIN_HITS,
             n_hits=pn, k_done=pk):
        return L.dpow_scan_device(miner._ctx, nonce, nlen, ntz, wb, 0, k0, k1, out, tz, max_hits, n_hits, k_done, None)

    assert call(out=None) == EINVAL
    assert call(out=idx.data_ptr() + 4) == EINVAL
    assert call(n_hits=None) == EINVAL
    assert call(k_done=None) == EINVAL
    assert call(nonce=None) == EINVAL
    assert call(wb=256) == EINVAL
    assert call(k0=5) == EINVAL
    assert call(nonce=bytes(1025), nlen=1025) == EINVAL
    assert call(max_hits=MIN_HITS - 1) == EINVAL
    assert call(k1=DPOW_K_LIMIT + 1) == ERANGE
    assert L.dpow_scan_device(None, nonce, 4, 1, 0, 0, 0, 4, idx.data_ptr(), None, MIN_HITS, pn, pk, None) == EINVAL
    # an empty window is exhausted without a launch; N > 32 scans and lists nothing
    r, i, d, k_done = miner.scan_cuda_page(nonce, 1, 0, 0, 9, 9)
    assert (r, i.numel(), d.numel(), k_done) == (EXHAUSTED, 0, 0, 9)
    assert miner.last_scan_device_stats.launches == 0
    r, i, d, k_done = miner.scan_cuda_page(nonce, 33, 0, 0, 0, 64)
    assert (r, i.numel(), k_done) == (EXHAUSTED, 0, 64)
    st = miner.last_scan_device_stats
    assert (st.launches, st.rounds, st.candidates) == (1, 1, 64 * 256)
    # the context is still usable, an 8-byte-aligned list that is not 16-byte aligned is fine, and a
    # device scan leaves dpow_stats alone
    miner.reset_stats()
    assert call(out=idx.data_ptr() + 8) == EXHAUSTED and kd.value == 4
    want = _ref_lists(_reference(nonce, 1, 0, 0, 0, 4))
    assert (idx[1:1 + n.value].tolist(), dep[:n.value].tolist()) == want and n.value > 0
    st = miner.stats()
    assert (st.searches, st.launches, st.candidates) == (0, 0, 0)


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
            miner.scan_cuda([1, 2, 3, 4], 2, k_end=8)
        assert e.value.code == EINVAL
    finally:
        miner.attach_node(None)
    assert miner.scan_cuda([1, 2, 3, 4], 0, k_end=1)[0][0].item() == 0
