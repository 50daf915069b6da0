"""The segment-inner fixture (tests/golden/seg_inner_hits.json) is what it says it is.

The lists come from tests/golden/fast_scan.c's all-hits mode (gen_golden.py --seg-inner, which
cross-checks that mode against the byte-wise oracle first).  Nothing here trusts the generator:
every entry's digest is recomputed with hashlib, and the conditions the GPU tests lean on (enough
entries, an N = 9 entry behind a D == 0 false positive for every W0, the N = 9 deep golden in w1,
the window shapes) are re-checked.  That every hit of a window is listed -- completeness -- is
the scanner's part; it is pinned by the generator's oracle walks, not here.
"""
import hashlib
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SEG = 1 << 24
K_LIMIT = (1 << 55) - 1  # include/dpow.h DPOW_K_LIMIT
NAMES = ["w0", "w1", "w2", "w3", "m0", "m3", "l56", "l67", "top"]


def load_cases():
    with open(os.path.join(HERE, "golden", "seg_inner_hits.json")) as f:
        doc = json.load(f)
    assert doc["ntz"] == 8
    return {c["name"]: c for c in doc["cases"]}


def secret_of(g):
    out, k = [g & 0xFF], g >> 8
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return bytes(out)


def tz_of(nonce, g):
    h = hashlib.md5(bytes(nonce) + secret_of(g)).hexdigest()
    return len(h) - len(h.rstrip("0"))


def n9_after_8(hits):
    """An entry with tz >= 9 behind an entry with tz = 8."""
    seen8 = False
    for _, tz in hits:
        if tz == 8:
            seen8 = True
        elif seen8 and tz >= 9:
            return True
    return False


def w0_of(case):
    return (len(case["nonce"]) % 64) // 4


@pytest.fixture(scope="module")
def cases():
    return load_cases()


def test_case_names_and_nonce_lengths(cases):
    assert list(cases) == NAMES
    assert {len(c["nonce"]) for c in cases.values()} == {0, 4, 8, 12, 64, 76}
    assert [len(cases[n]["nonce"]) for n in NAMES] == [0, 4, 8, 12, 64, 76, 4, 4, 4]
    for n in ("w1", "l56", "l67", "top"):
        assert cases[n]["nonce"] == [1, 2, 3, 4]
    for c in cases.values():  # the layouts with a segment-inner kernel: one final block, SH = 0, W0 <= 3
        assert len(c["nonce"]) % 4 == 0 and w0_of(c) <= 3
        assert all(0 <= b <= 255 for b in c["nonce"])


@pytest.mark.parametrize("name", NAMES)
def test_entries_are_sorted_inside_the_window_and_hashlib_agrees(cases, name):
    c = cases[name]
    gs = [g for g, _ in c["hits"]]
    assert gs == sorted(set(gs))
    assert all(c["k_begin"] <= g >> 8 < c["k_end"] for g in gs)
    for g, tz in c["hits"]:
        assert tz >= 8 and tz_of(c["nonce"], g) == tz, (name, g, tz)
    assert len(c["hits"]) >= 4


def test_window_shapes(cases):
    for c in cases.values():
        n_seg = (c["k_end"] - 1) // SEG - c["k_begin"] // SEG + 1
        assert c["k_begin"] >= SEG and 8 <= n_seg <= 65 and c["k_end"] <= K_LIMIT, c["name"]
    for n in ("w0", "w1", "w2", "w3", "m0", "m3"):  # unaligned at both ends
        assert cases[n]["k_begin"] % SEG and cases[n]["k_end"] % SEG, n
    assert cases["w1"]["k_begin"] // SEG == 1 and (cases["w1"]["k_end"] - 1) // SEG == 32
    for n, edge in (("l56", 1 << 40), ("l67", 1 << 48)):  # at least 4 segments on each side
        assert cases[n]["k_begin"] <= edge - 4 * SEG and edge + 4 * SEG <= cases[n]["k_end"], n
    assert cases["top"]["k_end"] == K_LIMIT and cases["top"]["k_begin"] <= K_LIMIT - 8 * SEG


def test_every_w0_has_an_n9_entry_behind_an_n8_one(cases):
    by_w0 = {}
    for c in cases.values():
        by_w0.setdefault(w0_of(c), []).append(n9_after_8(c["hits"]))
    assert sorted(by_w0) == [0, 1, 2, 3]
    assert all(any(v) for v in by_w0.values()), by_w0


def test_w1_holds_the_n9_deep_golden_first(cases, golden):
    e = next(x for x in golden["deep_hits"] if x["nonce"] == [1, 2, 3, 4] and x["ntz"] == 9)
    assert e["global_idx"] == 48853296051 and (e["global_idx"] >> 8) // SEG == 11
    hits = cases["w1"]["hits"]
    first9 = next(g for g, tz in hits if tz >= 9)
    assert first9 == e["global_idx"]
    assert n9_after_8(hits)
    assert sum(1 for g, tz in hits if g < first9) >= 4  # D == 0 false positives of an N = 9 search before it
