"""The per-layout fixture (tests/golden/layout_deep_hits.json) is what it says it is.

The lists come from tests/golden/fast_scan.c's all-hits mode (gen_golden.py --layouts, which
cross-checks the scanner's two-final-block layout against the byte-wise oracle first), at windows
placed by tests/golden/layout_hints.json.  Nothing here trusts the generator or the hints: every
entry's digest is recomputed with hashlib, the layout each case claims is the one the planner
gives its candidates, the cases cover every specialised layout <NBLK, W0, SH>
(md5_variants.h variant_exists), and a sample of windows is re-scanned with the byte-wise oracle,
which shares nothing with fast_scan.
"""
import hashlib
import json
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

import distpow

HERE = os.path.dirname(os.path.abspath(__file__))
SEG = 1 << 24
K_LIMIT = (1 << 55) - 1  # include/dpow.h DPOW_K_LIMIT
SHALLOW_OK = {"b1w13s1", "ls1", "ls2"}  # tz >= 9 not required of these (tools/layout_hints.py)
# windows re-scanned by the byte-wise oracle: two final blocks at chunk lengths 4 and 7, a
# midstate in front of two final blocks, one block at chunk length 7, and every tiny range
ORACLE_SAMPLE = ["len51", "len63", "b2w12s0", "mid115", "c7", "b1w12s3", "b1w13s0", "b1w13s1", "ls1", "ls2"]


def load_doc():
    with open(os.path.join(HERE, "golden", "layout_deep_hits.json")) as f:
        return json.load(f)


DOC = load_doc()
CASES = {c["name"]: c for c in DOC["cases"]}
NAMES = list(CASES)


def secret_of(g):
    out, k = [g & 0xFF], g >> 8
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return bytes(out)


def tz_of(nonce, g):
    h = hashlib.md5(bytes(nonce) + secret_of(g)).hexdigest()
    return len(h) - len(h.rstrip("0"))


def all_layouts():
    """md5_variants.h variant_exists."""
    return {(1, w0, sh) for w0 in range(14) for sh in range(4)} | {(2, w0, sh) for w0 in range(12, 16) for sh in range(4)}


def test_case_names_and_shapes():
    assert DOC["ntz"] == 8
    assert NAMES[:64] == [f"len{n:02d}" for n in range(64)]
    assert [len(CASES[n]["nonce"]) for n in NAMES[:64]] == list(range(64))
    assert NAMES[64:] == ["b2w12s2", "b2w12s1", "b2w12s0", "b1w12s3", "b1w13s0", "b1w13s1", "c5", "c6", "c7",
                          "mid69", "mid115", "mid190", "ls1", "ls2"]
    assert [len(CASES[n]["nonce"]) for n in NAMES[64:]] == [50, 49, 48, 51, 52, 53, 5, 22, 35, 69, 115, 190, 8, 56]
    for c in CASES.values():
        assert all(0 <= b <= 255 for b in c["nonce"])
        assert 1 <= c["k_begin"] < c["k_end"] <= K_LIMIT


def test_window_positions():
    """Chunk length 4 for len00 ... len63 and the midstate cases, the k ranges the other layouts
    need, at most two 2^24-k segments, an unaligned begin unless the chunk length's first k clips it."""
    def chunk_len(k):
        return len(secret_of(k << 8)) - 1
    for n in NAMES[:64] + ["mid69", "mid115", "mid190"]:
        c = CASES[n]
        assert chunk_len(c["k_begin"]) == chunk_len(c["k_end"] - 1) == 4, n
    for n, lo in (("b2w12s2", 1 << 32), ("b2w12s1", 1 << 40), ("b2w12s0", 1 << 48), ("c5", 1 << 32),
                  ("c6", 1 << 40), ("c7", 1 << 48)):
        assert CASES[n]["k_begin"] >= lo and chunk_len(CASES[n]["k_begin"]) == chunk_len(CASES[n]["k_end"] - 1), n
    assert [chunk_len(CASES[n]["k_begin"]) for n in ("c5", "c6", "c7")] == [5, 6, 7]
    for n, rng in (("b1w12s3", (1 << 16, 1 << 24)), ("b1w13s0", (1 << 8, 1 << 16)), ("b1w13s1", (1, 1 << 8)),
                   ("ls1", (1, 1 << 16)), ("ls2", (1, 1 << 16))):
        assert (CASES[n]["k_begin"], CASES[n]["k_end"]) == rng, n
    for n, c in CASES.items():
        if c["k_end"] <= SEG:
            continue
        assert c["k_end"] - c["k_begin"] <= 2 * SEG and (c["k_end"] % SEG == 0 or c["k_end"] == K_LIMIT), n
        clipped = c["k_begin"] == 1 << (8 * (chunk_len(c["k_begin"]) - 1))
        assert c["k_begin"] % SEG or clipped, n


@pytest.mark.parametrize("name", NAMES)
def test_entries_are_sorted_inside_the_window_and_hashlib_agrees(name):
    c = CASES[name]
    gs = [g for g, _ in c["hits"]]
    assert gs and gs == sorted(set(gs))  # strictly increasing
    assert all(c["k_begin"] <= g >> 8 < c["k_end"] for g in gs)
    for g, tz in c["hits"]:
        assert tz >= 8 and tz_of(c["nonce"], g) == tz, (name, g, tz)
    assert c["deep"] == any(tz >= 9 for _, tz in c["hits"])


@pytest.mark.parametrize("name", NAMES)
def test_layout_is_the_planners(name):
    """nblk / w0 / sh of the case are what the planner gives each entry's candidate and the window's
    ends: dpow_plan_window's launch over the entry's k, dpow_plan_candidate's block count, and the
    thread byte sitting at byte sh of word w0 of the words the kernel hashes."""
    c = CASES[name]
    lay = (c["nblk"], c["w0"], c["sh"])
    for k in [c["k_begin"], c["k_end"] - 1] + [g >> 8 for g, _ in c["hits"]]:
        pl = distpow.plan_window(c["nonce"], 0, 0, k, k + 1, 8)
        assert len(pl) == 1 and (pl[0].nblk, pl[0].w0, pl[0].sh) == lay and not pl[0].start_kernel, (name, k)
    for g, _ in c["hits"]:
        _, words, nblk = distpow.plan_candidate(c["nonce"], 0, 0, g)  # workerBits 0: local index = global index
        assert nblk == c["nblk"] and len(words) == 16 * nblk
        assert (words[c["w0"]] >> (8 * c["sh"])) & 0xFF == g & 0xFF
        _, zero, _ = distpow.plan_candidate(c["nonce"], 0, 0, g & ~0xFF)
        assert [i for i in range(len(words)) if words[i] != zero[i]] == ([c["w0"]] if g & 0xFF else [])


def test_ls_cases_run_the_spanning_kernels():
    """ls1 / ls2 at workerBits 0: the N = 8 and N = 9 windows are one launch
    that spans chunk lengths (the "_ls" kernels), one final block and two; at workerBits 8 (one thread
    byte, no spanning) the same lists reach the per-length kernels."""
    for name, nblk, lens in (("ls1", 1, (1, 2)), ("ls2", 2, (1, 2))):
        c = CASES[name]
        for ntz in (8, 9):
            pl = distpow.plan_window(c["nonce"], 0, 0, c["k_begin"], c["k_end"], ntz)
            assert [(p.nblk, p.sh, p.chunk_len, p.chunk_len_last) for p in pl] == [(nblk, 0) + lens], (name, ntz)
        pl = distpow.plan_window(c["nonce"], c["hits"][0][0] & 0xFF, 8, c["k_begin"], c["k_end"], 8)
        assert [(p.chunk_len, p.chunk_len_last) for p in pl] == [(1, 1), (2, 2)], name


def test_every_layout_is_covered():
    un = {(u["nblk"], u["w0"], u["sh"]) for u in DOC["unreachable"]}
    assert un == {(1, 13, 2), (1, 13, 3)} and len(DOC["unreachable"]) == 2
    assert all(u["reason"] for u in DOC["unreachable"])
    have = {(c["nblk"], c["w0"], c["sh"]) for c in CASES.values()}
    assert not have & un
    assert have | un == all_layouts() and len(all_layouts()) == 72
    # the unreachable ones have no k >= 1 that fits one block: every launch of those nonce lengths is two blocks
    for u in DOC["unreachable"]:
        ln = 4 * u["w0"] + u["sh"]
        assert ln + 1 + 1 + 9 > 64
        assert all(p.nblk == 2 or p.start_kernel for p in distpow.plan_window([7] * ln, 0, 0, 0, 1 << 25, 8))


def test_deep_everywhere_but_where_allowed():
    shallow = {n for n, c in CASES.items() if not c["deep"]}
    assert shallow <= SHALLOW_OK, shallow
    # deep layouts: every reachable one has a case with a tz >= 9 entry
    deep_layouts = {(c["nblk"], c["w0"], c["sh"]) for c in CASES.values() if c["deep"]}
    assert deep_layouts | {(1, 13, 1)} | {(1, 13, 2), (1, 13, 3)} == all_layouts()


def test_a_third_of_chunk_length_4_reach_their_n9_entry_in_the_second_segment():
    second = [n for n in NAMES[:64]
              if (next(g for g, tz in CASES[n]["hits"] if tz >= 9) >> 8) // SEG > CASES[n]["k_begin"] // SEG]
    assert 3 * len(second) >= 64, second


def _oracle_hits_of_thread_byte(oracle, nonce, tb, k0, k1):
    """Every N >= 8 hit of one thread byte over [k0, k1): the byte-wise oracle (workerBits 8: the
    partition of that one thread byte) walked hit by hit, the window split over host threads."""
    def part(a, b):
        out, k = [], a
        while k < b:
            r = oracle.mine_window(nonce, 8, tb, 8, k, b)
            if r is None:
                break
            out.append(r[1])
            k = (r[1] >> 8) + 1
        return out
    step = 1 << 21
    spans = [(a, min(k1, a + step)) for a in range(k0, k1, step)]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return [g for hs in ex.map(lambda s: part(*s), spans) for g in hs]


@pytest.mark.parametrize("name", ORACLE_SAMPLE)
def test_oracle_rescan_of_one_thread_byte_equals_the_list(oracle, name):
    """Completeness on a sample: for the thread byte of the case's deepest entry (every thread byte
    where the whole range is 255 k), the oracle's hits over the whole window are the list's."""
    c = CASES[name]
    deepest = max(c["hits"], key=lambda e: e[1])[0]
    tbs = range(256) if c["k_end"] <= 256 else [deepest & 0xFF]
    for tb in tbs:
        got = _oracle_hits_of_thread_byte(oracle, c["nonce"], tb, c["k_begin"], c["k_end"])
        assert got == [g for g, _ in c["hits"] if g & 0xFF == tb], (name, tb)
    assert deepest & 0xFF in tbs
