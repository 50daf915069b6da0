"""Host side of the census (dpow_census_merge, Census), no GPU needed: the fold of two windows'
censuses on hand-made structs, what it refuses (with `into` left as it was), and the Python
Census.merged against the C function."""
import ctypes

import pytest

import distpow
from distpow import Census, DPOW_NO_HIT, EINVAL
from distpow import _lib

D = _lib.CENSUS_DEPTHS
NONE = DPOW_NO_HIT


def _c(counts=(), firsts=(), tzs=(), deepest=None):
    """A dpow_census from the leading entries of its arrays; the rest is empty."""
    c = _lib.CensusC()
    for d in range(D):
        c.count_ge[d] = counts[d] if d < len(counts) else 0
        c.first_ge[d] = firsts[d] if d < len(firsts) else NONE
        c.first_tz[d] = tzs[d] if d < len(tzs) else 0
    c.deepest = max(len(counts) - 1, 0) if deepest is None else deepest
    return c


def _t(c):
    return tuple(c.count_ge), tuple(c.first_ge), tuple(c.first_tz), c.deepest


def _merge(into, nxt):
    return distpow.lib().dpow_census_merge(ctypes.byref(into) if into is not None else None,
                                           ctypes.byref(nxt) if nxt is not None else None)


def _low():   # a window of 1000 candidates from index 256: depth 2 at 300 (its depth 3), nothing deeper
    return _c((1000, 60, 4, 1), (256, 260, 300, 300), (0, 1, 3, 3))


def _high():  # a window above it: the first depth-1 candidate is depth 4
    return _c((500, 30, 2, 1, 1), (70000, 70010, 70010, 70010, 70010), (0, 4, 4, 4, 4))


def test_struct_is_the_headers():
    assert D == 33 and ctypes.sizeof(_lib.CensusC) == 33 * 8 + 33 * 8 + 33 * 4 + 4
    assert {"Census"} <= set(distpow.__all__)
    assert callable(distpow.Miner.census) and callable(distpow.Miner.census_page)


def test_merge_adds_counts_keeps_lower_firsts_takes_max_depth():
    a, b = _low(), _high()
    assert _merge(a, b) == 0
    assert tuple(a.count_ge)[:6] == (1500, 90, 6, 2, 1, 0)
    assert tuple(a.first_ge)[:6] == (256, 260, 300, 300, 70010, NONE)  # the lower window's, where it has one
    assert tuple(a.first_tz)[:6] == (0, 1, 3, 3, 4, 0)
    assert a.deepest == 4
    assert _t(b) == _t(_high())  # next is read only


def test_merge_with_an_empty_census_is_the_identity():
    a, e = _low(), _c()
    assert _merge(a, e) == 0 and _t(a) == _t(_low())
    assert _merge(e, a) == 0 and _t(e) == _t(_low())
    e2 = _c()
    assert _merge(e2, _c()) == 0 and _t(e2) == _t(_c())
    assert _t(_c()) == ((0,) * D, (NONE,) * D, (0,) * D, 0)


def _bad():
    return {
        "count increases with d": _c((10, 2, 3), (5, 6, 7), (0, 1, 2)),
        "count without a first": _c((10, 2, 1), (5, 6), (0, 1, 2), deepest=2),
        "first without a count": _c((10, 2), (5, 6, 7), (0, 1, 2), deepest=1),
        "firsts decrease with d": _c((10, 2, 1), (5, 9, 8), (0, 1, 2)),
        "first_tz below d": _c((10, 2, 1), (5, 6, 7), (0, 1, 1)),
        "deepest too low": _c((10, 2, 1), (5, 6, 7), (0, 1, 2), deepest=1),
        "deepest too high": _c((10, 2, 1), (5, 6, 7), (0, 1, 2), deepest=3),
        "deepest of an empty census": _c(deepest=1),
    }


@pytest.mark.parametrize("what", sorted(_bad()))
def test_merge_refuses_an_inconsistent_census_on_either_side(what):
    bad = _bad()[what]
    into = _low()
    assert _merge(into, bad) == EINVAL, what
    assert _t(into) == _t(_low())
    assert "dpow_census_merge" in _lib.last_error()
    before = _t(bad)
    assert _merge(bad, _high()) == EINVAL, what
    assert _t(bad) == before


def test_merge_refuses_null_and_a_window_that_is_not_above():
    a = _low()
    assert _merge(None, a) == EINVAL and _merge(a, None) == EINVAL and _merge(None, None) == EINVAL
    assert _t(a) == _t(_low())
    # next's first candidate lies below into's deepest first (300), at it, and just above it
    for g0, code in ((299, EINVAL), (300, EINVAL), (301, 0)):
        into, nxt = _low(), _c((5, 1), (g0, g0 + 1), (0, 1))
        assert _merge(into, nxt) == code, g0
        if code:
            assert _t(into) == _t(_low())
    into = _high()
    assert _merge(into, _low()) == EINVAL and _t(into) == _t(_high())  # the wrong way round


def test_python_merged_agrees_with_the_c_function():
    a, b = _low(), _high()
    pa, pb = Census._from_c(a), Census._from_c(b)
    assert _t(pa._to_c()) == _t(a)
    assert _merge(a, b) == 0
    m = pa.merged(pb)
    assert m == Census._from_c(a)
    assert m.first_ge[5] is None and m.first_ge[4] == 70010 and m.deepest == 4
    assert [m.exact(d) for d in range(6)] == [1410, 84, 4, 1, 1, 0] and m.exact(32) == 0
    assert m.secret(4) == distpow.secret_from_index(70010) and m.secret(5) is None
    assert Census.empty().merged(pa) == pa == pa.merged(Census.empty())
    assert Census.empty() == Census._from_c(_c())
    with pytest.raises(distpow.DpowError) as e:
        pb.merged(pa)
    assert e.value.code == EINVAL
