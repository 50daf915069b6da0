"""The batched scan's planner with a weight budget that never binds is the batched census's planner.

At ntz = 7 a part of n local indices weighs ceil(n / 2^28).  A launch holds at most 2^28 local
indices, so its parts' weights sum to at most 1 + the number of parts: at most 4097 for the 4096
tasks a call can hold, against a budget of 65536 / 4 = 16384.  dpow_scan_plan on the tasks' local
ranges must then return byte for byte what dpow_census_plan returns on their windows.  CPU only."""
import random

import pytest

import distpow


def _windows(seed, n, max_k):
    """n windows (k_begin, k_end, worker_bits) of up to max_k k: every width, some empty, one in 64 long."""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        wbits = rnd.randrange(10)
        k0 = rnd.choice((0, 3, 250, 65530, 1 << 24, rnd.randrange(1 << 40)))
        size = rnd.choice((0, 1, rnd.randrange(1, 40), rnd.randrange(1, 40), rnd.randrange(1, max_k)))
        if rnd.randrange(64) == 0:
            size = rnd.randrange(1, 64 * max_k)
        out.append((k0, k0 + size, wbits))
    return out


# A plan has a descriptor per 256 local indices at the least: windows sized to the budget keep it short,
# and those of the call's own budget are long enough for launches of 2^28 local indices.
MAX_K = {0: 1 << 13, 256: 4, 1 << 20: 200}


@pytest.mark.parametrize("cap", [0, 256, 1 << 20])
@pytest.mark.parametrize("seed, n", [(1, 1), (2, 7), (3, 300), (4, 4096)])
def test_scan_plan_at_ntz_7_is_census_plan(seed, n, cap):
    windows = _windows(seed, n, MAX_K[cap])
    local = [(k0 << (8 - w % 9), k1 << (8 - w % 9), 7) for k0, k1, w in windows]
    c_blocks, c_launches = distpow.census_plan(windows, cap)
    s_blocks, s_launches = distpow.scan_plan(local, cap, 65536)
    assert s_launches == c_launches and len(s_blocks) == len(c_blocks) > 0
    assert bytes(s_blocks) == bytes(c_blocks)
