"""The case table behind tests/golden/batch_queue_plans.json: inputs of the two launch planners
(dpow_batch_plan, dpow_queue_plan) and what is recorded of their outputs.  Shared by the recording
script (tests/golden/gen_batch_queue_plans.py) and tests/test_plan_golden.py.

A case is a short descriptor, expanded here to the planner's inputs, so that the file stays small:
  ["batch", n, shape, edge]   n windows; `shape` names their lengths, `edge` in {-1, 0, 1} ends them
                              below, at or above the end of round 1's slice
  ["queue", n, ages, left]    n live tasks; `ages` and `left` name the two input lists
Recorded per case: the launch count (batch) or the budget (queue), the group(s), the number of
entries and a digest of the entry list as the library returned it (the raw dpow_batch_range array).
"""
import hashlib

NS = (1, 2, 3, 255, 256, 257, 1024)
FIRST, CAP, MIN_SLICE = 1 << 20, 1 << 28, 256   # csrc/batch.h

BATCH_SHAPES = ("even", "mixed_bits", "long_among_short")
QUEUE_AGES = tuple("age%d" % a for a in range(10)) + ("cycle", "zero_beside_eight", "one_old")
QUEUE_LEFTS = ("long", "edges")


def pow2_floor(x):
    return 1 << (x.bit_length() - 1) if x else 0


def round_slice(r, n):
    return max(pow2_floor(min(FIRST << (2 * min(r, 8)), CAP) // n), MIN_SLICE)


def table():
    for n in NS:
        for shape in BATCH_SHAPES:
            for edge in (-1, 0, 1):
                yield ["batch", n, shape, edge]
    for n in NS:
        for ages in QUEUE_AGES:
            for left in QUEUE_LEFTS:
                yield ["queue", n, ages, left]


def batch_windows(n, shape, edge):
    """[(k_begin, k_end, worker_bits)]: local lengths that end `edge` from the end of round 1's slice."""
    two = round_slice(0, n) + round_slice(1, n) + edge        # local indices
    if shape == "even":            # worker_bits 8: one thread byte per k, local index = k
        return [(7, 7 + two, 8)] * n
    if shape == "mixed_bits":      # rbits 8, 5, 0, 8 (the % 9 quirk): lengths in k, rounded up
        out = []
        for i in range(n):
            wbits = (0, 3, 8, 9)[i % 4]
            rb = 8 - wbits % 9
            out.append((i, i + ((two + (1 << rb) - 1 + edge * (i % 3)) >> rb), wbits))
        return out
    out = [(3, 3 + 4 + edge, 0)] * n   # short windows of 3..5 k, one task of 2^22 k among them
    out[n // 2] = (1 << 24, (1 << 24) + (1 << 22) + edge, 0)
    return out


def queue_inputs(n, ages, left):
    if ages.startswith("age"):
        a = [int(ages[3:])] * n
    elif ages == "cycle":
        a = [i % 10 for i in range(n)]
    elif ages == "zero_beside_eight":     # one fresh task beside old ones
        a = [8] * n
        a[0] = 0
    else:                                 # one old task among fresh ones
        a = [0] * n
        a[n - 1] = 8
    if left == "long":
        lf = [1 << 40] * n
    else:   # around every task's own share of a batch of this size at its age, and very short
        lf = []
        for i in range(n):
            s = round_slice(a[i], n)
            lf.append((s - 1, s, s + 1, 1, 3 * s + 17)[i % 5])
    return lf, a


def digest(entries):
    return hashlib.sha256(bytes(entries)).hexdigest()[:16]


def record(case):
    """What the library in use plans for one case."""
    import distpow
    if case[0] == "batch":
        entries, launches = distpow.batch_plan(batch_windows(*case[1:]))
        groups = []
        for e in entries:
            if e.launch == len(groups):
                groups.append([e.group, e.rows])
        return [launches, groups, len(entries), digest(entries)]
    lf, a = queue_inputs(*case[1:])
    blocks, budget = distpow.queue_plan(lf, a)
    return [budget, blocks[0].group, len(blocks), digest(blocks)]
