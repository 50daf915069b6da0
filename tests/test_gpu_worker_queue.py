"""The worker's queue mode on the GPU (dpow_worker_set_queue, Worker(queue=True)): the first window
of each Mine goes through the worker's task queue, and the reference's protocol -- two messages per
task, the trace actions, the cache -- is what it is with the mode off.  Expected secrets come from
tests/golden/pow_golden.json and the CPU oracle."""
import random
import time

import pytest

import distpow
from distpow.worker import Worker

pytestmark = pytest.mark.gpu

N1 = [1, 2, 3, 4]


def actions(w, token=None):
    return [t["action"] for t in w.trace() if token is None or t["trace"] == token]


def test_mine_found_protocol_through_the_queue(golden):
    e = next(x for x in golden["first_hits"] if x["nonce"] == N1 and x["ntz"] == 6)
    with Worker(0, queue=True) as w:
        w.mine(N1, 6, 0, 0, token=11)
        r = w.next_result(30000)
        assert r.secret == bytes(e["secret"]) and r.token == 11
        assert w.next_result(100) is None
        w.found(N1, 6, 0, r.secret, token=11)
        assert w.next_result(5000).secret is None
        assert w.next_result(100) is None
        assert actions(w, 11) == ["WorkerMine", "CacheMiss", "WorkerResult", "CacheAdd", "WorkerCancel"]
        assert w.active_tasks() == 0


def test_first_window_without_a_hit_continues_on_a_context(golden):
    """N = 7 has no hit in k < 2^16: the queue answers EXHAUSTED and the miner goes on with dpow_search."""
    e = next(x for x in golden["first_hits"] if x["nonce"] == N1 and x["ntz"] == 7)
    assert e["global_idx"] >> 8 >= 1 << 16
    with Worker(0, queue=True) as w:
        w.mine(N1, 7, 0, 0, token=3)
        r = w.next_result(30000)
        assert r.secret == bytes(e["secret"]) == bytes([194, 170, 210, 13])
        w.found(N1, 7, 0, r.secret, token=3)
        assert w.next_result(5000).secret is None
        assert actions(w, 3) == ["WorkerMine", "CacheMiss", "WorkerResult", "CacheAdd", "WorkerCancel"]


def test_cancel_and_found_while_mining_send_two_nils():
    with Worker(0, queue=True) as w:
        w.mine(N1, 32, 1, 1, token=5)     # unreachable: mines until killed
        w.cancel(N1, 32, 1)               # at once: the kill may reach the task while it is still queued
        a, b = w.next_result(10000), w.next_result(10000)
        assert a is not None and b is not None and a.secret is None and b.secret is None
        assert w.next_result(100) is None
        assert actions(w, 5) == ["WorkerMine", "CacheMiss", "WorkerCancel"]
        w.mine(N1, 32, 3, 2, token=8)
        time.sleep(0.05)                  # past its first window: the kill reaches dpow_search
        w.found(N1, 32, 3, [1, 2, 3], token=8)
        assert w.next_result(10000).secret is None
        assert w.next_result(10000).secret is None
        assert actions(w, 8) == ["WorkerMine", "CacheMiss", "CacheAdd", "WorkerCancel"]
        assert w.active_tasks() == 0


def test_many_small_mines_at_once(oracle):
    """64 concurrent Mines of fresh nonces: every result is the oracle's first hit, two messages each."""
    rnd = random.Random(20251025)
    nonces = [bytes(rnd.randrange(256) for _ in range(4)) for _ in range(64)]
    want = {}
    for i, n in enumerate(nonces):
        r = oracle.mine_window(list(n), 3, 0, 0, 0, 1 << 16)
        assert r is not None
        want[i] = bytes(r[0])
    with Worker(0, queue=True) as w:
        for i, n in enumerate(nonces):
            w.mine(n, 3, 0, 0, token=i)
        got = {}
        for _ in range(64):
            r = w.next_result(20000)
            assert r is not None and r.error == 0 and r.secret is not None
            got[r.token] = r.secret
        assert got == want
        for i, n in enumerate(nonces):
            w.found(n, 3, 0, got[i], token=i)
        for _ in range(64):
            r = w.next_result(20000)
            assert r is not None and r.secret is None
        assert w.next_result(100) is None
        assert w.active_tasks() == 0


def test_queue_mode_off_is_the_default(golden):
    e = next(x for x in golden["first_hits"] if x["nonce"] == N1 and x["ntz"] == 5)
    with Worker(0) as w:
        w.set_queue(True)
        w.set_queue(False)
        w.mine(N1, 5, 0, 0, token=1)
        r = w.next_result(30000)
        assert r.secret == bytes(e["secret"])
        w.found(N1, 5, 0, r.secret, token=1)
        assert w.next_result(5000).secret is None
