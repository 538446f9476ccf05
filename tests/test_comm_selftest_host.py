"""What c2r_comm_selftest rests on, without a GPU: (a) the pattern of include/c2ray_hip.h restated in numpy -- its sums are
exact in every association, cannot pass through fp32, and notice a rank left out or added twice; (b) RcclComm.selftest turns
one rank's failure into every rank's, over gloo, with a stub in the engine's place."""
import multiprocessing as mp
import os
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
RANKS = (2, 3, 8, 64, 4095)


def splitmix64(i):
    i = np.asarray(i, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = i + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def pattern(i):
    """a(i) (odd, 30 significant bits) and e(i) in [-60, 60]"""
    h = splitmix64(i)
    a = ((np.uint64(1) << np.uint64(29)) + (h & np.uint64((1 << 29) - 1))) | np.uint64(1)
    e = ((h >> np.uint64(32)) % np.uint64(121)).astype(np.int64) - 60
    return a, e


def contributions(n, i):
    """v(r, i) for r = 0 .. n-1, shape (n, len(i)), and the closed form of their sum"""
    a, e = pattern(i)
    r1 = np.arange(1, n + 1, dtype=np.uint64)[:, None]
    v = np.ldexp((r1 * a[None, :]).astype(np.float64), e[None, :].astype(np.int32))
    expected = np.ldexp((np.uint64(n * (n + 1) // 2) * a).astype(np.float64), e.astype(np.int32))
    return v, expected


def sample_indices(rng, count=192):
    small = np.arange(0, 64, dtype=np.uint64)
    big = rng.integers(0, 1 << 40, size=count - 66, dtype=np.uint64)
    return np.concatenate([small, big, np.array([(1 << 40) - 1, 4 * 256 ** 3 + 47], dtype=np.uint64)])


def test_pattern_has_the_stated_shape():
    i = sample_indices(np.random.default_rng(1))
    a, e = pattern(i)
    assert np.all(a % np.uint64(2) == 1) and np.all(a >= 1 << 29) and np.all(a < 1 << 30)
    assert e.min() >= -60 and e.max() <= 60
    assert len(np.unique(a)) > len(i) // 2 and len(np.unique(e)) > 20     # both vary with i: a range at a wrong offset is seen
    # the largest partial sum of the largest communicator is an integer below 2^53
    assert 4095 * 4096 // 2 * ((1 << 30) - 1) < 1 << 53
    # splitmix64 as published (first output of a generator seeded with 0)
    assert int(splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("n", RANKS)
def test_sum_is_exact_in_every_association(n):
    rng = np.random.default_rng(n)
    v, expected = contributions(n, sample_indices(rng))
    assert np.array_equal(np.cumsum(v, axis=0)[-1], expected)             # rank order (np.cumsum adds sequentially)
    assert np.array_equal(np.cumsum(v[::-1], axis=0)[-1], expected)       # reverse order
    parts = [v[r] for r in range(n)]                                      # a random pairwise tree
    while len(parts) > 1:
        j, k = sorted(rng.choice(len(parts), size=2, replace=False))
        b = parts.pop(k)
        parts[j] = parts[j] + b
    assert np.array_equal(parts[0], expected)


@pytest.mark.parametrize("n", RANKS)
def test_closed_form_does_not_survive_fp32_nor_a_wrong_set_of_ranks(n):
    rng = np.random.default_rng(100 + n)
    v, expected = contributions(n, sample_indices(rng))
    assert np.all(expected.astype(np.float32).astype(np.float64) != expected)
    total = np.cumsum(v, axis=0)[-1]
    for r in {0, n // 2, n - 1}:
        assert np.all(total - v[r] != expected) and np.all(total + v[r] != expected)   # rank r left out / added twice
        if n > 1:
            assert np.all(v[r] != expected)                                            # ... or left un-reduced


class StubEngine:
    """what RcclComm needs of an engine; its self-test fails on rank `bad`"""
    bad = 1

    def __init__(self, rank):
        self.rank = rank

    @staticmethod
    def comm_available():
        return None

    @staticmethod
    def comm_unique_id():
        return b"\0" * 128

    def comm_size(self):
        return 1

    def comm_init(self, rank, size, uid):
        assert len(uid) == 128

    def comm_destroy(self):
        pass

    def comm_selftest(self, nslab=4):
        if self.rank == self.bad:
            raise RuntimeError(f"c2r_comm_selftest: the sum over the 2 ranks came back WRONG (stub, rank {self.rank})")
        return {"ranks": 2, "mismatches": [0, 0]}


def _rank(rank, port, bad, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    parallel = ge.load_package().parallel
    eng = StubEngine(rank)
    eng.bad = bad
    comm = parallel.RcclComm(eng, dist)
    try:
        q.put((rank, "ok", comm.selftest()))
    except RuntimeError as ex:
        q.put((rank, "raised", str(ex)))
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(bad):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000) + (0 if bad is None else 1 + bad)
    procs = [ctx.Process(target=_rank, args=(r, port, bad, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict()
    try:
        for _ in range(2):
            rank, what, val = q.get(timeout=300)
            got[rank] = (what, val)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return got


def test_rcclcomm_selftest_one_failure_is_everybodys():
    got = _two_ranks(1)
    assert got[0][0] == got[1][0] == "raised", got
    assert got[0][1] == got[1][1] and "rank 1: c2r_comm_selftest" in got[0][1] and "WRONG" in got[0][1], got


def test_rcclcomm_selftest_returns_every_ranks_report():
    got = _two_ranks(None)
    assert got[0] == got[1] == ("ok", {"ranks": 2, "mismatches": [0, 0]}), got
