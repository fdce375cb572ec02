"""The in-process world of tests/loopback_dist.py, checked without a GPU: its two collectives against a direct NumPy statement of
their semantics, uniq.first_seen through it with the NumPy tables of tests/test_uniq_sharded.py on the shard shapes that
tests/test_uniq_exchange_world_gpu.py runs on the device kernels, the two damage hooks (the comparison can fail), and a rank
that raises (the world ends at once, with that rank's exception)."""
import threading
import time

import numpy as np
import pytest
import torch

from tests import loopback_dist as LD
from tests.test_uniq_exchange_world_gpu import ORDERS, check_generator, mismatches, world_job
from tests.test_uniq_sharded import OracleTable, RowsTable

WORLDS = [1, 2, 3, 8]


def _splits(rng, world):
    """split[r][p] = rows rank r sends to rank p: unequal, about a third of them zero, one rank that sends nothing"""
    split = rng.integers(0, 7, size=(world, world))
    split[rng.random((world, world)) < 0.3] = 0
    split[world // 2] = 0
    return split


@pytest.mark.parametrize("cols", [None, 2], ids=["1-D", "rows_of_2"])
@pytest.mark.parametrize("world", WORLDS)
def test_all_to_all_single_against_its_numpy_statement(world, cols):
    """out of rank r = for p = 0 .. world - 1 in turn, the rows [cuts_p[r], cuts_p[r + 1]) of rank p's input"""
    rng = np.random.default_rng(10 * world + (cols or 0))
    split = _splits(rng, world)
    shape = lambda n: (n,) if cols is None else (n, cols)           # noqa: E731
    inputs = [rng.integers(-2 ** 62, 2 ** 62, size=shape(int(split[r].sum()))) for r in range(world)]
    cuts = [np.r_[0, np.cumsum(split[r])] for r in range(world)]
    expect = [np.concatenate([inputs[p][cuts[p][r]:cuts[p][r + 1]] for p in range(world)]) for r in range(world)]
    w = LD.World(world)

    def rank_fn(r):
        out = torch.full(shape(int(split[:, r].sum())), -1, dtype=torch.int64)
        w.all_to_all_single(out, torch.from_numpy(inputs[r].copy()), output_split_sizes=split[:, r].tolist(), input_split_sizes=split[r].tolist())
        return out.numpy()

    got = w.run(rank_fn)
    for r in range(world):
        assert np.array_equal(got[r], expect[r]), r
    assert w.all_to_all_calls == [1] * world


@pytest.mark.parametrize("world", WORLDS)
def test_all_to_all_single_without_splits_is_an_equal_split(world):
    """the form first_seen uses for the counts: input row p goes to rank p, output row p comes from rank p"""
    w = LD.World(world)
    inputs = [np.arange(world, dtype=np.int64) + 100 * r for r in range(world)]

    def rank_fn(r):
        out = torch.empty(world, dtype=torch.int64)
        w.all_to_all_single(out, torch.from_numpy(inputs[r].copy()))
        return out.numpy()

    got = w.run(rank_fn)
    for r in range(world):
        assert got[r].tolist() == [100 * p + r for p in range(world)]


def test_all_to_all_single_refuses_a_slice_of_the_wrong_length():
    """rank 1 promises room for 2 rows of rank 0, which sends it 3: rank 1's assertion is the error reported"""
    w = LD.World(2)
    split = {0: ([1, 3], [1, 0]), 1: ([0, 2], [2, 2])}              # rank: (input splits, output splits)

    def rank_fn(r):
        i, o = split[r]
        w.all_to_all_single(torch.zeros(sum(o), dtype=torch.int64), torch.zeros(sum(i), dtype=torch.int64), output_split_sizes=o, input_split_sizes=i)

    with pytest.raises(AssertionError, match="rank 1 expects 2 rows of rank 0, which sends 3"):
        w.run(rank_fn)


@pytest.mark.parametrize("cols", [None, 2], ids=["1-D", "rows_of_2"])
@pytest.mark.parametrize("world", WORLDS)
def test_all_gather_against_its_numpy_statement(world, cols):
    rng = np.random.default_rng(20 * world + (cols or 0))
    shape = (5,) if cols is None else (5, cols)
    inputs = [rng.integers(-2 ** 62, 2 ** 62, size=shape) for _ in range(world)]
    w = LD.World(world)

    def rank_fn(r):
        outs = [torch.full(shape, -1, dtype=torch.int64) for _ in range(world)]
        w.all_gather(outs, torch.from_numpy(inputs[r].copy()))
        return [o.numpy() for o in outs]

    got = w.run(rank_fn)
    for r in range(world):
        for p in range(world):
            assert np.array_equal(got[r][p], inputs[p]), (r, p)
    assert w.all_gather_calls == [1] * world


def test_the_world_exists_only_inside_its_ranks():
    w = LD.World(3)
    assert w.is_available() and not w.is_initialized()
    assert w.run(lambda r: (w.is_initialized(), w.get_world_size(), w.get_rank())) == [(True, 3, r) for r in range(3)]
    assert not w.is_initialized()


# ---- uniq.first_seen through the loopback, NumPy tables ------------------------------------------------------------------------
BRANCHES = {"device_rows": (RowsTable, "partition"), "torch_ops": (OracleTable, "partition"), "allgather": (OracleTable, "allgather")}


def _first_seen_world(monkeypatch, job, branch, damage=None, table_of=None):
    from circkit_amd import uniq
    make, exchange = BRANCHES[branch]
    w = LD.install(monkeypatch, job.world, damage)

    def rank_fn(rank):
        table = table_of(rank) if table_of else make()
        fs, keep = uniq.first_seen(table, torch.from_numpy(job.shards[rank].view(np.int64).copy()), base_index=int(job.bases[rank]),
                                   exchange=exchange)
        if branch == "device_rows":
            assert table.partitioned and table.gathered
        return fs.numpy(), keep.numpy()

    return w, w.run(rank_fn)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_the_shard_shapes_meet_their_conditions(world, order):
    """at least 10 % of the records have their first occurrence on another rank, the kept count is the number of distinct
    keys, every owner receives rows, the ~0 key sits on several ranks -- from the restatement alone"""
    check_generator(world_job(world, order))


@pytest.mark.parametrize("branch", sorted(BRANCHES))
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_first_seen_through_the_loopback(monkeypatch, world, order, branch):
    """every record of every rank equals uniq_keys.expected_first_seen over the joined shards, on all three branches"""
    job = world_job(world, order)
    w, results = _first_seen_world(monkeypatch, job, branch)
    assert mismatches(job, results) == 0
    if branch == "allgather":
        assert w.all_gather_calls == [2] * world and w.all_to_all_calls == [0] * world
    else:
        assert w.all_to_all_calls == [3] * world and w.all_gather_calls == [0] * world
    assert sum(int(keep.sum()) for _, keep in results) == len(np.unique(job.all_h))


@pytest.mark.parametrize("damage", [("roll", 3), ("own", 2)], ids=["answers_rolled_by_one", "only_the_own_slice_arrives"])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_damaged_exchanges_are_caught(monkeypatch, world, damage):
    """the comparison can fail: each damage hook gives mismatching records on every shape"""
    job = world_job(world, "descending")
    w, results = _first_seen_world(monkeypatch, job, "device_rows", damage=LD.Damage(*damage))
    assert w.all_to_all_calls == [3] * world
    assert mismatches(job, results) > 0


def test_the_monkeypatched_world_is_restored(monkeypatch):
    import torch.distributed as dist
    from circkit_amd import uniq
    with monkeypatch.context() as m:
        LD.install(m, 2)
        assert isinstance(uniq.dist, LD.World)
    assert uniq.dist is dist


class _Boom(RuntimeError):
    pass


@pytest.mark.parametrize("world", [2, 8])
def test_a_rank_that_raises_ends_the_world_at_once(monkeypatch, world):
    """rank 1's table raises in lookup_rows, between the second and the third all-to-all: its peers, waiting in the third, get
    BrokenBarrierError at once instead of the barrier's timeout, every thread ends, and rank 1's exception is the one reported"""
    class Failing(RowsTable):
        def lookup_rows(self, rows):
            raise _Boom("rank 1 cannot answer")

    job = world_job(world, "ascending")

    def table_of(rank):
        return Failing() if rank == 1 else RowsTable()

    t0 = time.monotonic()
    with pytest.raises(_Boom, match="rank 1 cannot answer"):
        _first_seen_world(monkeypatch, job, "device_rows", table_of=table_of)
    elapsed = time.monotonic() - t0
    assert elapsed < LD.BARRIER_TIMEOUT / 2, elapsed
    from circkit_amd import uniq
    assert uniq.dist.failed_rank == 1
    assert not [t for t in threading.enumerate() if t.name.startswith("loopback-rank-")]
