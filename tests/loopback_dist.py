"""An in-process world (TEST INFRASTRUCTURE ONLY): a stand-in for exactly the part of torch.distributed that
circkit_amd/uniq.py::first_seen touches -- is_available, is_initialized, get_world_size, all_to_all_single, all_gather --
with one thread per rank, so that the exchange runs at world > 1 in ONE process and on ONE GPU, on CPU tensors and on device
tensors alike.  No process group is opened and nothing is spawned.

    w = loopback_dist.install(monkeypatch, world)            # uniq.dist = w until the test ends
    results = w.run(lambda rank: uniq.first_seen(...))       # one thread per rank; the first exception is re-raised here

A collective, on every rank: (1) deposit the input tensor and its split cuts in the rank's slot, (2) synchronise the rank's own
current torch stream (the input is complete), (3) a barrier, (4) copy the peers' slices for this rank into `out` with plain
tensor assignment on the rank's own current stream, asserting that every slice has the length output_split_sizes promised,
(5) synchronise again, (6) a second barrier, after which the senders may reuse their buffers.

Nothing waits forever: the barrier has a timeout (BARRIER_TIMEOUT), a rank that raises aborts it -- its peers fail at once with
BrokenBarrierError --, and every thread is joined with a timeout; a thread still alive after the join fails the test.

Damage (negative controls; only DATA goes wrong, every size and every pointer stays what the caller asked for):
    Damage("roll", call=k)   the k-th all_to_all_single of every rank delivers its rows rolled by one
    Damage("own", call=k)    in the k-th all_to_all_single every rank receives only its own slice; the rows its peers owe it
                             arrive as zeros
"""
import threading
import time

import torch

BARRIER_TIMEOUT = 60.0


class Damage:
    def __init__(self, kind, call):
        assert kind in ("roll", "own") and call >= 1
        self.kind, self.call = kind, call


def _cuts(splits):
    cuts = [0]
    for s in splits:
        assert s >= 0, splits
        cuts.append(cuts[-1] + int(s))
    return cuts


def _sync(t):
    """waits for the calling rank's own current stream of t's device (a CPU tensor has none)"""
    if t.is_cuda:
        torch.cuda.current_stream(t.device).synchronize()


class World:
    def __init__(self, world, damage=None, timeout=BARRIER_TIMEOUT):
        assert world >= 1
        self.world = world
        self.damage = damage
        self.timeout = timeout
        self._barrier = threading.Barrier(world, timeout=timeout)
        self._local = threading.local()
        self._slots = [None] * world
        self.all_to_all_calls = [0] * world             # per rank, over the world's life
        self.all_gather_calls = [0] * world

    # ---- what uniq.first_seen asks of torch.distributed ---------------------------------------------------------------------
    def is_available(self):
        return True

    def is_initialized(self):
        return getattr(self._local, "rank", None) is not None           # only inside a rank's thread

    def get_world_size(self, group=None):
        return self.world

    def get_rank(self, group=None):
        return self._rank()

    def all_to_all_single(self, out, inp, output_split_sizes=None, input_split_sizes=None, group=None):
        r, world = self._rank(), self.world
        self.all_to_all_calls[r] += 1
        call = self.all_to_all_calls[r]
        if input_split_sizes is None:
            assert inp.shape[0] % world == 0, (inp.shape, world)
            input_split_sizes = [inp.shape[0] // world] * world
        if output_split_sizes is None:
            assert out.shape[0] % world == 0, (out.shape, world)
            output_split_sizes = [out.shape[0] // world] * world
        assert len(input_split_sizes) == world and len(output_split_sizes) == world
        cuts, ocuts = _cuts(input_split_sizes), _cuts(output_split_sizes)
        assert cuts[-1] == inp.shape[0], ("rank %d sends %d rows, its splits say %d" % (r, inp.shape[0], cuts[-1]))
        assert ocuts[-1] == out.shape[0], ("rank %d has room for %d rows, its splits say %d" % (r, out.shape[0], ocuts[-1]))
        assert out.shape[1:] == inp.shape[1:] and out.dtype == inp.dtype and inp.is_contiguous() and out.is_contiguous()
        self._slots[r] = (inp, cuts)
        _sync(inp)
        self._barrier.wait()
        dmg = self.damage if self.damage is not None and self.damage.call == call else None
        for p in range(world):
            src, c = self._slots[p]
            piece = src[c[r]:c[r + 1]]
            assert piece.shape[0] == output_split_sizes[p], ("rank %d expects %d rows of rank %d, which sends %d" % (
                r, output_split_sizes[p], p, piece.shape[0]))
            assert piece.shape[1:] == out.shape[1:] and piece.dtype == out.dtype
            if dmg is not None and dmg.kind == "own" and p != r:
                out[ocuts[p]:ocuts[p + 1]] = 0
            else:
                out[ocuts[p]:ocuts[p + 1]] = piece
        if dmg is not None and dmg.kind == "roll" and out.shape[0] > 1:
            out.copy_(out.roll(1, 0))
        _sync(out)
        self._barrier.wait()

    def all_gather(self, tensor_list, tensor, group=None):
        r, world = self._rank(), self.world
        self.all_gather_calls[r] += 1
        assert len(tensor_list) == world
        self._slots[r] = (tensor, None)
        _sync(tensor)
        self._barrier.wait()
        for p in range(world):
            src = self._slots[p][0]
            assert src.shape == tensor_list[p].shape and src.dtype == tensor_list[p].dtype, (r, p, src.shape, tensor_list[p].shape)
            tensor_list[p].copy_(src)
        _sync(tensor_list[0])
        self._barrier.wait()

    # ---- the ranks --------------------------------------------------------------------------------------------------------
    def _rank(self):
        r = getattr(self._local, "rank", None)
        assert r is not None, "a collective of the loopback world outside a rank's thread"
        return r

    def run(self, fn, join_timeout=None):
        """fn(rank) in one thread per rank; returns [fn(0), .., fn(world - 1)].  If a rank raises, the barrier is aborted (its
        peers end with BrokenBarrierError) and the first exception that is not such an echo is re-raised here."""
        results = [None] * self.world
        errors, lock = [], threading.Lock()                       # (rank, exception), in the order they happened

        def body(rank):
            self._local.rank = rank
            try:
                results[rank] = fn(rank)
            except BaseException as e:      # noqa: BLE001 -- reported to the caller below
                with lock:
                    errors.append((rank, e))
                self._barrier.abort()
            finally:
                self._local.rank = None

        threads = [threading.Thread(target=body, args=(r,), name="loopback-rank-%d" % r, daemon=True) for r in range(self.world)]
        for t in threads:
            t.start()
        deadline = time.monotonic() + (self.timeout + 30.0 if join_timeout is None else join_timeout)
        for t in threads:
            t.join(max(0.0, deadline - time.monotonic()))
        alive = [t.name for t in threads if t.is_alive()]
        if alive:
            self._barrier.abort()
            raise AssertionError("rank threads still alive after the join: %s" % ", ".join(alive))
        if errors:
            real = [(r, e) for r, e in errors if not isinstance(e, threading.BrokenBarrierError)]
            rank, e = (real or errors)[0]
            self.failed_rank = rank
            raise e
        return results


def install(monkeypatch, world, damage=None, timeout=BARRIER_TIMEOUT):
    """uniq.dist = a fresh World until monkeypatch undoes it (the end of the test)"""
    from circkit_amd import uniq
    w = World(world, damage, timeout)
    monkeypatch.setattr(uniq, "dist", w)
    return w
