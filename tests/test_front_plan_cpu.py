"""The front of a canonicalize batch on the CPU (canon_plan.h, through the emulator library): which build owns a batch of which
mode, and which kernels launch_canon's front stages launch with which grid.

tests/golden/canon_front_plan.json is the launch sequence of the commit it names, recorded from that commit's own stage_stream,
stage_rescue and stage_mixed (a host-only build with the launch macro redefined); the plan must reproduce it row for row.  The
other tests hold the plan to its rule: a build is launched when it owns a mode the batch may still have, and is full size when it
owns the mode the batch is expected to have."""
import ctypes
import itertools
import json
import os

import pytest

from tests import length_sets as LS
from tests.emu import emu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "canon_front_plan.json")
STREAM, RESCUE, MIXED = 0, 1, 2
N_CU, RESCUE_BPC = 256, 8


class Plan:
    def __init__(self):
        lib = ctypes.CDLL(emu.build())
        u32, i = ctypes.c_uint32, ctypes.c_int
        lib.emu_front_builds.restype = u32
        lib.emu_front_build.restype = ctypes.c_char_p
        lib.emu_front_build.argtypes = [u32, ctypes.POINTER(u32)]
        lib.emu_front_owns.argtypes = [u32, u32]
        lib.emu_stream_owns.argtypes = [u32, u32, i, i, i, u32]
        lib.emu_rescue_owns.argtypes = [i, i, u32]
        lib.emu_mixed_owns.argtypes = [i, u32]
        lib.emu_front_expected_mode.restype = u32
        lib.emu_front_expected_mode.argtypes = [u32, u32]
        lib.emu_front_plan.argtypes = [i, i, u32, u32, u32, u32, ctypes.POINTER(u32)]
        lib.emu_batch_mode_of.restype = u32
        lib.emu_batch_mode_of.argtypes = [ctypes.c_uint64] * 6 + [i]
        self.lib = lib
        self.builds = []                                # (name, stage, hash, aux, alpha, block, lds)
        for k in range(lib.emu_front_builds()):
            out = (u32 * 6)()
            name = lib.emu_front_build(k, out).decode()
            self.builds.append((name,) + tuple(out))

    def serves(self, k, aux, want_hash):
        """does build k take batches with these outputs (aux: index, strand or lmsr; else with or without the XXH3)"""
        _, _, b_hash, b_aux, _, _, _ = self.builds[k]
        return bool(b_aux) == aux and (aux or bool(b_hash) == want_hash)

    def owns(self, k, mode):
        return bool(self.lib.emu_front_owns(k, mode))

    def plan(self, aux, want_hash, host_mode, seen, G, nseg):
        out = (ctypes.c_uint32 * 24)()
        n = self.lib.emu_front_plan(int(aux), int(want_hash), host_mode, seen, G, nseg, out)
        assert 0 <= n <= 8
        return [(out[3 * k], bool(out[3 * k + 1]), out[3 * k + 2]) for k in range(n)]


@pytest.fixture(scope="module")
def P():
    return Plan()


def producible_modes(P, want_hash, aux):
    """every mode length_sets' restatement of batch_mode_of gives for some counts -- and batch_mode_of gives the same"""
    modes = set()
    n = 16
    for lng, two, short, bad in itertools.product((0, 1, 2, 8), (0, 3, 4, 16), (0, 7, 8, 16), (0, 1, 16)):
        if lng + two + short > n:
            continue
        c = dict(n=n, lng=lng, two=two, short=short, bad=bad, sampled=n)
        m = LS.mode_of_counts(c, want_hash, aux)
        assert m == P.lib.emu_batch_mode_of(two, lng, n, bad, n, short, int(want_hash and not aux)), c
        modes.add(m)
    return modes


def test_the_plan_is_the_recorded_launch_sequence(P):
    """(a) row for row: kernel, persistent twin or not, grid, workgroup size, dynamic LDS"""
    with open(GOLDEN) as f:
        gold = json.load(f)
    names = gold["kernels"]
    assert sorted(names) == sorted(b[0] for b in P.builds)
    assert len(gold["rows"]) == 4 * 7 * 16 * 5
    for aux, want_hash, host_mode, seen, G, nseg, launches in gold["rows"]:
        got = []
        for k, full, grid in P.plan(aux, want_hash, host_mode, seen, G, nseg):
            name, stage, _, _, _, block, lds = P.builds[k]
            got.append([names.index(name), int(stage == STREAM and not full), grid, block, lds])
        assert got == launches, (aux, want_hash, host_mode, seen, G, nseg)


@pytest.mark.parametrize("aux,want_hash", [(False, False), (False, True), (True, False), (True, True)])
def test_every_mode_has_one_owner(P, aux, want_hash):
    """(b) of the builds that serve a batch's outputs, exactly one streaming build owns a mode whose stream_mode is 1 or 2 (none
    a mode 3), and exactly one of the rescue and mixed builds owns any mode; the aux rescue build owns every mode."""
    modes = producible_modes(P, want_hash, aux)
    assert {m & 3 for m in modes} == {1, 2, 3} or (want_hash and not aux and {m & 3 for m in modes} == {1, 3})
    assert any(m & LS.MODE_ALPHA for m in modes) and any(m & LS.MODE_SHORT for m in modes)
    mine = [k for k in range(len(P.builds)) if P.serves(k, aux, want_hash)]
    for m in sorted(modes):
        streams = [k for k in mine if P.builds[k][1] == STREAM and P.owns(k, m)]
        behind = [k for k in mine if P.builds[k][1] != STREAM and P.owns(k, m)]
        assert len(streams) == (0 if m & 3 == 3 else 1), (m, streams)
        assert len(behind) == 1, (m, behind)
        if aux:
            assert P.builds[behind[0]][0] == "canon_rescue_kernel<true,true,false>"
        else:
            assert (P.builds[behind[0]][1] == MIXED) == (m & 3 == 3)
            assert bool(P.builds[behind[0]][4]) == bool(m & LS.MODE_ALPHA)
    # front_owns is the predicates, with the build's own template arguments
    for m in range(16):
        assert bool(P.lib.emu_rescue_owns(1, 0, m)) and bool(P.lib.emu_mixed_owns(int(bool(m & 4)), m)) == (m & 3 == 3)
        for rows in (1, 2):
            assert bool(P.lib.emu_stream_owns(rows, 2, 1, 1, 0, m)) == (m & 3 == rows)


GEOMETRIES = [(1, 1), (2 * N_CU - 1, 2 * N_CU - 1), (2 * N_CU + 1, 2 * N_CU + 1), (N_CU * RESCUE_BPC + 1, N_CU * RESCUE_BPC + 1), (32768, 32768)]


def full_grid(P, k, G, nseg):
    """the grid of build k when it is expected to run: one workgroup per virtual workgroup / segment; the rescue pass its
    persistent grid; the mixed N builds the resident grid their ticket feeds (five 4-wave workgroups per CU)"""
    _, stage, _, _, alpha, _, _ = P.builds[k]
    if stage == STREAM:
        return G
    if stage == RESCUE:
        return min(nseg, N_CU * RESCUE_BPC)
    return min(nseg, N_CU * 5) if alpha else nseg


@pytest.mark.parametrize("aux,want_hash", [(False, False), (False, True), (True, False), (True, True)])
def test_a_known_mode_launches_its_owners_at_full_size(P, aux, want_hash):
    """(c) host_mode set (the host has seen the offsets, or guesses): exactly the owners, in table order, all full size"""
    mine = [k for k in range(len(P.builds)) if P.serves(k, aux, want_hash)]
    for host_mode in sorted(producible_modes(P, want_hash, aux)):
        for seen, (G, nseg) in itertools.product(range(16), GEOMETRIES):
            got = P.plan(aux, want_hash, host_mode, seen, G, nseg)
            assert [k for k, _, _ in got] == [k for k in mine if P.owns(k, host_mode)], (host_mode, seen)
            assert all(full and grid == full_grid(P, k, G, nseg) for k, full, grid in got), (host_mode, seen, G, got)


@pytest.mark.parametrize("aux,want_hash", [(False, False), (False, True), (True, False), (True, True)])
def test_an_open_mode_launches_every_owner_once(P, aux, want_hash):
    """(d) host_mode 0 (the device decides): every mode's owners are in the plan, each build once; full size are exactly the
    owners of the expected mode -- what the last batch reported, stream_mode 1 while none has -- and they have their full grid"""
    mine = [k for k in range(len(P.builds)) if P.serves(k, aux, want_hash)]
    for seen, (G, nseg) in itertools.product(range(16), GEOMETRIES):
        got = P.plan(aux, want_hash, 0, seen, G, nseg)
        ks = [k for k, _, _ in got]
        assert ks == sorted(set(ks)) and set(ks) <= set(mine)
        for m in producible_modes(P, want_hash, aux):
            assert {k for k in mine if P.owns(k, m)} <= set(ks), (m, ks)
        expect = P.lib.emu_front_expected_mode(0, seen)
        assert expect == (seen if seen & 3 else (seen & 12) | 1)
        for k, full, grid in got:
            assert full == P.owns(k, expect), (seen, k)
            if full:
                assert grid == full_grid(P, k, G, nseg)
            else:
                assert grid == (min(G, 2 * N_CU) if P.builds[k][1] == STREAM else min(nseg, N_CU * RESCUE_BPC)), (seen, k, grid)
