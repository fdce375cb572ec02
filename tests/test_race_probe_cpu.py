"""The fiber schedules of tests/emu/emu.cpp must bite: tests/emu/race_probe_main.cpp holds four small LDS protocols, each with its
sync and without.  Every synced form gives the plain answer below under every schedule; every unsynced form gives a wrong one
under at least one schedule of the matrix (emu.SCHEDULES).  CAUGHT is the table of DESIGN section 26, asserted cell by cell: the
schedules are deterministic, so a cell that changes means the scheduler changed."""
import re

import pytest

from tests.emu import emu, race_probe

ROUNDS, WG, M32 = 4, 128, 2 ** 32 - 1
ALL = ("ascending",) + emu.SCHEDULES


def value(r, t):
    return 1000 * (r + 1) + 3 * t + 7


def expected():
    sums = [sum(value(0, k) for k in range(t)) & M32 for t in range(WG + 1)]
    return {
        "exchange": [value(0, n) for l in range(64) for n in (l ^ 1, (l + 1) & 63)],
        "produce_up": [value(0, 63 - l) for l in range(64)],
        "produce_down": [value(0, 63 - l) for l in range(64)],
        "reuse": [sum((r + 1) * value(r, l + 1) for r in range(ROUNDS)) & M32 if l < 63 else 0 for l in range(64)],
        "doubling": sums[:WG] + [sums[WG]] * WG,
    }


# unsynced form -> the schedules under which it gives a wrong answer
CAUGHT = {
    "exchange": {"ascending", "descending", "lone-wave", "random:1", "random:2"},
    "produce_up": {"descending", "lone-wave", "random:1", "random:2"},              # wave 0 produces: ascending hides it
    "produce_down": {"ascending", "random:1", "random:2"},                          # wave 1 produces: highest-first hides it
    "reuse": {"ascending", "descending", "lone-wave", "random:1", "random:2"},
    # reads downward, so running strictly downward hides it; lone-wave does not run strictly downward: the lane that completes a
    # barrier (lane 0 of wave 0) goes on first and has written lds[0] before lane 1 reads it
    "doubling": {"ascending", "lone-wave", "random:1", "random:2"},
}


@pytest.fixture(scope="module")
def runs():
    return {s: race_probe.run(schedule=s) for s in ALL}


def test_unset_is_ascending(runs):
    assert race_probe.run() == runs["ascending"]


@pytest.mark.parametrize("schedule", ALL)
def test_synced_forms_are_right_under_every_schedule(runs, schedule):
    exp = expected()
    assert {name for name, _ in runs[schedule]} == set(exp)
    for name, want in exp.items():
        assert runs[schedule][(name, "synced")] == want, (name, schedule)


@pytest.mark.parametrize("name", sorted(CAUGHT))
def test_unsynced_form_is_caught(runs, name):
    want = expected()[name]
    wrong = {s for s in ALL if runs[s][(name, "unsynced")] != want}
    print(name, "wrong under", sorted(wrong))
    assert wrong & set(emu.SCHEDULES), "no schedule of the matrix sees the missing sync of %s: the set is too weak" % name
    assert wrong == CAUGHT[name]


def test_random_is_reproducible_and_seeded(runs):
    assert race_probe.run(schedule="random:1") == runs["random:1"]
    assert runs["random:1"] != runs["random:2"]         # (the unsynced forms differ; the synced ones may not)


@pytest.mark.parametrize("schedule", ALL)
@pytest.mark.parametrize("k,what", [(0, ("wave collective",)), (1, ("workgroup barrier",)), (2, ("workgroup barrier",)),
                                    (3, ("wave collective", "workgroup barrier"))])       # (3: some wait in the one, some in the other)
def test_a_skipped_collective_is_still_a_reported_deadlock(k, what, schedule):
    """Whoever skips it and whatever the order: no fiber can move, and the report names a fiber that waits, its wave and its lane."""
    rc, out, err = race_probe.run_skip(k, schedule)
    assert rc == -6 and "finished" not in out                   # abort()
    m = re.search(r"emu: deadlock -- fiber (\d+) \(wave (\d+) lane (\d+)\) waits in a (.+) the others never reach", err)
    assert m, err
    f, w, l = int(m.group(1)), int(m.group(2)), int(m.group(3))
    assert (w, l) == (f >> 6, f & 63) and f < 128 and m.group(4) in what
    # never one that skipped and finished: lane 5 of wave 1, all of wave 0, lane 63 of wave 0 (3: nobody finishes)
    assert {0: (w, l) != (1, 5), 1: w == 1, 2: (w, l) != (0, 63), 3: True}[k]


def test_unknown_schedule_is_refused():
    with pytest.raises(AssertionError, match="unknown schedule"):
        race_probe.run(schedule="sideways")
