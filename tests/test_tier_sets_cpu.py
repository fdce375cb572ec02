"""The admission boundaries of stages A and C and of the mixed-length kernels on the CPU fiber emulator, at the product's slice sizes
(no triple is scaled: the slowest test of this file takes ~1.2 s on the build machine, the file ~7 s behind the emulator's build).

tests/tier_sets.py derives every boundary from the restated predicates; here
  * the restated constants and predicates are compared with the text of canon_config.h / circkit_canon.hip / canon_core.h / canon_mixed.h,
  * every record class's construction is proved from the records alone,
  * for every reachable triple of stage A, stage C (fed with what stage A's emulated workgroup deferred) and the two mixed builds
    one 4-wave workgroup runs with its LDS pre-filled with a pattern and a guard region behind the four slices
    (tests/emu/emu.py tier_footprint): the record of n_max is taken and right, the record of n_max + 1 goes where the table says,
    no footprint exceeds what the governing predicate returns, and a record held by wave w alone leaves the other slices and the
    guard untouched.
The sixteen-wave team stage and the global-scratch kernel are not emulated: tests/test_tier_boundaries_gpu.py runs them."""
import numpy as np
import pytest

from tests import length_sets as LS
from tests import seqsets
from tests import tier_sets as T
from tests.emu import emu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.lib()
    return oracle


def test_restated_constants_match_the_sources():
    got = T.source_constants()
    assert sorted(got) == sorted(T.EXPECTED_SOURCE)
    for name, want in T.EXPECTED_SOURCE.items():
        assert got[name] == want, "%s: the source says %r, tests/tier_sets.py restates %r" % (name, got[name], want)
    assert T.TEAM_WAVES * T.TEAM_SLICE_DW == 40176 < T.TIER_DW[4]             # the division truncates


def test_n_max_is_the_last_admitted_length():
    for name, f in T.PREDICATES.items():
        for cap in (T.CK_TIER_A, T.CK_MIXED_N_SLICE, T.BATCH_SLICE_DW[1], 4 * T.CK_TIER_A, T.TIER_DW[3], T.TEAM_WAVES * T.TEAM_SLICE_DW, T.GSLICE1_DW):
            nm = T.n_max(name, cap)
            assert f(nm) <= cap < f(nm + 1), (name, cap, nm)
            assert all(f(n) <= f(n + 1) for n in range(max(nm - 70, 0), nm + 70))
    assert T.probes(100) == [84, 99, 100, 101, 116, 117]


@pytest.mark.parametrize("cls", T.CLASSES)
def test_every_class_is_what_its_docstring_says(cls):
    """from the record alone: the alphabet, the one planted run per strand and nothing near its length, the strangers' distance
    from both runs, the owners of a tandem repeat's minimal key -- at every boundary length the tables use for the class"""
    lens = sorted({L for t in T.TRIPLES if t.cls == cls for L in T.probes(T.triple_n_max(t))} |
                  {L + d for L in T.single_switches()[0] + [T.single_switches()[1]] for d in (0, 1)})
    assert lens
    for k, L in enumerate(lens):
        T.check_class(cls, T.make(cls, L, 100 + k))
    assert T.make(cls, lens[0], 1) != T.make(cls, lens[0], 2) and T.make(cls, lens[0], 1) == T.make(cls, lens[0], 1)
    with pytest.raises(AssertionError):
        T.check_class(cls, T.make("byte" if cls != "byte" else "pure", lens[0], 1))


def test_the_table_names_every_combination_once():
    seen = [(t.stage, t.route, t.cls, t.pred) for t in T.TRIPLES] + [u[:4] for u in T.UNREACHABLE]
    assert len(seen) == len(set(seen))
    assert all(len(u) == 5 and len(u[4]) > 20 for u in T.UNREACHABLE)
    for stage in ("A", "C", "T"):
        seqs, tags = T.stage_batch(stage)
        data, offs = seqsets.pack(seqs)
        lens = [len(s) for s in seqs]
        for want_hash, aux in ((False, False), (True, False), (True, True)):
            assert LS.expected_mode(lens, data, offs, want_hash, aux) & 3 == 3
        assert [s for s, _ in zip(*T.stage_batch(stage, "reversed"))] != seqs and sorted(T.stage_batch(stage, "reversed")[0]) == sorted(seqs)
        assert {ti for ti, _ in tags if ti >= 0} == {i for i, t in enumerate(T.TRIPLES) if t.stage == stage}


# ---- footprints ---------------------------------------------------------------------------------------------------------------
def _expect(O, s):
    b, st, idx = seqsets.expected(O, s)
    return np.frombuffer(b, dtype=np.uint8), st, idx


def _workgroup_high_water(r, slice_dw):
    return max([w * slice_dw + h for w, h in enumerate(r["high_water"]) if h] or [0])


def _tier(stage, rec, wave, t4, solo=True):
    """The record as entry `wave` of a list whose other entries are an empty record (no LDS use), through stage A's workgroup and,
    for stage C, what that deferred through stage C's.  Returns (result of the stage, data, offs)."""
    data, offs = seqsets.pack([b"", rec])
    r = emu.tier_footprint(data, offs, T.STAGE_SLICE["A"], "tier", entries=[0] * wave + [1], solo=solo, team4=t4)
    assert r["status"] == 0 and r["guard_touched"] == 0
    if stage == "C":
        assert [e & 0x3FFFFFFF for e in r["deferred"]] == [1], "stage A was to pass the record on"
        assert (r["bytes"] == emu.S_OUT).all() and r["index"][1] == emu.S_IDX and r["strand"][1] == emu.S_STRAND
        r = emu.tier_footprint(data, offs, T.STAGE_SLICE["C"], "tier", entries=[0] * wave + r["deferred"], solo=solo, team4=t4)
    return r, data, offs


def _check_taken(O, r, rec, what):
    eb, es, ei = _expect(O, rec)
    assert r["deferred"] == [], what + ": deferred"
    assert np.array_equal(r["bytes"], eb), what + ": bytes"
    assert r["strand"][-1] == es and r["index"][-1] == ei, what + ": strand / index %s %s, expected %s %s" % (r["strand"][-1], r["index"][-1], es, ei)


def _check_passed_on(r, what):
    assert [e & 0x3FFFFFFF for e in r["deferred"]] == [len(r["index"]) - 1], what + ": not deferred"
    assert (r["bytes"] == emu.S_OUT).all() and r["index"][-1] == emu.S_IDX and r["strand"][-1] == emu.S_STRAND, what + ": deferred, but written"


TIER_TRIPLES = [t for t in T.TRIPLES if t.stage in ("A", "C")]


@pytest.mark.parametrize("t", TIER_TRIPLES, ids=lambda t: "%s-%s-%s-%s%s" % (t.stage, t.route, t.cls, t.pred, {None: "", True: "-busy", False: "-idle"}[t.t4]))
def test_stage_boundary_on_the_emulator(O, t):
    """All six probe lengths of the triple, the record in each of the four waves in turn.  Up to n_max: taken by the triple's route --
    one wave: only that wave's slice is touched, at most pred(n) dwords of it; team / wave 0 alone: at most pred(n) dwords from the
    workgroup's first slice on.  From n_max + 1: the next route of the same stage takes it, within ITS bound from the first slice
    on (a wave 1..3 that had admitted it would be seen in its neighbour's slice or in the guard), or the stage passes it on unwritten."""
    S, pred, nm = T.STAGE_SLICE[t.stage], T.PREDICATES[t.pred], T.triple_n_max(t)
    t4 = t.t4 is not False
    same_stage_next = t.nxt.startswith("stage %s" % t.stage)
    for k, L in enumerate(T.probes(nm)):
        for wave in range(4) if L in (nm, nm + 1) else (k % 4,):
            rec = T.make(t.cls, L, 40 + k + wave)
            what = "%s %s %s n=%d (n_max %+d) wave %d" % (t.stage, t.route, t.cls, L, L - nm, wave)
            r, _, _ = _tier(t.stage, rec, wave, t4)
            assert r["status"] == 0 and r["guard_touched"] == 0, what + ": guard region written"
            hw = r["high_water"]
            if L <= nm:
                _check_taken(O, r, rec, what)
                if t.route == "wave":
                    assert all(h == 0 for w, h in enumerate(hw) if w != wave), what + ": slices %s, only wave %d holds a record" % (hw, wave)
                    assert 0 < hw[wave] <= pred(L), what + ": %d dwords, the predicate says %d" % (hw[wave], pred(L))
                else:
                    assert 0 < _workgroup_high_water(r, S) <= pred(L), what + ": slices %s, the predicate says %d" % (hw, pred(L))
            elif same_stage_next:
                _check_taken(O, r, rec, what)
                # the wave that held it may have built a strand in its own slice before it refused; everything else lies within
                # the next route's pred(n) dwords from the first slice on
                for w, h in enumerate(hw):
                    assert w == wave or (w * S + h <= pred(L) if h else True), what + ": slices %s, the next route needs %d from the first slice on" % (hw, pred(L))
                assert hw[0] > 0, what + ": the next route starts in the first slice"
            else:
                _check_passed_on(r, what)
                assert _workgroup_high_water(r, S) <= 4 * S
        if t.route == "wave":
            # ...and without the team pass's wave-0-alone fallback: a record one wave holds is done before the pass
            r, _, _ = _tier(t.stage, T.make(t.cls, nm, 7), 2, t4, solo=False)
            _check_taken(O, r, T.make(t.cls, nm, 7), "no solo")
            assert [h > 0 for h in r["high_water"]] == [False, False, True, False] and r["guard_touched"] == 0


def test_tight_predicates_reach_their_last_dword(O):
    """The measurement sees the slice's last dword: the strand-only predicates and the N-mask predicate are exact (no slack), so
    at n_max of a 1280-dword slice the high-water mark IS 1280 -- a predicate one dword short would show as 1281 here."""
    for cls, pred in (("pure", "strand2"), ("few_n", "2n"), ("tie", "need2")):
        nm = T.n_max(pred, T.CK_TIER_A)
        if T.PREDICATES[pred](nm) == T.CK_TIER_A:
            r, _, _ = _tier("A", T.make(cls, nm, 3), 1, True)
            assert r["high_water"][1] <= T.CK_TIER_A and r["high_water"][2] == 0
            if pred != "need2":
                assert r["high_water"][1] == T.CK_TIER_A, (cls, r["high_water"])


MIXED_TRIPLES = [t for t in T.TRIPLES if t.stage in ("mixed", "mixed_n")]


@pytest.mark.parametrize("t", MIXED_TRIPLES, ids=lambda t: "%s-%s" % (t.stage, t.cls))
def test_mixed_kernel_boundary_on_the_emulator(O, t):
    """The lean routine's admission at all sixteen payload shifts (the alignment enters LeanGeom; lean_strand_dw is sized for the
    worst): n_max taken and right, n_max + 1 passed on with its slice untouched, every footprint within the predicate, the other
    waves' slices and the guard untouched.  The other probe lengths at the shift the wave index picks."""
    S, pred, nm = T.triple_cap(t), T.PREDICATES[t.pred], T.triple_n_max(t)
    lead, tail = b"G" * 32, b"G" * 32                         # (shorter than 48: passed on without LDS use; they keep the aligned chunks inside the payload)
    worst = 0
    for shift in range(16):
        for k, L in enumerate(T.probes(nm)):
            if L not in (nm, nm + 1) and shift != 3 * k:
                continue
            wave = (shift + k) % 4
            rec = T.make(t.cls, L, 60 + shift + k)
            seqs = [lead] + [b""] * ((wave - 1) % 4) + [rec, tail]
            data, offs = seqsets.pack(seqs)
            r = emu.tier_footprint(data, offs, S, t.stage, base_shift=shift, want_index=False, want_strand=False)
            what = "%s %s n=%d (n_max %+d) shift %d wave %d" % (t.stage, t.cls, L, L - nm, shift, wave)
            me = len(seqs) - 2
            lo, hi = int(offs[me]), int(offs[me + 1])
            assert r["status"] == 0 and r["guard_touched"] == 0, what
            hw = r["high_water"]
            assert all(h == 0 for w, h in enumerate(hw) if w != wave), what + ": slices %s" % hw
            passed = [e & 0x3FFFFFFF for e in r["deferred"]]
            if L <= nm:
                assert me not in passed, what + ": passed on"
                assert np.array_equal(r["bytes"][lo:hi], _expect(O, rec)[0]), what + ": bytes"
                assert 0 < hw[wave] <= pred(L), what + ": %d dwords, the predicate says %d" % (hw[wave], pred(L))
                worst = max(worst, hw[wave])
            else:
                assert me in passed and (r["bytes"][lo:hi] == emu.S_OUT).all() and hw[wave] == 0, what + ": slices %s, passed on %s" % (hw, passed)
                # the entry's alphabet flag says what was seen, not what was assumed: nobody has built the record, so it is flagged if
                # its first KiB shows a byte outside ACGT and not otherwise (a flag on a pure record costs it the 2-bit modes in
                # every stage behind); never the N-mask flag
                entry = [e for e in r["deferred"] if e & 0x3FFFFFFF == me][0]
                assert entry >> 30 == (2 if b"N" in rec[:1024] else 0), what + ": passed on as %#x" % entry
    # some shift comes within a dword of the sizing (the N build's candidate list, the slice's last dwords, is used on a tie only)
    assert worst >= pred(nm) - (T.LEAN_CAND_DW if t.stage == "mixed_n" else 0) - 1, worst
