"""tests/length_sets.py's "every length" sweeps, checked without a GPU: that each set is what it claims to be (every length, both
index parities, the mode it aims at with a margin, small enough for every record to be a sample), and -- where the device has no
counter to say which routine took a record -- that the emulator, at the geometry the product runs, sends at most 5 % of the
probes anywhere but the intended routine.  tests/test_canon_lengths_gpu.py runs the same sets on the device."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import length_sets as LS
from tests import seqsets
from tests.emu import emu

CAP = 0.05                                              # of the probes, at most, outside the routine the sweep aims at


def _packed(route, order):
    seqs, flags = LS.sweep(route, order)
    data, offs = seqsets.pack(seqs)
    return seqs, flags, data, offs, [len(s) for s in seqs]


@pytest.mark.parametrize("route", sorted(LS.ROUTES))
def test_every_length_is_present_at_both_index_parities(route):
    r = LS.ROUTES[route]
    want = set(r["lengths"]) | set(r["short"])
    parities = {}
    for order in LS.ORDERS:
        seqs, flags = LS.sweep(route, order)
        assert len(seqs) <= LS.CONTENT_SAMPLES                             # every record is a length and a content sample
        assert {len(s) for s, f in zip(seqs, flags) if f} == set(r["lengths"])
        assert sum(flags) == len(r["lengths"])                             # one probe per length
        assert want <= {len(s) for s in seqs}
        n_fill = r["filler"][0]
        assert n_fill == 0 or not any(flags[-n_fill:])                    # the filler is last
        assert all(set(s) <= set(b"ACGTN" if r["n"] else b"ACGT") for s in seqs)
        if r["n"]:                                                         # max(1, n // 100) N were aimed at every record
            assert all(1 <= s.count(b"N") <= max(1, len(s) // 100) for s in seqs if s)
        for i in range(order == "shifted", len(seqs) - n_fill):            # (not the filler)
            parities.setdefault(len(seqs[i]), set()).add(i & 1)
    assert all(parities[n] == {0, 1} for n in want), [n for n in want if parities[n] != {0, 1}][:8]
    a, _ = LS.sweep(route, "as_built")
    b, _ = LS.sweep(route, "shifted")
    assert b[1:] == a and len(b[0]) == r["filler"][1]                      # the same records, one filler record in front


@pytest.mark.parametrize("route", sorted(LS.ROUTES))
def test_expected_mode_with_a_margin(route):
    """The mode every output set of the route must report, from expected_mode, and the distance of the counts behind it from every
    threshold.  A factor 2 for the thresholds that are fractions one can miss by a factor 2: long records (1/8 for mode 3), two-word
    records (1/4 for mode 2), content samples outside ACGT (1/16 for MODE_ALPHA) -- and nothing at all of a kind where the mode
    must not carry it.  MODE_SHORT is a majority vote (half of the records <= 800 symbols): the set that must stay below it keeps a factor 2 (a
    quarter at most, hence its 2100 filler records), the one that must reach it cannot exceed the half by a factor 2 and keeps 1/8
    of the batch above it (5/8 at least)."""
    r = LS.ROUTES[route]
    for order in LS.ORDERS:
        seqs, flags, data, offs, lens = _packed(route, order)
        c = LS.mode_counts(lens, data, offs)
        for what, want in r["mode"].items():
            lmsr = what.startswith("lmsr")
            outs = what.split()[-1]
            aux = lmsr or "i" in outs or "s" in outs
            mode = LS.expected_mode(lens, data, offs, "h" in outs, aux)
            assert mode & 3 == want, (route, order, what, mode)
            assert bool(mode & LS.MODE_ALPHA) == r["n"]
        if r["n"]:
            assert c["bad"] * 8 >= c["sampled"]                            # 1/16 with a factor 2
        else:
            assert c["bad"] == 0
        first = next(iter(r["mode"].values()))
        if route.startswith("mixed"):
            assert c["lng"] * 4 >= c["n"]                                  # 1/8 with a factor 2
        elif route.startswith("two_word"):
            assert c["lng"] == 0 and c["two"] * 2 >= c["n"]                # 1/4 with a factor 2; mode 3 comes from the hash alone
        else:
            assert first == 1 and c["lng"] == 0 and c["two"] == 0
        if route == "stream_bytes":
            assert c["short"] * 4 <= c["n"]                                # not MODE_SHORT: 1/2 with a factor 2
            assert not LS.expected_mode(lens, data, offs, False, False) & LS.MODE_SHORT
        if route == "pair_bytes":
            assert c["short"] * 8 >= c["n"] * 5                            # MODE_SHORT: 5/8 at least
            assert LS.expected_mode(lens, data, offs, False, False) & LS.MODE_SHORT


def test_expected_mode_restates_the_rules():
    """expected_mode on hand-made batches on either side of every threshold (lengths only decide 1 / 2 / 3 and MODE_SHORT; the
    content rule needs bytes), and its content rule against the emulator's own restatement."""
    def mode(lens, want_hash=False, aux=False, n_every=0):
        seqs = [b"A" * n for n in lens]
        if n_every:
            seqs = [(b"N" + s[1:]) if i % n_every == 0 and s else s for i, s in enumerate(seqs)]
        data, offs = seqsets.pack(seqs)
        assert bool(LS.expected_mode(lens, data, offs, want_hash, aux) & LS.MODE_ALPHA) == bool(emu.alpha_rule(data, offs))
        return LS.expected_mode(lens, data, offs, want_hash, aux)
    assert mode([1000] * 7 + [2033]) == 3 and mode([1000] * 8 + [2033]) == 1
    assert mode([1000] * 7 + [2032]) == 1 and mode([1000] * 3 + [2032]) == 2 and mode([1000] * 3 + [1009]) == 2
    assert mode([1000] * 3 + [1008]) == 1
    assert mode([1500] * 4, want_hash=True) == 3 and mode([1500] * 4, want_hash=True, aux=True) == 2
    assert mode([1500] * 32, n_every=16) == 3 | LS.MODE_ALPHA and mode([1500] * 34, n_every=17) == 2
    assert mode([1000] * 32, n_every=16) == 1 | LS.MODE_ALPHA and mode([1000] * 34, n_every=17) == 1
    assert mode([800, 801]) == 1 | LS.MODE_SHORT and mode([800, 801, 801]) == 1
    assert mode([800] * 32, n_every=16) == 1 | LS.MODE_ALPHA            # MODE_SHORT only without MODE_ALPHA
    assert mode([0, 0, 3000, 700] * 2) == 3                              # ... and only in mode 1
    # the content rule looks at the first 1008 bytes only
    seqs = [b"A" * 1008 + b"N"] * 8
    data, offs = seqsets.pack(seqs)
    assert LS.expected_mode([1009] * 8, data, offs, False, False) == 2


def _emu_outputs(seqs, data, offs, outs, **kw):
    out, _, _, h, status, ndef = emu.canonicalize_batch(data, offs, want_hash="h" in outs, want_aux=False, hash_only="b" not in outs, **kw)
    assert status == 0 and ndef == 0
    exp, exp_h = O.canonicalize_batch(data, offs, True, True)
    if "b" in outs:
        assert np.array_equal(out, exp), [i for i in range(len(seqs)) if not np.array_equal(out[int(offs[i]):int(offs[i + 1])], exp[int(offs[i]):int(offs[i + 1])])][:5]
    else:
        assert (out == 0x3F).all()
    if "h" in outs:
        bad = np.nonzero(h != exp_h)[0]
        assert len(bad) == 0, (bad[:5], [len(seqs[i]) for i in bad[:5]])


STREAMING = [(route, order, outs, k) for route in sorted(LS.ROUTES) for order in LS.ORDERS for outs, k0 in LS.ROUTES[route]["staged"].items()
             for k in ((14, 15) if k0 in (14, 15) else (k0,))]


@pytest.mark.parametrize("route,order,outs,staged", STREAMING)
def test_streaming_sweeps_take_the_intended_routine(route, order, outs, staged):
    """Each streaming sweep through the emulator at the geometry of the product's build for its outputs (1: StreamC; 14 / 15: the pair
    builds; 16 / 13: the N builds without / with the hash; 17: the two-word build): bytes and hashes against the oracle, and of the
    records outside the batch's last group (never staged) and the XXH3 short classes (too short for the routine) at most 5 % of
    the number of probes may have been left to the passes behind."""
    r = LS.ROUTES[route]
    seqs, flags, data, offs, lens = _packed(route, order)
    _emu_outputs(seqs, data, offs, outs, staged=staged, slice_dw=4096, n_waves=8, alpha=r["n"])
    wpb, rpw, _ = emu.STAGED_GEOMETRIES[staged]
    last_group = (len(seqs) - 1) % (wpb * rpw) + 1
    assert last_group <= r["filler"][0]
    too_short = sum(1 for n in lens if n < min(r["lengths"]))
    missed = len(seqs) - last_group - too_short - emu.last_fast_count
    print(route, order, outs, staged, "probes", sum(flags), "left to the passes behind", missed)
    assert 0 <= missed <= CAP * sum(flags)


@pytest.mark.parametrize("route,order,outs", [(route, order, outs) for route in ("mixed", "mixed_n") for order in LS.ORDERS for outs in ("b", "bh", "h")])
def test_mixed_sweeps_take_the_lean_routines(route, order, outs):
    """The mixed sweeps through canon_mixed_segment with the product's slices (1280 dwords per wave; 1904 for the N builds), whole
    (a few seconds each): at most 5 % of the probes may go on to stage A, and with the hash at most 5 % may leave their XXH3 to the
    xxh3 pass -- of all probes in the pure build, of those beyond 1008 symbols in the N build (shorter records with N never fuse)."""
    r = LS.ROUTES[route]
    seqs, flags, data, offs, lens = _packed(route, order)
    _emu_outputs(seqs, data, offs, outs, staged=0, slice_dw=1904 if r["n"] else 1280, n_waves=12, alpha=r["n"], mixed=True)
    probes = sum(flags)
    print(route, order, outs, "probes", probes, "rescued", emu.last_rescued_count, "fused", emu.last_fused_hash_count)
    assert len(seqs) - emu.last_rescued_count <= CAP * probes
    if "h" in outs:
        fusable = [n for n, f in zip(lens, flags) if f and (n > LS.ONE_WORD_MAX or not r["n"])]
        assert len(fusable) - emu.last_fused_hash_count <= CAP * len(fusable)


@pytest.mark.parametrize("name", sorted(LS.CRAFTED))
def test_crafted_sets_as_device_batches_aim_at_their_mode(name):
    build, aim, outs = LS.CRAFTED[name]
    seqs = build()
    assert len(seqs) <= LS.CONTENT_SAMPLES
    data, offs = seqsets.pack(seqs)
    for o in outs:
        mode = LS.expected_mode([len(s) for s in seqs], data, offs, "h" in o, False)
        assert LS.crafted_mode_matches(aim, mode, o), (name, o, mode, aim)      # (MODE_ALPHA: the N builds; MODE_SHORT: the bytes-only pair build)
