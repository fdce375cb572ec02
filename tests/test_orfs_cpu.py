"""CPU-only checks of `circkit orfs`: the C restatement (tests/orfs_ref.c) against the reference's own unit tests (recorded
in tests/golden/ref_orfs_known_answers.json) and its proptests (lib/src/orfs.rs:571-670, restated as seeded property
tests), and the kernel's per-lane routine (circkit_amd/csrc/orfs.h, built for the host) against the restatement."""
import json
import os
import random

import numpy as np
import pytest

from tests import orfs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def known_answers():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "ref_orfs_known_answers.json")))["cases"]


def orf_seq(seq, start, length):
    """Orf::seq (lib/src/orfs.rs:19-36 with include_stop): `length` bytes cut cyclically from start."""
    return bytes(seq[(start + k) % len(seq)] for k in range(length))


@pytest.mark.parametrize("case", known_answers(), ids=lambda c: c["name"])
def test_restatement_known_answers(case):
    seq = case["seq"].encode()
    exp = [tuple(e) for e in case["expected"]]
    if case["call"] == "longest":
        got = [o[:4] for o in R.orfs_record(seq, strands=1, mode=0)]
    else:
        got = R.find_orfs(seq)
    assert got == exp
    if "expected_seq" in case:
        assert orf_seq(seq, got[0][0], got[0][3]) == case["expected_seq"].encode()


def _pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)[:int(offs[-1])], offs


@pytest.mark.parametrize("case", known_answers(), ids=lambda c: c["name"])
def test_lane_routine_known_answers(case):
    seq = case["seq"].encode()
    d, o = _pack([seq])
    _, got = R.lane_orfs_batch(d, o, strands=1, mode=0 if case["call"] == "longest" else 1)
    got = [(int(g["start"]), None if int(g["stop"]) == R.NONE else int(g["stop"]), int(g["wraps"]), int(g["length"])) for g in got]
    assert got == [tuple(e) for e in case["expected"]]


# ---- the reference's proptests, seeded ("[ATGC]{3,300}") -------------------------------------------------------------
def _random_seqs(seed, n=300):
    rng = random.Random(seed)
    return [bytes(rng.choice(b"ATGC") for _ in range(rng.randint(3, 300))) for _ in range(n)]


def bio_find_all(seq):
    """rust-bio 0.x seq_analysis::orf::Finder(ATG; TAA,TAG,TGA; min_len 0).find_all: a linear scan that keeps the open
    starts of each frame and closes all of them at the frame's next stop.  [(start, end, offset)]."""
    out, open_ = [], [[], [], []]
    for i in range(len(seq) - 2):
        c, f = seq[i:i + 3], i % 3
        if c == b"ATG":
            open_[f].append(i)
        elif c in (b"TAA", b"TAG", b"TGA"):
            out += [(s, i + 3, f) for s in open_[f]]
            open_[f] = []
    return out


def test_property_bio_orfs():
    for seq in _random_seqs(1):
        bio, ck = bio_find_all(seq), R.find_orfs(seq)
        for start, end, off in bio:
            m = [o for o in ck if o[0] == start and o[1] is not None and o[1] + 3 == end]
            assert m, (seq, start, end)
            assert m[0][2] == 0 and m[0][0] % 3 == off
        for o in ck:
            found = any(o[0] == b[0] and (o[1] or 0) + 3 == b[1] for b in bio)
            if o[2] == 0:
                assert found, (seq, o)
            if not found:
                assert o[2] != 0, (seq, o)


def test_property_bio_orfs_repeated():
    for seq in _random_seqs(2, 150):
        dup = seq * 4
        ck = {orf_seq(seq, o[0], o[3]) for o in R.find_orfs(seq)}
        for start, end, _ in bio_find_all(dup):
            assert dup[start:end] in ck, (seq, start, end)


def test_property_no_start_is_its_own_stop_and_lengths_divide_by_three():
    for seq in _random_seqs(3):
        for o in R.find_orfs(seq):
            assert o[1] != o[0]
            assert o[3] % 3 == 0


def test_property_longest_is_a_subset():
    for seq in _random_seqs(4):
        every = R.find_orfs(seq)
        longest = [o[:4] for o in R.orfs_record(seq, strands=1, mode=0)]
        assert len(longest) <= len(every)
        assert all(o in every for o in longest)


# ---- the kernel's per-lane routine against the restatement -----------------------------------------------------------
def adversarial_batch(rng, n=40):
    seqs = []
    for _ in range(n):
        alpha = rng.choice([b"ACGT", b"ATG", b"TAG", b"ATGN-", b"AT", b"ACGTacgt", b"TGA", b"ACGTN"])
        L = rng.choice([rng.randint(0, 12), rng.randint(0, 80), rng.randint(100, 400)])
        seqs.append(bytes(rng.choice(alpha) for _ in range(L)))
    seqs += [b"ATG" + b"C" * 30, b"C" * 31 + b"AT", b"GAT" + b"C" * 25, b"TAATG", b"AT", b"TA", b"ATGATGTAG", b"A", b""]
    return seqs


GRID_CODONS = [(["ATG"], ["TAA", "TAG", "TGA"]), (["ATG", "TAA"], ["TAA", "TAG", "TGA"]), (["ATG", "CTG", "TTG"], ["TAA", "TAG", "TGA"]),
               (["TAG", "ATG", "TGA"], ["TAG"]), (["NNA", "A-G", "AT"], ["TAA", "ATGA"]), (["ATG"], ["ATG", "TAG"])]


def random_params(rng):
    st, sp = rng.choice(GRID_CODONS)
    kw = dict(start_codons=st, stop_codons=sp, min_length=rng.choice([0, 0, 6, 75, 10 ** 9]), min_ratio=rng.choice([0, 0.5, 1, 1.5]),
              min_wraps=rng.randint(0, 3), max_wraps=rng.randint(0, 3), require_stop=rng.random() < 0.5,
              strands=rng.choice([1, 2, 3]), mode=rng.choice([0, 0, 1]))
    if rng.random() < 0.4:
        kw.update(min_length=0, min_ratio=0, min_wraps=0, max_wraps=3)
    return kw


def test_lane_routine_matches_restatement():
    rng = random.Random(7)
    for _ in range(300):
        seqs = adversarial_batch(rng)
        kw = random_params(rng)
        d, o = _pack(seqs)
        eo, e = R.orfs_batch(d, o, **kw)
        go, g = R.lane_orfs_batch(d, o, **kw)
        assert np.array_equal(eo, go), kw
        assert np.array_equal(e, g), kw


def test_lane_routine_every_length_mod_three():
    rng = random.Random(8)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(L)) for L in range(2, 600)]
    seqs += [b"ATG" + bytes(rng.choice(b"ACG") for _ in range(L)) for L in range(0, 200)]       # frames with no stop
    d, o = _pack(seqs)
    for mode in (0, 1):
        for mw in range(4):
            kw = dict(max_wraps=mw, mode=mode, strands=3)
            assert all(np.array_equal(a, b) for a, b in zip(R.orfs_batch(d, o, **kw), R.lane_orfs_batch(d, o, **kw))), kw


def test_ryu_format():
    assert [R.ryu_f64(x) for x in (1.0, 0.5, 0.00012, 1e-7, 3.0, 1e-5, 1.5e-6, 0.1)] == \
        ["1.0", "0.5", "0.00012", "1e-7", "3.0", "0.00001", "1.5e-6", "0.1"]


def test_library_exports_the_orf_entry_points():
    import __graft_entry__ as g
    g.build()
    import circkit_amd
    lib = circkit_amd.load_library()
    for s in ("circkit_orfs_batch_device", "circkit_orfs_status", "circkit_orfs_batch", "circkit_find_orfs"):
        assert hasattr(lib, s), s
    p = circkit_amd.orf_params(start_codons=["ATG", "CTG", "AT"], strands="both", mode="all")
    assert (p.n_start_codons, p.n_stop_codons, p.strands, p.mode) == (2, 3, 3, 1)
