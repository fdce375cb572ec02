"""CPU-only checks of monomerize: the C restatement (tests/mono_ref.c) against the reference's own unit tests (recorded in
tests/golden/ref_monomerize_known_answers.json), its proptests (lib/src/monomerize.rs:516-553, seeded) and its CLI fixtures;
the host driver circkit_amd.monomerize.monomerize_fasta (with the GPU batch call replaced by the restatement) against the
driver restatement byte for byte; the flag errors of the `python -m` wrapper; the complement-free sensitive form."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import mono_ref as R
from tests import mono_sets as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def known():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "ref_monomerize_known_answers.json")))


def known_cases():
    doc = known()

    def get(v):
        return doc["sequences"][v[1:]].encode() if v.startswith("@") else v.encode()
    return [(c["test"], get(c["seq"]), get(c["expected"]), dict(seed_len=c["seed_len"], max_mismatch=c["max_mismatch"],
                                                                 min_identity=c["min_identity"], sensitive=c["sensitive"]))
            for c in doc["cases"]]


def test_restatement_known_answers():
    cases = known_cases()
    assert len(cases) == 277
    names = {c[0] for c in cases}
    assert {"ambivirus", "single_pass_regressions", "overlap_percentage_rounds_down_to_nearest_nt", "sensitive_monomerization",
            "multimer_with_seed_repeated"} <= names
    for name, seq, exp, kw in cases:
        assert R.monomerize(seq, **kw) == exp, (name, kw)


def test_builder_errors():
    with pytest.raises(ValueError, match="overlap_dist and overlap_min_identity"):
        R.params(seed_len=4, max_mismatch=1, min_identity=0.95)
    for k in (0, 64, 100):
        with pytest.raises(ValueError, match="at least 1 and at most 63"):
            R.params(seed_len=k)
    from circkit_amd import api
    with pytest.raises(ValueError, match="overlap_dist and overlap_min_identity"):
        api.monomerize_params(4, 1, 0.95)


def smallest_period(s):
    """The smallest p dividing len(s) with s == s[:p] * (len(s) / p): below len(s) when s is itself a repeat."""
    n = len(s)
    return next(p for p in range(1, n + 1) if n % p == 0 and s == s[:p] * (n // p))


def test_proptest_concatenated_always_monomerizes():
    """x.x.x gives x for [ACGT]{12,100} (identity 0.95, seed 10).  An x that is itself periodic may come out shorter in the
    reference too: such samples are left out, and they are at most 1 % of the sample."""
    rng = random.Random(20240)
    skipped = 0
    for _ in range(2000):
        x = S.rand_seq(rng, rng.randint(12, 100))
        if smallest_period(x) < len(x):
            skipped += 1
            continue
        assert R.monomerize(x * 3, seed_len=10, min_identity=0.95) == x
    assert skipped <= 20


def test_proptest_small_mutations_outside_seed():
    """One substitution at index 10..90 of x.x for [ACGT]{100,200} still gives x."""
    rng = random.Random(20241)
    skipped = 0
    for _ in range(2000):
        x = S.rand_seq(rng, rng.randint(100, 200))
        if smallest_period(x) < len(x):
            skipped += 1
            continue
        cc = S.substituted(x + x, [rng.randrange(10, 90)])
        assert R.monomerize(cc, seed_len=10, min_identity=0.95) == cc[:len(x)]
    assert skipped <= 20


def test_identity_rounding_boundaries():
    """max_dist = ovl - floor(ovl * identity) in f64, at products that are an integer or an ulp away from one."""
    assert [S.max_dist(20, 0.94), S.max_dist(40, 0.94), S.max_dist(20, 0.95), S.max_dist(19, 0.95), S.max_dist(19, 0.9)] == [2, 3, 1, 1, 2]
    assert 20 * 0.94 == 18.799999999999997 and 40 * 0.94 == 37.599999999999994 and 20 * 0.95 == 19.0
    cases = S.identity_boundaries()
    assert len(cases) >= 36
    for rec, ident, ovl, nm, accepted in cases:
        e = R.end_index(rec, seed_len=5, min_identity=ident)
        assert e == (ovl if accepted else None), (ident, ovl, nm)


def test_work_counter_bounds_the_lazy_scan():
    """The restatement counts the bytes it compares: a poly-A record costs n/k passes over a shrinking text (quadratic for a
    plain search), a random record one pass."""
    e, work = R.end_index(b"A" * 2000, want_work=True, seed_len=10)
    assert e == 10 and 2000 * 2000 // 20 // 2 < work < 2000 * 2000
    rng = random.Random(3)
    e, work = R.end_index(S.rand_seq(rng, 2000), want_work=True, seed_len=10)
    assert e is None and work == 1990


# ---- the driver --------------------------------------------------------------------------------------------------------
def ref_batch(data, offsets, **kw):
    return R.batch(data, offsets, threads=2, **kw)


def both_drivers(text, **flags):
    from circkit_amd import monomerize as M
    exp = R.cli_monomerize(text, **flags)
    got = M.monomerize_fasta(text, batch_fn=ref_batch, **flags)
    assert got == exp
    return exp


@pytest.mark.parametrize("name", sorted(S.FIXTURES))
def test_driver_fixtures(name):
    d = os.path.join(S.EXAMPLES, name)
    text = open(os.path.join(d, "in.fasta"), "rb").read()
    fasta, table = both_drivers(text, **S.FIXTURES[name])
    assert table is None
    assert S.fasta_map(fasta) == S.fasta_map(open(os.path.join(d, "out.fasta"), "rb").read())
    for delim in (b",", b"\t"):
        fasta2, table = both_drivers(text, table_delim=delim, **S.FIXTURES[name])
        assert fasta2 == fasta and table.count(b"\n") == fasta.count(b">") + (1 if fasta else 0)


def test_driver_extended_realistic_input():
    text, n, originals = S.extended_realistic()
    assert n == 676
    for sens in (False, True):
        fasta, _ = both_drivers(text, min_identity=0.95, sensitive=sens)
        from oracle import oracle as O
        recs = O.read_fasta(fasta)
        if not sens:
            assert len(recs) == 676
            assert sum(O.full_seq(r) == originals[h] for h, r in recs) == 659
        else:
            assert len(recs) == 676


def test_driver_odd_inputs():
    rng = random.Random(5)
    x, y, z = S.rand_seq(rng, 120), S.rand_seq(rng, 90), S.rand_seq(rng, 40)
    lower = (x + x[:60]).lower()
    rna = (y + y).replace(b"T", b"U")
    spaced = z[:20] + b" " + z[20:] + z[:10] + b" " + z[10:]
    text = (b">lower case\n" + lower + b"\n>rna, with \"quotes\"\r\n" + rna[:70] + b"\r\n" + rna[70:] + b"\r\n>spaced\tid\n" + spaced +
            b"\n>short\nACGT\n>none\n" + S.rand_seq(rng, 200) + b"\n>empty\n\n>polyA\n" + b"A" * 77 + b"\n")
    for flags in (dict(), dict(keep_all=True), dict(keep_all=True, table_delim=b","), dict(table_delim=b"\t"), dict(min_identity=0.9, sensitive=True),
                  dict(max_mismatch=2, min_length=50, table_delim=b","), dict(max_length=100, keep_all=True, table_delim=b","),
                  dict(seed_length=5, min_overlap=30), dict(seed_length=63, keep_all=True), dict(min_overlap_percent=0.4, table_delim=b",")):
        fasta, table = both_drivers(text, **flags)
        if flags == dict(keep_all=True, table_delim=b","):
            assert fasta.count(b">") == 7 and b">lower case\n" + lower[:120] + b"\n" in fasta       # case kept, head whole
            assert b'"rna, with ""quotes""",180,90\n' in table and table.startswith(b"id,original_length,monomer_length\n")
            assert b">spaced\tid\n" + spaced[:40] + b"\n" in fasta          # the index counts normalized symbols, the cut is made in the raw bytes
    assert both_drivers(b"", table_delim=b",") == (b"", b"")
    assert both_drivers(b">only\nACGTACGTAC\n", table_delim=b",") == (b"", b"")


def run_module(args, stdin=b""):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "circkit_amd.monomerize"] + args, input=stdin, capture_output=True, cwd=ROOT, env=env,
                          timeout=300)


def test_module_flag_errors(tmp_path):
    """Status 2 for a bad flag value or both cut-offs, 1 for an identity outside [0, 1] or an unreadable input, 101 for
    --seed-length 64; none of these reaches the GPU."""
    inp = tmp_path / "in.fasta"
    inp.write_bytes(b">a\nACGTACGTACGTACGTACGTACGT\n")
    for args in (["--seed-length", "4"], ["--seed-length", "65"], ["--seed-length", "x"], ["--max-mismatch", "-1"],
                 ["--min-identity", "abc"], ["--max-mismatch", "1", "--min-identity", "0.9"], ["--no-such-flag"], ["--min-overlap", "-3"]):
        r = run_module([str(inp)] + args)
        assert r.returncode == 2 and r.stdout == b"", (args, r)
    for args in (["--min-identity", "1.5"], ["--min-identity", "-0.1"], ["--min-identity", "nan"]):
        r = run_module([str(inp)] + args)
        assert r.returncode == 1 and r.stdout == b"" and b"min_identity must be between 0.0 and 1.0" in r.stderr, (args, r)
    r = run_module([str(tmp_path / "missing.fasta")])
    assert r.returncode == 1 and r.stdout == b""
    r = run_module([str(inp), "--seed-length", "64"])
    assert r.returncode == 101 and r.stdout == b"" and b"at least 1 and at most 63" in r.stderr
    assert run_module([str(tmp_path / "missing.fasta"), "--seed-length", "64"]).returncode == 1       # the input is opened first


# ---- the sensitive form without a reverse complement ---------------------------------------------------------------------
def test_complement_table_is_a_bijection():
    tab = R.complement_table()
    assert len(tab) == 256 and len(set(tab)) == 256


def test_complement_free_sensitive_form_equals_the_literal_one():
    rng = random.Random(99)
    changed = total = 0
    for alpha in (b"ACGT", b"AC", b"ACGTN-", b"A"):
        for _ in range(400):
            n = rng.randint(0, 400)
            s = S.periodic(rng, n, rng.randint(1, 150), alpha, subs=rng.randint(0, 4))
            k = rng.choice((1, 2, 4, 5, 10, 20, 63))
            kw = rng.choice((dict(max_mismatch=0), dict(max_mismatch=1), dict(max_mismatch=5), dict(min_identity=0.95), dict(min_identity=0.9),
                             dict(min_identity=0.5)))
            lit = R.end_index(s, seed_len=k, sensitive=True, **kw)
            assert R.end_index_free(s, seed_len=k, **kw) == lit, (s, k, kw)
            changed += lit != R.end_index(s, seed_len=k, **kw)
            total += 1
    assert changed > total // 20           # the sensitive pass is exercised, not only its "nothing found" branch


def test_restatement_batch_equals_single_calls():
    rng = random.Random(4)
    seqs = S.every_length(rng, 120)
    data, offs = S.pack(seqs)
    for kw in (dict(seed_len=5, max_mismatch=1), dict(seed_len=10, min_identity=0.9, sensitive=True)):
        got = R.batch(data, offs, threads=3, **kw)
        exp = [R.end_index(s, **kw) for s in seqs]
        assert [None if int(g) == R.NONE else int(g) for g in got] == exp
