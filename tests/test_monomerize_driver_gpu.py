"""GPU: the driver circkit_amd.monomerize.monomerize_fasta and `python -m circkit_amd.monomerize` on the reference's four
CLI fixtures with the reference's flags, and on the extended realistic input, against the driver restatement
(tests/mono_ref.py) byte for byte and against the reference's out.fasta as id -> sequence maps."""
import os
import subprocess
import sys

import pytest

from tests import mono_ref as R
from tests import mono_sets as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_FLAGS = {"min_overlap": ["--min-overlap", "81"], "min_overlap_percent_0.51": ["--min-overlap-percent", "0.51"],
             "min_overlap_percent_1.0": ["--min-overlap-percent", "1.0"], "min_overlap_percent_1.5": ["--min-overlap-percent", "1.5"]}


def run_module(args, stdin=None):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "circkit_amd.monomerize"] + args, input=stdin, capture_output=True, cwd=ROOT, env=env,
                          timeout=600)


def own_stderr(r):
    """The program's stderr: without the line libdrm prints at device start-up on an installation that lacks its amdgpu.ids
    table (the HIP runtime's library, not this program, writes it)."""
    return b"".join(l for l in r.stderr.splitlines(True) if not l.rstrip().endswith(b"amdgpu.ids: No such file or directory"))


def fixture(name):
    d = os.path.join(S.EXAMPLES, name)
    return os.path.join(d, "in.fasta"), open(os.path.join(d, "in.fasta"), "rb").read(), open(os.path.join(d, "out.fasta"), "rb").read()


@pytest.mark.parametrize("name", sorted(S.FIXTURES))
def test_driver_on_the_fixtures(name):
    from circkit_amd import monomerize as M
    _, text, out = fixture(name)
    for delim in (None, b",", b"\t"):
        got = M.monomerize_fasta(text, table_delim=delim, **S.FIXTURES[name])
        assert got == R.cli_monomerize(text, table_delim=delim, **S.FIXTURES[name])
        assert S.fasta_map(got[0]) == S.fasta_map(out)


@pytest.mark.parametrize("name", sorted(S.FIXTURES))
def test_module_on_the_fixtures(name, tmp_path):
    path, text, out = fixture(name)
    exp, exp_csv = R.cli_monomerize(text, table_delim=b",", **S.FIXTURES[name])
    _, exp_tsv = R.cli_monomerize(text, table_delim=b"\t", **S.FIXTURES[name])
    # file to file with a table: silent success
    for ext, exp_table in ((".csv", exp_csv), (".tsv", exp_tsv)):
        o, t = tmp_path / ("out" + ext + ".fasta"), tmp_path / ("table" + ext)
        r = run_module([path, "-o", str(o), "--table", str(t), "--threads", "2"] + CLI_FLAGS[name])
        assert r.returncode == 0 and r.stdout == b"" and own_stderr(r) == b"", r
        assert o.read_bytes() == exp and t.read_bytes() == exp_table
        assert S.fasta_map(o.read_bytes()) == S.fasta_map(out)
    # stdin to stdout
    r = run_module(CLI_FLAGS[name], stdin=text)
    assert r.returncode == 0 and own_stderr(r) == b"" and r.stdout == exp


def test_extended_realistic_input(tmp_path):
    from circkit_amd import monomerize as M
    from oracle import oracle as O
    text, n, originals = S.extended_realistic()
    plain = M.monomerize_fasta(text, min_identity=0.95, table_delim=b",")
    assert plain == R.cli_monomerize(text, min_identity=0.95, table_delim=b",")
    recs = O.read_fasta(plain[0])
    assert len(recs) == n == 676 and sum(O.full_seq(r) == originals[h] for h, r in recs) == 659
    sens = M.monomerize_fasta(text, min_identity=0.95, sensitive=True)
    assert sens == R.cli_monomerize(text, min_identity=0.95, sensitive=True)
    inp, o = tmp_path / "in.fasta", tmp_path / "out.fasta"
    inp.write_bytes(text)
    r = run_module([str(inp), "--min-identity", "0.95", "--sensitive", "-o", str(o)])
    assert r.returncode == 0 and r.stdout == b"" and own_stderr(r) == b"" and o.read_bytes() == sens[0]
    r = run_module([str(inp), "--max-mismatch", "3", "--keep-all", "--min-length", "300", "--max-length", "2000", "--seed-length", "12"])
    assert r.returncode == 0 and own_stderr(r) == b""
    assert r.stdout == R.cli_monomerize(text, max_mismatch=3, keep_all=True, min_length=300, max_length=2000, seed_length=12)[0]
