"""`circkit orfs` (src/orfs.rs:25-192, flags src/commands.rs:174-244): argument handling on the CPU, and on the GPU the
output and --table byte for byte against the restatement of the writer (tests/orfs_ref.py cli_orfs)."""
import gzip
import os
import subprocess

import pytest

from tests import orfs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circkit_amd", "circkit")
REALISTIC = os.path.join(ROOT, "tests", "golden", "ref_examples", "nim_cated", "realistic_input.fasta")
HYPERFINE = ["--start-codons", "ATG,CTG,TTG", "--max-wraps", "0", "--include-stop", "--strand", "both"]
HYPERFINE_KW = dict(start_codons="ATG,CTG,TTG", max_wraps=0, include_stop=True, strand="both")


@pytest.fixture(scope="module", autouse=True)
def cli_binary():
    from circkit_amd import build
    build.build_all()
    assert os.path.exists(BIN)


def run(args, **kw):
    return subprocess.run([BIN] + args, capture_output=True, timeout=600, **kw)


def test_help_exits_0():
    r = run(["orfs", "--help"])
    assert r.returncode == 0 and b"orfs" in r.stdout


@pytest.mark.parametrize("args", [["--strand", "up"], ["--max-wraps", "x"], ["--min-ratio", "y"], ["-m", "-1"],
                                  ["--min-wraps=1.5"], ["--strand"], ["--bogus"]])
def test_bad_values_exit_2(args, tmp_path):
    r = run(["orfs", str(tmp_path / "missing.fa")] + args)
    assert r.returncode == 2, (args, r.stderr)


# ---- GPU ----------------------------------------------------------------------------------------------------------
def realistic():
    return open(REALISTIC, "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("name,args,kw", [("default", [], {}), ("hyperfine", HYPERFINE, HYPERFINE_KW),
                                          ("forward", ["--strand", "forward"], dict(strand="forward")),
                                          ("reverse", ["--strand", "reverse"], dict(strand="reverse")),
                                          ("loose", ["-m0", "--no-stop-required", "--min-wraps=1", "--min-ratio", "0.5"],
                                           dict(min_length=0, no_stop_required=True, min_wraps=1, min_ratio=0.5))])
def test_realistic_input_byte_identical(name, args, kw, tmp_path):
    data = realistic()
    exp, exp_csv = R.cli_orfs(data, table_delim=b",", **kw)
    _, exp_tsv = R.cli_orfs(data, table_delim=b"\t", **kw)
    assert exp, "the fixture yields ORFs"
    r = run(["orfs", REALISTIC, "-o", str(tmp_path / "o.fa"), "--table", str(tmp_path / "t.csv")] + args)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o.fa").read_bytes() == exp
    assert (tmp_path / "t.csv").read_bytes() == exp_csv
    r = run(["orfs", REALISTIC, "--table", str(tmp_path / "t.tsv")] + args)
    assert r.returncode == 0 and r.stdout == exp
    assert (tmp_path / "t.tsv").read_bytes() == exp_tsv


@pytest.mark.gpu
def test_stdin_gz_and_zst(tmp_path):
    data = realistic()
    exp, _ = R.cli_orfs(data, **HYPERFINE_KW)
    r = run(["orfs"] + HYPERFINE, input=data)                                   # stdin
    assert r.returncode == 0 and r.stdout == exp
    (tmp_path / "in.fa.gz").write_bytes(gzip.compress(data))
    r = run(["orfs", str(tmp_path / "in.fa.gz"), "-o", str(tmp_path / "o.fa.gz")] + HYPERFINE)
    assert r.returncode == 0, r.stderr
    assert gzip.decompress((tmp_path / "o.fa.gz").read_bytes()) == exp
    r = run(["orfs"] + HYPERFINE, input=gzip.compress(data))                   # compressed stdin
    assert r.returncode == 0 and r.stdout == exp
    # .zst both ways (libzstd): `circkit cat` is the host-only round trip that writes and reads it
    r = run(["decat", "-o", str(tmp_path / "in.fa.zst")], input=R_double(data))
    assert r.returncode == 0, r.stderr
    r = run(["orfs", str(tmp_path / "in.fa.zst"), "-o", str(tmp_path / "o.fa.zst")] + HYPERFINE)
    assert r.returncode == 0, r.stderr
    r = run(["decat", str(tmp_path / "o.fa.zst")])
    assert r.returncode == 0
    from oracle import oracle as O
    assert r.stdout == O.cli_decat(exp)


def R_double(data):
    """FASTA whose decat is `data`'s records (each sequence written twice)."""
    from oracle import oracle as O
    return O.cli_cat(data)


@pytest.mark.gpu
def test_empty_table_and_small_records(tmp_path):
    fa = b">a b\nATGAAATAA\n>c\nAT\n>d\natgccctag\n"
    exp, tab = R.cli_orfs(fa, min_length=0, table_delim=b",")
    r = run(["orfs", "-m", "0", "--table", str(tmp_path / "t.csv")], input=fa)
    assert r.returncode == 0 and r.stdout == exp
    assert (tmp_path / "t.csv").read_bytes() == tab
    r = run(["orfs", "--table", str(tmp_path / "e.csv")], input=fa)          # nothing of 75 nt: empty output, empty table
    assert r.returncode == 0 and r.stdout == b"" and (tmp_path / "e.csv").read_bytes() == b""


@pytest.mark.gpu
def test_one_symbol_record_exits_101():
    r = run(["orfs"], input=b">a\nATGAAATAA\n>b\nA\n")
    assert r.returncode == 101
