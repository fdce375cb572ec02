"""`circkit orfs` (src/orfs.rs:25-192, flags src/commands.rs:174-244): argument handling on the CPU, and on the GPU the
output and --table byte for byte against the restatement of the writer (tests/orfs_ref.py cli_orfs)."""
import gzip
import os
import random
import subprocess

import numpy as np
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


# ---- chunks, long records, many ORFs per chunk, messy FASTA, csv quoting -------------------------------------------------
def fasta(recs, width=None):
    out = []
    for h, s in recs:
        out.append(b">" + h + b"\n")
        out += [s[k:k + width] + b"\n" for k in range(0, len(s), width)] if width else [s + b"\n"]
    return b"".join(out)


def random_records(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [(b"r%d n=%d" % (k, L), lut[rng.integers(0, 4, int(L))].tobytes()) for k, L in enumerate(rng.integers(lo, hi, n))]


def run_chunked(args, chunk_mb, **kw):
    return run(args, env=dict(os.environ, CIRCKIT_CLI_CHUNK_MB=str(chunk_mb)), **kw)


def mapped_chunk_ends(data, chunk):
    """Where run_orfs cuts a mapped file: each chunk ends at the last record start ("\n>") in the next `chunk` bytes, the
    window doubling while it holds none."""
    ends, pos = [], 0
    while pos < len(data):
        want = chunk
        while True:
            if pos + want >= len(data):
                pos = len(data)
                break
            j = data.rfind(b"\n>", pos, pos + want)
            if j >= 0:
                pos = j + 1
                break
            want *= 2
        ends.append(pos)
    return ends


@pytest.mark.gpu
def test_1mb_chunks_and_a_record_longer_than_several(tmp_path):
    """CIRCKIT_CLI_CHUNK_MB=1: 8 MB of records with a 3.5 MB one among them, from a mapped file (whose reader doubles its
    window for the long record), from stdin and from gzip stdin (whose reader grows its buffer).  Output and table byte for
    byte."""
    recs = random_records(1, 1500, 200, 6000)
    recs.insert(700, (b"long record", random_records(2, 1, 3_500_000, 3_500_001)[0][1]))
    data = fasta(recs, width=70)
    assert len(mapped_chunk_ends(data, 1 << 20)) >= 5
    exp, exp_csv = R.cli_orfs(data, table_delim=b",")
    f = tmp_path / "in.fa"
    f.write_bytes(data)
    r = run_chunked(["orfs", str(f), "-o", str(tmp_path / "o.fa"), "--table", str(tmp_path / "t.csv")], 1)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o.fa").read_bytes() == exp
    assert (tmp_path / "t.csv").read_bytes() == exp_csv
    for stdin in (data, gzip.compress(data, 1)):
        r = run_chunked(["orfs"], 1, input=stdin)
        assert r.returncode == 0, r.stderr
        assert r.stdout == exp


@pytest.mark.gpu
def test_default_chunk_input_over_64mb(tmp_path):
    """The default 64 MB chunk, on a file a little over 64 MB: two chunks."""
    data = fasta(random_records(3, 34_000, 1900, 2100))
    assert 64 << 20 < len(data) < 70 << 20 and len(mapped_chunk_ends(data, 64 << 20)) == 2
    exp, _ = R.cli_orfs(data)
    f = tmp_path / "in.fa"
    f.write_bytes(data)
    r = run(["orfs", str(f), "-o", str(tmp_path / "o.fa")])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o.fa").read_bytes() == exp


@pytest.mark.gpu
def test_more_than_65536_orfs_in_one_chunk(tmp_path):
    """-m 0 --no-stop-required on start-dense records: one chunk of more than 65,536 ORFs, past the CLI's first ORF buffer,
    so the batch reports the total and runs again into a grown buffer."""
    rng = random.Random(5)
    units = [b"ATGTAAC", b"ATGAAATAAC", b"ATGCCCTGAGG"]
    data = fasta([(b"dense%d" % k, b"".join(rng.choice(units) for _ in range(2500))) for k in range(40)], width=60)
    exp, exp_csv = R.cli_orfs(data, min_length=0, no_stop_required=True, table_delim=b",")
    assert exp.count(b"\n>") + 1 > 65_536
    f = tmp_path / "in.fa"
    f.write_bytes(data)
    r = run(["orfs", str(f), "-m", "0", "--no-stop-required", "-o", str(tmp_path / "o.fa"), "--table", str(tmp_path / "t.csv")])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o.fa").read_bytes() == exp
    assert (tmp_path / "t.csv").read_bytes() == exp_csv


def messy_fasta():
    """CRLF and multi-line records; lowercase, U / u, IUPAC letters, '.' and '~'; spaces, tabs and a lone CR inside sequence
    lines; headers with ',', '"', a tab, and empty ones ('>' and '> x'); a 700 kb record, whose short ORFs have ratios
    below 1e-5.  Forward ORFs are cut from full_seq() at normalized coordinates, so the output follows wherever the two
    differ."""
    rng = random.Random(13)

    def dna(n):
        return bytearray(rng.choice(b"ACGT") for _ in range(n))

    def sprinkle(s, alphabet, k):
        for _ in range(k):
            s[rng.randrange(len(s))] = rng.choice(alphabet)
        return bytes(s)

    def lines(s, width, eol=b"\n"):
        return b"".join(bytes(s[k:k + width]) + eol for k in range(0, len(s), width))
    big = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(14).integers(0, 4, 700_000)].tobytes()
    return b"".join([
        b">crlf, comma\r\n" + lines(dna(1500), 60, b"\r\n"),
        b'>quote"d "header" here\n' + lines(sprinkle(dna(1500), b"acgtUuRYKMSWBDHVNn.~", 120), 70),
        b">tab\there\tx\n" + lines(sprinkle(dna(1500), b" \t\r", 40), 61),
        b">\n" + lines(dna(1200), 80),
        b"> x\n" + lines(sprinkle(dna(1200), b"acgtu", 300), 50),
        b'>a,b;c="d"\tz\n' + bytes(dna(900)) + b"\n",
        b">big 700 kb\n" + lines(big, 100),
        b">last, no newline\n" + bytes(dna(800)),
    ])


@pytest.mark.gpu
@pytest.mark.parametrize("name,args,kw", [("default", [], {}), ("hyperfine", HYPERFINE, HYPERFINE_KW),
                                          ("reverse", ["--strand", "reverse"], dict(strand="reverse")),
                                          ("short", ["-m", "0"], dict(min_length=0))])
def test_messy_fasta_byte_identical(name, args, kw, tmp_path):
    data = messy_fasta()
    f = tmp_path / "messy.fa"
    f.write_bytes(data)
    for ext, delim in (("csv", b","), ("tsv", b"\t")):
        exp, exp_t = R.cli_orfs(data, table_delim=delim, **kw)
        assert b'"' in exp_t                                            # some table field is quoted
        if name == "short":
            assert b"e-6\n" in exp_t                                    # ratios below 1e-5, in exponent form
        r = run(["orfs", str(f), "-o", str(tmp_path / "o.fa"), "--table", str(tmp_path / ("t." + ext))] + args)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "o.fa").read_bytes() == exp
        assert (tmp_path / ("t." + ext)).read_bytes() == exp_t


@pytest.mark.gpu
def test_one_symbol_record_in_the_third_chunk(tmp_path):
    """At 1 MB chunks, a 1-symbol record in the third chunk of a mapped file: status 101, after exactly the output of the
    two chunks before it."""
    chunk = 1 << 20
    data = fasta(random_records(6, 1500, 1000, 3000), width=80)
    at = data.index(b"\n>", mapped_chunk_ends(data, chunk)[0] + chunk + 100) + 1    # past the second chunk's window
    data = data[:at] + b">tiny\nA\n" + data[at:]
    ends = mapped_chunk_ends(data, chunk)
    assert ends[1] <= at < ends[2]
    exp, _ = R.cli_orfs(data[:ends[1]])
    assert exp
    with pytest.raises(ValueError):
        R.cli_orfs(data)
    f = tmp_path / "in.fa"
    f.write_bytes(data)
    r = run_chunked(["orfs", str(f)], 1)
    assert r.returncode == 101, r.stderr
    assert r.stdout == exp


@pytest.mark.gpu
def test_uniq_table_quotes_like_the_csv_crate(tmp_path):
    """uniq --table with ids that hold ',', '"' or a tab, and empty ids ('>' and '> x', as the kept id and as the duplicate):
    quoted where the csv crate quotes (QuoteStyle::Necessary), and an empty field written bare."""
    from oracle import oracle as O
    s1, s2, s3 = b"ACGTTGCA" * 5 + b"A", b"GATTACA" * 7, b"CCCGGGATAT" * 3

    def rot(s, k):
        return s[k:] + s[:k]
    recs = [(b"first", s1), (b"a,b desc", rot(s1, 3)), (b'q"t', rot(s1, 5)), (b"tab\tid x", s1), (b"", rot(s1, 1)),
            (b"", s2), (b" x", rot(s2, 2)), (b"plain", rot(s2, 4)), (b'"quoted"', s3), (b"x,y", rot(s3, 7)), (b"", rot(s3, 2))]
    data = fasta(recs)
    f = tmp_path / "in.fa"
    f.write_bytes(data)
    for ext, delim in (("csv", b","), ("tsv", b"\t")):
        exp_fa, exp_t = O.cli_uniq(data, delimiter=delim)
        assert b"\n" + delim + b"\n" in exp_t and delim + b"\n" in exp_t  # empty ids, bare
        t = tmp_path / ("t." + ext)
        r = run(["uniq", str(f), "-o", str(tmp_path / "o.fa"), "--table", str(t)])
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "o.fa").read_bytes() == exp_fa
        assert t.read_bytes() == exp_t
