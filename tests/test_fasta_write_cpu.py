"""CPU-only: the device FASTA writer's surface, and its routines (circkit_amd/csrc/fasta_write.h) run as fibers by a stand-alone
program (tests/emu/fasta_write_emu_main.cpp).  Per record the yardstick is the Python join b">" + head + label + b"\\n" + body +
b"\\n" (tests/fasta_write_sets.py); for whole files it is the pinned writers of canonicalize, uniq, rotate, cat, decat and orfs on
the reference's own fixtures, with the spans the host packer reports."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import fasta_sets
from tests import fasta_write_sets as S
from tests import orfs_ref
from tests import windows_ref as R
from tests.emu import fasta_write_emu as E

NAMES = {"circkit_fasta_write_device": 15, "circkit_fasta_write_status": 3, "circkit_fasta_write_text": 16}
ROTATE_FLAGS = {"rotate_5": dict(bases=5), "rotate_minus_5": dict(bases=-5), "rotate_0.25": dict(percent=0.25), "rotate_0.5": dict(percent=0.5)}


def test_the_surface():
    import __graft_entry__ as g
    g.build()
    import circkit_amd
    from circkit_amd import api
    from tests.test_abi import header_symbols
    lib = circkit_amd.load_library()
    syms = header_symbols()
    for name, n_args in NAMES.items():
        assert name in syms, "include/circkit.h does not declare %s" % name
        assert name in api.SIGNATURES and len(api.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name), "libcirckit_hip.so does not export %s" % name
    for method in ("fasta_write_device", "fasta_write_status", "fasta_write_text"):
        assert callable(getattr(api.Context, method))
    assert callable(circkit_amd.fasta_write_gpu)
    assert api.WINDOW_DTYPE == S.WINDOW_DTYPE and api.FASTA_SPAN_DTYPE.itemsize == 16


@pytest.fixture(scope="module")
def constants():
    return E.constants()


def test_the_sets_hold_what_they_promise(constants):
    T = constants["TILE_BYTES"]
    grid = S.grid_cases()
    assert {c.place["out_shift"] for c in grid} == {c.place["text_shift"] for c in grid} == {c.place["body_shift"] for c in grid} == set(range(16))
    recs, bad = S.expected(grid[0])
    assert bad == 0 and len(recs) == 8 + 34 * 34 and recs[:8] == [b">\n\n"] * 8 and {len(r) for r in recs} == set(range(3, 3 + 67))
    assert any(c.raw is not None for c in grid) and any(c.body is not None for c in grid)
    long_recs = S.expected(S.long_cases(T)[0])[0]
    assert any(len(r) > 3 * T for r in long_recs) and any(T < r.index(b"\n") < 2 * T for r in long_recs)
    assert [sum(len(r) for r in S.expected(c)[0]) for c in S.seam_cases(T)] == [T - 1, T, T + 1, 2 * T - 1, 2 * T + 1]
    assert {9, 10, 99, 100, 10 ** 9 - 1, 10 ** 9, 2 ** 32 - 1, 0} <= set(S.LABEL_STARTS)
    labels = S.label_cases()[0]
    assert {(int(s), int(st)) for s, st in zip(labels.labels["start"], labels.labels["strand"])} == {(s, st) for s in S.LABEL_STARTS for st in (0, 1)}
    assert np.bincount(labels.labels["record"].astype(np.int64))[0] > 30          # one header shared by many outputs
    assert S.label_of(1, 2 ** 32 - 1) == b"_RC_ORF4294967295" and S.label_of(0, 0) == b"_ORF0"
    names = {c.name for c in S.invalid_cases()}
    assert {"record_is_n_src", "header_is_n_heads", "head_one_past_the_text", "head_wraps", "raw_wraps", "strand_2", "reserved_1"} <= names


def test_device_routines_as_fibers(tmp_path, constants):
    """Every accepted case of tests/fasta_write_sets.py through record_length + write_tile in one child process; the program
    checks its canaries, that no input changed and that the lanes of each wave agree on their first record."""
    cases = S.accepted_cases(constants["TILE_BYTES"])
    got = E.run(cases, tmp_path)
    for c, g in zip(cases, got):
        S.check(c, g)


def test_fibers_capacity(tmp_path):
    cases = S.capacity_cases()
    got = E.run([c for c, _ in cases], tmp_path)
    for (c, ok), g in zip(cases, got):
        text, off, total, bad, refused = g
        if ok:
            S.check(c, g)
        elif c.name == "total_beyond_64_bits":
            assert (refused, total, text) == (E.REFUSED_CAPACITY, 2 ** 64 - 1, None) and off.tolist() == [0, 3 + int(c.head[0][1]) + 2 ** 63, 2 ** 64 - 1]
        else:
            recs, _ = S.expected(c)
            assert (refused, total, text) == (E.REFUSED_CAPACITY, sum(len(r) for r in recs), None), c.name     # (every output byte still canary)
            assert off.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in recs])]).tolist()


def test_fibers_overlap(tmp_path):
    cases = S.overlap_cases()
    assert sum(ok for _, ok in cases) == 4 and len(cases) == 10
    got = E.run([c for c, _ in cases], tmp_path)
    for (c, ok), g in zip(cases, got):
        if ok:
            S.check(c, g)
        else:
            assert g[4] == E.REFUSED_OVERLAP and g[0] is None and g[2] == sum(len(r) for r in S.expected(c)[0]), c.name


# ---- whole files, from host-parsed spans -------------------------------------------------------------------------------------
def parsed(text):
    p = fasta_sets.host(text)
    assert p["error"] is None
    recs = [p["data"][int(a):int(b)].tobytes() for a, b in zip(p["offsets"][:-1], p["offsets"][1:])]
    return p, recs


def written(tmp_path, case):
    (text, off, total, bad, refused), = E.run([case], tmp_path)
    assert refused == 0 and bad == 0 and total == len(text) == int(off[-1])
    return text


@pytest.mark.parametrize("name", sorted(S.golden_inputs()))
def test_canonicalize_and_uniq_files(tmp_path, name):
    text = S.golden_inputs()[name]
    p, recs = parsed(text)
    canon = [O.canonicalize(r) for r in recs]
    body, offs = S.pack(canon)
    assert written(tmp_path, S.Case(name, text, p["head"], body=body, offsets=offs, out_shift=5)) == O.cli_canonicalize(text)
    first = {}
    kept = [i for i, c in enumerate(canon) if first.setdefault(O.xxh3_64(c), i) == i]
    body, offs = S.pack([canon[i] for i in kept])
    assert written(tmp_path, S.Case(name, text, p["head"], body=body, offsets=offs, src=kept, out_shift=11)) == O.cli_uniq(text, True)[0]
    assert written(tmp_path, S.Case(name, text, p["head"], raw=p["raw"], src=kept, text_shift=3)) == O.cli_uniq(text, False)[0]


def window_inputs():
    return {k: v for k, v in S.golden_inputs().items() if k not in S.NOT_FOR_WINDOWS}


def test_the_window_fixtures_are_usable():
    for name, text in S.golden_inputs().items():
        same = all(O.normalize(raw)[0] == O.full_seq(raw) for _, raw in O.read_fasta(text))
        assert same == (name not in S.NOT_FOR_WINDOWS), name


@pytest.mark.parametrize("name", sorted(window_inputs()))
def test_rotate_cat_decat_files(tmp_path, name):
    text = window_inputs()[name]
    p, _ = parsed(text)
    lengths = np.diff(p["offsets"].astype(np.int64))
    runs = [(R.CAT, {}, O.cli_cat(text)), (R.DECAT, {}, O.cli_decat(text))]
    if name in ROTATE_FLAGS:
        flags = ROTATE_FLAGS[name]
        runs.append((R.ROTATE_BASES if "bases" in flags else R.ROTATE_PERCENT, flags, O.cli_rotate(text, **flags)))
    for kind, kw, want in runs:
        out, out_off, bad = R.gather(p["data"], p["offsets"], R.windows_of_records(lengths, kind, **kw))
        assert bad == 0
        assert written(tmp_path, S.Case(name, text, p["head"], body=out.tobytes(), offsets=out_off, out_shift=kind)) == want, (name, kind)


@pytest.mark.parametrize("include_stop", (False, True))
def test_orfs_file(tmp_path, include_stop):
    text = S.golden_inputs()["realistic_input"]
    p, _ = parsed(text)
    want = orfs_ref.cli_orfs(text, include_stop=include_stop)[0]
    orf_off, orfs = orfs_ref.orfs_batch(p["data"], p["offsets"], start_codons=["ATG"], min_length=75, max_wraps=3, require_stop=True, strands=3, mode=0)
    wins = R.orf_windows(orf_off, orfs, include_stop)
    out, out_off, bad = R.gather(p["data"], p["offsets"], wins)
    assert bad == 0 and len(wins) > 100 and (wins["strand"] == 1).any()
    assert written(tmp_path, S.Case("orfs", text, p["head"], body=out.tobytes(), offsets=out_off, labels=wins, out_shift=9)) == want
