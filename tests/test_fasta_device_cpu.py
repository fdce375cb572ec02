"""CPU-only: the device FASTA parser's surface, and its routines (circkit_amd/csrc/fasta_device.h) run as fibers by a stand-alone
program (tests/emu/fasta_emu_main.cpp) against the host packer circkit_fasta_parse on the same text with the same flags:
record count, consumed, every offset, every payload byte, every header and raw span, the format error."""
import numpy as np

from tests import fasta_sets as S
from tests.emu import fasta_emu

NAMES = {"circkit_fasta_parse_device": 11, "circkit_fasta_parse_status": 4, "circkit_fasta_parse_text": 14}


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
    for method in ("fasta_parse_device", "fasta_parse_status", "fasta_parse_text"):
        assert callable(getattr(api.Context, method))
    assert callable(circkit_amd.fasta_parse_gpu)
    assert api.FASTA_SPAN_DTYPE.itemsize == 16


def test_the_table_as_the_host_answers_it():
    """The corner cases the device parser was specified with, reproduced through the host routine."""
    h = S.host
    assert (h(b"")["records"], h(b"")["consumed"]) == (0, 0)
    assert (h(b"\n\r\n")["records"], h(b"\n\r\n")["consumed"]) == (0, 3)
    r = h(b"\r>a\nAC\n")
    assert r["records"] == 1 and r["head"].tolist() == [[2, 1]]
    assert h(b" >a\n")["error"] == S.FORMAT_ERROR
    r = h(b">abc")
    assert r["head"].tolist() == [[1, 3]] and r["raw"].tolist() == [[4, 0]] and len(r["data"]) == 0
    r = h(b">abc\r\n")
    assert r["head"].tolist() == [[1, 3]] and r["raw"].tolist() == [[6, 0]]
    r = h(b">a\n>b\nAC\n>c")
    assert r["records"] == 3 and r["offsets"].tolist() == [0, 0, 2, 2]
    r = h(b">a>b\nAC>G\n>c\nT")
    assert r["data"].tobytes() == b"ACNGT" and r["offsets"].tolist() == [0, 4, 5]
    r = h(b">a\nAC\r>b\nGG\n")
    assert r["records"] == 1 and r["data"].tobytes() == b"ACNNGG"
    r = h(b">a\nAC\n>b\nGG\n>c\nTT", True, False)
    assert (r["records"], r["consumed"]) == (2, 12)
    r = h(b">a\nACGT\nAC", True, False)
    assert (r["records"], r["consumed"]) == (0, 0)
    r = h(b">a\nAC\n>", True, False)
    assert (r["records"], r["consumed"]) == (1, 6)
    r = h(b"XYZ\nAC\n>b\nGG\n>c", False, False)
    assert (r["records"], r["consumed"]) == (2, 13) and r["head"][0].tolist() == [1, 2]
    r = h(b"\n\n>a\nAC", True, False)
    assert (r["records"], r["consumed"]) == (0, 2)


def test_the_sets_hold_what_they_promise():
    small, large = S.small_cases(), S.large_cases()
    assert sum(1 for c in small if c[0].startswith("random")) >= 4 * 300 - 300 and len(large) >= 4 * 40 - 40
    assert any(S.host(t, f, l)["error"] for _, t, f, l in small) and any(S.host(t, f, l)["error"] for _, t, f, l in large)
    assert any(S.host(t, f, l)["records"] > 100 for _, t, f, l in large)
    assert {(f, l) for _, _, f, l in small} == set(S.FLAG_PAIRS)


def run_and_compare(cases, tmp_path, places=None):
    got = fasta_emu.run([(t, f, l, (places[k] if places else {})) for k, (_, t, f, l) in enumerate(cases)], tmp_path)
    for (name, t, f, l), g in zip(cases, got):
        S.same(g, S.host(t, f, l), what=(name, f, l))


def test_small_texts(tmp_path):
    cases = S.small_cases()
    places = [dict(in_shift=k % 16, out_shift=(5 * k + 3) % 16) for k in range(len(cases))]
    run_and_compare(cases, tmp_path, places)


def test_large_texts(tmp_path):
    cases = S.large_cases()
    places = [dict(in_shift=(3 * k) % 16, out_shift=(7 * k + 1) % 16) for k in range(len(cases))]
    run_and_compare(cases, tmp_path, places)


def test_tile_edges(tmp_path):
    """What sits on a tile's seam: text lengths round one and two tiles, a record start as a tile's first and last byte, '\\n' as
    a tile's last byte with '>' the next tile's first, a header of 2.5 tiles, a line of 3 tiles, a tile of dropped bytes only."""
    T = fasta_emu.constants()["TILE_BYTES"]
    cases = S.tile_edge_texts(T)
    run_and_compare(cases, tmp_path, [dict(in_shift=k % 16, out_shift=(k + 9) % 16) for k in range(len(cases))])


def test_capacities_and_refusals(tmp_path):
    rng = np.random.default_rng(8)
    text = S.records_text(rng, 30, 333, width=60)
    exp = S.host(text)
    R, B = exp["records"], len(exp["data"])
    places = [dict(record_capacity=R, byte_capacity=B), dict(record_capacity=R - 1, byte_capacity=B), dict(record_capacity=R, byte_capacity=B - 1),
              dict(record_capacity=0, byte_capacity=0), dict(record_capacity=R + 5, byte_capacity=B + 100, out_shift=7)]
    got = fasta_emu.run([(text, True, True, p) for p in places], tmp_path)
    for g, refused in zip(got, (0, 1, 1, 1, 0)):
        assert g["refused"] == refused and (g["records"], g["bytes"], g["consumed"]) == (R, B, len(text))
        if refused:
            assert g["offsets"].tolist() == [0] and len(g["data"]) == 0          # (the program checked the canaries behind them)
        else:
            S.same(g, exp)
