"""CPU-only: the translate surface of the ABI, the restatement tests/translate_ref.py against hand-worked proteins and against
the sequence lines of `circkit orfs`, and the device routine circkit_amd/csrc/window_translate.h run as fibers by a stand-alone
program (tests/emu/translate_emu_main.cpp) against the restatement, residue for residue."""
import numpy as np
import pytest

from tests import orfs_ref
from tests import translate_ref as T
from tests import translate_sets as TS
from tests import windows_ref as R
from tests import windows_sets as S
from tests.test_windows_cpu import ORF_FLAGS

NAMES = {"circkit_windows_translate_device": 10, "circkit_translate_status": 3, "circkit_windows_translate": 11}

# the standard code, typed out codon by codon (NCBI table 1)
STANDARD = {
    "TTT": "F", "TTC": "F", "TTA": "L", "TTG": "L", "TCT": "S", "TCC": "S", "TCA": "S", "TCG": "S",
    "TAT": "Y", "TAC": "Y", "TAA": "*", "TAG": "*", "TGT": "C", "TGC": "C", "TGA": "*", "TGG": "W",
    "CTT": "L", "CTC": "L", "CTA": "L", "CTG": "L", "CCT": "P", "CCC": "P", "CCA": "P", "CCG": "P",
    "CAT": "H", "CAC": "H", "CAA": "Q", "CAG": "Q", "CGT": "R", "CGC": "R", "CGA": "R", "CGG": "R",
    "ATT": "I", "ATC": "I", "ATA": "I", "ATG": "M", "ACT": "T", "ACC": "T", "ACA": "T", "ACG": "T",
    "AAT": "N", "AAC": "N", "AAA": "K", "AAG": "K", "AGT": "S", "AGC": "S", "AGA": "R", "AGG": "R",
    "GTT": "V", "GTC": "V", "GTA": "V", "GTG": "V", "GCT": "A", "GCC": "A", "GCA": "A", "GCG": "A",
    "GAT": "D", "GAC": "D", "GAA": "E", "GAG": "E", "GGT": "G", "GGC": "G", "GGA": "G", "GGG": "G",
}


# ---- 1. the surface ----------------------------------------------------------------------------------------------------------
def test_the_surface():
    import ctypes
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
    for method in ("windows_translate_device", "translate_status", "windows_translate", "orf_proteins"):
        assert callable(getattr(api.Context, method))
    for fn in ("windows_translate", "orf_proteins", "translate_params"):
        assert callable(getattr(circkit_amd, fn))
    assert ctypes.sizeof(api.TranslateParams) == 72
    codes = T.genetic_codes()
    assert {1, 4, 11} <= set(api.GENETIC_CODES) and circkit_amd.GENETIC_CODES is api.GENETIC_CODES
    for k in (1, 4, 11):
        assert api.GENETIC_CODES[k].encode() == codes[k]
    p = api.translate_params(table=4, unknown="?", first_as_m=True)
    assert bytes(p.aa) == codes[4] and (p.unknown, p.first_as_m, bytes(p.reserved)) == (ord("?"), 1, bytes(6))
    assert bytes(api.translate_params(table=TS.DISTINCT).aa) == TS.DISTINCT and api.translate_params().first_as_m == 0
    with pytest.raises(ValueError):
        api.translate_params(table="FF")


# ---- 2. the restatement ------------------------------------------------------------------------------------------------------
def test_the_table_string_against_the_codon_dictionary():
    codes = T.genetic_codes()
    assert len(STANDARD) == 64 and codes[1] == codes[11] and all(len(v) == 64 for v in codes.values())
    for codon, residue in STANDARD.items():
        want = "W" if codon == "TGA" else residue
        assert T.translate(codon.encode(), codes[1]) == residue.encode(), codon
        assert T.translate(codon.encode(), codes[4]) == want.encode(), codon
        i = 16 * "TCAG".index(codon[0]) + 4 * "TCAG".index(codon[1]) + "TCAG".index(codon[2])
        assert chr(codes[1][i]) == residue and chr(codes[4][i]) == want
    assert [k for k in range(64) if codes[1][k] != codes[4][k]] == [14]


def one_window(seq, length, start=0, strand=0, first_as_m=False, aa=None):
    data, offs = S.pack_like([seq])
    out, off, bad = T.windows_translate(data, offs, R.windows([(length, 0, start, strand)]), aa or T.genetic_codes()[1], b"X", first_as_m)
    assert bad == 0 and off.tolist() == [0, len(out)]
    return bytes(out)


def test_hand_worked_proteins():
    from oracle import oracle as O
    assert one_window(b"ATGGCCAAGTAA", 12) == b"MAK*"
    rc = O.revcomp(b"ATGGCCAAGTAA")
    assert rc == b"TTACTTGGCCAT" and one_window(rc, 12, strand=1) == b"MAK*"
    assert one_window(b"CTGGCC", 6, first_as_m=True) == b"MA" and one_window(b"CTGGCC", 6) == b"LA"
    assert one_window(b"ATGNCC", 6) == b"MX" and one_window(b"NTGGCC", 6, first_as_m=True) == b"XA"
    assert one_window(b"A", 7) == b"KK"                              # AAAAAAA: two codons AAA and a symbol left over
    assert one_window(b"AT", 6, start=1) == b"YI"                    # TATATA: TAT ATA
    assert one_window(b"ATGGCCAAGTAA", 11) == b"MAK" and one_window(b"ATGGCCAAGTAA", 2) == b"" and one_window(b"", 9) == b""
    assert one_window(b"atgGCC", 6) == b"XA" and one_window(b"ATG-CC", 6) == b"MX"


@pytest.mark.parametrize("include_stop", (False, True))
@pytest.mark.parametrize("flags", ORF_FLAGS, ids=("default", "no-stop-required"))
def test_orf_window_proteins_are_the_translated_sequence_lines(flags, include_stop):
    seqs = S.orf_records()
    data, offs = S.pack_like(seqs)
    lines = S.sequence_lines(orfs_ref.cli_orfs(S.fasta_of(seqs), include_stop=include_stop, **flags)[0])
    kw = dict(start_codons=flags.get("start_codons", "ATG").split(","), min_length=75, max_wraps=flags.get("max_wraps", 3),
              require_stop=not flags.get("no_stop_required", False), strands=3, mode=0)
    orf_off, orfs = orfs_ref.orfs_batch(data, offs, **kw)
    wins = R.orf_windows(orf_off, orfs, include_stop)
    for aa, first_as_m in ((T.genetic_codes()[1], False), (T.genetic_codes()[4], True)):
        out, off, bad = T.windows_translate(data, offs, wins, aa, b"X", first_as_m)
        got = S.split(out, off)
        assert bad == 0 and len(lines) > 100 and got == [T.translate(l, aa, b"X", first_as_m) for l in lines]
        assert any(b"X" in g for g in got) and (not first_as_m or all(g[:1] in (b"M", b"X") for g in got))
        if include_stop and not flags and not first_as_m:
            assert all(g.endswith(b"*") and b"*" not in g[:-1] for g in got if b"X" not in g)


def test_the_numpy_restatement_is_the_loop():
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(TS.ALPHABET, dtype=np.uint8)
    seqs = S.orf_records() + [bytes(alphabet[rng.integers(0, len(alphabet), size=int(n))]) for n in rng.integers(0, 40, size=300)] + [b"", b"A", b"NN"]
    data, offs = S.pack_like(seqs)
    for aa, unknown, first_as_m in TS.CODES:
        out, off = T.translate_packed(data, offs, aa, unknown, first_as_m)
        assert S.split(out, off) == [T.translate(s, aa, unknown, first_as_m) for s in seqs]
    out, off = T.translate_packed(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), TS.TABLE_1)
    assert len(out) == 0 and off.tolist() == [0]


# ---- 3. the device routine on the CPU ----------------------------------------------------------------------------------------
def test_constants_move_the_boundary_cases():
    from tests.emu import translate_emu
    c = TS.constants()
    assert translate_emu.constants() == (c["TILE_RESIDUES"], c["TRANSLATE_WAVES"])
    shifted = dict(c, WSCAN_TILE=c["WSCAN_TILE"] * 2, TILE_RESIDUES=c["TILE_RESIDUES"] // 2)
    counts = lambda cc: sorted(len(case[3]) for case in TS.boundary_cases(np.random.default_rng(0), cc))
    assert counts(shifted) != counts(c)
    assert {c["WSCAN_TILE"] - 1, c["WSCAN_TILE"], c["WSCAN_TILE"] + 1, c["TILE_RESIDUES"] // 16 - 1, c["TILE_RESIDUES"] // 16 + 1} <= set(counts(c))
    totals = {int(TS.expected(case)[1][-1]) for case in TS.boundary_cases(np.random.default_rng(0), c) if case[0].startswith("tile")}
    assert {c["TILE_RESIDUES"] - 1, c["TILE_RESIDUES"], c["TILE_RESIDUES"] + 1} <= totals


def test_the_case_list_holds_what_it_names():
    cases = TS.all_cases()
    assert {p.get("in_shift", 0) for *_, p, _ in cases} == set(range(16)) == {p.get("out_shift", 0) for *_, p, _ in cases}
    assert {code for *_, code in cases} == set(TS.CODES) and any(p.get("lead", 0) for *_, p, _ in cases)
    wins = cases[0][3]
    for r, n in enumerate(TS.RECORD_LENGTHS):
        mine = wins[wins["record"] == r]
        assert {int(x) for x in mine["length"]} >= {x for x in TS.window_lengths(n) if x >= 0}
        assert {int(x) for x in mine["start"]} >= {x for x in TS.window_starts(n) if x >= 0} and set(mine["strand"][mine["reserved"] == 0]) >= {0, 1}
    c = TS.constants()
    spans = [w for w in cases[-1][3] if int(w["length"]) // 3 > 2 * c["TILE_RESIDUES"]]
    assert {int(w["strand"]) for w in spans} == {0, 1}


def test_device_routine_as_fibers(tmp_path):
    """Every case of tests/translate_sets.py through residue_length + translate_tile in one child process; the program checks
    its canaries, that the payload and the windows are unchanged and that the lanes of each wave agree on their first window."""
    from tests.emu import translate_emu
    cases = TS.all_cases()
    got = translate_emu.run([case[1:] for case in cases], tmp_path)
    for case, (out, out_off, total, bad) in zip(cases, got):
        exp, exp_off, exp_bad = TS.expected(case)
        assert np.array_equal(out_off, exp_off), case[0]
        assert total == len(exp) and bad == exp_bad, case[0]
        assert np.array_equal(out, exp), case[0]
    grid = TS.expected(cases[0])
    assert grid[2] > 10 and len(grid[0]) > 50_000
    known = grid[0] != ord("X")
    assert 0.2 < known.mean() < 0.8                                              # both kinds of codon in numbers


def test_fibers_refuse_a_short_capacity(tmp_path):
    from tests.emu import translate_emu
    case = TS.shift_cases(np.random.default_rng(3))[5]
    _, data, offs, wins, _, code = case
    exp, exp_off, _ = TS.expected(case)
    got = translate_emu.run([(data, offs, wins, dict(capacity=len(exp) - 1), code), (data, offs, wins, dict(capacity=0), code),
                             (data, offs, wins, dict(capacity=len(exp)), code)], tmp_path)
    for out, out_off, total, _ in got[:2]:
        assert out is None and total == len(exp) and np.array_equal(out_off, exp_off)      # (the program found every residue still canary)
    assert np.array_equal(got[2][0], exp)
