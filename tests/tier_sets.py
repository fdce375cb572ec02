"""Record sets that sit ON the admission boundaries of the LDS stages, their teams, the mixed-length kernels and the scratch.

Beyond the register and lean routines a record's route is decided by admission arithmetic: a predicate on its length n against
a slice capacity, exact, without slack (canon_core.h canon_record / team_pass, canon_kernels.h team_stage_block, circkit_canon.hip launch_single,
canon_mixed.h canon_lean_record).  This module holds
  * the predicates and the capacity table restated in Python, with a reader of the same constants from the source text, so that
    the restated copy cannot drift unnoticed (tests/test_tier_sets_cpu.py),
  * n_max(pred, cap): the largest admitted length, by bisection -- no boundary length is typed in here,
  * one record maker per ALPHABET CLASS; the class fixes which predicate governs the record whatever the draw, and check_class()
    proves it from the record alone,
  * TRIPLES: per stage the (class, predicate, capacity) triples the code can reach there, UNREACHABLE: the others with the reason,
  * the batches the emulator tests (CPU) and the device tests (GPU) run.
Pure Python + numpy: no GPU, no emulator."""
import os
import re
from collections import namedtuple

import numpy as np

from tests import seqsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circkit_amd", "csrc")


# ---- the predicates, restated (dwords a record of n symbols needs) ------------------------------------------------------------
def need_dw(bits, n):
    """canon_core.h need_dw<BITS>: the stored strand(s) + 2 words of extension each, the candidate bitmask, one word"""
    s = 32 // bits
    return (2 if bits == 8 else 1) * ((n + s - 1) // s + 2) + (n + 31) // 32 + 1


def need_dw_strand2(n):
    return (n + 15) // 16 + 2


def need_dw_2n(n):
    return (n + 15) // 16 + 2 + (n >> 5) + 2


def need_dw_strand4(n):
    return (n + 7) // 8 + 2


def lean_strand_dw(n):
    return 1 + (n + 30) // 16 + 2


def lean_mask_dw(n):
    return ((n + 30) // 16 + 3 + 1) // 2


LEAN_CAND_MAX = 16
LEAN_CAND_DW = LEAN_CAND_MAX + 2
WORST_CASE_SLACK = 64


def worst_case_dw(n):
    return 2 * ((n + 3) // 4 + 2) + (n + 31) // 32 + 1 + WORST_CASE_SLACK


PREDICATES = {
    "strand2": need_dw_strand2,                                     # pure ACGT, unique minimal key: the strand alone
    "need2": lambda n: need_dw(2, n),                               # pure ACGT, tied minimal key: + the candidate bitmask
    "2n": need_dw_2n,                                               # a few N: strand + N bitmask
    "strand4": need_dw_strand4,                                     # the 4-bit team: the strand alone
    "need4": lambda n: need_dw(4, n),                               # one wave in the 4-bit mode
    "need8": lambda n: need_dw(8, n),                               # byte mode
    "lean": lean_strand_dw,                                         # mixed-length kernel, pure build
    "lean_n": lambda n: lean_strand_dw(n) + lean_mask_dw(n) + LEAN_CAND_DW,    # ...its N build
    "worst": worst_case_dw,                                         # launch_single's pick of a one-wave slice
}

# ---- the capacities, restated -------------------------------------------------------------------------------------------------
CK_TIER_A, CK_TIER_B1, CK_TIER_B2 = 1280, 1900, 3324
TIER_DW = (CK_TIER_A, CK_TIER_B1, CK_TIER_B2, 9980, 40188)          # launch_single's one-wave slices
BATCH_SLICE_DW = (CK_TIER_A, 9980 // 4)                              # stages A and C, per wave; four waves to a workgroup
TEAM_WAVES = 16
TEAM_SLICE_DW = TIER_DW[4] // 16                                     # (truncates: the team stage has 16 x 2511 = 40176 dwords, not 40188)
CK_MIXED_N_SLICE = 1904
GSLICE1_DW = 1 << 20
TEAM_MAX_OWNERS = 8
STAGE_WAVES = {"A": 4, "C": 4, "T": TEAM_WAVES}
STAGE_SLICE = {"A": BATCH_SLICE_DW[0], "C": BATCH_SLICE_DW[1], "T": TEAM_SLICE_DW}


def stage_cap(stage, route):
    """dwords of a stage's route: one wave's slice, or the workgroup's slices together (team, wave 0 alone)"""
    return STAGE_SLICE[stage] * (1 if route == "wave" else STAGE_WAVES[stage])


def source_constants():
    """the same constants as the sources spell them (text, no compiler): name -> value, and the predicates' return expressions"""
    hip = open(os.path.join(CSRC, "canon_config.h")).read()
    canon = open(os.path.join(CSRC, "circkit_canon.hip")).read()
    core = open(os.path.join(CSRC, "canon_core.h")).read()
    mixed = open(os.path.join(CSRC, "canon_mixed.h")).read()

    def one(text, pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    c = {}
    for name in ("CK_TIER_A", "CK_TIER_B1", "CK_TIER_B2", "CK_MIXED_N_SLICE"):
        c[name] = int(one(hip, r"#define %s (\d+)" % name))
    c["TIER_DW"] = one(hip, r"TIER_DW\[N_TIERS\] = \{([^}]*)\}").strip()
    c["BATCH_SLICE_DW"] = one(hip, r"BATCH_SLICE_DW\[BATCH_TIERS - 1\] = \{([^}]*)\}").strip()
    c["TEAM_SLICE_DW"] = one(hip, r"TEAM_SLICE_DW = ([^;]*);")
    c["TIER_D_DW"] = one(hip, r"TIER_D_DW = ([^;]*);")
    c["TEAM_WAVES"] = int(one(hip, r"constexpr int TEAM_WAVES = (\d+);"))
    c["GSLICE1_DW"] = one(hip, r"GSLICE1_DW = ([^;]*);")
    c["worst_case_dw"] = one(hip, r"worst_case_dw\(uint64_t n\) \{ return ([^;]*); \}")
    c["single_handover"] = one(canon, r"if \(n == 1 && ([^)]*\) / 16 \+ 2 <= TIER_DW\[0\])\)")
    c["LEAN_CAND"] = one(mixed, r"constexpr uint32_t (LEAN_CAND_MAX = \d+, LEAN_CAND_DW = [^;]*);")
    c["lean_strand_dw"] = one(mixed, r"lean_strand_dw\(uint32_t n\) \{ return ([^;]*); \}")
    c["lean_mask_dw"] = one(mixed, r"lean_mask_dw\(uint32_t n\) \{ return ([^;]*); \}")
    c["lean_admission"] = one(mixed, r"if \((strand_dw \+ [^\n]*) > a\.slice_dw\) return 3;")
    c["need_dw"] = one(core, r"need_dw\(uint32_t n\)\s*\{\s*constexpr uint32_t S = 32 / BITS;\s*return ([^;]*);")
    c["need_dw_strand2"] = one(core, r"need_dw_strand2\(uint32_t n\) \{ return ([^;]*); \}")
    c["need_dw_2n"] = one(core, r"need_dw_2n\(uint32_t n\) \{ return ([^;]*); \}")
    c["need_dw_strand4"] = one(core, r"need_dw_strand4\(uint32_t n\) \{ return ([^;]*); \}")
    c["TEAM_MAX_OWNERS"] = int(one(core, r"constexpr uint32_t TEAM_MAX_OWNERS = (\d+);"))
    return c


# what source_constants() must read for the restated copy above to be the sources' arithmetic
EXPECTED_SOURCE = {
    "CK_TIER_A": CK_TIER_A, "CK_TIER_B1": CK_TIER_B1, "CK_TIER_B2": CK_TIER_B2, "CK_MIXED_N_SLICE": CK_MIXED_N_SLICE,
    "TIER_DW": "CK_TIER_A, CK_TIER_B1, CK_TIER_B2, %d, CK_LUT_STRIDE == 1 ? %du : 31996u" % TIER_DW[3:],
    "BATCH_SLICE_DW": "CK_TIER_A, %d / 4" % TIER_DW[3],
    "TEAM_SLICE_DW": "TIER_D_DW / 16", "TIER_D_DW": "TIER_DW[N_TIERS - 1]", "TEAM_WAVES": TEAM_WAVES,
    "GSLICE1_DW": "1ull << 20",
    "worst_case_dw": "2 * ((n + 3) / 4 + 2) + (n + 31) / 32 + 1 + %d" % WORST_CASE_SLACK,
    "single_handover": "(max_len + 15) / 16 + 2 <= TIER_DW[0]",
    "LEAN_CAND": "LEAN_CAND_MAX = %d, LEAN_CAND_DW = LEAN_CAND_MAX + 2" % LEAN_CAND_MAX,
    "lean_strand_dw": "1 + (n + 30) / 16 + 2", "lean_mask_dw": "((n + 30) / 16 + 3 + 1) / 2",
    "lean_admission": "strand_dw + (NM ? lean_mask_dw(n) + LEAN_CAND_DW : 0)",
    "need_dw": "(BITS == 8 ? 2 : 1) * ((n + S - 1) / S + 2) + (n + 31) / 32 + 1",
    "need_dw_strand2": "(n + 15) / 16 + 2", "need_dw_2n": "(n + 15) / 16 + 2 + (n >> 5) + 2", "need_dw_strand4": "(n + 7) / 8 + 2",
    "TEAM_MAX_OWNERS": TEAM_MAX_OWNERS,
}


# ---- boundaries by construction -----------------------------------------------------------------------------------------------
def n_max(pred, cap):
    """the largest n with pred(n) <= cap (pred: a name in PREDICATES or a function, non-decreasing in n), by bisection"""
    f = PREDICATES[pred] if isinstance(pred, str) else pred
    lo, hi = 0, 1 << 31                                 # f(lo) <= cap < f(hi)
    assert f(lo) <= cap < f(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f(mid) <= cap:
            lo = mid
        else:
            hi = mid
    return lo


def probes(nm):
    """the probe lengths round a boundary: the last admitted length, the first refused one, and a strand word / a mask word away"""
    return [nm - 16, nm - 1, nm, nm + 1, nm + 16, nm + 17]


# ---- record makers, one per alphabet class ------------------------------------------------------------------------------------
RUN_WIN, RUN_LOSE, RUN_CAP = 14, 11, 8          # the planted A-run, the planted T-run, the longest A- or T-run anywhere else
KEEP_OFF = 64                                   # N, gaps and strangers stay this far from both planted runs
CLASSES = ("pure", "pure_rc", "tie", "few_n", "few_n_rc", "gap", "byte")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CG = np.frombuffer(b"CG", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGTN-RY", b"TGCAN-YR")
TIE_PERIOD = 29


def _planted(rng, n):
    """Random ACGT in which no A-run and no T-run is longer than RUN_CAP (every ninth symbol, and symbol 0, is C or G -- cyclically
    too), then ONE A-run of RUN_WIN and ONE T-run of RUN_LOSE symbols, each between a C and a G.  The 16-symbol key that starts
    at the A-run is the forward strand's only minimal key, the one at the T-run's mirror the reverse strand's, and the forward
    strand's is the smaller: a unique minimal window on a known strand, no tie on either strand.  Returns (array, run starts)."""
    assert n >= 400
    s = _ACGT[rng.integers(0, 4, size=n)].copy()
    s[8::9] = _CG[rng.integers(0, 2, size=len(s[8::9]))]
    s[0] = _CG[rng.integers(0, 2)]
    p = int(rng.integers(1, n // 2 - RUN_WIN - 2))
    q = int(rng.integers(n // 2 + 1, n - RUN_LOSE - 2))
    for at, run, ch in ((p, RUN_WIN, ord("A")), (q, RUN_LOSE, ord("T"))):
        s[at - 1], s[at + run] = ord("C"), ord("G")
        s[at:at + run] = ch
    return s, (p, q)


def _far(x, n, runs):
    """x is at least KEEP_OFF symbols (cyclically) from the first and from the last symbol of both planted runs, and in neither"""
    return all(min((x - at) % n, (at + run - 1 - x) % n) >= KEEP_OFF for at, run in zip(runs, (RUN_WIN, RUN_LOSE)))


def _away(rng, n, runs, count):
    """`count` different positions 2 .. n - 3, each with its two neighbours far (_far) from both planted runs"""
    out = []
    while len(out) < count:
        x = int(rng.integers(2, n - 2))
        if x not in out and all(_far(y, n, runs) for y in (x - 1, x, x + 1)):
            out.append(x)
    return out


def make(cls, n, seed):
    """One record of `n` symbols of class `cls` (content drawn from `seed`):
      pure      ACGT, unique minimal window on the forward strand (_planted): need_dw_strand2 admits it, team_takes in teams
      pure_rc   its reverse complement: the reverse strand wins (the deferred reverse-strand winner, the index from fpos)
      tie       a tandem repeat of period 29 (whole units, then GC.. up to n; no minimal window reaches the seam): the minimal key has ~n / 29 owners on either strand, more than
                TEAM_MAX_OWNERS -- the team refuses it, one wave needs the candidate bitmask (need_dw<2>; else "moves on")
      few_n     pure + five N, all >= 64 symbols from both planted runs: the N-mask rule accepts it (need_dw_2n, team_takes_2n)
      few_n_rc  its reverse complement
      gap       pure + one '-' (>= 64 symbols from the runs) between two C: the N-mask build refuses it, the 4-bit mode takes it
                (need_dw<4> for one wave, need_dw_strand4 for the 4-bit team); '-' sorts below A, the window at the gap wins
      byte      pure + one 'R', outside the 4-bit alphabet: byte mode (need_dw<8>), wave 0 alone"""
    rng = np.random.default_rng([seed, n, CLASSES.index(cls)])
    if cls == "tie":
        # AAAAAAC, sixteen C / G, TTTTT, G: both strands' minimal 16-symbol windows (at the A-run; mirrored, at the T-run) lie inside a unit
        unit = b"AAAAAAC" + bytes(_CG[rng.integers(0, 2, size=TIE_PERIOD - 13)]) + b"TTTTTG"
        return unit * (n // TIE_PERIOD) + (b"GC" * TIE_PERIOD)[:n % TIE_PERIOD]
    s, runs = _planted(rng, n)
    if cls in ("few_n", "few_n_rc"):
        s[_away(rng, n, runs, 5)] = ord("N")
    elif cls == "gap":
        g = _away(rng, n, runs, 1)[0]
        s[g - 1], s[g], s[g + 1] = ord("C"), ord("-"), ord("C")    # forward: -C..., reverse: -G...: the forward strand wins
    elif cls == "byte":
        s[_away(rng, n, runs, 1)[0]] = ord("R")
    b = s.tobytes()
    return b.translate(_COMP)[::-1] if cls.endswith("_rc") else b


def _runs(a, ch):
    """cyclic runs of byte `ch` in array a: (lengths, starts), longest first"""
    m = a == ch
    if m.all():
        return np.array([len(a)]), np.array([0])
    k = int(np.argmin(m))                               # rotate so that position 0 is not in a run
    r = np.roll(m, -k)
    d = np.diff(np.concatenate(([0], r.astype(np.int8), [0])))
    st, en = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    ln = en - st
    o = np.argsort(-ln, kind="stable")
    return ln[o], (st[o] + k) % len(a)


def key_owners(b):
    """(owners of the minimal 16-symbol key on the forward strand, on the reverse strand) of an ACGT record"""
    out = []
    for s in (b, b.translate(_COMP)[::-1]):
        code = np.frombuffer(s.translate(bytes.maketrans(b"ACGT", b"\x00\x01\x02\x03")), dtype=np.uint8).astype(np.uint64)
        ext = np.concatenate((code, code[:16]))
        key = np.zeros(len(code), dtype=np.uint64)
        for k in range(16):
            key = (key << np.uint64(2)) | ext[k:k + len(code)]
        out.append(int((key == key.min()).sum()))
    return tuple(out)


def check_class(cls, b):
    """The class's construction, proved from the record alone (AssertionError otherwise): what the admission arithmetic may rely on."""
    a = np.frombuffer(b, dtype=np.uint8)
    n = len(a)
    others = sorted(set(b) - set(b"ACGT"))
    if cls == "tie":
        assert not others
        of, orc = key_owners(b)
        assert of > TEAM_MAX_OWNERS and orc > TEAM_MAX_OWNERS, (of, orc)
        return
    want = {"pure": [], "pure_rc": [], "few_n": [ord("N")], "few_n_rc": [ord("N")], "gap": [ord("-")], "byte": [ord("R")]}[cls]
    assert others == want, (cls, others)
    win, lose = (ord("T"), ord("A")) if cls.endswith("_rc") else (ord("A"), ord("T"))
    lw, sw = _runs(a, win)
    ll, sl = _runs(a, lose)
    # one run of RUN_WIN and nothing else beyond RUN_CAP on the winning strand; one of RUN_LOSE on the other: unique minimal
    # 16-symbol keys on both strands (a run of <= 16 owns one key), the winner's strictly smaller
    assert lw[0] == RUN_WIN and lw[1] <= RUN_CAP and ll[0] == RUN_LOSE and ll[1] <= RUN_CAP, (cls, lw[:2], ll[:2])
    for x in np.nonzero(~np.isin(a, _ACGT))[0]:
        for at, run in ((int(sw[0]), RUN_WIN), (int(sl[0]), RUN_LOSE)):
            assert min((int(x) - at) % n, (at + run - 1 - int(x)) % n) >= KEEP_OFF, (cls, int(x), at)
    if cls in ("few_n", "few_n_rc"):
        assert int((a == ord("N")).sum()) == 5
    if cls == "gap":
        g = int(np.nonzero(a == ord("-"))[0][0])
        assert (a == ord("-")).sum() == 1 and 0 < g < n - 1 and b[g - 1:g + 2] == b"C-C"


# ---- the boundary table -------------------------------------------------------------------------------------------------------
# stage: A / C (canon_kernel<4> at 1280 / 2495 dwords per wave), T (canon_team_kernel, 16 x 2511), mixed / mixed_n (the mixed-length
# kernel's pure / N build); route: wave (one wave, its slice), team (the workgroup's waves, all slices), solo (wave 0 alone, all
# slices); cls: the record class; pred: the governing predicate; t4: None = every build, True = only canon_kernel<4, true> (busy
# tiers), False = only canon_kernel<4, false> (idle tiers); nxt: who takes the record of n_max + 1.
Triple = namedtuple("Triple", "stage route cls pred t4 nxt")
TRIPLES = [
    Triple("A", "wave", "pure", "strand2", None, "stage A's team"),
    Triple("A", "wave", "pure_rc", "strand2", None, "stage A's team"),
    Triple("A", "wave", "tie", "need2", None, "stage A, wave 0 alone"),
    Triple("A", "wave", "few_n", "2n", None, "stage A's N-mask team"),
    Triple("A", "wave", "few_n_rc", "2n", None, "stage A's N-mask team"),
    Triple("A", "wave", "gap", "need4", None, "stage A's 4-bit team, or wave 0 alone"),
    Triple("A", "wave", "byte", "need8", None, "stage A, wave 0 alone"),
    Triple("A", "team", "pure", "strand2", None, "stage C's team"),
    Triple("A", "team", "pure_rc", "strand2", None, "stage C's team"),
    Triple("A", "team", "few_n", "2n", None, "stage C's N-mask team"),
    Triple("A", "team", "few_n_rc", "2n", None, "stage C's N-mask team"),
    Triple("A", "team", "gap", "strand4", True, "stage C's 4-bit team"),
    Triple("A", "solo", "tie", "need2", None, "stage C, wave 0 alone"),
    Triple("A", "solo", "gap", "need4", False, "stage C, wave 0 alone"),
    Triple("A", "solo", "byte", "need8", None, "stage C, wave 0 alone"),
    Triple("C", "team", "pure", "strand2", None, "the team stage"),
    Triple("C", "team", "pure_rc", "strand2", None, "the team stage"),
    Triple("C", "team", "few_n", "2n", None, "the team stage"),
    Triple("C", "team", "few_n_rc", "2n", None, "the team stage"),
    Triple("C", "team", "gap", "strand4", True, "the team stage's 4-bit team"),
    Triple("C", "solo", "tie", "need2", None, "the team stage, wave 0 alone"),
    Triple("C", "solo", "gap", "need4", False, "the team stage's 4-bit team"),
    Triple("C", "solo", "byte", "need8", None, "the team stage, wave 0 alone"),
    Triple("T", "team", "pure", "strand2", None, "the global scratch"),
    Triple("T", "team", "few_n", "2n", None, "the global scratch"),
    Triple("T", "team", "gap", "strand4", None, "the global scratch"),
    Triple("T", "solo", "tie", "need2", None, "the global scratch"),
    Triple("T", "solo", "byte", "need8", None, "the global scratch"),
    Triple("mixed", "wave", "pure", "lean", None, "stage A, one wave"),
    Triple("mixed", "wave", "pure_rc", "lean", None, "stage A, one wave"),
    Triple("mixed_n", "wave", "few_n", "lean_n", None, "stage A's N-mask team"),
    Triple("mixed_n", "wave", "few_n_rc", "lean_n", None, "stage A's N-mask team"),
    Triple("mixed_n", "wave", "pure", "lean_n", None, "stage A, one wave"),
]
# (stage, route, class, predicate): why no record ever meets this boundary
UNREACHABLE = [
    ("A", "solo", "pure", "strand2", "the team takes every pure record wave 0 alone could hold (same four slices)"),
    ("A", "solo", "few_n", "2n", "the N-mask team takes every such record wave 0 alone could hold"),
    ("A", "team", "tie", "strand2", "the team builds it and refuses it (more than TEAM_MAX_OWNERS owners): wave 0 alone decides, by need_dw<2>"),
    ("C", "wave", "pure", "strand2", "stage A's team has taken pure records up to four stage-A slices, more than one stage-C slice"),
    ("C", "wave", "tie", "need2", "stage A's wave 0 alone has taken ties up to four stage-A slices with the bitmask"),
    ("C", "wave", "few_n", "2n", "stage A's N-mask team has taken them up to four stage-A slices"),
    ("C", "wave", "gap", "need4", "stage A's 4-bit team (strand alone) or wave 0 alone (four slices) has taken more"),
    ("C", "wave", "byte", "need8", "stage A's wave 0 alone has taken byte records up to four stage-A slices"),
    ("C", "solo", "pure", "strand2", "stage C's team takes them"),
    ("C", "solo", "few_n", "2n", "stage C's N-mask team takes them"),
    ("T", "solo", "pure", "strand2", "the sixteen-wave team takes them"),
    ("T", "solo", "few_n", "2n", "the sixteen-wave N-mask team takes them"),
    ("T", "solo", "gap", "need4", "the team stage's 4-bit team (no idle build there) takes more than wave 0 alone could"),
    ("mixed", "wave", "tie", "lean", "admitted by the same predicate as pure, then refused on the tie: nothing new at the boundary"),
    ("mixed", "wave", "few_n", "lean", "a batch with N runs the N build; a stray N in the pure build is refused before admission matters"),
]


def triple_cap(t):
    if t.stage == "mixed":
        return CK_TIER_A
    if t.stage == "mixed_n":
        return CK_MIXED_N_SLICE
    return stage_cap(t.stage, t.route)


def triple_n_max(t):
    return n_max(t.pred, triple_cap(t))


def triples_of(stage):
    return [t for t in TRIPLES if t.stage == stage]


# launch_single: the host picks the smallest one-wave slice with worst_case_dw(n) <= TIER_DW[t]; the single launch ends where
# need_dw_strand2(n) > TIER_DW[0] (the batch pipeline takes over)
def single_switches():
    """n_max of launch_single's first four tiers (the fifth holds everything up to the hand-over) and the hand-over length"""
    return [n_max("worst", cap) for cap in TIER_DW[:4]], n_max("strand2", TIER_DW[0])


SINGLE_CLASSES = ("pure", "pure_rc", "tie", "few_n", "gap", "byte")


# ---- batches ------------------------------------------------------------------------------------------------------------------
def short_four(seed):
    """four tier-bound records of 2.1 .. 3 kb, two pure and two with N, which need the workgroup's decode tables after a run"""
    rng = np.random.default_rng([seed, 77])
    return [make(("pure", "few_n", "pure_rc", "few_n_rc")[k], int(rng.integers(2100, 3001)), seed + k) for k in range(4)]


def run_of(cls, n, seed, width=4):
    """`width` consecutive records of one length and class, different content (the tier loops deal entries wib, wib + wpb, ...:
    the waves of a workgroup hold them at the same time)"""
    return [make(cls, n, seed + k) for k in range(width)]


_BATCHES = {}


def stage_batch(stage, order="as_built", t4=None):
    """The boundary batch of a stage: for every reachable triple and every probe length a run of records (four; one in the team
    stage, whose workgroup holds one record at a time), each run followed by short_four().  `reversed`: the runs in reverse order.
    Every record is longer than 2032 symbols: the batch's mode is 3 whatever the outputs.  Returns (records, tags) with tags[i] =
    (triple index in TRIPLES or -1, length) of record i."""
    key = (stage, t4)
    if key not in _BATCHES:
        runs = []
        for ti, t in enumerate(TRIPLES):
            if t.stage != stage or (t4 is not None and t.t4 is not None and t.t4 != t4):
                continue
            for L in probes(triple_n_max(t)):
                seed = 1000 * ti + L % 997
                recs = run_of(t.cls, L, seed, 1 if stage == "T" else 4)
                runs.append(([(r, (ti, L)) for r in recs] + [(r, (-1, len(r))) for r in short_four(seed)]))
        _BATCHES[key] = runs
    runs = _BATCHES[key]
    flat = [x for run in (runs if order == "as_built" else runs[::-1]) for x in run]
    return [r for r, _ in flat], [tag for _, tag in flat]


ORDERS = ("as_built", "reversed")
