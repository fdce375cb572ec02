"""The emulator's implementation of every wave primitive (tests/emu/wave_prims_emu.h) against the contract restated in
tests/prims_ref.py, on the cases of tests/prims_sets.py -- the same op table (tests/prims/prims_ops.h) and the same cases that
tests/test_prims_gpu.py runs against the gfx950 device half of circkit_amd/csrc/wave_prims.h.  Also: the interface stays closed
(every primitive of either header is in the other, in the op table and in the yardstick), and the sets hold the edges they are for."""
import os
import re

import numpy as np
import pytest

from tests import prims_ref, prims_sets as S
from tests.emu import prims_emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circkit_amd", "csrc")


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in S.FAMILIES.items()}


@pytest.mark.parametrize("family", sorted(S.FAMILIES))
def test_emulator_keeps_the_contract(family, cases, tmp_path):
    cs = cases[family]
    assert 0 < len(cs) <= 600
    for nwaves, mode in ((1, S.PLAIN), (1, S.TIGHT), (4, S.TIGHT)):
        hdr, inputs, mems = S.pack(cs, mode)
        out, after = prims_emu.run(hdr, inputs, mems, nwaves, S.OUT_W, S.MEM_BYTES, tmp_path)
        S.check(cs, mode, nwaves, out, after)


# ------------------------------------------------------------------------------------------------
def _names(text):
    """the functions a header defines with CK_DEV (templates included)"""
    return set(re.findall(r"^CK_DEV\s+[\w:<>\s\*&]+?\b(\w+)\s*\(", text, flags=re.M))


def _device_half():
    text = open(os.path.join(CSRC, "wave_prims.h")).read()
    return text[text.index("#else"):text.index("#endif  // CK_WAVE_PRIMS_OVERRIDE")]


def test_the_interface_stays_closed():
    dev = _names(_device_half())
    emu = _names(open(os.path.join(ROOT, "tests", "emu", "wave_prims_emu.h")).read())
    assert len(dev) >= 60
    assert dev == emu, "only in the device half: %s; only in the emulator: %s" % (sorted(dev - emu), sorted(emu - dev))
    ops = open(os.path.join(ROOT, "tests", "prims", "prims_ops.h")).read()
    for name in sorted(dev):
        assert re.search(r"\bck::%s\b" % name, ops), "%s is not in the op table" % name
        assert callable(getattr(prims_ref, name, None)), "%s is not in the yardstick" % name
    # every operation of the op table is restated, and together they are there for every primitive
    assert set(S.OPS) == set(S.OP) == set(S.PRIMITIVES)
    assert {p for ps in S.PRIMITIVES.values() for p in ps} == dev
    # ... and every operation has cases
    used = {c.op for make in S.FAMILIES.values() for c in make()}
    assert used == set(S.OP), sorted(set(S.OP) - used)


def test_the_op_table_has_no_intrinsics_and_no_build_switch():
    ops = open(os.path.join(ROOT, "tests", "prims", "prims_ops.h")).read()
    code = re.sub(r"//[^\n]*", "", ops)
    for word in ("__builtin", "asm", "#if", "threadIdx", "blockIdx", "__shared__", "hip"):
        assert word not in code, word


def test_no_kernel_uses_a_perm_selector_outside_the_contract():
    """the emulator does not model v_perm_b32's selectors 8..11 (sign replication): no perm( call in csrc/ has a literal selector
    byte among them"""
    calls = 0
    for f in sorted(os.listdir(CSRC)):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
        for m in re.finditer(r"\bperm\s*\(", text):
            depth, k = 1, m.end()
            while depth:
                depth += {"(": 1, ")": -1}.get(text[k], 0)
                k += 1
            call = text[m.end():k - 1]
            calls += 1
            for lit in re.findall(r"\b0[xX][0-9a-fA-F]+\b|\b\d+\b", call.rsplit(",", 1)[-1]):
                v = int(lit.rstrip("uU"), 0)
                if v > 0xFF:                                # a whole selector (smaller literals are shifts and the like)
                    assert not any(8 <= (v >> s) & 0xFF <= 11 for s in (0, 8, 16, 24)), (f, call)
    assert calls > 10
    for c in S.words():
        if c.op == "PERM":
            sel = c.inp[:, 2]
            assert not any(((8 <= ((sel >> s) & 0xFF)) & (((sel >> s) & 0xFF) <= 11)).any() for s in (0, 8, 16, 24))


def test_sload_group_runs_at_every_group_of_the_stream_configurations():
    text = open(os.path.join(CSRC, "canon_config.h")).read()
    text = re.sub(r"//[^\n]*", "", text)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(CK_\w+)\s+(\d+)", text)}
    groups = set()
    for wpb, rpw in re.findall(r"ck::StreamCfg<\s*(\w+)\s*,\s*\w+\s*,\s*(\w+)\s*,\s*\w+\s*>", text):
        groups.add(int(defs.get(wpb, wpb)) * int(defs.get(rpw, rpw)))
    assert groups == set(S.SLOAD_GROUPS)


def _of(cs, op):
    return [c for c in cs if c.op == op]


def test_the_sets_hold_the_edges(cases):
    m = cases["minima"]
    for op in ("WAVE_MIN", "ROW_MIN16", "WAVE_MIN2", "HALF_MIN2", "HALF_MIN2_BCAST"):
        uniq = [c for c in _of(m, op) if (c.inp[:, 0] == c.inp[:, 0].min()).sum() == 1]
        assert {int(c.inp[:, 0].argmin()) for c in uniq} == set(range(64)), op
        assert any(c.inp[:, 0].min() >= 0x80000000 for c in uniq) and any(c.inp[:, 0].min() < 0x80000000 < c.inp[:, 0].max() for c in uniq)
        for a, b in ((15, 16), (31, 32), (47, 48)):
            assert any(c.inp[a, 0] == c.inp[b, 0] == c.inp[:, 0].min() and (c.inp[:, 0] == c.inp[:, 0].min()).sum() == 2 for c in _of(m, op)), (op, a)
        for v in (0, 0xFFFFFFFF):
            assert any((c.inp[:, 0] == v).all() for c in _of(m, op))
    for op in ("WAVE_MIN2", "HALF_MIN2", "HALF_MIN2_BCAST"):
        assert sum(c.inp[:, 0].argmin() // 16 != c.inp[:, 1].argmin() // 16 for c in _of(m, op)) >= 64
    s = cases["sums"]
    for op in ("ROWSUM4", "QUADSUM", "WAVE_SUM", "ADD64_PARTS", "MULHI64"):
        cs = _of(s, op)
        assert any((c.inp[:, 0] == 0xFFFFFFFF).all() for c in cs) and any((c.inp[:, 0] == 0).all() and c.inp[:, 1].any() for c in cs)
    assert any((c.inp[:, 0] == 0xFFFFFFFF).all() and (c.inp[:, 2] == 1).all() for c in _of(s, "ROWSUM4"))
    assert any((c.inp[:, 2] == 0xFFFFFFFF).all() and (c.inp[:, 0] == 1).all() for c in _of(s, "ROWSUM4"))
    lm = cases["lane_moves"]
    want = set(range(64)) | {64, 65, 127, 255, 256, 257, 0x40000000, 0xFFFFFFFF}
    uni = {int(c.inp[0, 1]) for c in _of(lm, "SHFL") if (c.inp[:, 1] == c.inp[0, 1]).all()}
    per = {int(v) for c in _of(lm, "SHFL") if not (c.inp[:, 1] == c.inp[0, 1]).all() for v in c.inp[:, 1]}
    assert want <= uni and want <= per
    assert {int(c.inp[0, 1]) for c in _of(lm, "READLANE")} == set(range(64))
    for op in ("BALLOT", "LANE_PRED"):
        masks = {int(prims_ref.ballot(c.inp[:, 0] & 1)[0]) if op == "BALLOT" else int(c.inp[0, 0]) | int(c.inp[0, 1]) << 32 for c in _of(lm, op)}
        assert {0, 2 ** 64 - 1, 0xFFFFFFFF, 0xFFFFFFFF << 32, 1, 1 << 63} <= masks, op
    w = cases["words"]
    assert {int(c.inp[0, 2]) for c in _of(w, "FUNNEL") if (c.inp[:, 2] == c.inp[0, 2]).all()} >= set(range(32))
    for op in ("ALIGNBIT", "LSHR64"):
        assert {int(c.inp[0, 2]) for c in _of(w, op) if (c.inp[:, 2] == c.inp[0, 2]).all()} >= set(range(64))
        assert any(len(set(c.inp[:, 2])) > 32 for c in _of(w, op))
    sel = {int((v >> s) & 0xFF) for c in _of(w, "PERM") for v in c.inp[:, 2] for s in (0, 8, 16, 24)}
    assert sel == set(S.PERM_ALLOWED)
    assert {int(c.inp[0, 0]) for c in _of(w, "LOW_MASK16")} >= {0, 1, 15, 16, 17, 2 ** 31, 2 ** 32 - 1}
    assert any(c.inp[0, 0] == 0 for c in _of(w, "FFS32_OR_NEG")) and any(((c.inp[:, 0] | c.inp[:, 1]) == 0).any() for c in _of(w, "FFS64_OR_NEG"))
    top = 255 * 255 * 4
    assert any((c.inp[:, 0] == 0xFFFFFFFF).all() and (c.inp[:, 2].astype(np.int64) + top >= 2 ** 32).any() and
               (c.inp[:, 2].astype(np.int64) + top < 2 ** 32).any() for c in _of(w, "UDOT4"))
    a = cases["access"]
    for op, wd in (("LOAD16", 16), ("LOAD4", 4), ("STORE16", 16), ("STORE8", 8), ("STORE4", 4)):
        assert {int(c.inp[0, 0]) % 16 for c in _of(a, op)} >= set(range(16))
        assert any(((c.inp[:, 0] < 4096) & (c.inp[:, 0] + wd > 4096)).any() for c in _of(a, op)), op
        for c in _of(a, op):                                # inside the memory, and no two lanes' bytes overlap
            o = np.sort(c.inp[:, 0].astype(np.int64))
            assert o[-1] + wd <= S.MEM_BYTES and (np.diff(o) >= wd).all()
    sl = cases["scalar_loads"]
    assert {int(c.inp[0, 0]) % 16 for c in _of(sl, "SLOAD_U64X2")} == {0, 8}
    assert {56, 4088} <= {int(c.inp[0, 0]) for c in _of(sl, "SLOAD_U64X2")}
    for g in S.SLOAD_GROUPS:
        cs = _of(sl, "SLOAD_GROUP_%d" % g)
        assert {int(c.inp[0, 1]) % 16 for c in cs} == {0, 8} and {int(c.inp[0, 0]) % 16 for c in cs} == {0, 8}
        assert any(c.inp[0, 0] < 4096 <= c.inp[0, 0] + 8 * g for c in cs) and any(c.inp[0, 1] < 4096 < c.inp[0, 1] + 24 for c in cs)
        assert any(c.inp[0, 1] // 64 != (c.inp[0, 1] + 23) // 64 for c in cs)
    for c in sl:                                            # distinct halves in every word that is loaded
        v = c.mem.view(np.uint64)
        assert ((v >> np.uint64(32)) != (v & np.uint64(0xFFFFFFFF))).all()
    d = cases["lds_dma"]
    for op in ("GLDS16", "GLDS16_S"):
        assert {int(c.inp[0, 0]) % 16 for c in _of(d, op)} >= set(range(16))
        assert len({int(c.inp[0, 1]) for c in _of(d, op)}) >= 5
