"""The streaming launch's geometry, restated in Python from the constants in the sources (the yardstick of
tests/test_gpu_parity.py's batches at the geometry edges and of tests/test_emu_kernel.py's check of batch_geometry itself).

batch_geometry (canon_config.h), which launch_canon (circkit_canon.hip) calls, cuts a batch of n records into G workgroups of
the streaming kernel (per_step records per
iteration: StreamC::GROUP = CK_STREAM_WPB * CK_STREAM_RPW, or StreamCAux::GROUP = WPB * RPW of StreamCfg<4, 4, 2, 1> when
index / strand are wanted), G = max(min(ceil(n / per_step), N_CU * CK_FAST_BPC), min(n, N_CU * 16)); the stages that walk
all records take all_cap = ceil(n / G) per segment, and when G >= 4096 and all_cap >= 2 << CK_TAPER_GENS the last
CK_TAPER_GENS generations of G / CK_TAPER_DIV segments taper off (canon_core.h seg_records) with all_cap raised until they
still hold n.  With the constants of this writing (16, 1, 4 * 2 = 8, 256, 128, 3, 16):
  G leaves its floor of 4096       n = 65 537 (bytes / + XXH3 / hash only)      n = 32 769 (+ index / strand)
  taper starts (all_cap 15 -> 16,  n = 61 441: 4096 segments, all_cap 18      n = 491 521: 32 768 segments, all_cap 18
  raised by the taper to 18)
  grid capped at 32 768 (one       n = 524 273 (524 288 = 32 768 * 16: every    n = 262 137
  workgroup walks several groups)  workgroup exactly one group)
geometry() below restates that arithmetic from the constants in the sources, and test_gpu_parity asserts the counts still sit
on both sides of each edge: a change of those constants fails there and points back at this list."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "circkit_amd", "csrc")
GEOMETRY_COUNTS = [32_768, 32_769, 61_440, 61_441, 61_442, 65_536, 65_537, 262_136, 262_137, 262_138, 491_520, 491_521, 491_522,
                   524_272, 524_273, 524_288, 524_289, 1_000_003]


def source_constants():
    hip = open(os.path.join(CSRC, "canon_config.h")).read() + open(os.path.join(CSRC, "canon_core.h")).read()
    c = {}
    for k in ("CK_STREAM_WPB", "CK_STREAM_RPW", "CK_FAST_BPC", "CK_TAPER_GENS", "CK_TAPER_DIV"):
        m = re.findall(r"#define %s (\d+)" % k, hip)
        assert len(m) == 1, (k, m)
        c[k] = int(m[0])
    m = re.findall(r"constexpr int N_CU = (\d+);", hip)
    assert len(m) == 1, m
    c["N_CU"] = int(m[0])
    m = re.findall(r"using StreamCAux = ck::StreamCfg<(\d+), (\d+), (\d+), (\d+)>;", hip)
    assert len(m) == 1, m
    wpb, _, rpw, _ = map(int, m[0])
    c["AUX_GROUP"] = wpb * rpw
    return c


def geometry(n, aux, c):
    """(G, all_cap, tapered) of launch_canon for a batch of n records."""
    per_step = c["AUX_GROUP"] if aux else c["CK_STREAM_WPB"] * c["CK_STREAM_RPW"]
    G = max(min(-(-n // per_step), c["N_CU"] * c["CK_FAST_BPC"]), min(n, c["N_CU"] * 16))
    all_cap, gens = -(-n // G), c["CK_TAPER_GENS"]
    if not (G >= 4096 and all_cap >= 2 << gens):
        return G, all_cap, False
    log2 = 0
    while (2 << log2) <= G // c["CK_TAPER_DIV"]:
        log2 += 1
    seg0 = G - gens * (1 << log2)
    while seg0 * all_cap + (1 << log2) * sum(all_cap >> j for j in range(1, gens + 1)) < n:
        all_cap += 1
    return G, all_cap, True
