"""The offsets walk of the host-buffer entry points (circkit_amd/csrc/ck_csr.h) under AddressSanitizer and UBSan: a
stand-alone driver (tests/san/csr_san_main.cpp) walks each offsets array in a heap block of exactly its size, and every verdict
is compared with a plain loop.  The walk has no HIP in it, so this is a CPU build."""
import os
import random
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = os.path.join(HERE, "san")
BIN = os.path.join(SAN, "csr_san")

OK, DECREASE, TOO_LONG = 0, 1, 2
NO_LIMIT = 0
NONE = (1 << 64) - 1             # the index the driver starts from: the walk leaves it alone without a fault


@pytest.fixture(scope="module")
def csr_san():
    srcs = [os.path.join(SAN, "csr_san_main.cpp")]
    deps = srcs + [os.path.join(ROOT, "circkit_amd", "csrc", "ck_csr.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", "-o", BIN] + srcs)
    return BIN


def walk(offsets, limit):
    """the yardstick: what every unit's own loop did, decrease before length at the same record"""
    for i in range(len(offsets) - 1):
        if offsets[i + 1] < offsets[i]:
            return DECREASE, i
        if limit != NO_LIMIT and offsets[i + 1] - offsets[i] >= limit:
            return TOO_LONG, i
    return OK, NONE


def cases():
    out = []
    L31, L32, top = 1 << 31, 1 << 32, (1 << 64) - 1
    for limit in (NO_LIMIT, L31, L32):
        out.append((limit, [0]))                                   # n = 0
        out.append((limit, [7]))                                   # n = 0 with a first offset that is not 0: the unit's own line
        out.append((limit, [0, 0]))                                # one empty record
        out.append((limit, [0, 5, 5, 9]))
        out.append((limit, [3, 2, 6, 9]))                          # a decrease at 0
        out.append((limit, [0, 4, 2, 6]))                          # in the middle
        out.append((limit, [0, 4, 6, 5]))                          # at n - 1
        out.append((limit, [0, 4, 2, 1]))                          # two decreases: the first
        for lim in (L31, L32):                                     # one below the limit and at it, first, middle and last
            for at in range(3):
                for length in (lim - 1, lim, lim + 1):
                    offs = [0]
                    for i in range(3):
                        offs.append(offs[-1] + (length if i == at else 3))
                    out.append((limit, offs))
        out.append((limit, [0, L32, L32 - 1, L32 + 5]))            # too long at 0, a decrease at 1: the lower index
        out.append((limit, [0, 4, 2, 2 + L32]))                    # a decrease at 1, too long at 2: the lower index
        out.append((limit, [5, 4]))                                # both at the same record: the difference wraps to 2^64 - 1
        out.append((limit, [0, L32 + 7, 3, 9]))                    # both at record 1 (it wraps too): the decrease
        out.append((limit, [0, top - 2, top - 1, top]))            # just under 2^64
        out.append((limit, [top - 2, top - 1, top, top]))
        out.append((limit, [top - 2, top, top - 1]))
        out.append((limit, [top - L31 + 1, top]))                  # a length of exactly 2^31 - 1 that ends at the top
        out.append((limit, [top - L31, top]))                      # and of exactly 2^31
        out.append((limit, [top - L32 + 1, top]))
        out.append((limit, [top - L32, top]))
        out.append((limit, [0, top]))
    out.append((1, [0, 0]))                                        # the smallest limit: an empty record reaches it
    out.append((2, [0, 1, 3]))
    rng = random.Random(11)
    for _ in range(300):
        n = rng.randint(0, 12)
        limit = rng.choice([NO_LIMIT, 1, 5, L31, L32])
        offs = [rng.choice([0, 0, 0, 9])]
        for _ in range(n):
            step = rng.choice([0, 1, 4, 5, 6, L31 - 1, L31, L32 - 1, L32, -1, -3])
            offs.append(max(0, offs[-1] + step))
        out.append((limit, offs))
    return out


def test_walk_under_asan_and_ubsan(csr_san, tmp_path):
    cs = cases()
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cs)))
        for limit, offs in cs:
            f.write(struct.pack("<QQ%dQ" % len(offs), limit, len(offs) - 1, *offs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([csr_san, str(path)], capture_output=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode(errors="replace")[-4000:]
    assert len(r.stdout) == 12 * len(cs)
    seen = set()
    for k, (limit, offs) in enumerate(cs):
        got = struct.unpack_from("<IQ", r.stdout, 12 * k)
        assert got == walk(offs, limit), (limit, offs, got)
        seen.add(got[0])
    assert seen == {OK, DECREASE, TOO_LONG}


def test_the_yardstick_itself():
    """the plain loop on the cases whose answer can be read off"""
    L31 = 1 << 31
    assert walk([0], L31) == (OK, NONE)
    assert walk([0, 0], L31) == (OK, NONE)
    assert walk([0, 4, 2, 6], L31) == (DECREASE, 1)
    assert walk([0, L31 - 1], L31) == (OK, NONE)
    assert walk([0, L31], L31) == (TOO_LONG, 0)
    assert walk([0, L31], NO_LIMIT) == (OK, NONE)
    assert walk([0, 1 << 32, 5], L31) == (TOO_LONG, 0)
    assert walk([0, 4, 2, 2 + L31], L31) == (DECREASE, 1)
