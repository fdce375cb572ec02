"""The gfx950 device half of circkit_amd/csrc/wave_prims.h against the contract restated in tests/prims_ref.py, bit for bit: the op
table of tests/prims/prims_ops.h (tests/prims/prims_probe.hip, built by tests/prims_probe.py with the product's flags) on the
cases of tests/prims_sets.py -- the same op table and cases that tests/test_prims_cpu.py runs against the emulator's
implementation, which is what the kernels are proven against on the CPU.  Every case runs as a workgroup of 64, 256 and 1024
threads in which every wave runs the case, in both surroundings (plain / tight); every wave must give the contract's results
(wave_in_block: its own index), and the inputs, results and global memory lie between canaries."""
import pytest

from tests import prims_sets as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in S.FAMILIES.items()}


@pytest.mark.parametrize("threads", (64, 256, 1024))
@pytest.mark.parametrize("family", sorted(S.FAMILIES))
def test_device_keeps_the_contract(family, threads, cases):
    from tests import prims_probe
    cs = cases[family]
    for mode in (S.PLAIN, S.TIGHT):
        hdr, inputs, mems = S.pack(cs, mode)
        out, after = prims_probe.run(hdr, inputs, mems, threads, S.OUT_W, S.MEM_BYTES)
        assert out.shape[1] == threads // 64
        S.check(cs, mode, threads // 64, out, after)
