"""tests/fullcheck.py on CPU tensors (no GPU): the whole-batch checker passes the oracle's own output at a chunk size that
cuts records apart, and names the right record for every kind of planted error -- including a first-seen entry whose
duplicate lies in an earlier chunk, and a record past the 2^32 mark of the offsets."""
import re

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import fullcheck, seqsets

CHUNK = 3_001            # odd: chunk boundaries fall inside records


@pytest.fixture(scope="module")
def batch():
    seqs = seqsets.random_mixed(61, 120, 0, 700) + seqsets.random_mixed(62, 40, 1, 400, b"ACGTN") + [b"", b"ACGT" * 60, b"A" * 333]
    seqs += seqs[:30]                                    # exact duplicates in a later chunk: non-trivial first-seen
    seqs.append(seqsets.revcomp_acgt(seqs[5][7:] + seqs[5][:7]))
    data, offs = seqsets.pack(seqs)
    out, hs, idx, st = O.canonicalize_batch_aux(data, offs, True, True, True, True, threads=2)
    fs = O.uniq_first_seen(hs)
    assert int((fs != np.arange(len(seqs))).sum()) >= 31
    t = {"d_bytes": torch.from_numpy(data), "d_offsets": torch.from_numpy(offs.astype(np.int64)), "n": len(seqs),
         "out_bytes": torch.from_numpy(out.copy()), "out_xxh3": torch.from_numpy(hs.view(np.int64).copy()),
         "out_index": torch.from_numpy(idx.view(np.int32).copy()), "out_strand": torch.from_numpy(st.copy()),
         "first_seen": torch.from_numpy(fs.view(np.int64).copy())}
    return t, offs


def _run(t, **over):
    kw = dict(t)
    kw.update(over)
    return fullcheck.check_batch(O, kw.pop("d_bytes"), kw.pop("d_offsets"), kw.pop("n"), chunk_bytes=CHUNK, **kw)


def _chunk_of(offs, r):
    """Chunk number check_batch gives record r (the same walk, for the test's own bookkeeping)."""
    k, r0, n = 0, 0, len(offs) - 1
    while r0 < n:
        r1 = min(n, max(int(np.searchsorted(offs, offs[r0] + np.uint64(CHUNK), side="right")) - 1, r0 + 1))
        if r0 <= r < r1:
            return k
        k, r0 = k + 1, r1
    raise IndexError(r)


def test_passes_the_oracles_own_output(batch):
    t, offs = batch
    got = _run(t)
    assert got["records"] == t["n"] and got["chunks"] > 10 and got["end_offset"] == int(offs[-1])
    assert _run(t, out_xxh3=None, out_index=None, first_seen=None)["records"] == t["n"]      # any subset of the outputs
    assert _run(t, out_bytes=None, out_strand=None)["records"] == t["n"]


def _planted(t, name, pos, val=None):
    x = t[name].clone()
    x[pos] = (x[pos] ^ 1) if val is None else val
    return {name: x}


def _fails(t, over, what, rec, offs):
    with pytest.raises(AssertionError) as e:
        _run(t, **over)
    msg = str(e.value)
    assert msg.startswith(what + " differs at record %d " % rec), msg
    assert "length %d, byte offset %d " % (int(offs[rec + 1] - offs[rec]), int(offs[rec])) in msg, msg
    return msg


def test_wrong_byte_in_the_last_record(batch):
    t, offs = batch
    n = t["n"]
    msg = _fails(t, _planted(t, "out_bytes", int(offs[n]) - 1), "canonical bytes", n - 1, offs)
    assert re.search(r"first at byte %d of the record" % (int(offs[n] - offs[n - 1]) - 1), msg)


def test_wrong_byte_in_a_record_across_a_chunk_boundary(batch):
    t, offs = batch
    # the record whose bytes straddle the CHUNK mark of the payload: the walk moves it whole into the second chunk
    r = next(i for i in range(t["n"]) if int(offs[i]) < CHUNK < int(offs[i + 1]) - 1)
    assert _chunk_of(offs, r) == 1 and _chunk_of(offs, r - 1) == 0
    _fails(t, _planted(t, "out_bytes", CHUNK), "canonical bytes", r, offs)
    # ... and the last byte of the last record of some chunk that is not the first
    r = next(i for i in range(1, t["n"] - 1) if _chunk_of(offs, i) == 3 and _chunk_of(offs, i + 1) == 4 and offs[i + 1] > offs[i])
    _fails(t, _planted(t, "out_bytes", int(offs[r + 1]) - 1), "canonical bytes", r, offs)


def test_wrong_hash_index_strand(batch):
    t, offs = batch
    _fails(t, _planted(t, "out_xxh3", 77), "xxh3", 77, offs)
    _fails(t, _planted(t, "out_index", 101, int(t["out_index"][101]) + 1), "index", 101, offs)
    _fails(t, _planted(t, "out_strand", t["n"] - 2), "strand", t["n"] - 2, offs)


def test_wrong_first_seen_whose_duplicate_is_in_an_earlier_chunk(batch):
    t, offs = batch
    fs = t["first_seen"].numpy()
    r = next(i for i in range(t["n"] - 1, 0, -1) if fs[i] != i and _chunk_of(offs, int(fs[i])) < _chunk_of(offs, i))
    _fails(t, _planted(t, "first_seen", r, r), "first_seen", r, offs)          # as if its earlier duplicate had been missed


def test_wrong_input_against_the_host_generator():
    L, n, base = 100, 500, 7 * 10 ** 9
    data = O.synth_fill(42, base, n * L)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    out, _ = O.canonicalize_batch(data, offs, True, False, threads=2)
    gen = fullcheck.synth_input(O, 42, base, threads=3)
    d = torch.from_numpy(data.copy())
    fullcheck.check_batch(O, d, torch.from_numpy(offs.astype(np.int64)), n, out_bytes=torch.from_numpy(out), chunk_bytes=CHUNK, host_input=gen)
    d[431 * L + 5] = ord("N")
    with pytest.raises(AssertionError, match=r"input \(device bytes vs the host generator\) differs at record 431 .*byte 5 of"):
        fullcheck.check_batch(O, d, torch.from_numpy(offs.astype(np.int64)), n, chunk_bytes=CHUNK, host_input=gen)


def test_names_offsets_past_4_gib():
    """Offsets need not start at 0: a batch whose records sit past the 2^32 mark of a (virtual) buffer is reported with its
    64-bit offset.  numpy views stand in for the buffer."""
    class Shifted:
        """d[a:b] of a buffer whose first `base` bytes are not materialised."""
        def __init__(self, arr, base):
            self.arr, self.base = arr, base

        def __getitem__(self, s):
            return self.arr[s.start - self.base:s.stop - self.base]
    seqs = seqsets.random_mixed(63, 50, 100, 300)
    data, offs = seqsets.pack(seqs)
    base = (1 << 32) + 12345
    out, hs = O.canonicalize_batch(data, offs, True, True, threads=2)
    out[int(offs[40]) + 3] ^= 4
    with pytest.raises(AssertionError, match=r"canonical bytes differs at record 40 \(length %d, byte offset %d = 0x[0-9a-f]+, >= 2\^32\)"
                       % (int(offs[41] - offs[40]), base + int(offs[40]))):
        fullcheck.check_batch(O, Shifted(data, base), offs + np.uint64(base), len(seqs), out_bytes=Shifted(out, base), out_xxh3=hs, chunk_bytes=CHUNK)
