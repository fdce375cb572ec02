"""CPU-only: the array yardstick tests/cluster_np.py against the definition's restatement tests/cluster_ref.py, exactly, on every
input set of tests/cluster_sets.py: every key, every offset and every pair, the forced-NO_KEY cases and the all-EMPTY rows
among them."""
import numpy as np
import pytest

from tests import cluster_np as N
from tests import cluster_ref as C
from tests import cluster_sets as S
from tests import sketch_ref as R
from tests import uniq_keys as K

NAMES = list(S.candidate_cases()) + ["past_the_emit_grid"]


def _case(name):
    return S.past_the_emit_grid() if name == "past_the_emit_grid" else S.candidate_cases()[name]


def test_fmix64_is_the_finalizer():
    rng = np.random.default_rng(5)
    h = np.concatenate([rng.integers(0, 1 << 64, size=2000, dtype=np.uint64), np.array([0, 1, 2 ** 63, 2 ** 64 - 1, 2 ** 33 - 1], dtype=np.uint64)])
    assert N.fmix64(h).tolist() == [R.fmix64(int(v)) for v in h]


@pytest.mark.parametrize("name", NAMES)
def test_candidates_equal_the_definition(name):
    rows, nb, bb = _case(name)
    exp_off, exp_pairs = S.expected_candidates(name)
    off, pairs = N.candidates(rows, nb, bb)
    assert off.dtype == np.uint64 and pairs.dtype == np.uint32 and pairs.shape == (len(exp_pairs), 2)
    assert np.array_equal(off, exp_off), name
    assert np.array_equal(pairs, exp_pairs), name


@pytest.mark.parametrize("name", [n for n in NAMES if n != "past_the_emit_grid"])
def test_band_keys_equal_the_definition(name):
    rows, nb, bb = _case(name)
    keys = N.band_keys(rows, nb, bb)
    assert keys.shape == (len(rows), nb) and keys.dtype == np.uint64
    for i, row in enumerate(rows):
        exp = [C.band_key([int(v) for v in row], b, bb) for b in range(nb)]
        assert keys[i].tolist() == [C.NO_KEY if k is None else k for k in exp], (name, i)


def test_the_shortcut_loses_no_shared_key():
    """maybe_shared keeps every position whose key another position holds, also where many keys differ in their low bits alone
    (which it cannot tell apart) and where the key is ~0; the first holder over its positions is the first holder over all."""
    rng = np.random.default_rng(6)
    pool = np.concatenate([rng.integers(0, 1 << 64, size=3000, dtype=np.uint64), (np.uint64(77) << np.uint64(40)) + np.arange(500, dtype=np.uint64),
                           np.array([2 ** 64 - 1, 0], dtype=np.uint64)])
    for n in (0, 1, 2, 5000, 70_000):
        flat = pool[rng.integers(0, len(pool), size=n)] if n > 1 else pool[:n]
        at = N.maybe_shared(flat)
        assert at.dtype == np.int64 and (np.diff(at) > 0).all()
        exp = K.expected_first_seen(flat)
        shared = np.flatnonzero(np.bincount(exp, minlength=n)[exp] > 1) if n else np.zeros(0, dtype=np.int64)
        assert np.isin(shared, at).all(), n
        assert np.array_equal(at[K.expected_first_seen(flat[at])], exp[at]), n
    flat = rng.integers(0, 1 << 64, size=5000, dtype=np.uint64)
    assert len(N.maybe_shared(flat)) == 0


def test_the_cases_hold_what_they_are_for():
    """The comparison above covers a forced NO_KEY, an all-EMPTY row and a record with several representatives."""
    rows, nb, bb = S.candidate_cases()["no_key_1bin"]
    keys = N.band_keys(rows, nb, bb)
    assert keys[0, 1] == keys[1, 1] == N.NO_KEY and not (rows[:2, 1] == N.EMPTY).any()
    rows, nb, bb = S.candidate_cases()["all_empty_rows"]
    assert (N.band_keys(rows, nb, bb)[[0, 3, 4, 8]] == N.NO_KEY).all()
    off, pairs = N.candidates(*S.candidate_cases()["several_earlier"])
    assert pairs[int(off[5]):int(off[6])].tolist() == [[2, 5], [0, 5], [4, 5]]
