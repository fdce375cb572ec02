"""CPU-only: the route every set of tests/cluster_route_sets.py takes through circkit_uniq_resolve_device, established from the
yardstick's keys -- conditions, not measurements -- and the constants the sets are built on, held against circkit_uniq.hip.
beyond_buckets (21 M keys) is only checked for its sizes here: the GPU test pays for its keys."""
import numpy as np
import pytest

from tests import cluster_np as N
from tests import cluster_route_sets as RS
from tests import uniq_keys as K

SMALL = [name for name in RS.SETS if name != "beyond_buckets"]


def test_the_constants_are_the_source_s():
    c = RS.source_constants()
    assert (c["BKT_MAX"], c["BKT_KEYS"]) == (K.BKT_MAX, K.BKT_KEYS) == (3072, 2600)
    assert c["BKT_MAX_LOG2"] == RS.BKT_MAX_LOG2 == 13 and c["CK_UNIQ_BUCKET_MIN"] == RS.BUCKET_MIN == 1 << 19
    assert RS.BUCKET_LIMIT == c["BKT_KEYS"] << c["BKT_MAX_LOG2"] == 21_299_200
    # bucket_log2 is the sizing rule as the issue of every bucketed test states it: the smallest 2^log2b in 64 .. 8192 buckets
    assert K.bucket_log2(1 << 19) == 8 and K.bucket_log2(RS.BUCKET_LIMIT) == 13
    assert K.bkt_of(np.array([0, 2 ** 56 - 1, 2 ** 56, 2 ** 64 - 1], dtype=np.uint64), 8).tolist() == [0, 0, 1, 255]


def test_the_key_counts_sit_on_their_side_of_the_thresholds():
    expect = {"direct_last": (1 << 19) - 64, "lds_first": 1 << 19, "lds_63": 524_349, "lds_5x3": 524_290, "no_key_flood": 1 << 19,
              "identical": 1 << 19, "beyond_buckets": 21_299_264}
    assert {name: RS.n_keys(name) for name in RS.SETS} == expect
    assert RS.n_keys("direct_last") < RS.BUCKET_MIN
    for name in RS.LDS + RS.FALLBACK:
        assert RS.BUCKET_MIN <= RS.n_keys(name) <= RS.BUCKET_LIMIT, name
    assert RS.n_keys("beyond_buckets") > RS.BUCKET_LIMIT and RS.n_keys("beyond_buckets") - 64 <= RS.BUCKET_LIMIT      # the smallest at 64 bands
    assert RS.n_keys("beyond_buckets") < 2 ** 32 - 1
    for name, (n, nb, bb, bins, _) in RS.SETS.items():
        assert nb * bb <= bins and bins in (16, 64), name
    assert [RS.SETS[name][1] for name in ("lds_63", "lds_5x3")] == [63, 5]                # divisions that no shift does


@pytest.mark.parametrize("name", SMALL)
def test_the_rows_are_what_the_set_says(name):
    rows, nb, bb = RS.rows_of(name)
    n, _, _, bins, _ = RS.SETS[name]
    assert rows.shape == (n, bins) and rows.dtype == np.uint64 and RS.keys_of(name).size == RS.n_keys(name)
    empty = rows == RS.EMPTY
    if name == "no_key_flood":
        assert 0.045 < empty.mean() < 0.055
        flood = int((RS.keys_of(name) == RS.EMPTY).sum())
        assert flood > 8 * K.BKT_MAX, flood                                               # all of them in the last bucket
    else:
        assert not empty.any() and not (RS.keys_of(name) == RS.EMPTY).any()


@pytest.mark.parametrize("name", RS.LDS)
def test_the_lds_sets_stay_in_lds_with_full_buckets(name):
    """No bucket above BKT_MAX rows, so no fallback; and the fullest holds 1800 or more (about 2048 +- 45 are expected per bucket)."""
    most = RS.max_bucket(name)
    print("%s: max bucket %d" % (name, most))
    assert 1800 <= most <= K.BKT_MAX, (name, most)


@pytest.mark.parametrize("name", RS.FALLBACK)
def test_the_fallback_sets_overfill_a_bucket(name):
    most = RS.max_bucket(name)
    print("%s: max bucket %d" % (name, most))
    assert most > K.BKT_MAX, (name, most)


def test_the_direct_set_would_fit_its_buckets_too():
    """direct_last differs from lds_first by one record: what separates their routes is the threshold alone."""
    most = RS.max_bucket("direct_last")
    print("direct_last: max bucket %d" % most)
    assert most <= K.BKT_MAX


@pytest.mark.parametrize("name", [n for n in SMALL if n != "identical"])
def test_the_answer_exercises_the_emit(name):
    rows, nb, bb = RS.rows_of(name)
    n = len(rows)
    off, pairs = RS.expected(name)
    off = off.astype(np.int64)
    assert len(off) == n + 1 and off[-1] == len(pairs) and (np.diff(off) >= 0).all()
    per_record = len(pairs) / n
    print("%s: %d pairs, %.3f per record" % (name, len(pairs), per_record))
    assert 0 < per_record < 4, (name, per_record)
    assert (pairs[:, 0] < pairs[:, 1]).all()
    bands = N.candidates(rows, nb, bb, keys=RS.keys_of(name), with_bands=True)[2]
    assert (bands == 0).any() and (bands == nb - 1).any() and (bands == nb // 2).any(), name        # the first, the last, a middle band propose
    counts = np.diff(off)
    two = np.flatnonzero(counts >= 2)
    assert len(two) and all(pairs[off[i], 0] != pairs[off[i] + 1, 0] for i in two[:100]), name      # two different earlier records
    assert counts[-1] >= 1, name                                                                       # the last record proposes
    if name != "no_key_flood":
        assert pairs[off[n - 1]:off[n], 0].size == 2                                                   # from band 0 and from the last band


def test_identical_is_closed_form():
    """64 keys of 8192 rows each: record i > 0 has exactly the pair (0, i)."""
    n = RS.SETS["identical"][0]
    keys = RS.keys_of("identical")
    assert len(np.unique(keys)) == 64 and (keys == keys[0]).all()
    off, pairs = RS.expected("identical")
    assert np.array_equal(off, np.r_[0, 0, np.arange(1, n)].astype(np.uint64))
    assert np.array_equal(pairs, np.stack([np.zeros(n - 1, dtype=np.uint32), np.arange(1, n, dtype=np.uint32)], axis=1))
