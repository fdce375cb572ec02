"""The shared scan (circkit_amd/csrc/ck_scan.h) on the CPU: the header compiled as fibers (tests/emu/scan_emu.py), one workgroup
of WG fibers per launch, for the (WG, ITEMS, Op) the units instantiate, against a sequential loop over Python integers.  What
runs here is the barrier placement of block_scan, the rounds of the second level and the bases of the last kernel: the code the
units' own fiber programs replace by a host loop.  Every case runs with the fibers as ascending and as descending threads
(E.run_both: between them the two orders expose each of block_scan's barriers), and everything is compared exactly."""
import random

import pytest

from tests.emu import scan_emu as E

M64 = E.M64
UNITS = [0, 1, 2, 3]                     # orfs, windows / translate, fasta_write, the compact


def values(rng, op, count, bits):
    """count random elements of op's type, each word below 2^bits."""
    if op is E.PAIR:
        return [(rng.getrandbits(1), rng.getrandbits(bits)) for _ in range(count)]
    if op is E.STATE:
        return [rng.choice((E.ST_PASS, E.ST_PASS, E.ST_HEADER, E.ST_SEQ)) for _ in range(count)]
    return [rng.getrandbits(bits) for _ in range(count)]


def words(rng, op, count, bits):
    """count random item words as they lie in device memory: for the compact WRITTEN | length, or 0."""
    if op is E.PAIR:
        return [(E.WRITTEN | rng.getrandbits(bits)) if rng.getrandbits(1) else 0 for _ in range(count)]
    return [rng.getrandbits(bits) for _ in range(count)]


@pytest.mark.parametrize("config", UNITS)
def test_block_scan(config, tmp_path):
    wg, _, op = E.CONFIGS[config]
    rng = random.Random(100 + config)
    bits = 64 if op is not E.SAT else 50          # the wrapping sums wrap; the saturating one has its own test
    rand = values(rng, op, wg, bits)
    rand[0] = rand[wg // 2 + 1] = rand[wg - 1] = op.identity
    ones = [(1, 1) if op is E.PAIR else 1] * wg
    got = E.run_both([(E.BLOCK_SCAN, config, rand, None), (E.BLOCK_SCAN, config, ones, None)], tmp_path)
    for vals, (before, totals) in zip((rand, ones), got):
        exp_before, exp_total = E.exclusive(op, vals)
        assert before == exp_before
        assert totals == [exp_total] * wg         # to every thread
    assert got[1][0] == ([(t, t) for t in range(wg)] if op is E.PAIR else list(range(wg)))


@pytest.mark.parametrize("config", UNITS)
def test_second_level_rounds(config, tmp_path):
    """The tile sums given directly, on both sides of a round and beyond two rounds."""
    wg, _, op = E.CONFIGS[config]
    rng = random.Random(200 + config)
    counts = [0, 1, wg - 1, wg, wg + 1, 2 * wg + 1]
    sums = [values(rng, op, n, 64 if op is not E.SAT else 48) for n in counts]
    got = E.run_both([(E.SUMS_EXCLUSIVE, config, s, None) for s in sums], tmp_path)
    for s, (excl, totals) in zip(sums, got):
        exp, exp_total = E.exclusive(op, s)
        assert excl == exp
        assert totals == [exp_total] * wg


@pytest.mark.parametrize("config", UNITS)
def test_tile_base(config, tmp_path):
    """Each thread's base and its loaded words, with a partial last tile, a full one and one item in a second tile; the sums are
    arbitrary, so that a base that ignored them would show."""
    wg, items, op = E.CONFIGS[config]
    tile = wg * items
    rng = random.Random(300 + config)
    cases = []
    for n in (1, tile - 1, tile, tile + 1):
        tiles = (n + tile - 1) // tile
        cases.append((E.TILE_BASE, config, words(rng, op, n, 40), values(rng, op, tiles, 40)))
    got = E.run_both(cases, tmp_path)
    for (_, _, w, sums), per_tile in zip(cases, got):
        assert len(per_tile) == len(sums)
        for t, (bases, loc) in enumerate(per_tile):
            mine = w[t * tile:(t + 1) * tile]
            mine += [0] * (tile - len(mine))
            assert loc == mine
            before, _ = E.exclusive(op, [op.item(x) for x in mine])
            assert bases == [op.combine(sums[t], before[k * items]) for k in range(wg)]


def ends_of(op, lengths):
    before, total = E.exclusive(op, lengths)
    return before[1:] + [total] if lengths else [], total


def test_composed_scan(tmp_path):
    """Tile sums, the rounds over them and the apply, as the units enqueue them, at fasta_write's (256, 2): no item, one, a second
    tile of one item, and one item in a second round of the second level (131 073 items)."""
    config = 2
    wg, items, op = E.CONFIGS[config]
    tile = wg * items
    rng = random.Random(400)
    lengths = [[rng.getrandbits(44) for _ in range(n)] for n in (0, 1, tile + 1, wg * tile + 1)]
    got = E.run_both([(E.COMPOSED, config, a, None) for a in lengths], tmp_path)
    for a, (ends, total) in zip(lengths, got):
        exp_ends, exp_total = ends_of(op, a)
        assert total == exp_total
        assert ends == exp_ends


@pytest.mark.parametrize("config", [0, 1])
def test_composed_scan_wide_tiles(config, tmp_path):
    """The same at 8 items a thread, wrapping (1024 wide) and saturating: two tiles and a part of a third."""
    wg, items, op = E.CONFIGS[config]
    rng = random.Random(450 + config)
    a = [rng.getrandbits(64 if op is E.ADD else 44) for _ in range(2 * wg * items + 3)]
    (ends, total), = E.run_both([(E.COMPOSED, config, a, None)], tmp_path)
    assert (ends, total) == ends_of(op, a)


def test_saturation_inside_a_tile(tmp_path):
    """The running sum reaches 2^64 - 1 in the middle of the second tile: everything behind is 2^64 - 1, nothing decreases."""
    config = 2
    wg, items, op = E.CONFIGS[config]
    tile = wg * items
    rng = random.Random(500)
    a = [rng.randrange(1, 1 << 30) for _ in range(2 * tile + 3)]
    at = tile + tile // 2 + 1
    a[at] = M64 - sum(a[:at]) - 5                  # five short of the top: the next item goes over it
    a[at + 1] = 7
    (ends, total), = E.run_both([(E.COMPOSED, config, a, None)], tmp_path)
    assert ends[at] == M64 - 5 and ends[at - 1] < 1 << 41
    assert all(e == M64 for e in ends[at + 1:]) and total == M64
    assert all(x <= y for x, y in zip(ends, ends[1:]))
    assert (ends, total) == ends_of(op, a)


@pytest.mark.parametrize("config", [1, 2])
def test_saturation_between_rounds(config, tmp_path):
    """The first round of tile sums ends three short of 2^64 - 1 and the second round's first sum goes over it: the carry
    saturates between two rounds and every later tile's base is 2^64 - 1."""
    wg, _, op = E.CONFIGS[config]
    rng = random.Random(600 + config)
    sums = [rng.randrange(1, 1 << 40) for _ in range(2 * wg + 1)]
    sums[wg - 1] = M64 - sum(sums[:wg - 1]) - 3
    sums[wg] = 10
    (excl, totals), = E.run_both([(E.SUMS_EXCLUSIVE, config, sums, None)], tmp_path)
    assert excl[wg] == M64 - 3                     # in front of the second round: not yet
    assert all(e == M64 for e in excl[wg + 1:]) and totals == [M64] * wg
    assert all(x <= y for x, y in zip(excl, excl[1:]))
    assert excl == E.exclusive(op, sums)[0]


def test_state_operand_order(tmp_path):
    """ck_fasta::next_state is not commutative: a header event in front of a sequence event leaves SEQ behind both, the other
    way round HEADER.  One workgroup with the two events, then the same with them swapped, then a random one."""
    config = 4
    wg, _, op = E.CONFIGS[config]
    assert op.combine(E.ST_HEADER, E.ST_SEQ) != op.combine(E.ST_SEQ, E.ST_HEADER)
    a, b = [E.ST_PASS] * wg, [E.ST_PASS] * wg
    a[5], a[70] = E.ST_HEADER, E.ST_SEQ            # in two different waves
    b[5], b[70] = E.ST_SEQ, E.ST_HEADER
    rnd = values(random.Random(700), op, wg, 0)
    got = E.run_both([(E.BLOCK_SCAN, config, v, None) for v in (a, b, rnd)] + [(E.SUMS_EXCLUSIVE, config, rnd + a + b, None)], tmp_path)
    (before_a, total_a), (before_b, total_b) = got[0], got[1]
    assert before_a == [E.ST_PASS] * 6 + [E.ST_HEADER] * 65 + [E.ST_SEQ] * (wg - 71) and total_a == [E.ST_SEQ] * wg
    assert before_b == [E.ST_PASS] * 6 + [E.ST_SEQ] * 65 + [E.ST_HEADER] * (wg - 71) and total_b == [E.ST_HEADER] * wg
    assert got[2] == (E.exclusive(op, rnd)[0], [E.exclusive(op, rnd)[1]] * wg)
    assert got[3] == (E.exclusive(op, rnd + a + b)[0], [E.ST_HEADER] * wg)      # three rounds: the state is carried across them
