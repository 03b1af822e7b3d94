"""k_leaf_wide4 (a first-level digit per workgroup, from its eight sub-regions per table) at the edges of its streams and of its ranged emit.

The streams: sub-regions that are EMPTY, in front of, between and behind those that hold words; last 16-byte pieces of 1 - 7 right words and of one
left word; a digit with no word at all of one table; sub-regions of more than 1024 pieces, and left sub-regions of more than one round of loads.
A form of the kernel that read a digit's sub-regions as ONE stream of pieces through a ring of loads was measured with these cases and not kept
(profiles/micro/join_leaf_stream/ab.txt); they stay for the next one.  The ranged emit: its stage of T / 2 records, and a digit with more.

Every case compares dev.join_group_count (keys, counts, first rows, joined rows, order) with an oracle, twice over the same columns - the first call
writes the record list, the second the ranged emit where the case says so - on a device context of its own with profiling on, so that the profiler
names are this test's launches.  Shapes as in test_join_tail_gpu.py unless a case says otherwise: a left table of 2^21 rows whose keys spread over
16 times the right table's range [LO, LO + 2^19), one in 16 inside it; the key window then has 20 bits: 512 digits of 2048 values."""
import numpy as np
import pytest

from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

W = 1 << 19                         # the right table's keys: [lo, lo + W)
NL = 1 << 21                        # rows of the left table
LO = 1000
TILE = 4096                         # MDB_TILE: keys per first-level tile below 2^25 rows; tile i of a table fills sub-region i % 8 of every digit
NSUB = 8                            # PART_NSUB
DIGITS = 512
LEAF4, RIGHT_PASS = "leaf_join_wide4", "part_scatter_l0_w32"


@pytest.fixture
def ctx():
    """a device context of this test's own, profiling on"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this environment")
    from midoridb_amd.dev import DeviceCtx
    c = DeviceCtx(0)
    c.prof_enable(True)
    yield c
    c.close()


def _np(t):
    return t.cpu().numpy()


def _left(rng, n_l=NL, keep=1 / 16):
    """n_l keys over 16 x the right table's range, about `keep` of them inside it"""
    kl = LO + W + rng.integers(0, 15 * W, n_l, dtype=np.int64)
    inside = rng.random(n_l) < keep
    kl[inside] = LO + rng.integers(0, W, int(inside.sum()), dtype=np.int64)
    return kl


def _per_key(keys):
    k = keys[(keys >= LO) & (keys < LO + W)] - LO
    return np.bincount(k, minlength=W)


def _check(ctx, dl, dr, expect, info):
    ek, ec, ef, ej = expect
    k, c, f, j = ctx.join_group_count(dl, None, dr, None)
    assert j == ej, (info, j, ej)
    assert np.array_equal(_np(k), ek) and np.array_equal(_np(c), ec), info
    assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), ef), info


def _two_calls(ctx, kl, kr, expect, info, ranged=None):
    """two calls over the same columns, both checked against the oracle; one partition level and k_leaf_wide4 in both"""
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    for call in range(2):
        _check(ctx, dl, dr, expect, (info, call))
        plan = ctx.last_plan()
        assert plan["levels"] == 1 and plan["minmax_pruned"], (info, call, plan)
        assert ctx.prof_read()[LEAF4][0] == call + 1, (info, call, ctx.prof_read())
    assert any("k_leaf_wide4" in s for s in ctx.prof_symbols(LEAF4)), (info, ctx.prof_symbols(LEAF4))
    if ranged is not None:
        assert bool(ctx.last_plan()["ranged_order"]) == ranged, (info, ctx.last_plan())


def test_empty_and_tiny_sub_regions(ctx):
    """A right table of 3 * 4096 + 5 rows is four first-level tiles: the sub-regions 0 - 2 of a digit receive some 8 words each, sub-region 3 the
    last tile's 5 words over ALL digits, the sub-regions 4 - 7 nothing.  Pieces of 1 - 7 valid words, streams that begin behind empty sub-regions
    (a digit without a word of tile 0) and end in front of them, and the loads beyond the stream's end sent to its first piece."""
    rng = np.random.default_rng(601)
    n_r = 3 * TILE + 5
    kr = LO + rng.integers(0, W, n_r, dtype=np.int64)
    kr[:2] = LO, LO + W - 1
    kl = _left(rng)
    assert _per_key(kr).max() <= 31 and _per_key(kl).max() <= 15
    assert NSUB - (n_r + TILE - 1) // TILE >= 3        # sub-regions of every digit that no tile writes to
    expect = orc.join_group_count(kl, None, kr, None)
    assert len(expect[0]) > 1000
    _two_calls(ctx, kl, kr, expect, "tiny right table")
    syms = ctx.prof_symbols(RIGHT_PASS)             # (the right pass in 4096-key tiles: what the count of empty sub-regions above rests on)
    assert any("out16" in s and "_t2" not in s and "_t4" not in s for s in syms), syms


@pytest.mark.parametrize("name", ["one key in 64", "96 right keys", "96 right keys, three left survivors"])
def test_digits_with_nothing_on_one_side(ctx, name):
    """The right table's keys thinned to one in 64 (4 words per right sub-region where the left ones hold 32); then 96 distinct right keys, 31
    rows each: at least 414 of the 512 digits have NO right word (their workgroups ask for nothing of the right table, find no partner and emit
    nothing) while left rows arrive in every digit; then the same right table against three left rows inside its range: digits with no LEFT word,
    most of them with no word at all."""
    rng = np.random.default_rng(610 + len(name))
    if name == "one key in 64":
        keys = LO + np.arange(0, W, 64, dtype=np.int64)
        keys[-1] = LO + W - 1
        kr = np.tile(keys, 2)
    else:
        keys = LO + rng.choice(W, 96, replace=False).astype(np.int64)
        keys[:2] = LO, LO + W - 1
        kr = np.tile(keys, 31)
        assert len(np.unique(kr)) < DIGITS - 400
    rng.shuffle(kr)
    if name.endswith("three left survivors"):
        kl = LO + W + rng.integers(0, 15 * W, NL, dtype=np.int64)
        kl[[5, 70001, NL - 2]] = [keys[7], keys[1], keys[7]]
    else:
        kl = _left(rng)
        kl[[11, 300000]] = keys[3]              # (a partner at least: groups to emit beside the digits that emit nothing)
    assert _per_key(kr).max() <= 31 and _per_key(kl).max() <= 15
    expect = orc.join_group_count(kl, None, kr, None)
    if name.endswith("three left survivors"):
        assert expect[0].tolist() == [keys[7], keys[1]] and expect[1].tolist() == [62, 31] and expect[2].tolist() == [5, 70001]
    else:
        assert len(expect[0]) >= 1
    _two_calls(ctx, kl, kr, expect, name)


def test_counts_that_are_no_multiple_of_a_piece(ctx):
    """The default shape - every one of 2^19 keys twice in the right table, one left row in 16 inside the range: some 256 right words (32 pieces)
    and 32 left words per sub-region - with one right row more and an odd number of left rows inside the range: whichever way the rows fall into
    the 4096 sub-regions of a table, a right one's count is no multiple of 8 and a left one's is odd."""
    rng = np.random.default_rng(620)
    kr = LO + np.append(np.tile(np.arange(W, dtype=np.int64), 2), 5)
    rng.shuffle(kr)
    kl = _left(rng)
    if int(((kl >= LO) & (kl < LO + W)).sum()) % 2 == 0:
        kl[np.flatnonzero(kl >= LO + W)[0]] = LO + 77
    assert len(kr) % 8 == 1 and int(((kl >= LO) & (kl < LO + W)).sum()) % 2 == 1
    assert (_per_key(kl) % 2 == 1).any() and _per_key(kl).max() <= 15 and _per_key(kr).max() == 3
    expect = orc.join_group_count(kl, None, kr, None)
    _two_calls(ctx, kl, kr, expect, "default shape", ranged=True)


def test_the_rings_go_round(ctx):
    """17 right rows for each of 2^21 keys - 35.6 * 10^6 rows in the right pass's 16384-key tiles, some 8700 words (1088 pieces) per sub-region, 8704
    pieces per digit: a thread takes more than one piece of a sub-region and its ring of four goes round, inside a sub-region and across its end.
    The left table: every key four times, one in four a fifth time - 8.9 * 10^6 rows inside the range, 17 408 words (8704 pieces) per digit, more
    than the eight per thread that are asked for in front of the barrier: the left ring goes round too - and 2^20 rows spread over 15 times the range
    above it, which the first level prunes.  The window has 22 bits: 8192 values per digit.  Oracle: the C hash join with 16 threads (the numpy oracle
    takes too long at this size; tables and oracle: 2 s on eight cores)."""
    from oracle import cpu
    rng = np.random.default_rng(630)
    w2 = 1 << 21
    n_r = 17 * w2
    kr = LO + ((np.arange(n_r, dtype=np.int64) * 2654435761) & (w2 - 1))      # (an odd multiplier: every key exactly 17 times, scattered)
    n_in = 4 * w2 + w2 // 4
    n_l = n_in + (1 << 20)
    kl = np.empty(n_l, dtype=np.int64)
    kl[:4 * w2] = LO + np.tile(np.arange(w2, dtype=np.int64), 4)
    kl[4 * w2:n_in] = LO + rng.choice(w2, w2 // 4, replace=False)
    kl[n_in:] = LO + w2 + rng.integers(0, 15 * w2, n_l - n_in, dtype=np.int64)
    rng.shuffle(kl)
    assert (n_r // (NSUB * DIGITS) + 7) // 8 > 1024             # pieces per right sub-region: more than one per thread
    assert (n_in // DIGITS + 1) // 2 > 8 * 1024                 # left pieces per digit: more than eight per thread
    ek, ec, ef, ej = cpu.hash_join_group_count(kl, None, kr, None, nthreads=16)
    assert ej == 17 * n_in and len(ek) == w2 and ec.max() == 85 and ec.min() == 68
    _two_calls(ctx, kl, kr, (ek, ec, ef, ej), "17 right rows a key")
    assert any("_t4" in s for s in ctx.prof_symbols(RIGHT_PASS)), ctx.prof_symbols(RIGHT_PASS)


def test_a_digit_with_more_groups_than_the_ranged_emit_stages(ctx):
    """The ranged emit sorts a digit's records by range in the 4 T bytes of the table it has read into registers - room for T / 2 records - and
    writes the rest from where it finds them.  2^19 + 2^15 keys, each with a left row, in a window of 20 bits (512 digits of T = 2048 values): more
    than 512 * T / 2 groups, so some digit has more than T / 2, whichever way the keys fall.  10.5 * 10^6 left rows: few enough groups per range
    of row ids for the ranged emit."""
    from oracle import cpu
    rng = np.random.default_rng(640)
    w2, n_l = (1 << 19) + (1 << 15), (1 << 23) + (1 << 21)
    kr = LO + np.tile(np.arange(w2, dtype=np.int64), 2)
    rng.shuffle(kr)
    kl = LO + w2 + rng.integers(0, 15 * w2, n_l, dtype=np.int64)
    kl[rng.choice(n_l, w2, replace=False)] = LO + np.arange(w2, dtype=np.int64)
    ek, ec, ef, ej = cpu.hash_join_group_count(kl, None, kr, None, nthreads=16)
    assert len(ek) == w2 and ej == 2 * w2
    _two_calls(ctx, kl, kr, (ek, ec, ef, ej), "more groups than the stage holds", ranged=True)
    plan = ctx.last_plan()
    assert plan["key_bits"] == 20 and plan["digits"] == DIGITS and len(ek) > DIGITS * (1 << (20 - 9)) // 2, plan
