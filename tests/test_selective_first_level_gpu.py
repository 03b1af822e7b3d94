"""The selective first level of the pruned left table (k_part_scatter<pf_key_cf_sel>, <pf_key_cf_sel_t2>): survivors of the right table's
key range are appended to a list of 2048 entries and written straight to their regions; a tile with more survivors is redone in rounds.

Every case compares dev.join_group_count (keys, counts, first rows, joined rows, order) with the numpy oracle, and tells which first-level
instance ran from the symbols the library recorded under the profiler name part_scatter_l0_pruned - each test has a device context of its
own, so the list holds what THIS test launched.

Sizes.  The operator takes the compact narrow form from 2^20 rows in all, its one-level plan from 2^21 rows in all (key windows of
2^15 ... 2^23 values), and two levels need more than 2^18 * 1.5 left rows: a left table of a few tiles reaches the pruned first level only
beside a right table of 2^21 rows.  The cases whose left table the issue fixes (3 * 8192 + 5 and 5 * 8192 rows) do that; the others use
2^20 rows per table (one level) or 2^19 (two levels).  A permutation of 3 * 8192 + 5 values has a lowest sixteenth of 1536 values, below
the smallest window the one-level plan takes: the learning case strides its keys by 64 (left: 64 * permutation; right: every value below a
sixteenth of that range, about 21 times each)."""
import numpy as np
import pytest

from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

PRUNED = "part_scatter_l0_pruned"
TILE2 = 8192
CAP = 2048                          # PART_SEL_CAP: a power of two, so the issue's survivor counts cover CAP - 1, CAP, CAP + 1
W = 1 << 16                         # the right table's keys: [0, W) - a compact window of 2^17 values
N1 = 128 * TILE2 + 5                # rows per table, one-level plan (odd; a partial last tile)
N2 = 64 * TILE2 + 5                 # rows per table, two-level plan (2^20 rows in all, fewer than 2^21)
SURVIVORS = [0, 1, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192]


@pytest.fixture
def ctx():
    """a device context of this test's own, profiling on: prof_symbols() then lists what this test launched and nothing else"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this environment")
    from midoridb_amd.dev import DeviceCtx
    c = DeviceCtx(0)
    c.prof_enable(True)
    yield c
    c.close()


@pytest.fixture
def tile2(monkeypatch):
    monkeypatch.setenv("MDB_TILE2_MIN", "1")


@pytest.fixture
def forced(monkeypatch):
    monkeypatch.setenv("MDB_SELECTIVE_L0", "2")


def _np(t):
    return t.cpu().numpy()


def _right(rng, n_r, lo=0, width=W):
    """n_r keys in [lo, lo + width), both ends present"""
    kr = lo + rng.integers(0, width, n_r, dtype=np.int64)
    kr[0], kr[1] = lo, lo + width - 1
    return kr


def _left(rng, n_l, width=W, keep=1 / 16):
    """n_l keys over 16 x the right table's range, about `keep` of them inside it"""
    kl = width + rng.integers(0, 15 * width, n_l, dtype=np.int64)
    inside = rng.random(n_l) < keep
    kl[inside] = rng.integers(0, width, int(inside.sum()), dtype=np.int64)
    return kl


def _syms(ctx):
    return ctx.prof_symbols(PRUNED)


def _ran_selective(ctx):
    return any("pf_key_cf_sel" in s for s in _syms(ctx))


def _ran_general(ctx):
    return any("pf_key_cf>" in s or "pf_key_cf_t2>" in s for s in _syms(ctx))


def _check(ctx, dl, dr, expect, info=None):
    ek, ec, ef, ej = expect
    k, c, f, j = ctx.join_group_count(dl, None, dr, None)
    assert j == ej, (info, j, ej)
    assert np.array_equal(_np(k), ek) and np.array_equal(_np(c), ec), info
    assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), ef), info


def _join(ctx, kl, kr, info=None, levels=1, selective=True):
    expect = orc.join_group_count(kl, None, kr, None)
    _check(ctx, ctx.to_dev(kl), ctx.to_dev(kr), expect, info)
    assert ctx.last_plan()["levels"] == levels, (info, ctx.last_plan())
    assert _ran_selective(ctx) == selective, (info, _syms(ctx))
    return expect


def test_the_second_join_over_the_same_columns_runs_the_selective_instance(ctx, tile2):
    """Variant D in miniature, nothing forced: the first call knows the columns from a key sample only and keeps the general instance; the
    second knows what the first delivered (one left row in 16 found a partner) and runs the selective one.  Both exact."""
    rng = np.random.default_rng(11)
    n_l, n_r = 3 * TILE2 + 5, 1 << 21
    kl = 64 * rng.permutation(n_l).astype(np.int64)
    kr = _right(rng, n_r, 0, 64 * n_l // 16)
    expect = orc.join_group_count(kl, None, kr, None)
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    _check(ctx, dl, dr, expect, "first call")
    assert ctx.last_plan()["levels"] == 1, ctx.last_plan()
    assert _ran_general(ctx) and not _ran_selective(ctx), _syms(ctx)
    _check(ctx, dl, dr, expect, "second call")
    assert _ran_selective(ctx), _syms(ctx)


@pytest.mark.parametrize("survivors", SURVIVORS)
def test_one_tile_with_a_given_number_of_survivors(ctx, tile2, forced, survivors):
    """One 8192-row tile holds exactly `survivors` rows inside the right table's range - below, at and above the list's capacity and its
    multiples - among tiles that keep one row in 16."""
    rng = np.random.default_rng(100 + survivors)
    kl = _left(rng, N1)
    t0 = 3 * TILE2
    kl[t0:t0 + TILE2] = W + rng.integers(0, 15 * W, TILE2, dtype=np.int64)
    at = t0 + rng.permutation(TILE2)[:survivors]
    kl[at] = rng.integers(0, W, survivors, dtype=np.int64)
    _join(ctx, kl, _right(rng, N1), survivors)


def test_every_row_survives_in_every_tile(ctx, tile2, forced, monkeypatch):
    """5 * 8192 left rows, all inside the right table's range: every tile overflows the list and is redone in rounds."""
    monkeypatch.setenv("MDB_MINMAX_PRUNE", "2")     # (nothing to prune by the key sample: the right table goes first all the same)
    rng = np.random.default_rng(12)
    kl = rng.permutation(W)[:5 * TILE2].astype(np.int64)
    _join(ctx, kl, _right(rng, 1 << 21), "all survive")


def test_tiles_of_4096_rows(ctx, forced):
    """The 4096-row form (tables below 2^25 rows without MDB_TILE2_MIN), with one tile above the list's capacity."""
    rng = np.random.default_rng(13)
    kl = _left(rng, N1)
    kl[8192:8192 + 4096] = rng.integers(0, W, 4096, dtype=np.int64)
    _join(ctx, kl, _right(rng, N1), "4096-row tiles")
    assert not any("_t2" in s for s in _syms(ctx)), _syms(ctx)


def test_left_keys_at_and_beside_the_ends_of_the_right_tables_range(ctx, tile2, forced):
    """The range test is inclusive: left keys equal to the right table's minimum and maximum join, minimum - 1 and maximum + 1 do not."""
    rng = np.random.default_rng(14)
    lo = 1000
    kl = lo + _left(rng, N1)
    kr = _right(rng, N1, lo, W)
    kl[[5, 77, TILE2 + 1, N1 - 1]] = lo
    kl[[6, 78, TILE2 + 2, N1 - 2]] = lo + W - 1
    kl[[7, 79, TILE2 + 3, N1 - 3]] = lo - 1
    kl[[8, 80, TILE2 + 4, N1 - 4]] = lo + W
    ek, ec, ef, ej = _join(ctx, kl, kr, "range ends")
    assert lo in ek and lo + W - 1 in ek and lo - 1 not in ek and lo + W not in ek


def test_disjoint_key_ranges_give_no_group(ctx, tile2, forced):
    rng = np.random.default_rng(15)
    kl = W + rng.integers(0, 15 * W, N1, dtype=np.int64)
    ek, ec, ef, ej = _join(ctx, kl, _right(rng, N1), "disjoint")
    assert len(ek) == 0 and ej == 0


@pytest.mark.parametrize("where", ["first_tile", "partial_last_tile"])
def test_survivors_in_one_tile_only(ctx, tile2, forced, where):
    rng = np.random.default_rng(16 + len(where))
    kl = W + rng.integers(0, 15 * W, N1, dtype=np.int64)
    if where == "first_tile":
        kl[:TILE2:3] = rng.integers(0, W, len(kl[:TILE2:3]), dtype=np.int64)
    else:
        kl[-5:] = rng.integers(0, W, 5, dtype=np.int64)
    ek, ec, ef, ej = _join(ctx, kl, _right(rng, N1), where)
    assert len(ek) > 0


def test_a_left_column_that_starts_one_element_into_its_buffer(ctx, tile2, forced):
    """The left column is a view 8 bytes off its buffer's 16-byte boundary (and of odd length): the selective instance counts positions
    from the aligned address below the first key."""
    rng = np.random.default_rng(18)
    kl, kr = _left(rng, N1), _right(rng, N1)
    assert N1 % 2 == 1
    buf = ctx.to_dev(np.concatenate([np.zeros(1, dtype=np.int64), kl]))
    dl = buf[1:]
    assert dl.data_ptr() % 16 == 8
    _check(ctx, dl, ctx.to_dev(kr), orc.join_group_count(kl, None, kr, None), "odd start")
    assert ctx.last_plan()["levels"] == 1 and _ran_selective(ctx) and not _ran_general(ctx), (ctx.last_plan(), _syms(ctx))


def test_a_region_overflow_ends_in_the_exact_layout(ctx, tile2, forced):
    """One left key through a whole tile: 8192 words for one region of some 1300 - the kernel reports it, the operator is redone with the
    exact layout, the answer is the oracle's."""
    rng = np.random.default_rng(19)
    kl = _left(rng, N1)
    kl[2 * TILE2:3 * TILE2] = 12345
    kr = _right(rng, N1)
    expect = orc.join_group_count(kl, None, kr, None)
    _check(ctx, ctx.to_dev(kl), ctx.to_dev(kr), expect, "region overflow")
    assert _ran_selective(ctx), _syms(ctx)
    assert int(expect[1].max()) >= TILE2


def test_the_two_level_pruned_plan(ctx, tile2, forced):
    """2^20 rows in all keep two partition levels (the one-level plan starts at 2^21): the same instance is their first."""
    rng = np.random.default_rng(20)
    kl = _left(rng, N2)
    kl[TILE2:2 * TILE2] = rng.integers(0, W, TILE2, dtype=np.int64)      # (one tile above the list's capacity)
    _join(ctx, kl, _right(rng, N2), "two levels", levels=2)


def test_the_knob_switches_the_selective_instance_off(ctx, tile2, monkeypatch):
    """MDB_SELECTIVE_L0=0: the general instance, also on the call that has learned that the join is selective."""
    monkeypatch.setenv("MDB_SELECTIVE_L0", "0")
    rng = np.random.default_rng(21)
    kl, kr = _left(rng, N1), _right(rng, N1)
    expect = orc.join_group_count(kl, None, kr, None)
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    for call in range(2):
        _check(ctx, dl, dr, expect, call)
    assert _ran_general(ctx) and not _ran_selective(ctx), _syms(ctx)
