"""The right table's first level of the one-level join in tiles of 16384 rows (k_part_scatter<pf_key_w32_out16_cf_t4>, 1024 threads, 16 rows
each): int64 columns of 2^25 rows and more without a NULL bitmap; MDB_TILE4_MIN=1 brings it to the small tables of these tests.

Every case compares dev.join_group_count (keys, counts, first rows, joined rows, order) with the numpy oracle, and tells which first-level
instance ran from the symbols the library recorded under the profiler name part_scatter_l0_w32 - each test has a device context of its own,
so the list holds what THIS test launched.

Sizes.  The operator takes its one-level plan (2-byte words for the right table) from 2^21 rows in all, for key windows of 2^15 ... 2^23
values: a right table of one or a few tiles stands beside a left table of 2^21 rows.  The right table's keys lie in [lo, lo + 2^16); the left
table's keys spread over 16 times that range, one in 16 inside it - the right table goes first and the left one is pruned by its key range,
as in the benchmark's variant D."""
import numpy as np
import pytest

from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

RIGHT = "part_scatter_l0_w32"
TILE4 = 16384
W = 1 << 16                         # the right table's keys: [lo, lo + W)
NL = 1 << 21                        # rows of the left table
T4, T2, PLAIN = "pf_key_w32_out16_cf_t4>", "pf_key_w32_out16_cf_t2>", "pf_key_w32_out16_cf>"


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
def tile4(monkeypatch):
    monkeypatch.setenv("MDB_TILE4_MIN", "1")


@pytest.fixture
def tile2(monkeypatch):
    monkeypatch.setenv("MDB_TILE2_MIN", "1")


def _np(t):
    return t.cpu().numpy()


def _right(rng, n_r, lo=0, width=W):
    """n_r keys in [lo, lo + width), both ends present"""
    kr = lo + rng.integers(0, width, n_r, dtype=np.int64)
    kr[0], kr[-1] = lo, lo + width - 1
    return kr


def _left(rng, n_l=NL, lo=0, width=W, keep=1 / 16):
    """n_l keys over 16 x the right table's range, about `keep` of them inside it"""
    kl = lo + width + rng.integers(0, 15 * width, n_l, dtype=np.int64)
    inside = rng.random(n_l) < keep
    kl[inside] = lo + rng.integers(0, width, int(inside.sum()), dtype=np.int64)
    return kl


def _syms(ctx):
    return ctx.prof_symbols(RIGHT)


def _ran(ctx, which):
    return any(which in s for s in _syms(ctx))


def _check(ctx, dl, dr, expect, info=None, null_r=None):
    ek, ec, ef, ej = expect
    k, c, f, j = ctx.join_group_count(dl, None, dr, null_r)
    assert j == ej, (info, j, ej)
    assert np.array_equal(_np(k), ek) and np.array_equal(_np(c), ec), info
    assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), ef), info


def _join(ctx, kl, kr, info=None, ran=T4, not_ran=()):
    expect = orc.join_group_count(kl, None, kr, None)
    _check(ctx, ctx.to_dev(kl), ctx.to_dev(kr), expect, info)
    assert _ran(ctx, ran), (info, _syms(ctx), ctx.last_plan())
    for other in not_ran:
        assert not _ran(ctx, other), (info, _syms(ctx))
    return expect


def _sampled_rows(n):
    """the rows of an n-row column that the operator's key sample reads: gc_sample_pos() of midoridb_amd/csrc/mdb_dev_join_internal.h (fmix64 of
    GC_NARROW_SAMPLE = 4096 multiples of the golden ratio, mod n), restated.  If the sampler changes, the 2^40 key of the test below may land in
    the sample; the call then never takes the compact narrow form, and the test says so before it asks which instance ran."""
    k = np.arange(1, 4097, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xFF51AFD7ED558CCD)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xC4CEB9FE1A85EC53)
    k ^= k >> np.uint64(33)
    return set((k % np.uint64(n)).tolist())


@pytest.mark.parametrize("n_r", [TILE4 - 1, TILE4, TILE4 + 1, 3 * TILE4 + 5, 128 * TILE4])
def test_tile_edges(ctx, tile4, n_r):
    """One row short of a tile, a tile, a tile and a row, three tiles and five rows, 128 tiles: full and partial tiles, grids of 8 ... 128
    workgroups of which 1 ... 128 have a tile."""
    rng = np.random.default_rng(200 + n_r % 1000)
    _join(ctx, _left(rng, lo=1000), _right(rng, n_r, 1000), n_r, not_ran=(T2, PLAIN))
    assert ctx.last_plan()["levels"] == 1, ctx.last_plan()


def test_the_key_range_comes_from_the_last_partial_tile(ctx, tile4):
    """The right table's smallest and largest key occur only in the last 5 rows of 3 * 16384 + 5 - the partial tile's (min, max) pair decides
    the range the left table is pruned by: left keys equal to it join, the keys one below and one above do not."""
    rng = np.random.default_rng(31)
    lo, n_r = 5000, 3 * TILE4 + 5
    hi = lo + W - 1
    kr = lo + 1 + rng.integers(0, W - 2, n_r, dtype=np.int64)
    kr[-5:] = [hi, lo + 7, lo, hi, lo]
    assert kr[:-5].min() > lo and kr[:-5].max() < hi
    kl = _left(rng, lo=lo)
    kl[kl == lo - 1] = lo + 3        # (the four values below are placed by hand only)
    kl[kl == hi + 1] = lo + 3
    kl[[3, 4099, NL - 1]] = lo
    kl[[5, 77777, NL - 2]] = hi
    kl[[7, 8193, NL - 3]] = lo - 1
    kl[[9, 16385, NL - 4]] = hi + 1
    ek, ec, ef, ej = _join(ctx, kl, kr, "range ends", not_ran=(T2, PLAIN))
    assert ctx.last_plan()["levels"] == 1, ctx.last_plan()
    assert lo in ek and hi in ek and lo - 1 not in ek and hi + 1 not in ek
    assert ec[ek == lo][0] == 2 * (kl == lo).sum() and ec[ek == hi][0] == 2 * (kl == hi).sum()


def test_a_full_region_ends_in_the_exact_layout(ctx, tile4):
    """2^21 right rows of which 63 in 64 hold one key: one digit receives some 16000 words of every tile, its eight sub-regions of some 1500
    words overflow, the kernel reports it and leaves the digit's words unwritten, the operator is redone with the exact layout.  (With the one
    key in EVERY row the sampled window has 2^14 values, below what the one-level plan takes - a two-level plan runs pf_key_w32; the 64th
    rows spread over [0, 2^16) keep the window at 2^17 values.)"""
    rng = np.random.default_rng(32)
    kl, kr = _left(rng), _right(rng, 1 << 21)
    same = rng.random(1 << 21) < 63 / 64
    same[[0, -1]] = False
    kr[same] = 12345
    kl[[11, 4097]] = 12345
    ek, ec, ef, ej = _join(ctx, kl, kr, "one right key")
    assert ctx.counters()["retries"] >= 1, ctx.last_plan()
    assert int(ec.max()) >= same.sum()


@pytest.mark.parametrize("where", ["first_in_tile", "last_in_tile"])
def test_a_right_key_outside_the_sampled_window(ctx, tile4, where):
    """One right row holds 2^40, at the first / last row of a tile and at a row the operator's key sample does not read: the window comes
    from the sample, the kernel meets the key, reports it, and the operator answers exactly in another form."""
    rng = np.random.default_rng(33)
    n_r = 128 * TILE4
    kl, kr = _left(rng), _right(rng, n_r)
    sampled = _sampled_rows(n_r)
    row = next(r for r in (t * TILE4 + (0 if where == "first_in_tile" else TILE4 - 1) for t in range(5, 128)) if r not in sampled)
    kr[row] = 1 << 40
    sampled_l = _sampled_rows(NL)
    kl[next(r for r in range(12345, NL) if r not in sampled_l)] = 1 << 40
    expect = orc.join_group_count(kl, None, kr, None)
    _check(ctx, ctx.to_dev(kl), ctx.to_dev(kr), expect, where)
    assert _syms(ctx), "no first level under part_scatter_l0_w32: the key sample saw the 2^40 key - does _sampled_rows() still restate gc_sample_pos()?"
    assert _ran(ctx, T4), (_syms(ctx), ctx.last_plan())
    ek, ec = expect[0], expect[1]
    assert (1 << 40) in ek and ec[ek == (1 << 40)][0] == 1


def test_a_right_table_with_a_null_bitmap_keeps_the_smaller_tiles(ctx, tile4, tile2):
    rng = np.random.default_rng(34)
    n_r = 3 * TILE4 + 5
    kl, kr = _left(rng), _right(rng, n_r)
    nulls = rng.random(n_r) < 0.1
    nulls[[0, n_r - 1]] = False
    expect = orc.join_group_count(kl, None, kr, nulls)
    _check(ctx, ctx.to_dev(kl), ctx.to_dev(kr), expect, "NULLs", null_r=ctx.nullbits_dev(nulls))
    assert not _ran(ctx, T4) and (_ran(ctx, T2) or _ran(ctx, PLAIN)), (_syms(ctx), ctx.last_plan())


def test_the_knob_switches_the_16384_row_tiles_off(ctx, tile4, tile2, monkeypatch):
    monkeypatch.setenv("MDB_TILE4", "0")
    rng = np.random.default_rng(35)
    _join(ctx, _left(rng), _right(rng, 3 * TILE4 + 5), "MDB_TILE4=0", ran=T2, not_ran=(T4,))


def test_the_4096_row_knob_switches_them_off_too(ctx, tile4, tile2, monkeypatch):
    """MDB_TILE2=0 asks for 4096-row tiles everywhere: neither of the larger forms."""
    monkeypatch.setenv("MDB_TILE2", "0")
    rng = np.random.default_rng(38)
    _join(ctx, _left(rng), _right(rng, 3 * TILE4 + 5), "MDB_TILE2=0", ran=PLAIN, not_ran=(T4, T2))


def test_a_table_of_2_21_rows_keeps_the_8192_row_tiles(ctx, tile2):
    """No MDB_TILE4_MIN: the 16384-row tiles start at 2^25 rows."""
    rng = np.random.default_rng(36)
    _join(ctx, _left(rng), _right(rng, 1 << 21), "below the threshold", ran=T2, not_ran=(T4,))


def test_two_calls_over_the_same_columns(ctx, tile4):
    """The second call knows what the first learned about the columns: the same instance, the same result."""
    rng = np.random.default_rng(37)
    kl, kr = _left(rng), _right(rng, 5 * TILE4 + 1)
    expect = orc.join_group_count(kl, None, kr, None)
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    for call in range(2):
        _check(ctx, dl, dr, expect, call)
        assert ctx.last_plan()["levels"] == 1, (call, ctx.last_plan())
    assert _syms(ctx) and all(T4 in s for s in _syms(ctx)), _syms(ctx)
    assert ctx.prof_read()[RIGHT][0] == 2, ctx.prof_read()[RIGHT]
