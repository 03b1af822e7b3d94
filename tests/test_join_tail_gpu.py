"""The tail of the one-level join + GROUP BY + COUNT(*): k_leaf_wide4 (a first-level digit per workgroup) and behind it k_order_leaf_sparse - ranges
of 2^16 first row ids ranked through a bitmap, at most 8192 groups each, two workgroups per CU, the prefixes of a range's bitmap words as 16-bit
words.

Every case compares dev.join_group_count (keys, counts, first rows, joined rows, order) with the numpy oracle, twice over the same columns: the
leaf writes its records straight into the ordering kernel's ranges from the SECOND call on (the first one tells how many groups to expect).  Each
test has a device context of its own, so what the library recorded under its profiler names is what this test launched.

Sizes.  The one-level plan with k_leaf_wide4 is taken from 2^21 rows in all, for key windows of 2^19 ... 2^23 values and at most 31 right / 15 left
rows per key.  Unless a case says otherwise: a left table of 2^21 rows (32 ranges of row ids) whose keys spread over 16 times the right table's
range [lo, lo + 2^19) - the left table is pruned by that range, which is the key window the plan is chosen for -, and a right table that
holds each of its 2^19 keys twice."""
import numpy as np
import pytest

from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

W = 1 << 19                         # the right table's keys: [lo, lo + W)
NL = 1 << 21                        # rows of the left table
LO = 1000
RANGE_BITS = 16                     # ORDER_RANGE_BITS: first row ids per range of the ordering kernel
RANGE_CAP = 8192                    # ORDER_RANGE_CAP: groups a range holds
LEAF4, LEAF_WIDE, ORDER = "leaf_join_wide4", "leaf_join_wide", "order_leaf_sparse"


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


def _right(rng, lo=LO, width=W, times=2):
    """every key of [lo, lo + width) `times` times, shuffled"""
    kr = lo + np.tile(np.arange(width, dtype=np.int64), times)
    rng.shuffle(kr)
    return kr


def _outside(rng, n, lo=LO, width=W):
    """n keys above the right table's range, within 16 times its width"""
    return lo + width + rng.integers(0, 15 * width, n, dtype=np.int64)


def _left(rng, n_l=NL, lo=LO, width=W, keep=1 / 16, first_key=0):
    """n_l keys over 16 x the right table's range, about `keep` of them inside it - from lo + first_key on: the keys below are the case's to place"""
    kl = _outside(rng, n_l, lo, width)
    inside = rng.random(n_l) < keep
    kl[inside] = lo + rng.integers(first_key, width, int(inside.sum()), dtype=np.int64)
    return kl


def _per_key(keys, lo=LO, width=W):
    """rows per key of [lo, lo + width)"""
    k = keys[(keys >= lo) & (keys < lo + width)] - lo
    return np.bincount(k, minlength=width)


def _per_range(expect, n_l):
    """groups per range of 2^16 first row ids, by the oracle"""
    return np.bincount(expect[2] >> RANGE_BITS, minlength=((n_l - 1) >> RANGE_BITS) + 1)


def _check(ctx, dl, dr, expect, info=None):
    ek, ec, ef, ej = expect
    k, c, f, j = ctx.join_group_count(dl, None, dr, None)
    assert j == ej, (info, j, ej)
    assert np.array_equal(_np(k), ek) and np.array_equal(_np(c), ec), info
    assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), ef), info


def _two_calls(ctx, kl, kr, expect, info=None, ranged=True, leaf=LEAF4):
    """two calls over the same columns, both checked; the second one with the ranged emit and the ordering kernel behind it -> (dl, dr)"""
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    for call in range(2):
        _check(ctx, dl, dr, expect, (info, call))
        plan = ctx.last_plan()
        assert plan["levels"] == 1, (info, call, plan)
    assert ctx.prof_symbols(leaf), (info, ctx.prof_read())
    if ranged is not None:
        assert bool(ctx.last_plan()["ranged_order"]) == ranged, (info, ctx.last_plan())
        assert bool(ctx.prof_symbols(ORDER)) == ranged, (info, ctx.prof_read())
    return dl, dr


# ------------------------------------------------------------------ the ordering kernel

def test_ranges_without_groups_between_ranges_with_groups(ctx):
    """Ranges 0, 2, 5 and 31 hold thousands of groups, range 7 exactly one, every other range none: workgroups that leave at once beside workgroups
    that rank, and the output position of a range is the sum over all ranges before it, empty ones included."""
    rng = np.random.default_rng(401)
    kl = _outside(rng, NL)
    for r in (0, 2, 5, 31):
        rows = np.arange(r << RANGE_BITS, (r + 1) << RANGE_BITS)
        rows = rows[rng.random(rows.size) < 0.1]
        kl[rows] = LO + rng.integers(1, W, rows.size, dtype=np.int64)
    kl[(7 << RANGE_BITS) + 777] = LO          # (key LO occurs nowhere else in the left table)
    kr = _right(rng)
    expect = orc.join_group_count(kl, None, kr, None)
    per = _per_range(expect, NL)
    assert per[7] == 1 and all(1000 < per[r] < RANGE_CAP for r in (0, 2, 5, 31)) and per.sum() == per[[0, 2, 5, 7, 31]].sum(), per
    assert _per_key(kl).max() <= 15
    _two_calls(ctx, kl, kr, expect, "sparse ranges")


def test_groups_at_the_first_and_at_the_last_row(ctx):
    """A table of 2^21 + 12345 rows - the last range holds 12345 row ids -; one group begins at row 0, another at the last row."""
    rng = np.random.default_rng(402)
    n_l = NL + 12345
    kl = _left(rng, n_l, first_key=2)
    kl[0], kl[-1] = LO, LO + 1
    kr = _right(rng)
    expect = orc.join_group_count(kl, None, kr, None)
    ek, ec, ef, ej = expect
    assert ef[0] == 0 and ek[0] == LO and ef[-1] == n_l - 1 and ek[-1] == LO + 1 and ec[0] == ec[-1] == 2
    assert _per_key(kl).max() <= 15
    _two_calls(ctx, kl, kr, expect, "first and last row")


def _range0(groups):
    """rows 0 ... groups - 1 carry distinct keys with a partner, the rest of range 0 none; the other ranges one row in 16, of other keys"""
    rng = np.random.default_rng(403)
    kl = _left(rng, first_key=RANGE_CAP + 1)
    kl[:1 << RANGE_BITS] = _outside(rng, 1 << RANGE_BITS)
    kl[:groups] = LO + rng.permutation(RANGE_CAP + 1)[:groups]
    kr = _right(rng)
    expect = orc.join_group_count(kl, None, kr, None)
    per = _per_range(expect, NL)
    assert per[0] == groups and per[1:].max() < RANGE_CAP // 2 + 256, per
    # (the ranged form is taken while the groups expected, an eighth added, fill the average range to two thirds of what is left of it after 1024:
    # order_ranges_apply() of mdb_dev_order.hip)
    assert per.sum() * 9 // 8 <= (RANGE_CAP - 1024) * 2 // 3 * len(per), per.sum()
    assert _per_key(kl).max() <= 15
    return kl, kr, expect


def test_a_range_of_exactly_8192_groups(ctx):
    """The most a range holds, and the largest prefix the kernel's 16-bit prefix words take: ranked here, no retry."""
    kl, kr, expect = _range0(RANGE_CAP)
    before = ctx.counters()["retries"]
    _two_calls(ctx, kl, kr, expect, "8192 groups in range 0")
    assert ctx.counters()["retries"] == before, ctx.last_plan()


def test_a_range_of_8193_groups_takes_the_record_list(ctx):
    """One group more than a range holds: the leaf reports the full range, the operator is redone with the record list and its sort - exact."""
    kl, kr, expect = _range0(RANGE_CAP + 1)
    before = ctx.counters()["retries"]
    _two_calls(ctx, kl, kr, expect, "8193 groups in range 0", ranged=None)
    assert ctx.counters()["retries"] > before or not ctx.last_plan()["ranged_order"], (ctx.counters(), ctx.last_plan())


def _one_hot_key(right_rows):
    """key LO: `right_rows` right rows and 15 left rows; every other key twice in the right table"""
    rng = np.random.default_rng(404)
    kl = _left(rng, first_key=1)
    kl[rng.choice(NL, 15, replace=False)] = LO
    kr = np.concatenate([_right(rng), np.full(right_rows - 2, LO, dtype=np.int64)])
    rng.shuffle(kr)
    assert _per_key(kl).max() == 15 and _per_key(kl)[0] == 15 and _per_key(kr).max() == right_rows
    return kl, kr, orc.join_group_count(kl, None, kr, None)


def test_31_right_and_15_left_rows_of_a_key(ctx):
    """The largest counts k_leaf_wide4's fields hold: COUNT(*) = 465."""
    kl, kr, expect = _one_hot_key(31)
    ek, ec = expect[0], expect[1]
    assert ec[ek == LO][0] == 465
    _two_calls(ctx, kl, kr, expect, "31 x 15")


def test_32_right_rows_of_a_key_go_through_the_wide_leaf(ctx):
    """One right row more than the 5-bit field holds: the checksum notices, k_leaf_wide answers exactly."""
    kl, kr, expect = _one_hot_key(32)
    ek, ec = expect[0], expect[1]
    assert ec[ek == LO][0] == 480
    _two_calls(ctx, kl, kr, expect, "32 x 15", ranged=None, leaf=LEAF_WIDE)


def test_output_columns_of_exactly_g_rows_and_of_one_row_less(ctx):
    """The ordering kernel is launched before the host knows the group count and writes no row beyond the caller's columns: columns of exactly G
    rows are filled, with G - 1 rows the operator returns its capacity error and the rows behind the columns stay as they were."""
    import torch
    from ctypes import byref, c_uint64
    from midoridb_amd.dev import MDB_ORDER_FIRST, _ptr
    rng = np.random.default_rng(405)
    kl, kr = _left(rng), _right(rng)
    expect = orc.join_group_count(kl, None, kr, None)
    ek, ec, ef, ej = expect
    G, guard = len(ek), 4096
    dl, dr = _two_calls(ctx, kl, kr, expect, "default columns")

    def call(cap):
        ok = torch.full((cap + guard,), -7, dtype=torch.int64, device=dl.device)
        oc = torch.full((cap + guard,), -7, dtype=torch.int64, device=dl.device)
        of = torch.full((cap + guard,), -7, dtype=torch.int32, device=dl.device)
        g, j = c_uint64(), c_uint64()
        rc = ctx.lib.mdb_dev_join_group_count(ctx.h, _ptr(dl), None, dl.numel(), _ptr(dr), None, dr.numel(), MDB_ORDER_FIRST, _ptr(ok), _ptr(oc), _ptr(of),
                                              cap, byref(g), byref(j))
        for t in (ok, oc, of):
            assert bool((t[cap:] == -7).all()), ("written beyond the columns", cap)
        return rc, ok, oc, of, g.value, j.value

    rc, ok, oc, of, g, j = call(G)
    assert rc == 0 and g == G and j == ej and ctx.last_plan()["ranged_order"], (rc, g, ctx.last_plan())
    assert np.array_equal(_np(ok[:G]), ek) and np.array_equal(_np(oc[:G]), ec)
    assert np.array_equal(_np(of[:G]).view(np.uint32).astype(np.int64), ef)
    rc = call(G - 1)[0]
    assert rc != 0 and b"group output capacity" in ctx.lib.mdb_dev_last_error(ctx.h), (rc, ctx.lib.mdb_dev_last_error(ctx.h))


# ------------------------------------------------------------------ few groups, and none

@pytest.mark.parametrize("name", ["no survivors", "three survivors", "usual density"])
def test_left_tables_of_few_survivors(ctx, name):
    """No left row inside the right table's key range (no group, nothing to order), exactly three (two groups: ranges with a single record between
    empty ones), one row in 16 (some 32 words per left sub-region of the leaf, odd counts among them)."""
    rng = np.random.default_rng(500 + len(name))
    kr = _right(rng)
    if name == "usual density":
        kl = _left(rng)
    else:
        kl = _outside(rng, NL)
        if name == "three survivors":
            kl[[5, 70001, NL - 2]] = [LO + 9, LO + W - 1, LO + 9]
    expect = orc.join_group_count(kl, None, kr, None)
    ek, ec, ef, ej = expect
    if name == "no survivors":
        assert len(ek) == 0 and ej == 0
    elif name == "three survivors":
        assert ek.tolist() == [LO + 9, LO + W - 1] and ec.tolist() == [4, 2] and ef.tolist() == [5, 70001]
    else:
        assert (_per_key(kl) % 2 == 1).any() and _per_key(kl).max() <= 15
    _two_calls(ctx, kl, kr, expect, name, ranged=None if name == "no survivors" else True)
