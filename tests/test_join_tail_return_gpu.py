"""Join + GROUP BY + COUNT(*) for a caller that reads its result in stream order (mdb_dev_results_in_stream_order, what DeviceCtx promises when it is
bound to torch's current stream): on the path whose leaf kernel fills the ordering kernel's ranges the call returns when the leaf kernel's status words
have arrived, and the ordering kernel - the one that writes the result columns - runs behind the return.

Tables: the left keys a permutation of [0, n), the right keys a permutation mod n / 16 (the benchmark's variant D), at the smallest power of two
the one-level ranged form takes in this shape: 2^22 + 2^22 rows.  (k_leaf_wide4 asks for a key window of 2^19 values at least - ten bits below the
first level's nine -, and the window of n / 16 right keys, padded by a sixteenth + 4096 at either end, reaches that from n / 16 = 2^18 on; at 2^20 +
2^20 rows the window has 2^17 values and the plan is the one-level form WITHOUT the ranged emit: measured, ranged_order 0.)

Every case calls the operator twice over the same columns (the first call tells how many groups to expect, the ranged form is taken from the
second one on) and asserts ranged_order == 1 and last_return_was_early() on that second call: a case cannot pass on another path.  Keys, counts,
first rows (the order) and the joined rows are compared with oracle.cpu.hash_join_group_count."""
from ctypes import byref, c_uint64

import numpy as np
import pytest

from oracle import cpu
from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

N = 1 << 22
RANGE_BITS = 16                     # ORDER_RANGE_BITS: first row ids per range of the ordering kernel
RANGE_CAP = 8192                    # ORDER_RANGE_CAP: groups a range holds


@pytest.fixture
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this environment")
    from midoridb_amd.dev import DeviceCtx
    c = DeviceCtx(0)
    yield c
    c.close()


def _tables(n):
    kl, kr = orc.gen_keys(n, 0, n, 42, 0), orc.gen_keys(n, 0, n, 43, n // 16)
    return kl, kr, cpu.hash_join_group_count(kl, None, kr, None)


@pytest.fixture(scope="module")
def std():
    """the 2^22-row tables and what the oracle says of them: computed once, read only"""
    return _tables(N)


def _np(t):
    return t.cpu().numpy()


def _same(res, expect):
    k, c, f, j = res
    ek, ec, ef, ej = expect
    return (j == ej and np.array_equal(_np(k), ek) and np.array_equal(_np(c), ec)
            and np.array_equal(_np(f).view(np.uint32).astype(np.int64), ef))


def _early(ctx):
    return bool(ctx.last_plan()["ranged_order"]) and ctx.last_return_was_early()


def _warm(ctx, kl, kr, expect):
    """the first call over fresh columns (not ranged: nothing known of them yet), then the second: ranged, returned early, right -> (dl, dr)"""
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    assert _same(ctx.join_group_count(dl, None, dr, None), expect)
    assert not ctx.last_return_was_early(), ctx.last_plan()
    res = ctx.join_group_count(dl, None, dr, None)
    assert ctx.last_plan()["ranged_order"] == 1 and ctx.last_return_was_early() == 1, ctx.last_plan()
    assert _same(res, expect)
    return dl, dr


def _outs(ctx, cap):
    import torch
    return (torch.full((cap,), -7, dtype=torch.int64, device=ctx.device), torch.full((cap,), -7, dtype=torch.int64, device=ctx.device),
            torch.full((cap,), -7, dtype=torch.int32, device=ctx.device))


def test_a_stream_ordered_reader_sees_the_result(ctx, std):
    """Clones queued on torch's stream right behind the return - the ordering kernel may not have started - hold the oracle's result."""
    kl, kr, expect = std
    dl, dr = _warm(ctx, kl, kr, expect)
    out = _outs(ctx, N)
    k, c, f, j = ctx.join_group_count(dl, None, dr, None, out=out)
    copies = (k.clone(), c.clone(), f.clone(), j)
    assert _early(ctx), ctx.last_plan()
    assert _same(copies, expect)


def test_two_calls_back_to_back_into_different_columns(ctx, std):
    """No synchronisation between two early returns: the second call's first fill and kernels reuse the status block and the arena that the first
    call's ordering kernel still reads - in stream order - and both results are right."""
    kl, kr, expect = std
    dl, dr = _warm(ctx, kl, kr, expect)
    out1, out2 = _outs(ctx, N), _outs(ctx, N)
    r1 = ctx.join_group_count(dl, None, dr, None, out=out1)
    e1 = _early(ctx)
    r2 = ctx.join_group_count(dl, None, dr, None, out=out2)
    e2 = _early(ctx)
    assert e1 and e2
    assert _same(r1, expect) and _same(r2, expect)


def _bunched():
    """Left keys: rows 0 ... 12287 hold the keys 0 ... 12287, the other keys of [0, n / 16) lie evenly over the rest of the table, every other row holds a
    key outside.  First right column: every key of [0, n / 16) but [2048, 12288) - 5200 groups begin in the first range of 2^16 rows; second right
    column, same length: every key of [0, n / 16) 16 times - 15400 groups begin there, more than a range holds."""
    rng = np.random.default_rng(77)
    w, bunch = N // 16, 12288
    kl = np.full(N, -1, dtype=np.int64)
    kl[:bunch] = np.arange(bunch)
    rows = bunch + (np.arange(w - bunch, dtype=np.int64) * (N - bunch)) // (w - bunch)
    kl[rows] = bunch + rng.permutation(w - bunch)
    free = np.flatnonzero(kl < 0)
    kl[free] = w + rng.permutation(N - w)[:free.size]
    keep = np.concatenate([np.arange(2048), np.arange(bunch, w)])
    kr1 = np.concatenate([np.tile(keep, N // keep.size), keep[:N % keep.size]]).astype(np.int64)
    kr2 = np.tile(np.arange(w, dtype=np.int64), 16)
    rng.shuffle(kr1)
    rng.shuffle(kr2)
    assert kr1.size == kr2.size == N and np.bincount(kr1).max() <= 31
    e1, e2 = cpu.hash_join_group_count(kl, None, kr1, None), cpu.hash_join_group_count(kl, None, kr2, None)
    assert np.bincount(e1[2] >> RANGE_BITS).max() < RANGE_CAP - 1024 < RANGE_CAP < np.bincount(e2[2] >> RANGE_BITS)[0]
    return kl, kr1, kr2, e1, e2


def test_a_retry_behind_an_early_order(ctx):
    """The right column is overwritten in place between two calls: a range of row ids now holds more groups than its region.  The ordering kernel
    is queued before the host sees that; the record-list form is queued behind it on the same stream and writes the columns again."""
    kl, kr1, kr2, e1, e2 = _bunched()
    dl, dr = _warm(ctx, kl, kr1, e1)
    first = dr.clone()
    dr.copy_(ctx.to_dev(kr2))
    res = ctx.join_group_count(dl, None, dr, None)
    plan = ctx.last_plan()
    assert plan["ranged_order"] == 0 and not ctx.last_return_was_early(), plan    # (the leaf ran again, into the record list)
    assert _same(res, e2)
    assert _same(ctx.join_group_count(dl, None, dr, None), e2)
    dr.copy_(first)
    res = ctx.join_group_count(dl, None, dr, None)
    assert _early(ctx), ctx.last_plan()
    assert _same(res, e1)


def test_output_columns_of_one_row_less_than_the_groups(ctx, std):
    """The capacity error arrives with the ordering kernel queued: nothing is written behind the columns, and the context's next call is right."""
    from midoridb_amd.dev import MDB_ORDER_FIRST, _ptr
    kl, kr, expect = std
    dl, dr = _warm(ctx, kl, kr, expect)
    cap, guard = len(expect[0]) - 1, 4096
    out = _outs(ctx, cap + guard)
    g, j = c_uint64(), c_uint64()
    rc = ctx.lib.mdb_dev_join_group_count(ctx.h, _ptr(dl), None, N, _ptr(dr), None, N, MDB_ORDER_FIRST, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), cap,
                                          byref(g), byref(j))
    assert rc != 0 and b"group output capacity" in ctx.lib.mdb_dev_last_error(ctx.h), (rc, ctx.lib.mdb_dev_last_error(ctx.h))
    for t in out:
        assert bool((t[cap:] == -7).all()), "written beyond the columns"
    res = ctx.join_group_count(dl, None, dr, None)
    assert _early(ctx), ctx.last_plan()
    assert _same(res, expect)


def test_a_partial_last_tile_and_range(ctx):
    """2^22 + 4097 rows: the last tile of both passes and the last range of row ids are partly filled."""
    kl, kr, expect = _tables(N + 4097)
    _warm(ctx, kl, kr, expect)


def test_complete_on_return_when_the_caller_has_not_opted_in(ctx, std):
    """Switched off, the same path waits for its ordering kernel as before: the same result, and the getter says so."""
    kl, kr, expect = std
    ctx.results_in_stream_order(False)
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    for call in range(2):
        res = ctx.join_group_count(dl, None, dr, None)
        assert not ctx.last_return_was_early()
        assert _same(res, expect), call
    assert ctx.last_plan()["ranged_order"] == 1, ctx.last_plan()
    ctx.results_in_stream_order(True)
    res = ctx.join_group_count(dl, None, dr, None)
    assert _early(ctx), ctx.last_plan()
    assert _same(res, expect)
