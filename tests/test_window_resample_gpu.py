"""A remembered key sample whose window the column has outgrown: the three operators that take a compact window from the key sample alone
(the any-order join + GROUP BY, mdb_dev_group_count_keys, and mdb_dev_group_count's band / tile sort) run the sample-window-form loop of
midoridb_amd/csrc/mdb_dev_keyform.hip.  On a key outside the window of a REMEMBERED sample they take the sample again, once, and answer from
the new window.

Each case calls its operator three times on the same device buffers (the memo is keyed by the columns' addresses): the first call takes the
sample, the second is served the remembered one (last_plan().samples == 0), and before the third one key far outside the window
(the column's maximum + 2^22, the padded window being at most 2^21 values wide) is written in place - at a row the key sample reads, so
that the second sample sees it and the widened window serves the call.  Every result equals the numpy oracle's."""
import numpy as np
import pytest

from midoridb_amd import dev as D
from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

LO = 10**12 + 12345                 # far from the int32 range: the window is the compact one
SPAN = 1 << 20
N_ONE = 1 << 21                     # rows of the one-column cases (the forms' floor)
N_SIDE = 1 << 20                    # rows per table of the join (the form needs 2^21 in all)


@pytest.fixture
def ctx():
    """a device context of this test's own: nothing remembered, no distrust left over from another test"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this environment")
    c = D.DeviceCtx(0)
    yield c
    c.close()


def _np(t):
    return t.cpu().numpy()


def _first_sampled_row(n):
    """row of sample 0 of an n-row column: gc_sample_pos(0, n) of midoridb_amd/csrc/mdb_dev_join_internal.h"""
    return int(orc.fmix64(np.array([0x9E3779B97F4A7C15], dtype=np.uint64))[0] % np.uint64(n))


def _sorted_pairs(keys, counts):
    o = np.argsort(keys, kind="stable")
    return keys[o], counts[o]


def _join_unordered(ctx, cols, host):
    k, c, j = ctx.join_group_count_unordered(cols[0], None, cols[1], None)
    ek, ec, _, ej = orc.join_group_count(host[0], None, host[1], None)
    gk, gc = _sorted_pairs(_np(k), _np(c))
    wk, wc = _sorted_pairs(ek, ec)
    assert j == ej and np.array_equal(gk, wk) and np.array_equal(gc, wc)
    assert ctx.last_join_unordered()


def _group_keys(ctx, cols, host):
    got = ctx.group_count_keys(cols[0], None)
    assert got is not None
    gk, gc = _sorted_pairs(_np(got[0]), _np(got[1]))
    vals, cnt = np.unique(host[0], return_counts=True)
    assert np.array_equal(gk, vals) and np.array_equal(gc, cnt)


def _group_ordered(ctx, cols, host):
    f, c = ctx.group_count(cols[0], None)
    ef, ec = orc.group_count(host[0], None)
    assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), ef) and np.array_equal(_np(c), ec)


CASES = {
    # operator: (call + check, rows per column, the column the stale key is written into)
    "join_group_count_unordered": (_join_unordered, (N_SIDE, N_SIDE), 1),
    "group_count_keys": (_group_keys, (N_ONE,), 0),
    "group_count": (_group_ordered, (N_ONE,), 0),
}


@pytest.mark.parametrize("op", list(CASES))
def test_stale_remembered_window_is_sampled_again_once(ctx, op):
    call, rows, stale_col = CASES[op]
    rng = np.random.default_rng(len(op))
    host = [rng.integers(LO, LO + SPAN, n, dtype=np.int64) for n in rows]
    cols = [ctx.to_dev(h) for h in host]
    samples = []
    for round_ in range(3):
        if round_ == 2:
            row, far = _first_sampled_row(rows[stale_col]), int(host[stale_col].max()) + (1 << 22)
            host[stale_col][row] = far
            cols[stale_col][row] = far
        call(ctx, cols, host)
        samples.append(ctx.last_plan()["samples"])
        print("%s call %d: samples %d, retries %d" % (op, round_, samples[-1], ctx.last_plan()["retries"]))
    assert samples[0] >= 1, samples
    assert samples[1] == 0, samples         # served the remembered sample
    assert samples[2] >= 1, samples         # the remembered window no longer holds the column: sampled again
