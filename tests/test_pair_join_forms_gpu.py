"""Which form of the pair join (mdb_dev_join_pairs) and of the payload joins (mdb_dev_join_payload, mdb_dev_join_payload_multi) answers a call:
the host code of midoridb_amd/csrc/mdb_dev_pairs.hip, reached through the exported operators.

Each case has a device context of its own with the profiler on and makes ONE operator call unless it says otherwise (the profiler is reset
between the calls of a case).  Every call's result is compared bit for bit with oracle.np_oracle.join_pairs (payload cells: with numpy), and
then the call is pinned: the list of its launches that are not the radix partition's (profiler names that do not start with part_, sort_,
dest_ or orderby_; those are pinned by test_partition_forms_gpu.py) as one line name=launches, the plan record's payload_form,
payload_tables, key_bits, levels, pairs_identity, samples and retries.  The expected records (EXPECT) were taken on an MI355X from the
library as it was before the host code was split into call record, status read-back and form functions; a change of the host code that
takes another form, launches one more kernel or drops one shows up as a diff of such a record.

Sizes: the smallest that reach each branch, nothing above 2^21 + 5 rows per table."""
import numpy as np
import pytest

from midoridb_amd import dev as D
from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

PREFIXES = ("part_", "sort_", "dest_", "orderby_")
TINY_ROWS = 2048                    # TINY_ROWS of mdb_dev_join_internal.h: GC_THREADS * LEAF_BATCH
TINY_PAIRS_CAP = 65536              # TINY_PAIRS_CAP of mdb_dev_pairs.hip
N = 1 << 20
ROW_ORDER = {"MDB_ROWJOIN": "2"}    # the row-order payload form for left tables below 2^24 rows too


@pytest.fixture
def ctx():
    """a device context of this test's own, profiling on: prof_read() then holds what this test launched and nothing else"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this environment")
    c = D.DeviceCtx(0)
    c.prof_enable(True)
    yield c
    c.close()


def _np(t):
    return t.cpu().numpy()


def pin(ctx):
    """the record of the call just made: (launch line, payload_form, payload_tables, key_bits, levels, pairs_identity, samples, retries);
    resets the profiler for the case's next call"""
    line = " ".join("%s=%d" % (name, cnt) for name, (cnt, _ms) in sorted(ctx.prof_read().items()) if cnt and not name.startswith(PREFIXES))
    p = ctx.last_plan()
    assert bool(p["pairs_identity"]) == ctx.last_pairs_identity()
    ctx.prof_reset()
    return (line, p["payload_form"], p["payload_tables"], p["key_bits"], p["levels"], p["pairs_identity"], p["samples"], p["retries"])


def _launched(record):
    return sum(int(item.split("=")[1]) for item in record[0].split())


def _sampled_rows(n):
    """the rows of an n-row column that the operators' key sample (k_key_sample) reads: gc_sample_pos() of mdb_dev_join_internal.h (fmix64
    of GC_NARROW_SAMPLE = 4096 multiples of the golden ratio, mod n), restated"""
    k = np.arange(1, 4097, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xFF51AFD7ED558CCD)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xC4CEB9FE1A85EC53)
    k ^= k >> np.uint64(33)
    return set((k % np.uint64(n)).tolist())


# ------------------------------------------------------------------------------------------------ operator calls, each checked

def _check_pairs(got, kl, nl, kr, nr):
    el, er = orc.join_pairs(kl, nl, kr, nr)
    l, r = got
    assert l.numel() == len(el) and r.numel() == len(er), (l.numel(), len(el))
    assert np.array_equal(_np(l).view(np.uint32).astype(np.int64), el) and np.array_equal(_np(r).view(np.uint32).astype(np.int64), er)
    return _np(l).view(np.uint32)


def _pairs(ctx, kl, kr, nl=None, nr=None):
    _check_pairs(ctx.join_pairs(ctx.to_dev(kl), ctx.nullbits_dev(nl), ctx.to_dev(kr), ctx.nullbits_dev(nr)), kl, nl, kr, nr)
    return pin(ctx)


def _partner_rows(kl, kr):
    """row of kr that holds each key of kl (kr unique, every key of kl present)"""
    assert len(np.unique(kr)) == len(kr)
    order = np.argsort(kr, kind="stable")
    pos = np.searchsorted(kr[order], kl)
    assert np.array_equal(kr[order][pos], kl)
    return order[pos]


def _cells_equal(got, pay, rows):
    assert got is not None and len(got) == len(pay)
    for g, p in zip(got, pay):
        assert np.array_equal(_np(g).view(np.int64), p[rows].view(np.int64))


def _payload_tables(seed, span_bits, cells):
    """2^20 left rows, unique right keys drawn from a span of 2^span_bits values, every left key present on the right"""
    rng = np.random.default_rng(seed)
    kr = np.unique(rng.integers(0, 1 << span_bits, N, dtype=np.int64)) - 12345
    rng.shuffle(kr)
    kl = kr[rng.integers(0, len(kr), N)]
    pay = [rng.integers(-2**62, 2**62, len(kr), dtype=np.int64), rng.standard_normal(len(kr))][:cells]
    return rng, kl, kr, pay


def _payload_served(ctx, kl, kr, pay, form, dl=None, dr=None):
    got = ctx.join_payload(ctx.to_dev(kl) if dl is None else dl, None, ctx.to_dev(kr) if dr is None else dr, None, [ctx.to_dev(p) for p in pay])
    assert got is not None and ctx.last_plan()["payload_form"] == form, ctx.last_plan()
    _cells_equal(got, pay, _partner_rows(kl, kr))
    return pin(ctx)


def _payload_declined(ctx, kl, kr, pay, nl=None, dl=None, dr=None):
    got = ctx.join_payload(ctx.to_dev(kl) if dl is None else dl, ctx.nullbits_dev(nl), ctx.to_dev(kr) if dr is None else dr, None,
                           [ctx.to_dev(p) for p in pay])
    assert got is None and ctx.last_plan()["payload_form"] == 0, ctx.last_plan()
    return pin(ctx)


# ------------------------------------------------------------------------------------------------ join_pairs cases

def c_tiny(ctx):
    """5 x 7 rows, a duplicate on each side, one NULL each: one workgroup"""
    kl = np.array([3, 9, 3, 4, 1], dtype=np.int64)
    kr = np.array([9, 3, 8, 3, 1, 4, 9], dtype=np.int64)
    nl, nr = np.zeros(5, dtype=bool), np.zeros(7, dtype=bool)
    nl[4], nr[6] = True, True
    return [_pairs(ctx, kl, kr, nl, nr)]


def c_tiny_overflow(ctx):
    """TINY_ROWS x TINY_ROWS rows of one key: more pairs than the one-workgroup kernel's buffers hold, the general path answers.  Checked
    against the closed form (pair p = (p // TINY_ROWS, p % TINY_ROWS)), not the O(n^2) oracle"""
    k = np.full(TINY_ROWS, 42, dtype=np.int64)
    assert TINY_ROWS * TINY_ROWS > TINY_PAIRS_CAP
    l, r = ctx.join_pairs(ctx.to_dev(k), None, ctx.to_dev(k), None)
    assert l.numel() == r.numel() == TINY_ROWS * TINY_ROWS
    p = np.arange(TINY_ROWS * TINY_ROWS, dtype=np.int64)
    for part in (slice(0, 1000), slice(-1000, None)):
        assert np.array_equal(_np(l[part]).astype(np.int64), p[part] // TINY_ROWS) and np.array_equal(_np(r[part]).astype(np.int64), p[part] % TINY_ROWS)
    return [pin(ctx)]


def _narrow_tables():
    rng = np.random.default_rng(23)
    n_l, n_r = 600_000, 500_000
    kr = rng.permutation(3 * n_r)[:n_r].astype(np.int64) - n_r
    kl = rng.integers(-n_r, 2 * n_r, n_l, dtype=np.int64)
    return kl, kr, rng.random(n_l) < 0.02


def c_unique_right_narrow(ctx):
    """unique right keys, 2 % NULL left keys, 1.1 * 10^6 rows in all, a window of 2^21 key values: the one-level form; with MDB_ONE_LEVEL=0
    (unique_right_narrow_two_levels) two levels of hash | row id words, one record per pair, the ordering sort"""
    kl, kr, nl = _narrow_tables()
    return [_pairs(ctx, kl, kr, nl)]


def c_unique_right_row_ids(ctx):
    """... with the narrow forms switched off: row-id arrays beside 64-bit hashes"""
    ctx.set_narrow_keys(0)
    kl, kr, nl = _narrow_tables()
    return [_pairs(ctx, kl, kr, nl)]


def c_one_level(ctx):
    """two permutations of 2^20: one partition level, match[] compaction; every left row has its one partner"""
    rng = np.random.default_rng(24)
    kl, kr = rng.permutation(N).astype(np.int64), rng.permutation(N).astype(np.int64)
    l = _check_pairs(ctx.join_pairs(ctx.to_dev(kl), None, ctx.to_dev(kr), None), kl, None, kr, None)
    assert ctx.last_pairs_identity() and np.array_equal(l, np.arange(N, dtype=np.uint32))
    return [pin(ctx)]


def c_one_level_dup_right(ctx):
    """... with one right key twice: the one-level form says so, the dup side is remembered, the swapped unique-left call answers through the
    pair sort.  The second call over the same columns skips the attempt that failed"""
    rng = np.random.default_rng(24)
    kl, kr = rng.permutation(N).astype(np.int64), rng.permutation(N).astype(np.int64)
    kr[7] = kr[8]
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    out = []
    for _call in range(2):
        _check_pairs(ctx.join_pairs(dl, None, dr, None), kl, None, kr, None)
        assert not ctx.last_pairs_identity()
        out.append(pin(ctx))
    assert _launched(out[1]) < _launched(out[0]), out
    return out


def c_unique_left_few_pairs(ctx):
    """unique left keys, a right key twice, 1000 pairs: fewer than the pair sort takes (SORT_PACK_MIN_ROWS = 2^18 of mdb_dev_sort.hip:
    mdb_sort_pairs declines) - a permutation sorted by left row id and two gathers"""
    rng = np.random.default_rng(33)
    n = 300_000
    kl = rng.permutation(n).astype(np.int64)
    kr = 10**6 + np.arange(n, dtype=np.int64)
    hit = rng.choice(n, 1000, replace=False)
    kr[hit] = rng.choice(n, 1000, replace=False)
    kr[hit[1]] = kr[hit[0]]
    return [_pairs(ctx, kl, kr)]


def c_general(ctx):
    """duplicates on both sides: count / scan / emit over the histogram-free layout"""
    rng = np.random.default_rng(25)
    return [_pairs(ctx, rng.integers(0, 800_000, 600_000, dtype=np.int64), rng.integers(0, 800_000, 1_000_000, dtype=np.int64))]


def c_general_stable(ctx):
    """... and one key with 5000 right rows: redone with the right side in row-id order (the stable exact layout)"""
    rng = np.random.default_rng(26)
    n_l, n_r = 600_000, 1_000_000
    kl = rng.integers(0, 800_000, n_l, dtype=np.int64)
    kr = rng.integers(0, 800_000, n_r, dtype=np.int64)
    kl[rng.choice(n_l, 300, replace=False)] = 77
    kr[rng.choice(n_r, 5000, replace=False)] = 77
    return [_pairs(ctx, kl, kr)]


def c_no_pairs(ctx):
    """disjoint key sets of 2^20 rows each: J = 0"""
    rng = np.random.default_rng(34)
    return [_pairs(ctx, rng.permutation(N).astype(np.int64), N + rng.permutation(N).astype(np.int64))]


def c_empty_tables(ctx):
    """n_l = 0, then n_r = 0: nothing is launched"""
    k, none = np.arange(10, dtype=np.int64), np.zeros(0, dtype=np.int64)
    out = [_pairs(ctx, none, k), _pairs(ctx, k, none)]
    assert out[0][0] == out[1][0] == ""
    return out


def c_remembered_narrow_meets_wide_key(ctx):
    """the narrow decision is remembered by the columns; then one left key of the same device tensor becomes 2^40"""
    kl, kr, nl = _narrow_tables()
    dl, dn, dr = ctx.to_dev(kl), ctx.nullbits_dev(nl), ctx.to_dev(kr)
    _check_pairs(ctx.join_pairs(dl, dn, dr, None), kl, nl, kr, None)
    out = [pin(ctx)]
    row = int(np.flatnonzero(~nl)[1000])
    kl[row] = 1 << 40
    dl[row] = 1 << 40
    _check_pairs(ctx.join_pairs(dl, dn, dr, None), kl, nl, kr, None)
    return out + [pin(ctx)]


# ------------------------------------------------------------------------------------------------ join_payload cases

def _served(seed, span_bits, cells, form):
    def case(ctx):
        _, kl, kr, pay = _payload_tables(seed, span_bits, cells)
        return [_payload_served(ctx, kl, kr, pay, form)]
    return case


def _inside_and_absent(kr):
    """a key inside the right table's key range that the table does not hold"""
    have = set(kr.tolist())
    return next(v for v in range(int(kr.min()) + 1000, int(kr.max())) if v not in have)


def c_left_key_without_partner(ctx):
    """... and the verdict is remembered: the second call over the same columns launches nothing"""
    _, kl, kr, pay = _payload_tables(35, 21, 1)
    kl[5] = _inside_and_absent(kr)
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    out = [_payload_declined(ctx, kl, kr, pay, dl=dl, dr=dr), _payload_declined(ctx, kl, kr, pay, dl=dl, dr=dr)]
    assert out[0][0] != "" and out[1][0] == "", out
    return out


def c_right_key_twice(ctx):
    _, kl, kr, pay = _payload_tables(36, 21, 1)
    kr = np.concatenate([kr, kr[:1]])
    return [_payload_declined(ctx, kl, kr, [np.concatenate([pay[0], pay[0][:1]])])]


def c_null_left_key(ctx):
    _, kl, kr, pay = _payload_tables(37, 21, 1)
    nl = np.zeros(N, dtype=bool)
    nl[77] = True
    return [_payload_declined(ctx, kl, kr, pay, nl=nl)]


def c_remembered_window_wrong(ctx):
    """a served call; then both key tensors are overwritten in place with keys from a window 2^32 higher: the remembered window meets keys
    outside it, is forgotten, and the second attempt - a fresh sample - serves the call"""
    _, kl, kr, pay = _payload_tables(38, 21, 1)
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    out = [_payload_served(ctx, kl, kr, pay, 1, dl=dl, dr=dr)]
    kl2, kr2 = kl + (1 << 32), kr + (1 << 32)
    dl.copy_(ctx.to_dev(kl2))
    dr.copy_(ctx.to_dev(kr2))
    return out + [_payload_served(ctx, kl2, kr2, pay, 1, dl=dl, dr=dr)]


def c_key_outside_sampled_window(ctx):
    """nothing remembered; one left key of 2^20 lies far outside the rest, in a row the key sample does not read: not served.  The next call,
    on fresh columns, is served and right"""
    _, kl, kr, pay = _payload_tables(39, 21, 1)
    row = next(r for r in range(5000, 6000) if r not in _sampled_rows(N))
    assert row not in _sampled_rows(len(kl))
    kl[row] = 1 << 40
    out = [_payload_declined(ctx, kl, kr, pay)]
    _, kl, kr, pay = _payload_tables(40, 21, 1)
    return out + [_payload_served(ctx, kl, kr, pay, 1)]


def _multi(ctx, drop_a_key):
    rng = np.random.default_rng(41)
    kb = np.unique(rng.integers(0, 1 << 21, N, dtype=np.int64)) - 12345
    rng.shuffle(kb)
    kc = rng.permutation(kb)
    kl = kb[rng.integers(0, len(kb), N)]
    if drop_a_key:
        kc = kc[kc != kl[9]]
    pb, pc = rng.integers(-2**62, 2**62, len(kb), dtype=np.int64), rng.standard_normal(len(kc))
    got = ctx.join_payload_multi(ctx.to_dev(kl), [(ctx.to_dev(kb), [ctx.to_dev(pb)]), (ctx.to_dev(kc), [ctx.to_dev(pc)])], int(kb.min()), int(kb.max()))
    if drop_a_key:
        assert got is None and ctx.last_plan()["payload_form"] == 0, ctx.last_plan()
    else:
        assert got is not None and ctx.last_plan()["payload_form"] == 3, ctx.last_plan()
        _cells_equal(got[0], [pb], _partner_rows(kl, kb))
        _cells_equal(got[1], [pc], _partner_rows(kl, kc))
    return [pin(ctx)]


def c_multi_served(ctx):
    return _multi(ctx, False)


def c_multi_second_table_lacks_a_key(ctx):
    return _multi(ctx, True)


CASES = {
    "tiny": ({}, c_tiny),
    "tiny_overflow": ({}, c_tiny_overflow),
    "unique_right_narrow": ({}, c_unique_right_narrow),
    "unique_right_narrow_two_levels": ({"MDB_ONE_LEVEL": "0"}, c_unique_right_narrow),
    "unique_right_row_ids": ({}, c_unique_right_row_ids),
    "one_level": ({}, c_one_level),
    "one_level_dup_right": ({}, c_one_level_dup_right),
    "unique_left_few_pairs": ({}, c_unique_left_few_pairs),
    "general": ({}, c_general),
    "general_stable": ({}, c_general_stable),
    "no_pairs": ({}, c_no_pairs),
    "empty_tables": ({}, c_empty_tables),
    "remembered_narrow_meets_wide_key": ({}, c_remembered_narrow_meets_wide_key),
    "payload_one_level_one_cell": ({}, _served(28, 21, 1, 1)),
    "payload_one_level_two_cells": ({}, _served(29, 21, 2, 1)),
    "payload_two_levels_one_cell": ({}, _served(30, 27, 1, 2)),
    "payload_two_levels_two_cells": ({}, _served(31, 29, 2, 2)),
    "payload_row_order_one_cell": (ROW_ORDER, _served(28, 21, 1, 3)),
    "payload_row_order_two_cells": (ROW_ORDER, _served(29, 21, 2, 3)),
    "payload_left_key_without_partner": ({}, c_left_key_without_partner),
    "payload_right_key_twice": ({}, c_right_key_twice),
    "payload_null_left_key": ({}, c_null_left_key),
    "payload_remembered_window_wrong": ({}, c_remembered_window_wrong),
    "payload_key_outside_sampled_window": ({}, c_key_outside_sampled_window),
    "payload_multi_served": (ROW_ORDER, c_multi_served),
    "payload_multi_second_table_lacks_a_key": (ROW_ORDER, c_multi_second_table_lacks_a_key),
}

# per case and call: (launches, payload_form, payload_tables, key_bits, levels, pairs_identity, samples, retries)
EXPECT = {
    "tiny": [("tiny_join_pairs=1", 0, 0, 0, 0, 0, 0, 0)],
    "tiny_overflow": [("leaf_pairs_count=1 leaf_pairs_emit=1 leaf_pairs_unique=1 scan_small=5 tiny_join_pairs=1", 0, 0, 0, 0, 0, 0, 0)],
    "unique_right_narrow": [("key_sample=1 leaf_pairs_wide=1 match_count=1 match_emit=1 scan_small=1", 0, 0, 0, 0, 0, 1, 0)],
    "unique_right_narrow_two_levels": [("key_sample=1 leaf_pairs_unique=1 order_leaf=1 scan_apply=1 scan_reduce=1 scan_spine=1", 0, 0, 0, 0, 0, 1, 0)],
    "unique_right_row_ids": [("leaf_pairs_unique=1 order_leaf=1 scan_apply=1 scan_reduce=1 scan_spine=1", 0, 0, 0, 0, 0, 0, 0)],
    "one_level": [("key_sample=1 leaf_pairs_wide=1 match_count=1 match_emit=1 scan_small=1", 0, 0, 0, 0, 1, 1, 0)],
    "one_level_dup_right": [("key_sample=2 leaf_pairs_wide=2 match_count=2 match_emit=1 pairs_leaf=1 pairs_pack=1 scan_small=3", 0, 0, 0, 0, 0, 2, 0),
        ("leaf_pairs_wide=1 match_count=1 match_emit=1 pairs_leaf=1 pairs_pack=1 scan_small=2", 0, 0, 0, 0, 0, 0, 0)],
    "unique_left_few_pairs": [("gather32=2 leaf_pairs_unique=2 order_leaf=1 scan_apply=5 scan_reduce=5 scan_spine=5 widen32=1", 0, 0, 0, 0, 0, 0, 0)],
    "general": [("key_sample=2 leaf_pairs_count=1 leaf_pairs_emit=1 leaf_pairs_wide=2 match_count=2 scan_apply=1 scan_reduce=1 scan_small=2 scan_spine=1", 0, 0, 0, 0, 0, 2, 0)],
    "general_stable": [("key_sample=2 leaf_pairs_count=2 leaf_pairs_emit=1 leaf_pairs_wide=2 match_count=2 scan_apply=4 scan_reduce=4 scan_small=6 scan_spine=4", 0, 0, 0, 0, 0, 2, 0)],
    "no_pairs": [("key_sample=1 leaf_pairs_wide=1 match_count=1 scan_small=1", 0, 0, 0, 0, 0, 1, 0)],
    "empty_tables": [("", 0, 0, 0, 0, 0, 0, 0),
        ("", 0, 0, 0, 0, 0, 0, 0)],
    "remembered_narrow_meets_wide_key": [("key_sample=1 leaf_pairs_wide=1 match_count=1 match_emit=1 scan_small=1", 0, 0, 0, 0, 0, 1, 0),
        ("leaf_pairs_unique=2 leaf_pairs_wide=1 match_count=1 order_leaf=1 scan_apply=1 scan_reduce=1 scan_small=1 scan_spine=1", 0, 0, 0, 0, 0, 0, 0)],
    "payload_one_level_one_cell": [("key_sample=1 leaf_pairs_payload=1", 1, 1, 22, 1, 0, 1, 0)],
    "payload_one_level_two_cells": [("key_sample=1 leaf_pairs_payload=2", 1, 1, 22, 1, 0, 1, 0)],
    "payload_two_levels_one_cell": [("key_sample=1 leaf_pairs_payload=1", 2, 1, 28, 2, 0, 1, 0)],
    "payload_two_levels_two_cells": [("key_sample=1 leaf_pairs_payload=1", 2, 1, 30, 2, 0, 1, 0)],
    "payload_row_order_one_cell": [("key_sample=1 rowjoin_leaf=1 rowjoin_offsets=2 rowjoin_place=1 rowjoin_tile_sort=1 rowjoin_tile_sort_r=2", 3, 1, 22, 1, 0, 1, 0)],
    "payload_row_order_two_cells": [("key_sample=1 rowjoin_leaf=1 rowjoin_offsets=2 rowjoin_place=1 rowjoin_tile_sort=1 rowjoin_tile_sort_r=2", 3, 1, 22, 1, 0, 1, 0)],
    "payload_left_key_without_partner": [("key_sample=1 leaf_pairs_payload=1", 0, 0, 0, 0, 0, 1, 0),
        ("", 0, 0, 0, 0, 0, 0, 0)],
    "payload_right_key_twice": [("key_sample=1 leaf_pairs_payload=1", 0, 0, 0, 0, 0, 1, 0)],
    "payload_null_left_key": [("key_sample=1 leaf_pairs_payload=1", 0, 0, 0, 0, 0, 1, 0)],
    "payload_remembered_window_wrong": [("key_sample=1 leaf_pairs_payload=1", 1, 1, 22, 1, 0, 1, 0),
        ("key_sample=1 leaf_pairs_payload=2", 1, 1, 22, 1, 0, 1, 0)],
    "payload_key_outside_sampled_window": [("key_sample=1 leaf_pairs_payload=1", 0, 0, 0, 0, 0, 1, 0),
        ("key_sample=1 leaf_pairs_payload=1", 1, 1, 22, 1, 0, 1, 0)],
    "payload_multi_served": [("rowjoin_leaf=1 rowjoin_offsets=3 rowjoin_place=1 rowjoin_tile_sort=1 rowjoin_tile_sort_r=4", 3, 2, 21, 1, 0, 0, 0)],
    "payload_multi_second_table_lacks_a_key": [("rowjoin_leaf=1 rowjoin_offsets=3 rowjoin_place=1 rowjoin_tile_sort=1 rowjoin_tile_sort_r=4", 0, 0, 0, 0, 0, 0, 0)],
}


@pytest.mark.parametrize("case", list(CASES))
def test_pair_join_form(ctx, monkeypatch, case):
    env, call = CASES[case]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    got = call(ctx)
    print("RECORD %r: %r," % (case, got))
    assert got == EXPECT[case], (case, got, EXPECT[case])
