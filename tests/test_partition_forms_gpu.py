"""Every launch site of the radix partition's host code (midoridb_amd/csrc/mdb_dev_partition.hip), reached through the exported operators.

Each case has a device context of its own with the profiler on, makes ONE operator call (records_4_bytes: two - its form rests on what the
first call learned), compares the result with the numpy oracle (or with numpy itself) and then asserts the whole list of partition
launches of that call: for every profiler name that starts with part_, sort_, dest_ or orderby_ the number of launches (prof_read) and the
kernel instances launched under it (prof_symbols).  The expected lists (EXPECT) were recorded on an MI355X and are written as the partition
calls an operator makes; a change of the partition's host code that picks another instance, launches one more kernel or drops one shows up
as a diff of such a list.  The last test checks that, taken together, the cases reach every (name, instance) pair the host code can launch
(REACHED); the one launch site that no exported entry point reaches is named beside it with the reason (NOT_REACHED).

Sizes.  Nothing above 2^21 + 5 rows per table.  The join + GROUP BY operator takes the compact narrow form from 2^20 rows in all, its
one-level plan from 2^21 rows in all (key windows of 2^15 ... 2^23 values), and two partition levels need more than 1.5 * 2^18 left rows:
the two-level cases use 2^19 + 5 rows per table, the one-level ones 2^20 + 5."""
import numpy as np
import pytest

from midoridb_amd import dev as D
from oracle import np_oracle as orc

pytestmark = pytest.mark.gpu

PREFIXES = ("part_", "sort_", "dest_", "orderby_")
TILE2 = 8192
N2 = 64 * TILE2 + 5                 # rows per table of the two-level join + GROUP BY cases (2^20 rows in all)
N1 = 128 * TILE2 + 5                # ... of the one-level cases (2^21 rows in all)
W = 1 << 16                         # pruned cases: the right table's keys lie in [0, W), the left table's in [0, 16 * W)


@pytest.fixture
def ctx():
    """a device context of this test's own, profiling on: prof_read() / prof_symbols() then hold what this test launched and nothing else"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this environment")
    c = D.DeviceCtx(0)
    c.prof_enable(True)
    yield c
    c.close()


def _np(t):
    return t.cpu().numpy()


def _short(symbol):
    """k_part_scatter<pf_key_cf> -> pf_key_cf; every other kernel by its name"""
    return symbol[len("k_part_scatter<"):-1] if symbol.startswith("k_part_scatter<") else symbol.replace(" ", "")


def launches(ctx):
    """the partition launches of this context as one line: name=launches:instance+instance ... for every profiler name of PREFIXES, sorted"""
    out = []
    for name, (cnt, _ms) in sorted(ctx.prof_read().items()):
        if cnt and name.startswith(PREFIXES):
            out.append("%s=%d:%s" % (name, cnt, "+".join(sorted(_short(x) for x in ctx.prof_symbols(name)))))
    return " ".join(out)


# ------------------------------------------------------------------------------------------------ data

def _right(rng, n_r, width=W):
    kr = rng.integers(0, width, n_r, dtype=np.int64)
    kr[0], kr[1] = 0, width - 1
    return kr


def _left(rng, n_l, width=W, keep=1 / 16):
    """keys over 16 x the right table's range, about `keep` of them inside it"""
    kl = width + rng.integers(0, 15 * width, n_l, dtype=np.int64)
    inside = rng.random(n_l) < keep
    kl[inside] = rng.integers(0, width, int(inside.sum()), dtype=np.int64)
    return kl


def _perms(rng, n):
    return rng.permutation(n).astype(np.int64) + 77, rng.permutation(n).astype(np.int64) + 77


# ------------------------------------------------------------------------------------------------ operator calls, each checked

def _gc(ctx, kl, kr, nl=None, nr=None, dl=None):
    ek, ec, ef, ej = orc.join_group_count(kl, nl, kr, nr)
    k, c, f, j = ctx.join_group_count(ctx.to_dev(kl) if dl is None else dl, ctx.nullbits_dev(nl), ctx.to_dev(kr), ctx.nullbits_dev(nr))
    assert j == ej, (j, ej)
    assert np.array_equal(_np(k), ek) and np.array_equal(_np(c), ec)
    assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), ef)


def _gc_i32(ctx, kl, kr):
    import torch
    ek, ec, ef, ej = orc.join_group_count(kl, None, kr, None)
    dl, dr = torch.from_numpy(kl.astype(np.int32)).to(ctx.device), torch.from_numpy(kr.astype(np.int32)).to(ctx.device)
    k, c, f, j = ctx.join_group_count_i32(dl, dr)
    assert j == ej and np.array_equal(_np(k), ek) and np.array_equal(_np(c), ec)
    assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), ef)


def _gc_unordered(ctx, kl, kr):
    ek, ec, _, ej = orc.join_group_count(kl, None, kr, None)
    k, c, j = ctx.join_group_count_unordered(ctx.to_dev(kl), None, ctx.to_dev(kr), None)
    got = dict(zip(_np(k).tolist(), _np(c).tolist()))
    assert len(got) == k.numel() and got == dict(zip(ek.tolist(), ec.tolist())) and j == ej
    assert ctx.last_join_unordered()


def _gc_multi(ctx, kl, rights):
    k, c, f, j = ctx.join_group_count_multi(ctx.to_dev(kl), None, [(ctx.to_dev(r), None) for r in rights])
    cnt = np.ones(len(kl), dtype=np.int64)
    for r in rights:
        vals, n = np.unique(r, return_counts=True)
        pos = np.clip(np.searchsorted(vals, kl), 0, len(vals) - 1)
        cnt *= np.where(vals[pos] == kl, n[pos], 0)
    keys, first, inv = np.unique(kl, return_index=True, return_inverse=True)
    tot = np.bincount(inv, weights=cnt.astype(np.float64)).astype(np.int64)
    keep = tot > 0
    o = np.argsort(first[keep], kind="stable")
    assert np.array_equal(_np(k), keys[keep][o]) and np.array_equal(_np(c), tot[keep][o]) and j == int(tot.sum())
    assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), first[keep][o])


def _group(ctx, k):
    ef, ec = orc.group_count(k, None)
    f, c = ctx.group_count(ctx.to_dev(k), None)
    assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), ef) and np.array_equal(_np(c), ec)


def _pairs(ctx, kl, kr, nl=None, nr=None):
    el, er = orc.join_pairs(kl, nl, kr, nr)
    l, r = ctx.join_pairs(ctx.to_dev(kl), ctx.nullbits_dev(nl), ctx.to_dev(kr), ctx.nullbits_dev(nr))
    assert l.numel() == len(el)
    assert np.array_equal(_np(l).astype(np.int64), el) and np.array_equal(_np(r).astype(np.int64), er)


def _payload(ctx, kl, kr, pay, form):
    """a foreign-key join: every left row has exactly one partner, whose cells it receives"""
    vals = np.sort(kr)
    assert len(np.unique(kr)) == len(kr)
    er = np.argsort(kr, kind="stable")[np.searchsorted(vals, kl)]
    got = ctx.join_payload(ctx.to_dev(kl), None, ctx.to_dev(kr), None, [ctx.to_dev(p) for p in pay])
    assert got is not None and ctx.last_plan()["payload_form"] == form, ctx.last_plan()
    for g, p in zip(got, pay):
        assert np.array_equal(_np(g).view(np.int64), p[er].view(np.int64))


def _sort(ctx, v):
    perm = _np(ctx.sort_perm([(ctx.to_dev(v), None, None, D.T_INT64, False)], len(v))).view(np.uint32)
    assert np.array_equal(perm, np.argsort(v, kind="stable"))


def _distinct(ctx, cols):
    n = len(cols[0])
    sel = _np(ctx.distinct_sel([(ctx.to_dev(c), None, None, D.T_INT64, False) for c in cols], n)).view(np.uint32)
    _, first = np.unique(np.stack(cols, axis=1), axis=0, return_index=True)
    assert np.array_equal(sel, np.sort(first))


def _group_multi(ctx, cols):
    n = len(cols[0])
    f, c = ctx.group_count_multi([(ctx.to_dev(x), None, None, D.T_INT64, False) for x in cols], n)
    _, first, cnt = np.unique(np.stack(cols, axis=1), axis=0, return_index=True, return_counts=True)
    o = np.argsort(first, kind="stable")
    assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), first[o]) and np.array_equal(_np(c), cnt[o])


def _by_dest(ctx, k, nl, n_dest, with_rid, keys32):
    ek, ec = orc.partition_by_dest(k, nl, n_dest)
    res = ctx.partition_by_dest(ctx.to_dev(k), ctx.nullbits_dev(nl), n_dest, with_rid=with_rid, keys32=keys32)
    out, counts = res[0], res[1]
    assert counts == ec.tolist()
    got = _np(out).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(ec)])
    for d in range(n_dest):
        assert np.array_equal(np.sort(got[off[d]:off[d + 1]]), np.sort(ek[off[d]:off[d + 1]]))
    if with_rid:
        r = _np(res[2]).view(np.uint32)
        assert np.array_equal(k[r], got) and len(np.unique(r)) == len(r) and not nl[r].any()


# ------------------------------------------------------------------------------------------------ the cases

def c_two_levels(ctx):
    _gc(ctx, *_perms(np.random.default_rng(1), N2))


def c_two_levels_nulls(ctx):
    rng = np.random.default_rng(2)
    kl, kr = _perms(rng, N2)
    _gc(ctx, kl, kr, rng.random(N2) < 0.05, rng.random(N2) < 0.05)


def c_two_levels_pruned(ctx):
    rng = np.random.default_rng(3)
    _gc(ctx, _left(rng, N2), _right(rng, N2))
    assert ctx.last_plan()["levels"] == 2 and ctx.last_plan()["minmax_pruned"], ctx.last_plan()


def c_one_level(ctx):
    _gc(ctx, *_perms(np.random.default_rng(4), N1))
    assert ctx.last_plan()["levels"] == 1, ctx.last_plan()


def c_one_level_off(ctx):
    _gc(ctx, *_perms(np.random.default_rng(4), N1))
    assert ctx.last_plan()["levels"] == 2, ctx.last_plan()


def c_records_folded(ctx):
    """2^21 + 5 left rows: the ordering of the group records by first row takes two levels, whose first folds the 8-byte records into
    4-byte words (every COUNT fits beside the row id)"""
    _gc(ctx, *_perms(np.random.default_rng(40), (1 << 21) + 5))
    assert ctx.last_plan()["levels"] == 2, ctx.last_plan()


def c_records_4_bytes(ctx):
    """... and the second call over the same columns (this case makes two: the form rests on what the first one learned) has its leaf
    kernel write 4-byte records: nothing to fold"""
    rng = np.random.default_rng(41)
    kl, kr = _perms(rng, (1 << 21) + 5)
    expect = orc.join_group_count(kl, None, kr, None)
    dl, dr = ctx.to_dev(kl), ctx.to_dev(kr)
    for call in range(2):
        k, c, f, j = ctx.join_group_count(dl, None, dr, None)
        assert j == expect[3] and np.array_equal(_np(k), expect[0]) and np.array_equal(_np(c), expect[1]), call
        assert np.array_equal(_np(f).view(np.uint32).astype(np.int64), expect[2]), call


def c_one_level_pruned(ctx):
    rng = np.random.default_rng(5)
    _gc(ctx, _left(rng, N1), _right(rng, N1))
    assert ctx.last_plan()["levels"] == 1 and ctx.last_plan()["minmax_pruned"], ctx.last_plan()


def c_one_level_pruned_right_nulls(ctx):
    rng = np.random.default_rng(6)
    nr = rng.random(N1) < 0.1
    nr[:2] = False
    _gc(ctx, _left(rng, N1), _right(rng, N1), None, nr)


def c_one_level_pruned_odd_start(ctx):
    """the left column starts 8 bytes off a 16-byte boundary: only the selective first level reads it"""
    rng = np.random.default_rng(7)
    kl, kr = _left(rng, N1), _right(rng, N1)
    buf = ctx.to_dev(np.concatenate([np.zeros(1, dtype=np.int64), kl]))
    assert buf[1:].data_ptr() % 16 == 8
    _gc(ctx, kl, kr, dl=buf[1:])


def c_semijoin(ctx):
    """few right rows over the whole of the left table's range: the left table's second level drops rows through the right table's bitmap"""
    rng = np.random.default_rng(8)
    n_l = 1 << 21
    kl = rng.permutation(n_l).astype(np.int64)
    kr = rng.integers(0, n_l, 40_000, dtype=np.int64)
    _gc(ctx, kl, kr)
    assert ctx.last_plan()["semijoin"] != 0 and ctx.last_plan()["levels"] == 2, ctx.last_plan()


def c_i32_two_levels(ctx):
    _gc_i32(ctx, *_perms(np.random.default_rng(9), N2))


def c_i32_one_level(ctx):
    _gc_i32(ctx, *_perms(np.random.default_rng(10), N1))


def c_i32_pruned(ctx):
    rng = np.random.default_rng(11)
    _gc_i32(ctx, _left(rng, N2), _right(rng, N2))


def c_plain_narrow(ctx):
    """keys too sparse for the compact form (a 2^31-wide range): 32-bit hashes, hashed leaf tables"""
    rng = np.random.default_rng(12)
    kl = rng.integers(0, 2**31 - 5, N2, dtype=np.int64)
    kr = rng.choice(kl, N2)
    _gc(ctx, kl, kr)
    assert ctx.last_plan()["key_form"] == 1, ctx.last_plan()


def c_plain_narrow_pruned(ctx):
    rng = np.random.default_rng(13)
    kl = rng.integers(0, 2**31 - 5, N2, dtype=np.int64)
    kr = rng.choice(kl[kl < (2**31) // 16], N2)
    _gc(ctx, kl, kr)
    assert ctx.last_plan()["key_form"] == 1 and ctx.last_plan()["minmax_pruned"], ctx.last_plan()


def c_form64(ctx):
    """keys outside any 2^32 window: 64-bit hashes, row ids beside the left table's words"""
    rng = np.random.default_rng(14)
    kl = rng.integers(-2**62, 2**62, N2, dtype=np.int64)
    kr = rng.choice(kl, N2)
    _gc(ctx, kl, kr)
    assert ctx.last_plan()["key_form"] == 0, ctx.last_plan()


def c_form64_pruned(ctx):
    rng = np.random.default_rng(15)
    kl = rng.integers(0, 2**44, N2, dtype=np.int64)
    kr = rng.choice(kl[kl < 2**40], N2)
    _gc(ctx, kl, kr)
    assert ctx.last_plan()["key_form"] == 0 and ctx.last_plan()["minmax_pruned"], ctx.last_plan()


def c_skew_exact(ctx):
    """a key on 3 rows in 10 overflows its fixed-capacity region: the operator is redone with the exact (histogram) layout"""
    rng = np.random.default_rng(16)
    kl = np.concatenate([np.full(300_000, 7), rng.integers(0, 10**9, 700_000)]).astype(np.int64)
    kr = np.concatenate([np.full(200_000, 7), rng.integers(0, 10**9, 600_000), kl[300_000:500_000]]).astype(np.int64)
    rng.shuffle(kl)
    rng.shuffle(kr)
    _gc(ctx, kl, kr)
    assert ctx.counters()["retries"] >= 1


def c_multi(ctx):
    rng = np.random.default_rng(17)
    n = (1 << 20) + 5               # (the one-pass form of several right tables takes left tables from 2^20 rows)
    kl, kr = _perms(rng, n)
    _gc_multi(ctx, kl, [kr, rng.permutation(n).astype(np.int64)[: n - 999] + 77])
    assert ctx.last_join_multi(), ctx.last_plan()


def c_group_by(ctx):
    rng = np.random.default_rng(18)
    _group(ctx, rng.integers(0, N1 // 4, N1, dtype=np.int64))


def c_group_by_unique(ctx):
    _group(ctx, np.random.default_rng(19).permutation(N1).astype(np.int64))


def c_unordered(ctx):
    """the any-order join + GROUP BY: the sharded operator's sender and receiver at world 1"""
    _gc_unordered(ctx, *_perms(np.random.default_rng(20), 1 << 21))


def c_unordered_window_2e28(ctx):
    """a key window of 2^28 values: 4-byte words from the first level, and the receiver's own level over them (mdb_partition_words_level)"""
    rng = np.random.default_rng(21)
    kl, kr = _perms(rng, 1 << 21)
    _gc_unordered(ctx, 128 * kl, 128 * kr)


def c_pairs_narrow(ctx):
    rng = np.random.default_rng(23)
    n_l, n_r = 600_000, 500_000
    kr = rng.permutation(3 * n_r)[:n_r].astype(np.int64) - n_r
    kl = rng.integers(-n_r, 2 * n_r, n_l, dtype=np.int64)
    _pairs(ctx, kl, kr, rng.random(n_l) < 0.02)


def c_pairs_wide(ctx):
    ctx.set_narrow_keys(0)
    c_pairs_narrow(ctx)


def c_pairs_one_level(ctx):
    rng = np.random.default_rng(24)
    n = 1 << 20
    _pairs(ctx, rng.permutation(n).astype(np.int64), rng.permutation(n).astype(np.int64))


def c_pairs_general(ctx):
    """duplicates on both sides: the general pair join, two histogram-free levels with row ids"""
    rng = np.random.default_rng(25)
    _pairs(ctx, rng.integers(0, 800_000, 600_000, dtype=np.int64), rng.integers(0, 800_000, 1_000_000, dtype=np.int64))


def c_pairs_multi_chunk_leaf(ctx):
    """... and one key with 5000 right rows: redone with the right side in row-id order (the stable exact layout)"""
    rng = np.random.default_rng(26)
    n_l, n_r = 600_000, 1_000_000
    kl = rng.integers(0, 800_000, n_l, dtype=np.int64)
    kr = rng.integers(0, 800_000, n_r, dtype=np.int64)
    kl[rng.choice(n_l, 300, replace=False)] = 77
    kr[rng.choice(n_r, 5000, replace=False)] = 77
    _pairs(ctx, kl, kr)


def c_pairs_small_dups(ctx):
    """one partition level of the exact stable layout"""
    rng = np.random.default_rng(27)
    kl = np.concatenate([np.full(300, 9), np.arange(100, 1100)]).astype(np.int64)
    kr = np.concatenate([np.full(5000, 9), np.arange(100, 600), np.zeros(70)]).astype(np.int64)
    rng.shuffle(kl)
    rng.shuffle(kr)
    _pairs(ctx, kl, kr)


def _payload_case(ctx, seed, span_bits, cells, form):
    rng = np.random.default_rng(seed)
    kr = np.unique(rng.integers(0, 1 << span_bits, 1 << 20, dtype=np.int64)) - 12345
    kl = kr[rng.integers(0, len(kr), 1 << 20)]
    pay = [rng.integers(-2**62, 2**62, len(kr), dtype=np.int64), rng.standard_normal(len(kr))][:cells]
    _payload(ctx, kl, kr, pay, form)


def c_payload_one_level_one_cell(ctx):
    _payload_case(ctx, 28, 21, 1, 1)


def c_payload_one_level_two_cells(ctx):
    _payload_case(ctx, 29, 21, 2, 1)


def c_payload_two_levels_one_cell(ctx):
    _payload_case(ctx, 30, 27, 1, 2)


def c_payload_two_levels_two_cells(ctx):
    _payload_case(ctx, 31, 29, 2, 2)


def c_sort_packed(ctx):
    _sort(ctx, np.random.default_rng(32).integers(-10**6, 10**6, 300_001, dtype=np.int64))


def c_sort_general(ctx):
    """a 64-bit value range does not fit the packed word: least-significant-digit passes"""
    _sort(ctx, np.random.default_rng(34).integers(-2**62, 2**62, 20_001, dtype=np.int64))


def c_distinct(ctx):
    rng = np.random.default_rng(35)
    _distinct(ctx, [rng.integers(0, 300, 300_001, dtype=np.int64), rng.integers(0, 300, 300_001, dtype=np.int64)])


def c_group_multi(ctx):
    rng = np.random.default_rng(36)
    _group_multi(ctx, [rng.integers(0, 300, 300_001, dtype=np.int64), rng.integers(0, 300, 300_001, dtype=np.int64)])


def c_group_multi_sorted(ctx):
    rng = np.random.default_rng(37)
    _group_multi(ctx, [rng.integers(0, 300, 300_001, dtype=np.int64), rng.integers(0, 300, 300_001, dtype=np.int64)])


def _dest_case(ctx, with_rid, keys32):
    rng = np.random.default_rng(38)
    k = rng.integers(-10**9, 10**9, 200_001, dtype=np.int64)
    _by_dest(ctx, k, rng.random(len(k)) < 0.03, 8, with_rid, keys32)


def c_dest(ctx):
    _dest_case(ctx, False, False)


def c_dest_rid(ctx):
    _dest_case(ctx, True, False)


def c_dest_keys32(ctx):
    _dest_case(ctx, False, True)


def c_dest_rid_keys32(ctx):
    _dest_case(ctx, True, True)


T2, T4 = {"MDB_TILE2_MIN": "1"}, {"MDB_TILE2_MIN": "1", "MDB_TILE4_MIN": "1"}
SEL = {"MDB_SELECTIVE_L0": "2"}
NO_ROWJOIN = {"MDB_ROWJOIN": "0"}
ONE_OFF = {"MDB_ONE_LEVEL": "0"}
# name -> (environment, the call)
CASES = {
    "two_levels": ({}, c_two_levels),
    "two_levels_tile2": (T2, c_two_levels),
    "two_levels_nulls": ({}, c_two_levels_nulls),
    "two_levels_pruned": ({}, c_two_levels_pruned),
    "two_levels_pruned_tile2": (T2, c_two_levels_pruned),
    "two_levels_selective": (SEL, c_two_levels_pruned),
    "two_levels_selective_tile2": ({**SEL, **T2}, c_two_levels_pruned),
    "two_levels_one_level_off": (ONE_OFF, c_one_level_off),
    "records_folded": (ONE_OFF, c_records_folded),
    "records_folded_tile2": ({**ONE_OFF, **T2}, c_records_folded),
    "records_4_bytes": (ONE_OFF, c_records_4_bytes),
    "semijoin": ({"MDB_ONE_LEVEL": "0", "MDB_SEMIJOIN": "1", "MDB_SEMIJOIN_SLICE": "13"}, c_semijoin),
    "one_level": ({}, c_one_level),
    "one_level_tile2": (T2, c_one_level),
    "one_level_tile4": (T4, c_one_level),
    "one_level_tile4_off": ({**T4, "MDB_TILE4": "0"}, c_one_level),
    "one_level_tile2_off": ({**T4, "MDB_TILE2": "0"}, c_one_level),
    "one_level_words16_off": ({"MDB_WORDS16": "0"}, c_one_level),
    "one_level_pruned": ({}, c_one_level_pruned),
    "one_level_pruned_tile4": (T4, c_one_level_pruned),
    "one_level_pruned_right_nulls": (T4, c_one_level_pruned_right_nulls),
    "one_level_selective": (SEL, c_one_level_pruned),
    "one_level_selective_odd_start": ({**SEL, **T2}, c_one_level_pruned_odd_start),
    "i32_two_levels": ({}, c_i32_two_levels),
    "i32_one_level": ({}, c_i32_one_level),
    "i32_pruned": ({}, c_i32_pruned),
    "plain_narrow": ({}, c_plain_narrow),
    "plain_narrow_pruned": ({}, c_plain_narrow_pruned),
    "form64": ({}, c_form64),
    "form64_pruned": ({}, c_form64_pruned),
    "skew_exact": ({}, c_skew_exact),
    "multi": ({}, c_multi),
    "group_by": ({}, c_group_by),
    "group_by_unique": ({}, c_group_by_unique),
    "unordered": ({}, c_unordered),
    "unordered_window_2e28": ({}, c_unordered_window_2e28),
    "pairs_narrow": ({}, c_pairs_narrow),
    "pairs_narrow_two_levels": (ONE_OFF, c_pairs_narrow),
    "pairs_wide": ({}, c_pairs_wide),
    "pairs_one_level": ({}, c_pairs_one_level),
    "pairs_general": ({}, c_pairs_general),
    "pairs_multi_chunk_leaf": ({}, c_pairs_multi_chunk_leaf),
    "pairs_small_dups": ({}, c_pairs_small_dups),
    "payload_one_level_one_cell": (NO_ROWJOIN, c_payload_one_level_one_cell),
    "payload_one_level_two_cells": (NO_ROWJOIN, c_payload_one_level_two_cells),
    "payload_two_levels_one_cell": (NO_ROWJOIN, c_payload_two_levels_one_cell),
    "payload_two_levels_two_cells": (NO_ROWJOIN, c_payload_two_levels_two_cells),
    "sort_packed": ({}, c_sort_packed),
    "sort_general": ({}, c_sort_general),
    "distinct": ({}, c_distinct),
    "group_multi": ({}, c_group_multi),
    "group_multi_sorted": ({"MDB_GROUP_MULTI_PACKED": "0"}, c_group_multi_sorted),
    "dest": ({}, c_dest),
    "dest_rid": ({}, c_dest_rid),
    "dest_keys32": ({}, c_dest_keys32),
    "dest_rid_keys32": ({}, c_dest_rid_keys32),
}


# ------------------------------------------------------------------------------------------------ the expected launches
#
# Written as the partition calls an operator makes, each with the launches of its layout; E() adds them up into the line launches() gives.

def E(*calls):
    total = {}
    for call in calls:
        for item in call.split():
            name, rest = item.split("=")
            cnt, inst = rest.split(":")
            have = total.setdefault(name, [0, set()])
            have[0] += int(cnt)
            have[1] |= set(inst.split("+"))
    return " ".join("%s=%d:%s" % (name, c, "+".join(sorted(i))) for name, (c, i) in sorted(total.items()))


L0, L0W, L0P, L0R = "part_scatter_l0", "part_scatter_l0_w32", "part_scatter_l0_pruned", "part_scatter_l0_rid"
L1, L1W, L1R = "part_scatter_l1", "part_scatter_l1_w32", "part_scatter_l1_rid"


def fast1(name0, inst0):
    """the histogram-free first level alone (mdb_part_request.level0_only)"""
    return "%s=1:%s" % (name0, inst0)


def fast2(name0, inst0, name1, inst1):
    """two histogram-free levels, the tile descriptors of the second built from the first one's region cursors"""
    return "%s=1:%s %s=1:%s part_region_tiles=1:k_part_region_tiles_scan part_build_tiles=1:k_part_build_tiles_regions" % (name0, inst0, name1, inst1)


def exact1(name0, inst0, hist="part_hist_l0=1:k_part_hist<true,false>"):
    """one level of the exact layout: segment words, histogram, scatter, the children's starts"""
    return "part_seg0=1:k_part_seg0 %s %s=1:%s part_children=1:k_part_children" % (hist, name0, inst0)


def exact2(name0, inst0, name1, inst1):
    return exact1(name0, inst0) + " part_build_tiles=1:k_part_build_tiles part_hist_l1=1:k_part_hist<false,false> %s=1:%s part_children=1:k_part_children" % (name1, inst1)


MINMAX, MINMAX64 = "part_minmax=1:k_part_minmax_reduce", "part_minmax=1:k_part_minmax64_reduce"
LEFT, LEFT_T2, LEFT32 = fast2(L0, "pf_key_cf", L1, "pf_word"), fast2(L0, "pf_key_cf_t2", L1, "pf_word"), fast2(L0, "pf_key", L1, "pf_word")
RIGHT, RIGHT32 = fast2(L0W, "pf_key_w32_cf", L1W, "pf_word_w32"), fast2(L0W, "pf_key_w32", L1W, "pf_word_w32")
LEFT_RID = fast2(L0R, "pf_key_rid", L1R, "pf_word_rid")
# the group records ordered by first row: one exact level up to 2^21 left rows, two histogram-free levels of folded records above;
# few records among many rows: two histogram-free levels of 8-byte records first (k_order_leaf_sparse's leaves)
ORDER = exact1("sort_scatter_l0", "pf_word_hist_raw", "sort_hist_l0=1:k_part_hist<false,true>")
RAW2 = fast2("sort_scatter_l0", "pf_word_raw", "sort_scatter_l1", "pf_word_raw")
ORDER_FOLDED = fast2("sort_scatter_l0_w32", "pf_word_raw_w32", "sort_scatter_l1_w32", "pf_word_raw_w32")
ORDER_FOLDED_T2 = fast2("sort_scatter_l0_w32", "pf_word_raw_w32_t2", "sort_scatter_l1_w32", "pf_word_raw_w32")
SORT_PACKED = "orderby_leaf=1:k_sort_leaf orderby_pack=1:k_sort_pack orderby_range=1:k_sort_ranges"


def pruned2(inst0, right=RIGHT, inst1="pf_word", name1=L1):
    return E(fast2(L0P, inst0, name1, inst1), right, MINMAX, ORDER)


def one_level(left, right, name0=L0):
    return E(fast1(name0, left), fast1(L0W, right), ORDER)


def one_level_pruned(left, right):
    return E(fast1(L0P, left), fast1(L0W, right), MINMAX, RAW2, ORDER)


def dest(inst):
    return E(exact1("dest_scatter", inst, "dest_hist=1:k_part_hist<true,false>"))


PAIRS_FIRST = [fast1(L0, "pf_key_cf")] * 4      # the general pair join comes behind two attempts of the unique-key forms
EXPECT = {
    "two_levels": E(LEFT, RIGHT, ORDER),
    "two_levels_tile2": E(LEFT_T2, RIGHT, ORDER),
    "two_levels_nulls": E(LEFT, RIGHT, ORDER),
    "two_levels_pruned": pruned2("pf_key_cf"),
    "two_levels_pruned_tile2": pruned2("pf_key_cf_t2"),
    "two_levels_selective": pruned2("pf_key_cf_sel"),
    "two_levels_selective_tile2": pruned2("pf_key_cf_sel_t2"),
    "two_levels_one_level_off": E(LEFT, RIGHT, ORDER),
    "records_folded": E(LEFT, RIGHT, ORDER_FOLDED),
    "records_folded_tile2": E(LEFT_T2, RIGHT, ORDER_FOLDED_T2),
    "records_4_bytes": E(*[LEFT, RIGHT, ORDER_FOLDED] * 2),
    "semijoin": pruned2("pf_key_cf", inst1="pf_word_semi", name1="part_scatter_l1_semi"),
    "one_level": one_level("pf_key_cf", "pf_key_w32_out16_cf"),
    "one_level_tile2": one_level("pf_key_cf_t2", "pf_key_w32_out16_cf_t2"),
    "one_level_tile4": one_level("pf_key_cf_t2", "pf_key_w32_out16_cf_t4"),
    "one_level_tile4_off": one_level("pf_key_cf_t2", "pf_key_w32_out16_cf_t2"),
    "one_level_tile2_off": one_level("pf_key_cf", "pf_key_w32_out16_cf"),
    "one_level_words16_off": one_level("pf_key_cf", "pf_key_w32_cf"),
    "one_level_pruned": one_level_pruned("pf_key_cf", "pf_key_w32_out16_cf"),
    "one_level_pruned_tile4": one_level_pruned("pf_key_cf_t2", "pf_key_w32_out16_cf_t4"),
    "one_level_pruned_right_nulls": one_level_pruned("pf_key_cf_t2", "pf_key_w32_out16_cf_t2"),
    "one_level_selective": one_level_pruned("pf_key_cf_sel", "pf_key_w32_out16_cf"),
    "one_level_selective_odd_start": one_level_pruned("pf_key_cf_sel_t2", "pf_key_w32_out16_cf_t2"),
    "i32_two_levels": E(LEFT32, RIGHT32, ORDER),
    "i32_one_level": one_level("pf_key", "pf_key_w32_out16"),
    "i32_pruned": pruned2("pf_key", RIGHT32),
    "plain_narrow": E(LEFT32, RIGHT32, ORDER),
    "plain_narrow_pruned": pruned2("pf_key", RIGHT32),
    "form64": E(LEFT_RID, LEFT32, ORDER),
    "form64_pruned": E(fast2("part_scatter_l0_rid_pruned", "pf_key_rid_r64", L1R, "pf_word_rid"), fast2(L0, "pf_key_mm64", L1, "pf_word"), MINMAX64, ORDER),
    # the plain narrow form first, then - a region overflowed - both tables through the exact layout of the 64-bit form
    "skew_exact": E(LEFT32, RIGHT32, exact2(L0, "pf_key_rid_hist", L1, "pf_word_rid_hist"), exact2(L0, "pf_key_hist", L1, "pf_word_hist"), ORDER),
    "multi": E(LEFT, RIGHT, RIGHT, ORDER),
    "group_by": E(LEFT, ORDER),
    "group_by_unique": E(LEFT, ORDER),
    "unordered": E(*[fast1(L0W, "pf_key_w32_out16_cf")] * 2),
    "unordered_window_2e28": E(*[fast1(L0W, "pf_key_w32_cf"), "part_scatter_l1_w32=1:pf_word_w32_out16"] * 2),
    "pairs_narrow": E(*[fast1(L0, "pf_key_cf")] * 2),
    "pairs_narrow_two_levels": E(LEFT32, LEFT32, ORDER),
    "pairs_wide": E(LEFT_RID, LEFT_RID, ORDER),
    "pairs_one_level": E(*[fast1(L0, "pf_key_cf")] * 2),
    "pairs_general": E(*PAIRS_FIRST, LEFT_RID, LEFT_RID),
    "pairs_multi_chunk_leaf": E(*PAIRS_FIRST, LEFT_RID, LEFT_RID, exact2("part_scatter_l0_stable", "pf_key_rid_stable_hist", "part_scatter_l1_stable", "pf_word_rid_stable_hist"),
                                exact2(L0, "pf_key_rid_hist", L1, "pf_word_rid_hist")),
    "pairs_small_dups": E(*[exact1(L0, "pf_key_rid_hist")] * 5, exact1("part_scatter_l0_stable", "pf_key_rid_stable_hist")),
    "payload_one_level_one_cell": E(fast1(L0, "pf_key_cf"), fast1("part_scatter_l0_pay", "pf_key_cf_pay")),
    "payload_one_level_two_cells": E(fast1(L0, "pf_key_cf"), fast1("part_scatter_l0_pay", "pf_key_cf_pay")),
    "payload_two_levels_one_cell": E(LEFT, fast2("part_scatter_l0_pay", "pf_key_cf_pay", "part_scatter_l1_pay", "pf_word_pay")),
    "payload_two_levels_two_cells": E(LEFT, fast2("part_scatter_l0_pay", "pf_key_cf_pay", "part_scatter_l1_pay", "pf_word_pay")),
    "sort_packed": E(SORT_PACKED, RAW2),
    "sort_general": E("orderby_hist=8:k_part_hist<false,false> orderby_load=1:k_sort_load orderby_scatter=8:pf_word_rid_stable_hist"),
    "distinct": E("orderby_range=1:k_sort_ranges", exact1(L0, "pf_key_rid_hist"), ORDER),
    "group_multi": E("orderby_range=1:k_sort_ranges", exact1(L0, "pf_key_rid_hist"), ORDER),
    "group_multi_sorted": E(SORT_PACKED, RAW2, ORDER),
    "dest": dest("pf_key_hist_dest"),
    "dest_rid": dest("pf_key_rid_hist_dest"),
    "dest_keys32": dest("pf_key_hist_dest"),
    "dest_rid_keys32": dest("pf_key_rid_hist_dest"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_partition_launches(ctx, monkeypatch, case):
    env, call = CASES[case]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    call(ctx)
    got = launches(ctx)
    print(case, got)
    assert got == EXPECT[case], (case, got, EXPECT[case])


# every (profiler name, kernel instance) the partition's host code can launch (its kernels: k_part_* and the k_part_scatter<pf_*> instances),
# in the order of the code: the levels' common kernels, the histogram-free first level, the histogram-free last level, the exact levels,
# mdb_partition_words_level, mdb_sort_pass
REACHED = """
part_seg0:k_part_seg0 part_region_tiles:k_part_region_tiles_scan part_build_tiles:k_part_build_tiles_regions part_build_tiles:k_part_build_tiles
part_children:k_part_children part_minmax:k_part_minmax_reduce part_minmax:k_part_minmax64_reduce
sort_scatter_l0_w32:pf_word_raw_w32_t2 sort_scatter_l0_w32:pf_word_raw_w32 sort_scatter_l0:pf_word_raw
part_scatter_l0_w32:pf_key_w32_out16_cf_t4 part_scatter_l0_w32:pf_key_w32_out16_cf_t2 part_scatter_l0_w32:pf_key_w32_out16_cf part_scatter_l0_w32:pf_key_w32_out16
part_scatter_l0_w32:pf_key_w32_cf part_scatter_l0_w32:pf_key_w32
part_scatter_l0_pay:pf_key_cf_pay part_scatter_l0_rid_pruned:pf_key_rid_r64 part_scatter_l0_rid:pf_key_rid part_scatter_l0:pf_key_mm64
part_scatter_l0_pruned:pf_key_cf_sel_t2 part_scatter_l0_pruned:pf_key_cf_sel part_scatter_l0_pruned:pf_key_cf_t2 part_scatter_l0_pruned:pf_key_cf part_scatter_l0_pruned:pf_key
part_scatter_l0:pf_key_cf_t2 part_scatter_l0:pf_key_cf part_scatter_l0:pf_key
part_scatter_l1_pay:pf_word_pay part_scatter_l1_rid:pf_word_rid sort_scatter_l1_w32:pf_word_raw_w32 sort_scatter_l1:pf_word_raw part_scatter_l1_w32:pf_word_w32
part_scatter_l1_semi:pf_word_semi part_scatter_l1:pf_word
sort_hist_l0:k_part_hist<false,true> dest_hist:k_part_hist<true,false> part_hist_l0:k_part_hist<true,false> part_hist_l1:k_part_hist<false,false>
sort_scatter_l0:pf_word_hist_raw part_scatter_l0_stable:pf_key_rid_stable_hist part_scatter_l1_stable:pf_word_rid_stable_hist
dest_scatter:pf_key_rid_hist_dest dest_scatter:pf_key_hist_dest part_scatter_l0:pf_key_rid_hist part_scatter_l0:pf_key_hist
part_scatter_l1:pf_word_rid_hist part_scatter_l1:pf_word_hist
part_scatter_l1_w32:pf_word_w32_out16
orderby_hist:k_part_hist<false,false> orderby_scatter:pf_word_rid_stable_hist
""".split()
# launch sites that no exported entry point reaches, and why
NOT_REACHED = {
    "mdb_partition_words_level with out16_shift = 0 (part_scatter_l1_w32:pf_word_w32, a pair the partition's own last level does reach)":
        "its one caller, mdb_shard_join, passes out16_shift = 32 - kbits, and mdb_shard_plan_make serves windows of at most 2^30 values: never 0",
}


def test_the_cases_reach_every_launch_site():
    """the union of the expected lists' (name, instance) pairs, for the partition's own kernels, is the list above - no GPU needed for that:
    every case asserts its list"""
    got = set()
    for line in EXPECT.values():
        for item in line.split():
            name, rest = item.split("=")
            got |= {"%s:%s" % (name, inst) for inst in rest.split(":")[1].split("+") if inst.startswith(("pf_", "k_part_"))}
    assert len(REACHED) == len(set(REACHED))
    assert got == set(REACHED), (sorted(got - set(REACHED)), sorted(set(REACHED) - got))
