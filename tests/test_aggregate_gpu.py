"""SUM / MIN / MAX / AVG on the device (mdb_dev_group_aggregate and the statements that reach it).  An extension - upstream knows COUNT only
(midorisql.l:139-142) - so nothing here is pinned to the reference: the operator is checked against numpy restatements in this file
(integer sums wrap like numpy's int64; DOUBLE sums of multiples of 1/8 are exact in every order and must equal numpy's bit for bit,
arbitrary doubles stay inside the standard any-order bound around math.fsum), the statements against a naive restatement over Python
lists (`naive`)."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
ROWS = [1, 63, 64, 65, 4095, 4096, 4097, 2 ** 18 + 1]
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ numpy restatement of the operator

def _image(bits, is_double):
    """the order-preserving 64-bit image mdb_dev_sort_perm documents: IEEE order with -0.0 before +0.0; INT64 order"""
    b = bits.view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    if is_double:
        return np.where(b >> np.uint64(63) != 0, ~b, b ^ top)
    return b ^ top


def _unimage(u, is_double):
    top = np.uint64(1) << np.uint64(63)
    if is_double:
        return np.where(u >> np.uint64(63) != 0, u ^ top, ~u)
    return u ^ top


def expect(D, gid, G, cells, valid, op, ty):
    """-> (8-byte result cells as int64 bits, NULL flags) of one aggregate: gid[i] = group of row i, cells = the 8-byte cells as int64 bits"""
    cnt = np.bincount(gid[valid], minlength=G)
    is_double = ty == D.T_DOUBLE
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if op in (D.AGG_SUM, D.AGG_AVG):
            s = np.zeros(G, dtype=np.float64 if is_double else np.int64)
            np.add.at(s, gid[valid], cells[valid].view(np.float64) if is_double else cells[valid])
            if op == D.AGG_AVG:
                s = s.astype(np.float64) / np.maximum(cnt, 1).astype(np.float64)
            out = s.view(np.int64).copy()
        else:
            img = _image(cells, is_double)
            acc = np.full(G, np.iinfo(np.uint64).max if op == D.AGG_MIN else 0, dtype=np.uint64)
            (np.minimum if op == D.AGG_MIN else np.maximum).at(acc, gid[valid], img[valid])
            out = _unimage(acc, is_double).view(np.int64).copy()
    out[cnt == 0] = 0
    return out, cnt == 0


def make_stream(rng, n, G, null_key=True):
    """gid in first-occurrence numbering, first[], and one 8-byte key per group (the key of one group NULL when there are two or more)"""
    gid = np.concatenate([rng.permutation(G), rng.integers(0, G, n - G)]).astype(np.int64)
    rng.shuffle(gid)
    _, first_of = np.unique(gid, return_index=True)
    order = np.argsort(first_of)                        # group numbers by first occurrence
    rank = np.empty(G, dtype=np.int64)
    rank[order] = np.arange(G)
    gid = rank[gid]
    first = np.sort(first_of).astype(np.int32)
    keyval = (np.arange(G, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)).view(np.int64)    # distinct: an odd multiplier
    keys = keyval[gid].copy()
    knull = np.zeros(n, dtype=bool)
    if null_key and G >= 2:
        knull = gid == G // 2
        keys[knull] = rng.integers(-5, 5, int(knull.sum()))      # (what lies under a NULL key does not matter)
    return gid, first, keys, knull


def run_head_cases():
    """(n, the sorted positions at which runs begin) for the run finder's 1024-position chunks and 64-position words: one run, a run per row,
    and three runs whose heads are the last position of a chunk, the first of the next, position 63 / 64 of a word, the stream's last row"""
    three = {1023: [(0, 63, 64), (0, 64, 1022)], 1024: [(0, 63, 64), (0, 64, 1023)], 1025: [(0, 63, 64), (0, 1023, 1024)],
             2049: [(0, 1023, 1024), (0, 2047, 2048)]}
    return [(n, h) for n in (1023, 1024, 1025, 2049) for h in [(0,), tuple(range(n))] + three[n]]


def run_head_id(case):
    n, heads = case
    return f"{n}-G{len(heads)}" + (f"-{heads[1]}-{heads[2]}" if len(heads) == 3 else "")


def stream_with_run_heads(rng, n, heads):
    """Two key columns whose stable ascending sort has its runs begin at exactly the sorted positions `heads` (heads[0] == 0): the run at
    heads[s] holds the key (s // 2 - 1, s % 2), the first run's first column is NULL (NULLs sort first).  The rows come in random stream
    order, so a run's group - groups are numbered by first occurrence - is not its place in the sorted order.
    -> gid, first[], (cells, nulls) of the two key columns"""
    G = len(heads)
    srt = np.repeat(np.arange(G, dtype=np.int64), np.diff(list(heads) + [n]))      # the run of every sorted position
    rng.shuffle(srt)                                                               # ... of every stream position
    _, first_of = np.unique(srt, return_index=True)
    rank = np.empty(G, dtype=np.int64)
    rank[np.argsort(first_of)] = np.arange(G)
    k1, k2 = srt // 2 - 1, srt % 2
    k1null = (srt == 0) & (G >= 2)
    k1[k1null] = 99                                                                # (what lies under a NULL key does not matter)
    return rank[srt], np.sort(first_of).astype(np.int32), (k1, k1null), (k2, np.zeros(n, dtype=bool))


def int_cells(rng, n):
    v = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    small = rng.random(n) < 0.5
    v[small] = rng.integers(-1000, 1000, int(small.sum()))
    v[rng.random(n) < 0.05] = I64_MIN
    v[rng.random(n) < 0.05] = I64_MAX
    v[rng.random(n) < 0.05] = 0
    v[rng.random(n) < 0.05] = -1
    return v


def eighths(rng, n):
    """multiples of 1/8 below 2^20 in magnitude: every sum of up to 2^18 + 1 of them is exact, whatever the order"""
    return rng.integers(-(2 ** 23) + 1, 2 ** 23, n).astype(np.float64) / 8.0


def null_cells(rng, gid, G, n):
    """10 % NULL cells, and every cell of group 1 NULL when there are three groups or more"""
    vnull = rng.random(n) < 0.1
    if G >= 3:
        vnull |= gid == 1
    return vnull


class Column:
    """a column on the device: identity (cells in stream order), or a base table read through a row-id vector with MDB_NO_ROW in it;
    misaligned: the values start 8 bytes off a 16-byte boundary"""

    def __init__(self, dev, D, rng, cells, nulls, through_rid=False, misaligned=False):
        n = len(cells)
        self.valid = ~nulls
        self.cells = cells
        if through_rid:
            m = n + 7
            place = rng.permutation(m)[:n]                      # row of the base table that stream position i reads
            base = rng.integers(-9, 9, m).astype(np.int64)
            base_null = rng.random(m) < 0.5
            base[place] = cells
            base_null[place] = nulls
            rid = place.astype(np.uint32)
            norow = rng.random(n) < 0.05
            rid[norow] = D.NO_ROW
            self.valid = self.valid & ~norow
            self.rid = dev.to_dev(rid)
            cells, nulls = base, base_null
        else:
            self.rid = None
        if misaligned:
            self.values = dev.to_dev(np.concatenate([[0], cells]).astype(np.int64))[1:]
            assert self.values.data_ptr() % 16 == 8
        else:
            self.values = dev.to_dev(cells)
        self.nullbits = dev.nullbits_dev(nulls) if nulls.any() or through_rid else None


def run_and_check(dev, D, keys, n, first, G, gid, aggs, want_form):
    """aggs: [(op, type, Column)]; every result cell and NULL flag against the restatement; -> the result bytes"""
    outs, nulls, form = dev.group_aggregate(keys, n, first, [(op, ty, c.values, c.nullbits, c.rid) for op, ty, c in aggs])
    assert form == want_form, (form, want_form, n, G)
    got_bytes = []
    for (op, ty, c), o, nb in zip(aggs, outs, nulls):
        e, enull = expect(D, gid, G, c.cells, c.valid, op, ty)
        g = o.cpu().numpy().view(np.int64)
        assert np.array_equal(nb, enull), (op, ty, n, G, int((nb != enull).sum()))
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, (op, ty, n, G, bad[:5], g[bad[:5]], e[bad[:5]])
        got_bytes.append(g.tobytes() + nb.tobytes())
    return got_bytes


def group_counts(dev, n, naggs):
    lds = dev.group_aggregate_lds_groups(naggs)
    return sorted({g for g in (1, 2, 64, lds, lds + 1, n) if g <= n}), lds


@pytest.mark.parametrize("n", ROWS)
def test_operator_integer_cells_every_row_and_group_count(dev, n):
    """SUM (wrapping), MIN, MAX, AVG over INT64 cells with INT64_MIN / INT64_MAX / 0 / -1 among them: 10 % NULL cells, a group that is
    all NULL, a NULL group key, values read through row ids with MDB_NO_ROW, a column 8 bytes off a 16-byte boundary - in the LDS form up
    to its group limit and in the sorted form beyond"""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(1000 + n)
    counts, lds = group_counts(dev, n, 4)
    for G in counts:
        gid, first, keys, knull = make_stream(rng, n, G)
        v = int_cells(rng, n)
        vnull = null_cells(rng, gid, G, n)
        plain = Column(dev, D, rng, v, vnull)
        off = Column(dev, D, rng, v, vnull, misaligned=True)
        via = Column(dev, D, rng, v, vnull, through_rid=True)
        kcol = Column(dev, D, rng, keys, knull, misaligned=(G % 2 == 0))
        dkeys = [(kcol.values, kcol.nullbits, None, D.T_INT64, False)]
        aggs = [(D.AGG_SUM, D.T_INT64, off), (D.AGG_MIN, D.T_INT64, via), (D.AGG_MAX, D.T_INT64, plain), (D.AGG_AVG, D.T_INT64, via)]
        run_and_check(dev, D, dkeys, n, dev.to_dev(first), G, gid, aggs, 1 if G <= lds else 2)
    if n > 64:          # a wrapping sum for certain: many INT64_MAX in one group
        gid = np.zeros(n, dtype=np.int64)
        big = Column(dev, D, rng, np.full(n, I64_MAX, dtype=np.int64), np.zeros(n, dtype=bool))
        keys1 = dev.to_dev(np.zeros(n, dtype=np.int64))
        first1 = dev.to_dev(np.zeros(1, dtype=np.int32))
        run_and_check(dev, D, [(keys1, None, None, D.T_INT64, False)], n, first1, 1, gid, [(D.AGG_SUM, D.T_INT64, big)], 1)
        assert int(expect(D, gid, 1, big.cells, big.valid, D.AGG_SUM, D.T_INT64)[0][0]) == wrap64(n * int(I64_MAX)) != n * int(I64_MAX)


@pytest.mark.parametrize("n", ROWS)
def test_operator_double_cells_bit_exact_in_both_forms(dev, n):
    """cells that are multiples of 1/8 below 2^20: SUM and AVG equal numpy bit for bit (the sorted form: a floating-point sum is never
    order-free); MIN / MAX alone are order-free and take the LDS form"""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(2000 + n)
    counts, lds4 = group_counts(dev, n, 4)
    lds2 = dev.group_aggregate_lds_groups(2)
    for G in counts:
        gid, first, keys, knull = make_stream(rng, n, G)
        d = eighths(rng, n).view(np.int64)
        vnull = null_cells(rng, gid, G, n)
        plain = Column(dev, D, rng, d, vnull)
        off = Column(dev, D, rng, d, vnull, misaligned=True)
        via = Column(dev, D, rng, d, vnull, through_rid=True)
        kcol = Column(dev, D, rng, keys, knull)
        dkeys = [(kcol.values, kcol.nullbits, None, D.T_INT64, False)]
        dfirst = dev.to_dev(first)
        run_and_check(dev, D, dkeys, n, dfirst, G, gid,
                      [(D.AGG_SUM, D.T_DOUBLE, off), (D.AGG_AVG, D.T_DOUBLE, via), (D.AGG_MIN, D.T_DOUBLE, plain), (D.AGG_MAX, D.T_DOUBLE, via)], 2)
        run_and_check(dev, D, dkeys, n, dfirst, G, gid, [(D.AGG_MIN, D.T_DOUBLE, via), (D.AGG_MAX, D.T_DOUBLE, off)], 1 if G <= lds2 else 2)


@pytest.mark.parametrize("case", run_head_cases(), ids=run_head_id)
def test_operator_sorted_form_run_heads_at_chunk_and_word_edges(dev, case):
    """the sorted form (a DOUBLE sum) over two key columns, the runs' heads on the run finder's chunk and word edges: bit for bit numpy's"""
    from midoridb_amd import dev as D
    n, heads = case
    rng = np.random.default_rng(2500 + n + len(heads) + heads[-1])
    gid, first, (k1, k1null), (k2, k2null) = stream_with_run_heads(rng, n, heads)
    G = len(heads)
    c1, c2 = Column(dev, D, rng, k1, k1null), Column(dev, D, rng, k2, k2null, misaligned=True)
    dkeys = [(c1.values, c1.nullbits, None, D.T_INT64, False), (c2.values, c2.nullbits, None, D.T_INT64, False)]
    vd = Column(dev, D, rng, eighths(rng, n).view(np.int64), null_cells(rng, gid, G, n), misaligned=True)
    run_and_check(dev, D, dkeys, n, dev.to_dev(first), G, gid, [(D.AGG_SUM, D.T_DOUBLE, vd)], 2)


@pytest.mark.parametrize("n", [1, 65, 4097, 2 ** 18 + 1])
def test_operator_without_keys_and_identity(dev, n):
    """nkeys == 0: one group over all rows (first may be None); MDB_AGG_IDENTITY: group i is row i - the cell itself, converted for AVG,
    NULL kept"""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(3000 + n)
    v, d = int_cells(rng, n), eighths(rng, n).view(np.int64)
    vnull = rng.random(n) < 0.1
    vi, vd = Column(dev, D, rng, v, vnull, through_rid=True), Column(dev, D, rng, d, vnull, misaligned=True)
    gid = np.zeros(n, dtype=np.int64)
    ints = [(D.AGG_SUM, D.T_INT64, vi), (D.AGG_MIN, D.T_INT64, vi), (D.AGG_MAX, D.T_INT64, vi), (D.AGG_AVG, D.T_INT64, vi),
            (D.AGG_MIN, D.T_DOUBLE, vd), (D.AGG_MAX, D.T_DOUBLE, vd)]
    run_and_check(dev, D, [], n, None, 1, gid, ints, 1)
    run_and_check(dev, D, [], n, None, 1, gid, ints + [(D.AGG_SUM, D.T_DOUBLE, vd), (D.AGG_AVG, D.T_DOUBLE, vd)], 2)
    run_and_check(dev, D, D.AGG_IDENTITY, n, None, n, np.arange(n), ints + [(D.AGG_SUM, D.T_DOUBLE, vd), (D.AGG_AVG, D.T_DOUBLE, vd)], 3)
    allnull = Column(dev, D, rng, v, np.ones(n, dtype=bool))
    outs, nulls, form = dev.group_aggregate([], n, None, [(D.AGG_SUM, D.T_INT64, allnull.values, allnull.nullbits, None),
                                                         (D.AGG_AVG, D.T_DOUBLE, allnull.values, allnull.nullbits, None)])
    assert [bool(x[0]) for x in nulls] == [True, True] and int(outs[0][0]) == 0 and float(outs[1][0]) == 0.0


def test_operator_key_through_row_ids_and_composite_keys(dev):
    """a group key read through a row-id vector with MDB_NO_ROW in it (such a key is NULL: one group); two key columns (DOUBLE compared by
    its bits: -0.0 and +0.0 are two groups) always take the sorted form"""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(77)
    n, G = 5000, 37
    gid, first, keys, knull = make_stream(rng, n, G)
    kcol = Column(dev, D, rng, keys, knull, through_rid=True)
    knull2 = ~kcol.valid                                        # rows at "no row" join the NULL-key group
    gid2 = gid.copy()
    gid2[knull2] = G // 2
    _, first_of = np.unique(gid2, return_index=True)
    order = np.argsort(first_of)
    G2 = len(order)
    rank = np.full(G, -1, dtype=np.int64)
    rank[np.unique(gid2)[order]] = np.arange(G2)
    gid2 = rank[gid2]
    first2 = np.sort(first_of).astype(np.int32)
    v = Column(dev, D, rng, int_cells(rng, n), rng.random(n) < 0.1)
    dkeys = [(kcol.values, kcol.nullbits, kcol.rid, D.T_INT64, False)]
    run_and_check(dev, D, dkeys, n, dev.to_dev(first2), G2, gid2, [(D.AGG_SUM, D.T_INT64, v), (D.AGG_MAX, D.T_INT64, v)], 1)
    # two key columns: (a in {0, 1, 2}, b in {-0.0, +0.0, 1.5, NULL})
    a = rng.integers(0, 3, n).astype(np.int64)
    bvals = np.array([-0.0, 0.0, 1.5, 7.0]).view(np.int64)
    bi = rng.integers(0, 4, n)
    b, bnull = bvals[bi], bi == 3
    combo = a * 4 + bi
    _, first_of = np.unique(combo, return_index=True)
    order = np.argsort(first_of)
    rank = np.full(12, -1, dtype=np.int64)
    rank[np.unique(combo)[order]] = np.arange(len(order))
    gid3 = rank[combo]
    ka, kb = Column(dev, D, rng, a, np.zeros(n, dtype=bool)), Column(dev, D, rng, b, bnull)
    two = [(ka.values, None, None, D.T_INT64, False), (kb.values, kb.nullbits, None, D.T_DOUBLE, False)]
    f, c = dev.group_count_multi(two, n)
    assert np.array_equal(f.cpu().numpy(), np.sort(first_of))
    run_and_check(dev, D, two, n, f, len(order), gid3, [(D.AGG_SUM, D.T_INT64, v), (D.AGG_MIN, D.T_INT64, v), (D.AGG_AVG, D.T_INT64, v)], 2)


def test_operator_lds_knob_and_reproducibility(dev, monkeypatch):
    """MDB_AGG_LDS=0: identical results through the sorted form.  Two calls over the same input give the same bytes, in both forms and
    for DOUBLE SUM (no floating-point atomics: the order of every sum is fixed by n, the permutation and the launch geometry)"""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(5)
    n, G = 2 ** 18 + 1, 64
    gid, first, keys, knull = make_stream(rng, n, G)
    vnull = null_cells(rng, gid, G, n)
    vi = Column(dev, D, rng, int_cells(rng, n), vnull, through_rid=True)
    any_double = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)).view(np.int64)
    vd = Column(dev, D, rng, any_double, vnull, misaligned=True)
    kcol = Column(dev, D, rng, keys, knull)
    dkeys, dfirst = [(kcol.values, kcol.nullbits, None, D.T_INT64, False)], dev.to_dev(first)
    ints = [(D.AGG_SUM, D.T_INT64, vi), (D.AGG_MIN, D.T_INT64, vi), (D.AGG_MAX, D.T_DOUBLE, vd), (D.AGG_AVG, D.T_INT64, vi)]
    a1 = run_and_check(dev, D, dkeys, n, dfirst, G, gid, ints, 1)
    a2 = run_and_check(dev, D, dkeys, n, dfirst, G, gid, ints, 1)
    assert a1 == a2
    monkeypatch.setenv("MDB_AGG_LDS", "0")
    b1 = run_and_check(dev, D, dkeys, n, dfirst, G, gid, ints, 2)
    b2 = run_and_check(dev, D, dkeys, n, dfirst, G, gid, ints, 2)
    monkeypatch.delenv("MDB_AGG_LDS")
    assert b1 == b2 == a1
    call = lambda: dev.group_aggregate(dkeys, n, dfirst, [(D.AGG_SUM, D.T_DOUBLE, vd.values, vd.nullbits, None),
                                                         (D.AGG_AVG, D.T_DOUBLE, vd.values, vd.nullbits, None)])
    (o1, m1, f1), (o2, m2, f2) = call(), call()
    assert f1 == f2 == 2
    for x, y in zip(o1 + m1, o2 + m2):
        assert (x.cpu().numpy() if hasattr(x, "cpu") else x).tobytes() == (y.cpu().numpy() if hasattr(y, "cpu") else y).tobytes()


@pytest.mark.parametrize("n,G", [(4097, 65), (2 ** 18 + 1, 1), (2 ** 18 + 1, 4097)])
def test_operator_double_sum_within_the_any_order_bound(dev, n, G):
    """arbitrary normal doubles: |SUM - math.fsum| <= (c - 1) u / (1 - (c - 1) u) * sum |x| with u = 2^-53 and c the group's non-NULL
    cells - the standard bound for a sum taken in any order; AVG is that sum divided by c"""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(9000 + n + G)
    gid, first, keys, knull = make_stream(rng, n, G)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    vnull = null_cells(rng, gid, G, n)
    vd = Column(dev, D, rng, x.view(np.int64), vnull)
    kcol = Column(dev, D, rng, keys, knull)
    outs, nulls, form = dev.group_aggregate([(kcol.values, kcol.nullbits, None, D.T_INT64, False)], n, dev.to_dev(first),
                                            [(D.AGG_SUM, D.T_DOUBLE, vd.values, vd.nullbits, None), (D.AGG_AVG, D.T_DOUBLE, vd.values, vd.nullbits, None)])
    assert form == 2
    s, avg = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    order = np.argsort(gid, kind="stable")
    bounds = np.searchsorted(gid[order], np.arange(G + 1))
    for g in range(G):
        rows = order[bounds[g]:bounds[g + 1]]
        cells = x[rows][~vnull[rows]]
        c = len(cells)
        assert bool(nulls[0][g]) == (c == 0) and bool(nulls[1][g]) == (c == 0)
        if not c:
            continue
        exact = math.fsum(cells.tolist())
        bound = (c - 1) * U / (1 - (c - 1) * U) * math.fsum(np.abs(cells).tolist())
        assert abs(float(s[g]) - exact) <= bound, (g, c, float(s[g]), exact, bound)
        assert float(avg[g]) == float(s[g]) / float(c)


def test_operator_min_max_over_double_specials_and_points_in_time(dev):
    """-0.0 lies before +0.0, the infinities and the denormals have their IEEE places - in both forms; DATE / DATETIME cells are 8-byte
    integers (time_t)"""
    from midoridb_amd import dev as D
    tiny = 5e-324
    groups = [[-0.0, 0.0], [0.0, -0.0, 0.0], [np.inf, 1.0, -np.inf], [tiny, -tiny, 0.0], [-tiny, -0.0], [tiny, 0.0], [2.0 ** -1040, 3.0], [-np.inf], [np.inf]]
    want = [(-0.0, 0.0), (-0.0, 0.0), (-np.inf, np.inf), (-tiny, tiny), (-tiny, -0.0), (0.0, tiny), (2.0 ** -1040, 3.0), (-np.inf, -np.inf), (np.inf, np.inf)]
    cells = np.array([x for g in groups for x in g], dtype=np.float64)
    gid = np.array([i for i, g in enumerate(groups) for _ in g], dtype=np.int64)
    rng = np.random.default_rng(3)
    p = rng.permutation(len(cells))
    cells, gid = cells[p], gid[p]
    _, first_of = np.unique(gid, return_index=True)
    order = np.argsort(first_of)
    rank = np.empty(len(groups), dtype=np.int64)
    rank[order] = np.arange(len(groups))
    keys = dev.to_dev(gid * 1000 - 3)
    first = dev.to_dev(np.sort(first_of).astype(np.int32))
    col = Column(dev, D, rng, cells.view(np.int64), np.zeros(len(cells), dtype=bool))
    dkeys = [(keys, None, None, D.T_INT64, False)]
    for extra, form in (([], 1), ([(D.AGG_SUM, D.T_DOUBLE, col)], 2)):
        aggs = [(D.AGG_MIN, D.T_DOUBLE, col), (D.AGG_MAX, D.T_DOUBLE, col)] + extra
        outs, nulls, f = dev.group_aggregate(dkeys, len(cells), first, [(op, ty, c.values, c.nullbits, c.rid) for op, ty, c in aggs])
        assert f == form
        lo, hi = outs[0].cpu().numpy(), outs[1].cpu().numpy()
        for g, (wlo, whi) in enumerate(want):
            assert lo[rank[g]].tobytes() == np.float64(wlo).tobytes(), (g, lo[rank[g]], wlo)
            assert hi[rank[g]].tobytes() == np.float64(whi).tobytes(), (g, hi[rank[g]], whi)
    t = np.array([1577833200, -86400, 0, 4102441200, 1577833200], dtype=np.int64)        # time_t cells, one before 1970
    tc = Column(dev, D, rng, t, np.array([False, False, True, False, False]))
    outs, nulls, f = dev.group_aggregate([], 5, None, [(D.AGG_MIN, D.T_INT64, tc.values, tc.nullbits, None), (D.AGG_MAX, D.T_INT64, tc.values, tc.nullbits, None)])
    assert (int(outs[0][0]), int(outs[1][0]), f) == (-86400, 4102441200, 1)


def test_operator_refuses_first_rows_that_do_not_belong_to_the_keys(dev):
    from midoridb_amd import dev as D
    from midoridb_amd.dev import DeviceError
    keys = dev.to_dev(np.array([1, 2, 3, 1, 2, 3, 4], dtype=np.int64))
    v = dev.to_dev(np.arange(7, dtype=np.int64))
    d = dev.to_dev(np.arange(7, dtype=np.float64))
    first = dev.to_dev(np.array([0, 1, 2], dtype=np.int32))               # the group of key 4 is missing
    for agg in ((D.AGG_SUM, D.T_INT64, v, None, None), (D.AGG_SUM, D.T_DOUBLE, d, None, None)):
        with pytest.raises(DeviceError):
            dev.group_aggregate([(keys, None, None, D.T_INT64, False)], 7, first, [agg])


# ------------------------------------------------------------------------------------------------ statements

def wrap64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= 1 << 63 else x


def as_double(bits):
    return np.array([bits], dtype=np.int64).view(np.float64)[0]


def naive(rows, group_cols, aggs, count=False):
    """rows: tuples with None for NULL (DOUBLE cells as floats).  Groups in first-occurrence order; aggs: [(fn, column index, is_double)];
    -> [group cells + (COUNT(*) if count) + aggregate cells], an aggregate without a non-NULL cell is None.  Sums of floats are taken
    exactly (math.fsum): the tests' DOUBLE cells are multiples of 1/8, whose sums are exact in every order."""
    groups, order = {}, []
    for r in rows:
        k = tuple(r[c] for c in group_cols)
        if k not in groups:
            groups[k] = []
            order.append(k)
        groups[k].append(r)
    out = []
    for k in order:
        cells = list(k) + ([len(groups[k])] if count else [])
        for fn, c, is_double in aggs:
            xs = [r[c] for r in groups[k] if r[c] is not None]
            if not xs:
                cells.append(None)
            elif fn == "MIN":
                cells.append(min(xs))
            elif fn == "MAX":
                cells.append(max(xs))
            else:
                s = math.fsum(xs) if is_double else wrap64(sum(xs))
                cells.append(s if fn == "SUM" else float(s) / float(len(xs)))
        out.append(tuple(cells))
    return out


def sql_rows(db, sql):
    """-> (names, types, rows): DOUBLE cells as floats, NULL as None"""
    res = db.query(sql, step_cursor=True)
    rows = []
    for i in range(res.nrows):
        rows.append(tuple(None if res.nulls[c][i] else (float(as_double(int(res.columns[c][i]))) if res.types[c] == 3 else int(res.columns[c][i]))
                          for c in range(len(res.names))))
    return res.names, res.types, rows


def reference_order(keys):
    """the result column order of the reference (mdb_reference_column_order) over these column names"""
    from midoridb_amd.lib import load_library
    lib = load_library()
    lib.mdb_reference_column_order.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.mdb_reference_column_order.restype = ctypes.c_int
    buf = ctypes.create_string_buffer(128 * len(keys))
    for i, k in enumerate(keys):
        buf[128 * i:128 * i + len(k)] = k.encode()
    order = (ctypes.c_int * len(keys))()
    assert lib.mdb_reference_column_order(buf, len(keys), order) == 0
    return [keys[i] for i in order]


def by_name(names, rows, wanted):
    idx = [names.index(w) for w in wanted]
    return [tuple(r[i] for i in idx) for r in rows]


A_COLS = ["A.k", "A.k2", "A.v", "A.d", "A.t", "A.u", "A.b", "A.pk"]


@pytest.fixture(scope="module")
def world():
    """A: 3000 rows, 40 values of k (one of them NULL), NULL cells everywhere but in pk; B: duplicated keys, some without partner in A"""
    from midoridb_amd.query import DB
    rng = np.random.default_rng(42)
    n = 3000
    k = rng.integers(0, 40, n).astype(np.int64) * 1000003 - 17
    k2 = rng.integers(0, 3, n).astype(np.int64)
    v = rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int64)
    v[rng.random(n) < 0.02] = I64_MAX
    v[rng.random(n) < 0.02] = I64_MIN
    d = eighths(rng, n)
    t = 1577833200 + 86400 * rng.integers(0, 400, n).astype(np.int64)
    u = 1577833200 + rng.integers(0, 10 ** 7, n).astype(np.int64)
    b = rng.integers(0, 2, n).astype(np.int64)
    pk = rng.permutation(n).astype(np.int64) + 5
    cols = [k, k2, v, d, t, u, b, pk]
    nulls = [rng.random(n) < 0.03, np.zeros(n, dtype=bool)] + [rng.random(n) < 0.1 for _ in range(5)] + [np.zeros(n, dtype=bool)]
    nulls[2] |= k == k[0]                       # the group of the first row: every v NULL
    db = DB()
    db.execute("CREATE TABLE A (k INT, k2 INT, v INT, d DOUBLE, t DATE, u DATETIME, b TINYINT, pk INT PRIMARY KEY);")
    db.append_columns("A", [c.view(np.int64) if c.dtype == np.float64 else c for c in cols], [x.astype(np.uint8) for x in nulls])
    A = [tuple(None if nulls[c][i] else (float(cols[c][i]) if c == 3 else int(cols[c][i])) for c in range(8)) for i in range(n)]
    m = 5000
    kb = rng.integers(0, 50, m).astype(np.int64) * 1000003 - 17           # values 40 ... 49 have no partner in A
    w = rng.integers(-1000, 1000, m).astype(np.int64)
    e = eighths(rng, m)
    bn = [rng.random(m) < 0.03, rng.random(m) < 0.1, rng.random(m) < 0.1]
    db.execute("CREATE TABLE B (kb INT, w INT, e DOUBLE);")
    db.append_columns("B", [kb, w, e.view(np.int64)], [x.astype(np.uint8) for x in bn])
    B = [tuple(None if bn[c][i] else (float(e[i]) if c == 2 else int((kb, w)[c][i])) for c in range(3)) for i in range(m)]
    db.execute("CREATE TABLE E (k INT, v INT, d DOUBLE);")
    yield db, A, B
    db.close()


ALL8 = [("SUM", 2, False), ("MIN", 2, False), ("MAX", 2, False), ("AVG", 2, False), ("SUM", 3, True), ("AVG", 3, True), ("MIN", 3, True), ("MAX", 4, False)]
ALL8_SQL = "SUM(v), MIN(v), MAX(v), AVG(v), SUM(d), AVG(d), MIN(d), MAX(t)"
ALL8_NAMES = ["SUM(A.v)", "MIN(A.v)", "MAX(A.v)", "AVG(A.v)", "SUM(A.d)", "AVG(A.d)", "MIN(A.d)", "MAX(A.t)"]
ALL8_TYPES = [1, 1, 1, 3, 3, 3, 3, 4]


def test_sql_ungrouped_all_functions_with_count(world):
    db, A, B = world
    names, types, rows = sql_rows(db, f"SELECT {ALL8_SQL}, COUNT(*) FROM A;")
    assert names == [x for x in reference_order(["COUNT(*)"] + ALL8_NAMES + A_COLS) if x not in A_COLS]      # every column through the reference's order
    assert [types[names.index(x)] for x in ALL8_NAMES + ["COUNT(*)"]] == ALL8_TYPES + [1]
    assert by_name(names, rows, ["COUNT(*)"] + ALL8_NAMES) == naive(A, [], ALL8, count=True)
    # a WHERE clause thins the stream before it is one group; types of MIN / MAX are the column's own (DATETIME 5, TINYINT 2)
    names, types, rows = sql_rows(db, "SELECT MIN(u), MAX(b), SUM(b), AVG(b) FROM A WHERE k2 = 1 AND v > 0;")
    assert [types[names.index(x)] for x in ["MIN(A.u)", "MAX(A.b)", "SUM(A.b)", "AVG(A.b)"]] == [5, 2, 1, 3]
    kept = [r for r in A if r[1] == 1 and r[2] is not None and r[2] > 0]
    assert by_name(names, rows, ["MIN(A.u)", "MAX(A.b)", "SUM(A.b)", "AVG(A.b)"]) == naive(kept, [], [("MIN", 5, False), ("MAX", 6, False), ("SUM", 6, False), ("AVG", 6, False)])


def test_sql_grouped_one_and_two_columns_aliases_and_counters(world):
    db, A, B = world
    c0 = db.aggregate_calls()
    names, types, rows = sql_rows(db, f"SELECT k, {ALL8_SQL}, COUNT(*) FROM A GROUP BY k;")
    assert names == [x for x in reference_order(["COUNT(*)"] + ALL8_NAMES + A_COLS) if x not in A_COLS[1:]]
    assert by_name(names, rows, ["A.k", "COUNT(*)"] + ALL8_NAMES) == naive(A, [0], ALL8, count=True)
    assert db.aggregate_calls() == (c0[0], c0[1] + 1)           # SUM(d): a floating-point sum takes the sorted form
    names, types, rows = sql_rows(db, "SELECT k, SUM(v) AS total, MIN(A.d) lo, MAX(t) FROM A GROUP BY k;")
    assert sorted(names) == sorted(["A.k", "total", "lo", "MAX(A.t)"])
    assert by_name(names, rows, ["A.k", "total", "lo", "MAX(A.t)"]) == naive(A, [0], [("SUM", 2, False), ("MIN", 3, True), ("MAX", 4, False)])
    assert db.aggregate_calls() == (c0[0] + 1, c0[1] + 1)       # order-free aggregates, one key column, 40 groups: the LDS form
    names, types, rows = sql_rows(db, "SELECT k, k2, SUM(v), AVG(d), COUNT(*) FROM A GROUP BY k, k2;")
    assert by_name(names, rows, ["A.k", "A.k2", "COUNT(*)", "SUM(A.v)", "AVG(A.d)"]) == naive(A, [0, 1], [("SUM", 2, False), ("AVG", 3, True)], count=True)
    names, types, rows = sql_rows(db, "SELECT k2, k, MAX(v) FROM A GROUP BY k, k2;")
    assert by_name(names, rows, ["A.k", "A.k2", "MAX(A.v)"]) == naive(A, [0, 1], [("MAX", 2, False)])
    assert db.aggregate_calls() == (c0[0] + 1, c0[1] + 3)       # two key columns: sorted segments
    # the same aggregate twice is one result column
    names, types, rows = sql_rows(db, "SELECT SUM(v), k, SUM(A.v) FROM A GROUP BY k;")
    assert sorted(names) == ["A.k", "SUM(A.v)"]


def test_sql_having_order_by_limit_distinct_where(world):
    db, A, B = world
    g = naive(A, [0], [("SUM", 2, False), ("AVG", 3, True)], count=True)         # (k, COUNT, SUM(v), AVG(d))
    names, types, rows = sql_rows(db, "SELECT k, SUM(v), AVG(d), COUNT(*) FROM A GROUP BY k HAVING SUM(v) > 1000;")
    assert by_name(names, rows, ["A.k", "COUNT(*)", "SUM(A.v)", "AVG(A.d)"]) == [r for r in g if r[2] is not None and r[2] > 1000]
    names, types, rows = sql_rows(db, "SELECT k, SUM(v) AS s, AVG(d), COUNT(*) FROM A GROUP BY k HAVING s <= 1000 AND AVG(d) > 0.0;")
    assert by_name(names, rows, ["A.k", "COUNT(*)", "s", "AVG(A.d)"]) == [r for r in g if r[2] is not None and r[2] <= 1000 and r[3] is not None and r[3] > 0.0]
    # ORDER BY an aggregate: NULL sorts before every value, so DESC puts it last; ties keep the groups' order
    ranked = sorted(g, key=lambda r: (r[2] is not None, r[2] if r[2] is not None else 0), reverse=True)
    names, types, rows = sql_rows(db, "SELECT k, SUM(v) FROM A GROUP BY k ORDER BY SUM(v) DESC LIMIT 3;")
    assert by_name(names, rows, ["A.k", "SUM(A.v)"]) == [(r[0], r[2]) for r in ranked[:3]]
    names, types, rows = sql_rows(db, "SELECT k, SUM(v) AS s FROM A GROUP BY k ORDER BY s;")
    assert [r[names.index("s")] for r in rows] == [r[2] for r in sorted(g, key=lambda r: (r[2] is not None, r[2] if r[2] is not None else 0))]
    names, types, rows = sql_rows(db, "SELECT k, AVG(d) FROM A GROUP BY k ORDER BY AVG(A.d) DESC LIMIT 2, 4;")
    by_avg = sorted(g, key=lambda r: (r[3] is not None, r[3] if r[3] is not None else 0.0), reverse=True)
    assert by_name(names, rows, ["A.k", "AVG(A.d)"]) == [(r[0], r[3]) for r in by_avg[2:6]]
    # DISTINCT over the grouped stream: MAX(b) per (k, k2) has three values (0, 1, NULL) at most
    per = naive(A, [0, 1], [("MAX", 6, False)])
    seen, want = set(), []
    for r in per:
        if (r[1], r[2]) not in seen:
            seen.add((r[1], r[2]))
            want.append((r[1], r[2]))
    names, types, rows = sql_rows(db, "SELECT DISTINCT k2, MAX(b) FROM A GROUP BY k, k2;")
    assert by_name(names, rows, ["A.k2", "MAX(A.b)"]) == want and len(want) < len(per)
    # WHERE before grouping
    kept = [r for r in A if r[1] is not None and r[1] != 1 and r[3] is not None and r[3] < 100.0]
    names, types, rows = sql_rows(db, "SELECT k, SUM(d), MIN(v) FROM A WHERE k2 <> 1 AND d < 100.0 GROUP BY k;")
    assert by_name(names, rows, ["A.k", "SUM(A.d)", "MIN(A.v)"]) == naive(kept, [0], [("SUM", 3, True), ("MIN", 2, False)])


def test_sql_joins_take_the_materialising_plan(world):
    """A JOIN B ... GROUP BY A.k with B's keys duplicated: for COUNT(*) alone the fused join + GROUP BY operator answers (no joined row
    exists anywhere); beside SUM(B.w) the join is materialised and the result's joined_rows says so"""
    db, A, B = world
    Bk = {}
    for b in B:
        if b[0] is not None:
            Bk.setdefault(b[0], []).append(b)
    J = [a + b for a in A if a[0] is not None for b in Bk.get(a[0], [])]
    res = db.query("SELECT k, SUM(w), SUM(e), MAX(pk), COUNT(*) FROM A JOIN B ON A.k = B.kb GROUP BY k;", step_cursor=True)
    assert res.joined_rows == len(J) > len(A)
    names, types, rows = sql_rows(db, "SELECT k, SUM(w), SUM(e), MAX(pk), COUNT(*) FROM A JOIN B ON A.k = B.kb GROUP BY k;")
    assert by_name(names, rows, ["A.k", "COUNT(*)", "SUM(B.w)", "SUM(B.e)", "MAX(A.pk)"]) == naive(J, [0], [("SUM", 9, False), ("SUM", 10, True), ("MAX", 7, False)], count=True)
    assert by_name(names, rows, ["A.k", "COUNT(*)"]) == by_name(*sql_rows(db, "SELECT k, COUNT(*) FROM A JOIN B ON A.k = B.kb GROUP BY k;")[::2], ["A.k", "COUNT(*)"])
    # LEFT JOIN: a row of A without partner contributes NULL cells of B - skipped; a group without any partner is NULL
    L = []
    for a in A:
        hit = [a + b for b in Bk.get(a[0], [])] if a[0] is not None else []
        L += hit if hit else [a + (None, None, None)]
    names, types, rows = sql_rows(db, "SELECT k2, SUM(w), MIN(e), AVG(w), COUNT(*) FROM A LEFT JOIN B ON A.k = B.kb WHERE pk < 400 GROUP BY k2;")
    Lw = [r for r in L if r[7] < 400]
    assert by_name(names, rows, ["A.k2", "COUNT(*)", "SUM(B.w)", "MIN(B.e)", "AVG(B.w)"]) == naive(Lw, [1], [("SUM", 9, False), ("MIN", 10, True), ("AVG", 9, False)], count=True)
    names, types, rows = sql_rows(db, "SELECT pk, SUM(w) FROM A LEFT JOIN B ON A.k = B.kb WHERE pk < 40 GROUP BY pk;")
    Lp = [r for r in L if r[7] < 40]
    assert by_name(names, rows, ["A.pk", "SUM(B.w)"]) == naive(Lp, [7], [("SUM", 9, False)])
    assert any(r[1] is None for r in by_name(names, rows, ["A.pk", "SUM(B.w)"]))
    names, types, rows = sql_rows(db, "SELECT SUM(v), MAX(w) FROM B RIGHT JOIN A ON A.k = B.kb WHERE pk < 400;")
    assert by_name(names, rows, ["SUM(A.v)", "MAX(B.w)"]) == naive(Lw, [], [("SUM", 2, False), ("MAX", 9, False)])


def test_sql_group_by_a_measured_distinct_key_is_the_identity(world):
    """GROUP BY over a PRIMARY KEY column measured to hold no value twice: group i is row i - the cells themselves, converted for AVG, NULL
    kept; neither form's counter moves"""
    db, A, B = world
    c0 = db.aggregate_calls()
    names, types, rows = sql_rows(db, "SELECT pk, SUM(v), AVG(v), MIN(d), MAX(t), AVG(d), COUNT(*) FROM A GROUP BY pk;")
    want = naive(A, [7], [("SUM", 2, False), ("AVG", 2, False), ("MIN", 3, True), ("MAX", 4, False), ("AVG", 3, True)], count=True)
    assert by_name(names, rows, ["A.pk", "COUNT(*)", "SUM(A.v)", "AVG(A.v)", "MIN(A.d)", "MAX(A.t)", "AVG(A.d)"]) == want and len(want) == len(A)
    assert db.aggregate_calls() == c0


def test_sql_empty_input_gives_no_row(world):
    db, A, B = world
    for sql in ["SELECT SUM(v) FROM E;", "SELECT SUM(v), COUNT(*) FROM E;", "SELECT k, SUM(d) FROM E GROUP BY k;", "SELECT AVG(v), MIN(d) FROM A WHERE pk < 0;",
                "SELECT k, MAX(v) FROM A WHERE pk < 0 GROUP BY k;", "SELECT SUM(v) FROM A LIMIT 0;"]:
        assert sql_rows(db, sql)[2] == [], sql
    assert sql_rows(db, "SELECT COUNT(*) FROM E;")[2] == []            # (what the two must stay consistent with)
    assert sql_rows(db, "SELECT SUM(v) FROM A WHERE v IS NULL;")[2] == [(None,)]     # rows, but no non-NULL cell: one row, NULL


def test_sql_results_kept_on_the_device(world):
    db, A, B = world
    want = naive(A, [0], [("SUM", 2, False), ("AVG", 3, True), ("MIN", 4, False)])
    db.results_on_device(True)
    try:
        names, types, cols, nrows, joined, ms = db.query_device("SELECT k, SUM(v), AVG(d), MIN(t) FROM A GROUP BY k;")
        nulls = db.last_device_nulls
    finally:
        db.results_on_device(False)
    assert nrows == len(want)
    got = []
    for i in range(nrows):
        row = []
        for w in ["A.k", "SUM(A.v)", "AVG(A.d)", "MIN(A.t)"]:
            c = names.index(w)
            isnull = nulls[c] is not None and bool(nulls[c][i])
            row.append(None if isnull else (float(cols[c][i]) if types[c] == 3 else int(cols[c][i])))
        got.append(tuple(row))
    assert got == want
    assert [types[names.index(w)] for w in ["SUM(A.v)", "AVG(A.d)", "MIN(A.t)"]] == [1, 3, 4]


def test_sql_many_groups_cross_the_lds_limit(dev):
    """one group column and order-free aggregates: the LDS form up to mdb_dev_group_aggregate_lds_groups(naggs) groups, sorted segments
    beyond - the counters say which, the rows are the same kind of rows"""
    from midoridb_amd.query import DB
    lds = dev.group_aggregate_lds_groups(2)
    rng = np.random.default_rng(8)
    with DB() as db:
        db.execute("CREATE TABLE T (k INT, v INT);")
        n = 3 * (lds + 1)
        k = (np.arange(n, dtype=np.int64) % (lds + 1)) * 7 - 100
        v = rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int64)
        db.append_columns("T", [k, v])
        T = [(int(k[i]), int(v[i])) for i in range(n)]
        c0 = db.aggregate_calls()
        names, types, rows = sql_rows(db, f"SELECT k, SUM(v), MAX(v) FROM T WHERE k < {int(k[lds])} GROUP BY k;")
        assert by_name(names, rows, ["T.k", "SUM(T.v)", "MAX(T.v)"]) == naive([r for r in T if r[0] < int(k[lds])], [0], [("SUM", 1, False), ("MAX", 1, False)])
        assert db.aggregate_calls() == (c0[0] + 1, c0[1]) and len(rows) == lds
        names, types, rows = sql_rows(db, "SELECT k, SUM(v), MAX(v) FROM T GROUP BY k;")
        assert by_name(names, rows, ["T.k", "SUM(T.v)", "MAX(T.v)"]) == naive(T, [0], [("SUM", 1, False), ("MAX", 1, False)])
        assert db.aggregate_calls() == (c0[0] + 1, c0[1] + 1) and len(rows) == lds + 1


def test_sharded_mode_refuses_the_aggregates():
    """at world 2 on one GPU (the test transport of tests/_dist_gpu_worker.py): every rank gets the refusal, before any exchange"""
    from tests.test_dist_gpu import _run
    out = _run("agg", 2, 29633, worker="_aggregate_dist_worker.py", timeout=300)
    assert "sharded aggregates refused ok" in out
