"""COUNT(DISTINCT col) on the device (mdb_dev_group_count_distinct and the statements that reach it).  An extension - upstream knows
COUNT(*) only - so nothing here is pinned to the reference: the operator is checked against a numpy restatement (`expect`: per group
len(np.unique(canonical non-NULL cells)), -0.0 taken as +0.0), the statements against SQLite and against a naive restatement over Python
lists (`naive`).  Streams, columns and the statement helpers are those of tests/test_aggregate_gpu.py."""
import sqlite3

import numpy as np
import pytest

from tests.test_aggregate_gpu import Column, by_name, make_stream, null_cells, run_head_cases, run_head_id, sql_rows, stream_with_run_heads

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
ROWS = [1, 63, 64, 65, 4095, 4096, 4097, 2 ** 18 + 1]
KNOB = "MDB_COUNT_DISTINCT_BITMAP"


# ------------------------------------------------------------------------------------------------ numpy restatement of the operator

def canonical(cells, is_double):
    """the 8-byte cells as int64 bits; DOUBLE: -0.0 is +0.0 (mdb_set_canonical)"""
    c = cells.copy()
    if is_double:
        c[(c.view(np.uint64) << np.uint64(1)) == 0] = 0
    return c


def expect(gid, G, cells, valid, is_double):
    """out[g] = len(np.unique(canonical cells of group g)) - for all groups at once: the valid (group, cell) pairs in order, every pair that
    differs from the one before counts for its group.  Up to 65 groups the sentence is also evaluated word for word."""
    c, g = canonical(cells, is_double)[valid], gid[valid]
    order = np.lexsort((c, g))
    c, g = c[order], g[order]
    new = np.ones(len(c), dtype=bool)
    new[1:] = (c[1:] != c[:-1]) | (g[1:] != g[:-1])
    out = np.bincount(g[new], minlength=G).astype(np.int64)
    if G <= 65:
        assert out.tolist() == [len(np.unique(c[g == k])) for k in range(G)]
    return out


def ranged_cells(rng, n, gid, G, lo, span, vnull):
    """cells in [lo, lo + span), both ends present in non-NULL cells where two such cells exist"""
    v = lo + rng.integers(0, span, n).astype(np.int64)
    free = np.nonzero(gid != 1)[0] if G >= 3 else np.arange(n)      # (null_cells makes every cell of group 1 NULL)
    if len(free) >= 2:
        v[free[0]], v[free[-1]] = lo, lo + span - 1
        vnull[free[0]] = vnull[free[-1]] = False
    return v


def full_range_cells(rng, n):
    v = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    v[rng.random(n) < 0.3] = rng.integers(-3, 3)
    v[rng.random(n) < 0.1] = I64_MIN
    v[rng.random(n) < 0.1] = I64_MAX
    if n >= 2:
        v[0], v[-1] = I64_MIN, I64_MAX
    return v


def double_cells(rng, n):
    """few different values, many repeats, both zeros"""
    d = rng.integers(-4, 5, n).astype(np.float64) / 4.0
    d[rng.random(n) < 0.2] = -0.0
    d[rng.random(n) < 0.2] = 0.0
    return d.view(np.int64)


def run_and_check(dev, D, keys, n, first, G, gid, cols, want_forms):
    """cols: [(type, Column, (min, max) or None)]; every count against the restatement; -> the counts"""
    outs, forms = dev.group_count_distinct(keys, n, first, [(ty, c.values, c.nullbits, c.rid, rng_) for ty, c, rng_ in cols], groups=G)
    assert forms == want_forms, (forms, want_forms, n, G)
    got = []
    for i, ((ty, c, _), o) in enumerate(zip(cols, outs)):
        e = expect(gid, G, c.cells, c.valid, ty == D.T_DOUBLE)
        g = o.cpu().numpy()
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, (i, ty, n, G, bad[:5], g[bad[:5]], e[bad[:5]])
        got.append(g)
    return got


def both_ways(dev, D, monkeypatch, keys, n, first, G, gid, cols, want_forms):
    """as the forms decide, then every column through the sorted form (the knob): the same counts"""
    a = run_and_check(dev, D, keys, n, first, G, gid, cols, want_forms)
    monkeypatch.setenv(KNOB, "0")
    dev.lib.mdb_dev_reload_knobs()
    try:
        b = run_and_check(dev, D, keys, n, first, G, gid, cols, [3 if f == 3 else 2 for f in want_forms])
    finally:
        monkeypatch.delenv(KNOB)
        dev.lib.mdb_dev_reload_knobs()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    return a


@pytest.mark.parametrize("n", ROWS)
def test_operator_every_row_and_group_count(dev, monkeypatch, n):
    """INT64 cells inside ranges of 1, 64, 65 and 1000 values with both ends present (bitmap: the word edge of a group's words), full-range
    INT64 cells with INT64_MIN and INT64_MAX among them - without a range, and with one whose span overflows -, DOUBLE cells with both
    zeros: 10 % NULL cells, a group that is all NULL (count 0), a NULL group key, a column read through row ids with MDB_NO_ROW, a column
    8 bytes off a 16-byte boundary.  One key: the LDS table up to its group limit, sorted runs beyond (G = n from 4097 rows on).  All seven
    columns in ONE call, in different forms; then all again through the sorted form."""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(7000 + n)
    for G in sorted({g for g in (1, 2, 3, 65, n) if g <= n}):
        gid, first, keys, knull = make_stream(rng, n, G)
        kcol = Column(dev, D, rng, keys, knull, misaligned=(G % 2 == 0))
        dkeys = [(kcol.values, kcol.nullbits, None, D.T_INT64, False)]
        cols = []
        for span, kw in ((1, {}), (64, {"misaligned": True}), (65, {"through_rid": True}), (1000, {})):
            vnull = null_cells(rng, gid, G, n)
            lo = int(rng.integers(-2000, 2000))
            v = ranged_cells(rng, n, gid, G, lo, span, vnull)
            cols.append((D.T_INT64, Column(dev, D, rng, v, vnull, **kw), (lo, lo + span - 1)))
        vnull = null_cells(rng, gid, G, n)
        wide = full_range_cells(rng, n)
        cols.append((D.T_INT64, Column(dev, D, rng, wide, vnull, through_rid=True), None))
        cols.append((D.T_INT64, Column(dev, D, rng, wide, vnull, misaligned=True), (I64_MIN, I64_MAX)))
        cols.append((D.T_DOUBLE, Column(dev, D, rng, double_cells(rng, n), vnull, misaligned=True), None))
        got = both_ways(dev, D, monkeypatch, dkeys, n, dev.to_dev(first), G, gid, cols, [1, 1, 1, 1, 2, 2, 2])
        if G >= 3:
            assert all(int(g[1]) == 0 for g in got)             # the group whose cells are all NULL counts 0


def test_operator_step_a_lds_table_and_sorted_runs_agree(dev, monkeypatch):
    """the same rows grouped by one key (the LDS table) and by two (sorted runs; the second key is constant or splits nothing): the same
    counts; a DOUBLE key compares by its bits"""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(71)
    n, G = 20000, 300
    assert G <= dev.group_count_distinct_lds_groups() < n
    gid, first, keys, knull = make_stream(rng, n, G)
    kcol = Column(dev, D, rng, keys, knull)
    const = dev.to_dev(np.full(n, 7, dtype=np.int64))
    same = Column(dev, D, rng, (gid % 5).astype(np.float64).view(np.int64), np.zeros(n, dtype=bool))       # a function of the group
    vnull = null_cells(rng, gid, G, n)
    v = ranged_cells(rng, n, gid, G, -30, 90, vnull)
    cols = [(D.T_INT64, Column(dev, D, rng, v, vnull), (-30, 59)), (D.T_DOUBLE, Column(dev, D, rng, double_cells(rng, n), vnull, through_rid=True), None)]
    k1 = (kcol.values, kcol.nullbits, None, D.T_INT64, False)
    dfirst = dev.to_dev(first)
    a = both_ways(dev, D, monkeypatch, [k1], n, dfirst, G, gid, cols, [1, 2])
    b = both_ways(dev, D, monkeypatch, [k1, (const, None, None, D.T_INT64, False)], n, dfirst, G, gid, cols, [1, 2])
    c = both_ways(dev, D, monkeypatch, [(same.values, None, None, D.T_DOUBLE, True), k1], n, dfirst, G, gid, cols, [1, 2])
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c))
    # twice the same call: the same bytes
    again = run_and_check(dev, D, [k1], n, dfirst, G, gid, cols, [1, 2])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, again))


@pytest.mark.parametrize("case", run_head_cases(), ids=run_head_id)
def test_operator_sorted_runs_heads_at_chunk_and_word_edges(dev, monkeypatch, case):
    """two key columns - sorted runs whatever G is: one run, a run per row, and three runs whose heads are the last position of a
    1024-position chunk, the first of the next, position 63 / 64 of a word of head bits and the stream's last row (n around one and two
    chunks).  A ranged and a DOUBLE column, as the forms decide and both sorted: exactly the restatement's counts"""
    from midoridb_amd import dev as D
    n, heads = case
    rng = np.random.default_rng(7600 + n + len(heads) + heads[-1])
    gid, first, (k1, k1null), (k2, k2null) = stream_with_run_heads(rng, n, heads)
    G = len(heads)
    c1, c2 = Column(dev, D, rng, k1, k1null, misaligned=True), Column(dev, D, rng, k2, k2null)
    dkeys = [(c1.values, c1.nullbits, None, D.T_INT64, False), (c2.values, c2.nullbits, None, D.T_INT64, False)]
    vnull = null_cells(rng, gid, G, n)
    v = ranged_cells(rng, n, gid, G, -7, 40, vnull)
    cols = [(D.T_INT64, Column(dev, D, rng, v, vnull, through_rid=True), (-7, 32)),
            (D.T_DOUBLE, Column(dev, D, rng, double_cells(rng, n), vnull), None)]
    both_ways(dev, D, monkeypatch, dkeys, n, dev.to_dev(first), G, gid, cols, [1, 2])


def test_operator_long_spans_and_the_bitmap_bound(dev, monkeypatch):
    """a group of more than 1024 words is counted by a workgroup; G x (span rounded up to 64) at MDB_COUNT_DISTINCT_BITMAP_BITS exactly
    is the bitmap form, one value more is the sorted form (one group and a wide promised range: the cells are few)"""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(72)
    n, G = 50000, 3
    gid, first, keys, knull = make_stream(rng, n, G)
    kcol = Column(dev, D, rng, keys, knull)
    vnull = null_cells(rng, gid, G, n)
    span = 64 * 1024 + 1
    v = ranged_cells(rng, n, gid, G, 10 ** 12, span, vnull)
    cols = [(D.T_INT64, Column(dev, D, rng, v, vnull), (10 ** 12, 10 ** 12 + span - 1))]
    both_ways(dev, D, monkeypatch, [(kcol.values, kcol.nullbits, None, D.T_INT64, False)], n, dev.to_dev(first), G, gid, cols, [1])
    bits = dev.count_distinct_bitmap_bits()
    assert bits == 1 << 30
    m = 4097
    w = rng.integers(0, bits, m).astype(np.int64)
    w[0], w[-1] = 0, bits - 1
    col = Column(dev, D, rng, w, np.zeros(m, dtype=bool))
    zero = np.zeros(m, dtype=np.int64)
    got = run_and_check(dev, D, [], m, None, 1, zero, [(D.T_INT64, col, (0, bits - 1)), (D.T_INT64, col, (0, bits)), (D.T_INT64, col, (-1, bits - 1))], [1, 2, 2])
    assert int(got[0][0]) == len(np.unique(w))
    # with groups: G x 64 bits per group
    gid2, first2, keys2, knull2 = make_stream(rng, m, m, null_key=False)
    k2 = dev.to_dev(keys2)
    inside, outside = (0, 64 * (bits // 64 // m) - 1), (0, 64 * (bits // 64 // m))
    small = Column(dev, D, rng, rng.integers(0, 50, m).astype(np.int64), np.zeros(m, dtype=bool))
    run_and_check(dev, D, [(k2, None, None, D.T_INT64, False)], m, dev.to_dev(first2), m, gid2, [(D.T_INT64, small, inside), (D.T_INT64, small, outside)], [1, 2])


def test_operator_a_range_that_lies_gives_the_sorted_form_and_right_counts(dev):
    """the promised range misses one cell (the true max + 1 is present; then a cell below min): counts are right, the form is 2, the
    context serves the next call"""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(73)
    n, G = 4097, 65
    gid, first, keys, knull = make_stream(rng, n, G)
    kcol = Column(dev, D, rng, keys, knull)
    dkeys, dfirst = [(kcol.values, kcol.nullbits, None, D.T_INT64, False)], dev.to_dev(first)
    vnull = null_cells(rng, gid, G, n)
    v = ranged_cells(rng, n, gid, G, 100, 200, vnull)
    honest = Column(dev, D, rng, v, vnull)
    run_and_check(dev, D, dkeys, n, dfirst, G, gid, [(D.T_INT64, honest, (100, 299))], [1])
    for pos, value in ((n // 2, 300), (n - 2, 99), (0, I64_MIN), (3, I64_MAX)):
        w, wnull = v.copy(), vnull.copy()
        w[pos], wnull[pos] = value, False
        liar = Column(dev, D, rng, w, wnull)
        run_and_check(dev, D, dkeys, n, dfirst, G, gid, [(D.T_INT64, liar, (100, 299)), (D.T_INT64, honest, (100, 299))], [2, 1])
    run_and_check(dev, D, dkeys, n, dfirst, G, gid, [(D.T_INT64, honest, (100, 299))], [1])
    # a range with nothing in it (max < min) is no promise at all
    run_and_check(dev, D, dkeys, n, dfirst, G, gid, [(D.T_INT64, honest, (5, 4))], [2])


def test_operator_refuses_first_rows_that_do_not_belong_to_the_keys(dev):
    from midoridb_amd import dev as D
    from midoridb_amd.dev import DeviceError
    keys = dev.to_dev(np.array([1, 2, 3, 1, 2, 3, 4], dtype=np.int64))
    const = dev.to_dev(np.zeros(7, dtype=np.int64))
    v = dev.to_dev(np.arange(7, dtype=np.int64) % 3)
    first = dev.to_dev(np.array([0, 1, 2], dtype=np.int32))               # the group of key 4 is missing
    k1 = (keys, None, None, D.T_INT64, False)
    for dkeys in ([k1], [k1, (const, None, None, D.T_INT64, False)]):    # the LDS table; sorted runs
        with pytest.raises(DeviceError) as ei:
            dev.group_count_distinct(dkeys, 7, first, [(D.T_INT64, v, None, None, (0, 2))])
        assert "group_count_distinct" in str(ei.value)
    wrong = dev.to_dev(np.array([0, 1, 2, 5], dtype=np.int32))            # as many groups as runs, but row 5 is nobody's first row
    with pytest.raises(DeviceError) as ei:
        dev.group_count_distinct([k1, (const, None, None, D.T_INT64, False)], 7, wrong, [(D.T_INT64, v, None, None, None)])
    assert "belongs to no group" in str(ei.value)
    good = dev.to_dev(np.array([0, 1, 2, 6], dtype=np.int32))
    for dkeys in ([k1], [k1, (const, None, None, D.T_INT64, False)]):
        outs, forms = dev.group_count_distinct(dkeys, 7, good, [(D.T_INT64, v, None, None, (0, 2)), (D.T_INT64, v, None, None, None)])
        assert forms == [1, 2] and outs[0].tolist() == outs[1].tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_operator_without_keys_and_identity(dev, monkeypatch, n):
    """nkeys == 0: one group over all rows (first may be None); MDB_AGG_IDENTITY: group i is row i - 1 for a valid cell, else 0; a column
    whose cells are all NULL counts 0"""
    from midoridb_amd import dev as D
    rng = np.random.default_rng(7400 + n)
    vnull = rng.random(n) < 0.1
    v = 5 + rng.integers(0, 40, n).astype(np.int64)
    vi = Column(dev, D, rng, v, vnull.copy(), through_rid=True)
    vd = Column(dev, D, rng, double_cells(rng, n), vnull.copy(), misaligned=True)
    allnull = Column(dev, D, rng, v, np.ones(n, dtype=bool))
    cols = [(D.T_INT64, vi, (5, 44)), (D.T_DOUBLE, vd, None), (D.T_INT64, allnull, (5, 44)), (D.T_INT64, allnull, None)]
    got = both_ways(dev, D, monkeypatch, [], n, None, 1, np.zeros(n, dtype=np.int64), cols, [1, 2, 1, 2])
    assert int(got[2][0]) == 0 and int(got[3][0]) == 0
    got = both_ways(dev, D, monkeypatch, D.AGG_IDENTITY, n, None, n, np.arange(n), cols, [3, 3, 3, 3])
    assert np.array_equal(got[0], vi.valid.astype(np.int64)) and not got[2].any()


# ------------------------------------------------------------------------------------------------ statements

def naive(rows, group_cols, cd_cols, count=False):
    """rows: tuples with None for NULL.  Groups in first-occurrence order -> [group cells + (COUNT(*) if count) + one count of different
    non-NULL cells per column of cd_cols]"""
    groups, order = {}, []
    for r in rows:
        k = tuple(r[c] for c in group_cols)
        if k not in groups:
            groups[k] = []
            order.append(k)
        groups[k].append(r)
    return [tuple(list(k) + ([len(groups[k])] if count else []) + [len({r[c] for r in groups[k] if r[c] is not None}) for c in cd_cols]) for k in order]


def none_first(r):
    return tuple((0, 0) if v is None else (1, v) for v in r)


@pytest.fixture(scope="module")
def world():
    """A: 3000 rows, 40 values of k and NULL (41 groups), NULL cells everywhere but in k2 and pk, every v of the first row's group NULL; B: one
    row for some of A's pk values, several for others, none for most.  The same tables in SQLite."""
    from midoridb_amd.query import DB
    rng = np.random.default_rng(43)
    n = 3000
    k = rng.integers(0, 40, n).astype(np.int64) * 1000003 - 17
    k2 = rng.integers(0, 3, n).astype(np.int64)
    v = rng.integers(-20, 80, n).astype(np.int64)
    d = rng.integers(-8, 9, n).astype(np.float64) / 8.0
    s = [f"s{int(x)}" for x in rng.integers(0, 25, n)]
    t = 1577833200 + 86400 * rng.integers(0, 30, n).astype(np.int64)
    pk = rng.permutation(n).astype(np.int64) + 5
    nulls = [rng.random(n) < 0.03, np.zeros(n, dtype=bool)] + [rng.random(n) < 0.1 for _ in range(4)] + [np.zeros(n, dtype=bool)]
    nulls[2] |= k == k[0]
    s = [None if nulls[4][i] else s[i] for i in range(n)]
    db = DB()
    db.execute("CREATE TABLE A (k INT, k2 INT, v INT, d DOUBLE, s VARCHAR(8), t DATE, pk INT PRIMARY KEY);")
    db.append_columns("A", [k, k2, v, d.view(np.int64), s, t, pk], [x.astype(np.uint8) for x in nulls[:4]] + [None] + [x.astype(np.uint8) for x in nulls[5:]])
    cols = [k, k2, v, d, s, t, pk]
    A = [tuple(None if nulls[c][i] else (float(d[i]) if c == 3 else s[i] if c == 4 else int(cols[c][i])) for c in range(7)) for i in range(n)]
    m = 2000
    kb = rng.integers(0, 1000, m).astype(np.int64) + 5                    # partners for pk values 5 ... 1004 only
    w = rng.integers(0, 12, m).astype(np.int64)
    wn = rng.random(m) < 0.2
    db.execute("CREATE TABLE B (kb INT, w INT);")
    db.append_columns("B", [kb, w], [None, wn.astype(np.uint8)])
    B = [(int(kb[i]), None if wn[i] else int(w[i])) for i in range(m)]
    db.execute("CREATE TABLE E (k INT, v INT, d DOUBLE);")
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE A (k INT, k2 INT, v INT, d DOUBLE, s TEXT, t INT, pk INT)")
    con.executemany("INSERT INTO A VALUES (?,?,?,?,?,?,?)", A)
    con.execute("CREATE TABLE B (kb INT, w INT)")
    con.executemany("INSERT INTO B VALUES (?,?)", B)
    con.execute("CREATE TABLE E (k INT, v INT, d DOUBLE)")
    yield db, A, B, con
    con.close()
    db.close()


def both(world, sql, wanted, ordered=False):
    """the statement's rows (the wanted columns by name) - checked against SQLite: as a multiset, or row for row under ORDER BY; every
    cell non-NULL where it is a count"""
    db, A, B, con = world
    names, types, rows = sql_rows(db, sql)
    got = by_name(names, rows, wanted)
    for nm in wanted:
        if nm.startswith("COUNT("):
            assert types[names.index(nm)] == 1 and all(r[names.index(nm)] is not None for r in rows), (sql, nm)
    lite = [tuple(r) for r in con.execute(sql.rstrip(";")).fetchall()]
    if ordered:
        assert got == lite, sql
    else:
        assert sorted(got, key=none_first) == sorted(lite, key=none_first), sql
    return got


def test_sql_without_group_by_and_the_form_counters(world):
    db, A, B, con = world
    c0 = db.count_distinct_calls()
    assert both(world, "SELECT COUNT(DISTINCT v) FROM A;", ["COUNT(DISTINCT A.v)"]) == naive(A, [], [2])
    assert db.count_distinct_calls() == (c0[0] + 1, c0[1])                # an INTEGER column of 100 values: the bitmap
    assert both(world, "SELECT COUNT(DISTINCT d) FROM A;", ["COUNT(DISTINCT A.d)"]) == naive(A, [], [3])
    assert db.count_distinct_calls() == (c0[0] + 1, c0[1] + 1)            # DOUBLE: sorted
    got = both(world, "SELECT COUNT(DISTINCT s), COUNT(DISTINCT t), COUNT(DISTINCT A.pk), COUNT(DISTINCT k) FROM A WHERE k2 = 1;",
               ["COUNT(DISTINCT A.s)", "COUNT(DISTINCT A.t)", "COUNT(DISTINCT A.pk)", "COUNT(DISTINCT A.k)"])
    assert got == naive([r for r in A if r[1] == 1], [], [4, 5, 6, 0])
    assert db.count_distinct_calls() == (c0[0] + 5, c0[1] + 1)            # VARCHAR ids, DATE, pk and k (4 * 10^7 values, one group): the bitmap


def test_sql_grouped_by_one_and_two_columns_beside_other_aggregates(world):
    db, A, B, con = world
    got = both(world, "SELECT k, COUNT(DISTINCT v) FROM A GROUP BY k;", ["A.k", "COUNT(DISTINCT A.v)"])
    assert got == naive(A, [0], [2]) and got[0][1] == 0 and len(got) == 41         # the first row's group: every v NULL, count 0 - not NULL
    got = both(world, "SELECT k, k2, COUNT(DISTINCT A.d) AS dd, COUNT(DISTINCT s) FROM A GROUP BY k, k2;", ["A.k", "A.k2", "dd", "COUNT(DISTINCT A.s)"])
    assert got == naive(A, [0, 1], [3, 4])
    a0, c0 = db.aggregate_calls(), db.count_distinct_calls()
    names, types, rows = sql_rows(db, "SELECT k, COUNT(*), SUM(v), AVG(d), COUNT(DISTINCT v), COUNT(DISTINCT t) FROM A GROUP BY k;")
    assert sum(db.aggregate_calls()) == sum(a0) + 1 and db.count_distinct_calls() == (c0[0] + 2, c0[1])
    assert by_name(names, rows, ["A.k", "COUNT(*)", "COUNT(DISTINCT A.v)", "COUNT(DISTINCT A.t)"]) == naive(A, [0], [2, 5], count=True)
    a0, c0 = db.aggregate_calls(), db.count_distinct_calls()
    both(world, "SELECT k2, COUNT(*), SUM(v), AVG(d), COUNT(DISTINCT v) FROM A GROUP BY k2;",
         ["A.k2", "COUNT(*)", "SUM(A.v)", "AVG(A.d)", "COUNT(DISTINCT A.v)"])
    assert sum(db.aggregate_calls()) == sum(a0) + 1 and sum(db.count_distinct_calls()) == sum(c0) + 1


def test_sql_over_the_joined_table_of_a_left_join(world):
    db, A, B, con = world
    got = both(world, "SELECT k, COUNT(DISTINCT w), COUNT(*) FROM A LEFT JOIN B ON A.pk = B.kb GROUP BY k;", ["A.k", "COUNT(DISTINCT B.w)", "COUNT(*)"])
    assert len(got) == 41 and all(r[1] is not None for r in got)
    got = both(world, "SELECT pk, COUNT(DISTINCT w) FROM A LEFT JOIN B ON A.pk = B.kb WHERE k2 = 2 GROUP BY pk;", ["A.pk", "COUNT(DISTINCT B.w)"])
    assert sum(1 for r in got if r[1] == 0) > 500 and max(r[1] for r in got) > 1       # unmatched rows: count 0, not NULL
    both(world, "SELECT COUNT(DISTINCT w), COUNT(DISTINCT kb) FROM A LEFT JOIN B ON A.pk = B.kb WHERE k2 = 0;", ["COUNT(DISTINCT B.w)", "COUNT(DISTINCT B.kb)"])


def test_sql_having_order_by_limit_distinct(world):
    db, A, B, con = world
    got = both(world, "SELECT k, COUNT(DISTINCT v) FROM A GROUP BY k HAVING COUNT(DISTINCT v) > 45;", ["A.k", "COUNT(DISTINCT A.v)"])
    assert got == [r for r in naive(A, [0], [2]) if r[1] > 45] and 0 < len(got) < 40
    both(world, "SELECT k, COUNT(DISTINCT v) AS z FROM A GROUP BY k HAVING z > 45 AND z < 60;", ["A.k", "z"])
    both(world, "SELECT k, COUNT(DISTINCT A.v) AS z FROM A GROUP BY k ORDER BY z DESC, k;", ["A.k", "z"], ordered=True)
    both(world, "SELECT k, COUNT(DISTINCT s) FROM A GROUP BY k ORDER BY COUNT(DISTINCT s), k DESC LIMIT 7;", ["A.k", "COUNT(DISTINCT A.s)"], ordered=True)
    got = both(world, "SELECT DISTINCT COUNT(DISTINCT v) FROM A GROUP BY k;", ["COUNT(DISTINCT A.v)"])
    assert len(got) == len(set(got)) < 40
    names, types, rows = sql_rows(db, "SELECT k, COUNT(DISTINCT v) FROM A GROUP BY k LIMIT 5;")
    assert by_name(names, rows, ["A.k", "COUNT(DISTINCT A.v)"]) == naive(A, [0], [2])[:5]


def test_sql_group_by_a_measured_distinct_key_is_the_identity(world):
    db, A, B, con = world
    c0 = db.count_distinct_calls()
    got = both(world, "SELECT pk, COUNT(*), COUNT(DISTINCT v), COUNT(DISTINCT d) FROM A GROUP BY pk;",
               ["A.pk", "COUNT(*)", "COUNT(DISTINCT A.v)", "COUNT(DISTINCT A.d)"])
    assert got == naive(A, [6], [2, 3], count=True) and len(got) == len(A) and {r[2] for r in got} == {0, 1}
    assert db.count_distinct_calls() == c0                               # group i is row i: neither form


def test_sql_empty_input_gives_no_row(world):
    db, A, B, con = world
    for sql in ["SELECT COUNT(DISTINCT v) FROM E;", "SELECT COUNT(DISTINCT v), COUNT(*) FROM E;", "SELECT k, COUNT(DISTINCT d) FROM E GROUP BY k;",
                "SELECT COUNT(DISTINCT v) FROM A WHERE pk < 0;", "SELECT k, COUNT(DISTINCT v) FROM A WHERE pk < 0 GROUP BY k;"]:
        assert sql_rows(db, sql)[2] == [], sql
    assert sql_rows(db, "SELECT COUNT(DISTINCT v) FROM A WHERE v IS NULL;")[2] == [(0,)]     # rows, but no non-NULL cell: one row, 0


def test_sql_result_column_name_and_place(world):
    from tests.test_aggregate_gpu import reference_order
    db, A, B, con = world
    cols = ["A.k", "A.k2", "A.v", "A.d", "A.s", "A.t", "A.pk"]
    names, types, rows = sql_rows(db, "SELECT COUNT(DISTINCT v), SUM(v), COUNT(*), COUNT(DISTINCT A.s) FROM A;")
    keys = ["COUNT(*)", "COUNT(DISTINCT A.v)", "SUM(A.v)", "COUNT(DISTINCT A.s)"]
    assert names == [x for x in reference_order(keys + cols) if x not in cols]


def test_sharded_mode_refuses_count_distinct():
    """at world 2 on one GPU (the test transport of tests/_dist_gpu_worker.py): every rank gets the refusal, before any exchange"""
    from tests.test_dist_gpu import _run
    out = _run("cd", 2, 29637, worker="_count_distinct_dist_worker.py", timeout=300)
    assert "sharded count distinct refused ok" in out
