"""SELECT A.x, A.y, COUNT(*) FROM A JOIN B ON A.x = B.x AND A.y = B.y GROUP BY A.x, A.y  and  SELECT COUNT(*) over the same join through
DB.query: the fused join + GROUP BY operator on the two tables' PACKED keys (mdb_exec_join.c: composite_fused_plan; mdb_dev_join_key_pack ->
mdb_dev_join_group_count -> mdb_dev_join_key_unpack).

Every served statement is compared, ORDER INCLUDED, with
  (a) the same statement under MDB_COMPOSITE_FUSED=0 (pair join on the packed key + multi-field GROUP BY),
  (b) the same statement under MDB_COMPOSITE_JOIN=0 (pair join on the first equality, the others as filters),
  (c) a restatement written here: `np_equi` of tests/test_composite_join_gpu.py (A-major joined rows) -> the joined rows' key tuples in
      first-occurrence order with their counts (`nested_loop` of tests/test_outer_join_gpu.py for the statements that are not served),
  (d) SQLite, as a multiset (not for LIMIT without a total ORDER BY, whose rows depend on the group order),
and mdb_database_composite_fused() must rise by exactly 1 with the knobs unset - mdb_database_composite_joins() staying where it is - and
by 0 under either knob: a silent fallback fails the test.
"""
import numpy as np
import pytest

from tests.test_composite_join_gpu import bulk_rows, np_equi, rows_of, small_ab, two_key_table
from tests.test_outer_join_gpu import check_sqlite, eq, lt, make_db, nested_loop, result_rows, val

pytestmark = pytest.mark.gpu

KNOBS = ("MDB_COMPOSITE_FUSED", "MDB_COMPOSITE_JOIN")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ---------------------------------------------------------------------------------------------- helpers

def ways(db, sql, monkeypatch, taken=1, query=result_rows, norm=None, knobs=True):
    """the statement with the knobs unset, then under each knob -> (names, rows) of the first run; equal names, equal rows in equal
    order (norm: applied to the rows first - `sorted` when the order is left open), counters as said"""
    norm = norm or (lambda r: r)
    f0, j0 = db.composite_fused(), db.composite_joins()
    on = query(db, sql)
    assert db.composite_fused() == f0 + taken, (sql, db.composite_fused() - f0)
    if taken:
        assert db.composite_joins() == j0, sql		# (no pair join ran)
    for knob in KNOBS if knobs else ():
        monkeypatch.setenv(knob, "0")
        f1 = db.composite_fused()
        off = query(db, sql)
        monkeypatch.delenv(knob)
        assert db.composite_fused() == f1, (knob, sql)
        assert off[0] == on[0], (knob, sql)
        assert norm(off[1]) == norm(on[1]), (knob, sql)
    return on


def np_groups(ac, an, bc, bn, kc, keep_a=None, keep_b=None):
    """the join ON every column of kc equal (A-major), rows kept by keep_a / keep_b (bool per row of A / B) -> [(key tuple, COUNT)] in the
    order of each tuple's first joined row"""
    ia, ib = np_equi([ac[c] for c in kc], [an[c] for c in kc], [bc[c] for c in kc], [bn[c] for c in kc])
    keep = np.ones(len(ia), dtype=bool)
    if keep_a is not None:
        keep &= keep_a[ia]
    if keep_b is not None:
        keep &= keep_b[ib]
    ia = ia[keep]
    if not len(ia):
        return []
    tuples = np.stack([ac[c][ia] for c in kc], axis=1)
    uniq, first, cnt = np.unique(tuples, axis=0, return_index=True, return_counts=True)
    return [(tuple(int(v) for v in uniq[o]), int(cnt[o])) for o in np.argsort(first, kind="stable")]


def loop_groups(J, key_of):
    """joined tuples (nested_loop) -> [(key tuple, COUNT)] in first-occurrence order"""
    out = {}
    for t in J:
        k = key_of(t)
        out[k] = out.get(k, 0) + 1
    return list(out.items())


def shape(groups, names, colmap, having=None, order=None, distinct=False, limit=None):
    """HAVING -> the select list -> DISTINCT -> ORDER BY -> LIMIT over [(key tuple, COUNT)]; colmap: result column name -> key index or "n" """
    g = [x for x in groups if having is None or having(*x)]
    if order is not None:
        g = sorted(g, key=lambda x: order(*x))		# (stable; the tests order totally)
    rows = [tuple(cnt if colmap[nm] == "n" else key[colmap[nm]] for nm in names) for key, cnt in g]
    if distinct:
        rows = list(dict.fromkeys(rows))
    if limit is not None:
        rows = rows[limit[0]:limit[0] + limit[1]]
    return rows


XY = {"A.xa": 0, "B.xb": 0, "A.ya": 1, "B.yb": 1, "COUNT(*)": "n"}
SQLITE_XY = {"A.xa": "xa", "B.xb": "xb", "A.ya": "ya", "B.yb": "yb", "COUNT(*)": "COUNT(*)"}
ON_XY = "A.xa = B.xb AND A.ya = B.yb"


def sqlite_check(tabs, sql, names, rows, exprs=SQLITE_XY):
    """check_sqlite wants `SELECT *` and result names `table.column`: the select list goes in through the names"""
    head, rest = sql.split(" FROM ", 1)
    sel = [exprs[nm] for nm in names]
    if head.startswith("SELECT DISTINCT"):
        sel[0] = "DISTINCT " + sel[0]
    check_sqlite(tabs, "SELECT * FROM " + rest, ["_." + e for e in sel], rows)


# ---------------------------------------------------------------------------------------------- 1. two key columns, every clause

# (sql after the select list, select list, colmap additions, shape() arguments, sqlite?)
def xy_cases():
    g = "GROUP BY A.xa, A.ya"
    return [
        (f"A.xa, A.ya, COUNT(*) FROM A JOIN B ON {ON_XY} {g}", {}, {}, True),
        (f"xb, yb, COUNT(*) FROM A JOIN B ON {ON_XY} GROUP BY B.xb, B.yb", {}, {}, True),					# group fields from B
        (f"yb, xa, COUNT(*) FROM A JOIN B ON {ON_XY} GROUP BY B.yb, A.xa", {}, {}, True),					# mixed, not ON's order
        (f"ya, xa, COUNT(*) FROM A JOIN B ON B.yb = A.ya AND xb = xa GROUP BY ya, xa", {}, {}, True),				# ON the other way round
        (f"xa, ya FROM A JOIN B ON {ON_XY} {g}", {}, {}, True),									# no COUNT(*)
        (f"COUNT(*) FROM A JOIN B ON {ON_XY} {g}", {}, {}, True),								# nothing but
        (f"xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} {g} HAVING COUNT(*) > 2", {}, {"having": lambda k, n: n > 2}, True),
        (f"xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} {g} HAVING A.ya > 3", {}, {"having": lambda k, n: k[1] > 3}, True),
        (f"xa, yb, COUNT(*) FROM A JOIN B ON {ON_XY} GROUP BY xa, yb HAVING yb < 9 AND COUNT(*) > 1", {},
         {"having": lambda k, n: k[1] < 9 and n > 1}, True),
        (f"xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} {g} ORDER BY ya, xa", {}, {"order": lambda k, n: (k[1], k[0])}, True),
        (f"xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} {g} ORDER BY xa DESC, ya", {}, {"order": lambda k, n: (-k[0], k[1])}, True),
        (f"xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} {g} LIMIT 3, 5", {}, {"limit": (3, 5)}, False),
        (f"xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} {g} ORDER BY ya DESC, xa LIMIT 2, 7", {},
         {"order": lambda k, n: (-k[1], k[0]), "limit": (2, 7)}, True),
        (f"xa AS kx, ya, COUNT(*) AS n FROM A JOIN B ON {ON_XY} {g}", {"kx": 0, "n": "n"}, {}, True),				# aliases
        (f"xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} WHERE va < 7 {g}", {}, {"a": lambda ac, an: ~an[3] & (ac[3] < 7)}, True),	# WHERE: A through a selection vector
        (f"xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} WHERE wb > 4 {g}", {}, {"b": lambda bc, bn: ~bn[3] & (bc[3] > 4)}, True),
        (f"xb, ya, COUNT(*) FROM A JOIN B ON {ON_XY} WHERE wb > 4 AND va < 7 AND ta > 0 GROUP BY xb, ya HAVING COUNT(*) > 1", {},
         {"a": lambda ac, an: ~an[3] & (ac[3] < 7), "b": lambda bc, bn: ~bn[3] & (bc[3] > 4), "having": lambda k, n: n > 1}, True),
    ]


@pytest.mark.parametrize("na,nb,xs,ys", [(150, 170, 4, 12), (5000, 6000, 4, 300)])
def test_two_key_columns_every_clause(na, nb, xs, ys, monkeypatch):
    """150 x 170 rows: the operator's single-workgroup form (below 2048 rows); 5000 x 6000: its partitioned forms; 8 % NULLs per key column"""
    tabs = small_ab(100 + na, na=na, nb=nb, xs=xs, ys=ys, extra=True)
    (_, ac, an), (_, bc, bn) = tabs["A"], tabs["B"]
    db = make_db(tabs)
    try:
        for tail, more, how, lite in xy_cases():
            sql = f"SELECT {tail};"
            how = dict(how)
            keep_a = how.pop("a")(ac, an) if "a" in how else None
            keep_b = how.pop("b")(bc, bn) if "b" in how else None
            names, rows = ways(db, sql, monkeypatch)
            groups = np_groups(ac, an, bc, bn, (0, 1), keep_a, keep_b)
            colmap = {**XY, **more}
            exp = shape(groups, names, colmap, **how)
            assert rows == exp, sql
            assert len(groups) > 20 and (len(rows) > 1 or "LIMIT" in sql), sql
            if lite:
                sqlite_check(tabs, sql, names, rows, {**SQLITE_XY, "kx": "xa", "n": "COUNT(*)"})
        # count-only, with and without a pushed WHERE
        for where, ka, kb in (("", None, None), (" WHERE va < 7 AND wb > 4", ~an[3] & (ac[3] < 7), ~bn[3] & (bc[3] > 4))):
            sql = f"SELECT COUNT(*) FROM A JOIN B ON {ON_XY}{where};"
            names, rows = ways(db, sql, monkeypatch)
            total = sum(n for _, n in np_groups(ac, an, bc, bn, (0, 1), ka, kb))
            assert names == ["COUNT(*)"] and rows == [(total,)] and total > 50, sql
            sqlite_check(tabs, sql, names, rows)
        # a WHERE that leaves no row of A: no group, and COUNT(*) over zero rows returns no row
        assert ways(db, f"SELECT xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} WHERE va < 0 GROUP BY xa, ya;", monkeypatch)[1] == []
        assert ways(db, f"SELECT COUNT(*) FROM A JOIN B ON {ON_XY} WHERE va < 0;", monkeypatch)[1] == []
    finally:
        db.close()


def test_the_restatement_agrees_with_the_nested_loop():
    tabs = small_ab(250, extra=True)
    (_, ac, an), (_, bc, bn) = tabs["A"], tabs["B"]
    J = nested_loop([[a] for a in rows_of(tabs, "A")], rows_of(tabs, "B"), lambda t: eq(val(t[0], 0), val(t[1], 0)) and eq(val(t[0], 1), val(t[1], 1)), "JOIN")
    assert loop_groups(J, lambda t: (t[0][0], t[0][1])) == np_groups(ac, an, bc, bn, (0, 1)) and len(J) > 100


# ---------------------------------------------------------------------------------------------- 2. the shape of the issue

def test_8_by_5000_values_at_40000_rows(monkeypatch):
    rng = np.random.default_rng(5)
    n = 40_000
    ac, an = two_key_table(rng, n, 8, 5000, 1)
    bc, bn = two_key_table(rng, n, 8, 5000, 10**6)
    tabs = {"A": ("xa INT, ya INT, ta INT", ac, an), "B": ("xb INT, yb INT, tb INT", bc, bn)}
    db = make_db(tabs)
    try:
        for where, keep_a in (("", None), (" WHERE ta < 30000", ac[2] < 30000)):
            groups = np_groups(ac, an, bc, bn, (0, 1), keep_a)
            sql = f"SELECT A.xa, A.ya, COUNT(*) FROM A JOIN B ON {ON_XY}{where} GROUP BY A.xa, A.ya;"
            names, rows = ways(db, sql, monkeypatch, query=bulk_rows)
            assert rows == shape(groups, names, XY) and 10_000 < len(rows) < 30_000, sql
            sqlite_check(tabs, sql, names, rows)
            sql = f"SELECT COUNT(*) FROM A JOIN B ON {ON_XY}{where};"
            names, rows = ways(db, sql, monkeypatch, query=bulk_rows)
            assert rows == [(sum(c for _, c in groups),)], sql
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 3. three and four key columns

def keyed_table(rng, n, doms, tag0, null_frac=0.08):
    cols = [rng.integers(0, d, n, dtype=np.int64) for d in doms] + [np.arange(tag0, tag0 + n, dtype=np.int64)]
    nulls = [rng.random(n) < null_frac for _ in doms] + [np.zeros(n, dtype=bool)]
    return cols, nulls


@pytest.mark.parametrize("na,nb", [(150, 170), (5000, 6000)])
@pytest.mark.parametrize("nk", [3, 4])
def test_three_and_four_key_columns(nk, na, nb, monkeypatch):
    rng = np.random.default_rng(10 * nk + na)
    doms = [3, 4, 2, 2][:nk] if na < 1000 else [5, 40, 3, 2][:nk]
    ac, an = keyed_table(rng, na, doms, 0)
    bc, bn = keyed_table(rng, nb, doms, 10**6)
    a_names, b_names = ["xa", "ya", "za", "ua"][:nk], ["xb", "yb", "zb", "ub"][:nk]
    tabs = {"A": (", ".join(f"{c} INT" for c in a_names + ["ta"]), ac, an), "B": (", ".join(f"{c} INT" for c in b_names + ["tb"]), bc, bn)}
    colmap = {"COUNT(*)": "n", **{f"A.{c}": i for i, c in enumerate(a_names)}, **{f"B.{c}": i for i, c in enumerate(b_names)}}
    lite = {"COUNT(*)": "COUNT(*)", **{f"A.{c}": c for c in a_names}, **{f"B.{c}": c for c in b_names}}
    on = " AND ".join(f"A.{a} = B.{b}" for a, b in zip(a_names, b_names))
    groups = np_groups(ac, an, bc, bn, tuple(range(nk)))
    assert len(groups) > 15
    db = make_db(tabs)
    try:
        # group fields in ON's order from A; reversed, sides alternating
        mixed = [f"{'A' if i % 2 else 'B'}.{(a_names if i % 2 else b_names)[i]}" for i in reversed(range(nk))]
        for fields in ([f"A.{c}" for c in a_names], mixed):
            sql = f"SELECT {', '.join(fields)}, COUNT(*) FROM A JOIN B ON {on} GROUP BY {', '.join(fields)};"
            names, rows = ways(db, sql, monkeypatch)
            assert rows == shape(groups, names, colmap), sql
            sqlite_check(tabs, sql, names, rows, lite)
        sql = f"SELECT {', '.join(mixed)}, COUNT(*) FROM A JOIN B ON {on} GROUP BY {', '.join(mixed)} HAVING {mixed[0]} > 0 ORDER BY {mixed[1]} DESC, {', '.join(mixed)} LIMIT 1, 9;"
        names, rows = ways(db, sql, monkeypatch)
        i0, i1 = colmap[mixed[0]], colmap[mixed[1]]
        exp = shape(groups, names, colmap, having=lambda k, n: k[i0] > 0, order=lambda k, n: (-k[i1],) + tuple(k[colmap[f]] for f in mixed), limit=(1, 9))
        assert rows == exp and len(rows) == 9, sql
        sqlite_check(tabs, sql, names, rows, lite)
        names, rows = ways(db, f"SELECT COUNT(*) FROM A JOIN B ON {on};", monkeypatch)
        assert rows == [(sum(c for _, c in groups),)]
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 4. VARCHAR key columns

def test_varchar_key_columns(monkeypatch):
    from midoridb_amd.query import DB
    rng = np.random.default_rng(7)
    pool = ["ann", "bob", "cy", "dee", None]

    def table(n, tag0):
        return [(pool[int(rng.integers(0, 5))], int(rng.integers(0, 4)), pool[int(rng.integers(0, 5))], tag0 + i) for i in range(n)]

    def lit(v):
        return "NULL" if v is None else (f"'{v}'" if isinstance(v, str) else str(v))
    A, B = table(150, 100), table(170, 500)
    tabs = {nm: (decl, [[r[c] for r in rows] for c in range(4)], [[r[c] is None for r in rows] for c in range(4)])
            for nm, decl, rows in (("A", "sa VARCHAR(8), ka INT, ra VARCHAR(8), ta INT", A), ("B", "sb VARCHAR(8), kb INT, rb VARCHAR(8), tb INT", B))}
    with DB() as db:
        for nm, (decl, _, _) in tabs.items():
            db.execute(f"CREATE TABLE {nm} ({decl});")
        for name, rows in (("A", A), ("B", B)):
            db.execute(f"INSERT INTO {name} VALUES " + ", ".join("(" + ", ".join(lit(v) for v in r) + ")" for r in rows) + ";")
        for on_sql, kc, fields in (("sa = sb AND ka = kb", (0, 1), ["sa", "kb"]), ("ka = kb AND rb = ra AND sa = sb", (1, 2, 0), ["rb", "sa", "ka"])):
            J = nested_loop([[a] for a in A], B, lambda t: all(eq(val(t[0], c), val(t[1], c)) for c in kc), "JOIN")
            groups = loop_groups(J, lambda t: tuple(t[0][c] for c in kc))
            colmap = {"COUNT(*)": "n"}
            for i, c in enumerate(kc):
                colmap["A." + "sa ka ra".split()[c]] = colmap["B." + "sb kb rb".split()[c]] = i
            sql = f"SELECT {', '.join(fields)}, COUNT(*) FROM A JOIN B ON {on_sql} GROUP BY {', '.join(fields)};"
            names, rows = ways(db, sql, monkeypatch)
            assert rows == shape(groups, names, colmap) and len(rows) > 10, sql
            sqlite_check(tabs, sql, names, rows, {"COUNT(*)": "COUNT(*)", **{nm: nm.split(".")[1] for nm in colmap if "." in nm}})
            names, rows = ways(db, f"SELECT COUNT(*) FROM A JOIN B ON {on_sql};", monkeypatch)
            assert rows == [(len(J),)]


# ---------------------------------------------------------------------------------------------- 5. nothing can match

def test_disjoint_ranges_answer_without_rows(monkeypatch):
    rng = np.random.default_rng(10)
    ac, an = two_key_table(rng, 300, 4, 10, 0, 0.05)
    bc, bn = two_key_table(rng, 200, 4, 10, 1000, 0.05, y_lo=50)		# yb in [50, 60): no ya
    db = make_db({"A": ("xa INT, ya INT, ta INT", ac, an), "B": ("xb INT, yb INT, tb INT", bc, bn)})
    try:
        db.query("SELECT COUNT(*) FROM A;")
        calls = db.counters()["operator_calls"]
        names, rows = ways(db, f"SELECT xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} GROUP BY xa, ya;", monkeypatch, knobs=False)
        assert rows == [] and len(names) == 3
        names, rows = ways(db, f"SELECT COUNT(*) FROM A JOIN B ON {ON_XY};", monkeypatch, knobs=False)
        assert rows == [] and names == ["COUNT(*)"]		# (COUNT(*) over zero rows returns no row)
        assert db.counters()["operator_calls"] == calls	# no join / GROUP BY operator ran
        ways(db, f"SELECT xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} GROUP BY xa, ya;", monkeypatch)
        ways(db, f"SELECT COUNT(*) FROM A JOIN B ON {ON_XY};", monkeypatch)
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 6. results on the device, any order

def test_results_on_device_and_groups_any_order(monkeypatch):
    tabs = small_ab(66, na=5000, nb=6000, xs=4, ys=300, extra=True)
    (_, ac, an), (_, bc, bn) = tabs["A"], tabs["B"]
    groups = np_groups(ac, an, bc, bn, (0, 1))
    sql = f"SELECT A.xa, B.yb, COUNT(*) FROM A JOIN B ON {ON_XY} GROUP BY A.xa, B.yb;"
    db = make_db(tabs)
    try:
        host = ways(db, sql, monkeypatch)
        assert host[1] == shape(groups, host[0], XY)
        db.results_on_device(True)
        assert ways(db, sql, monkeypatch) == host		# (fetched from the device on first use)
        f0 = db.composite_fused()
        names, types, cols, nrows, joined, _ = db.query_device(sql)
        assert db.composite_fused() == f0 + 1 and names == host[0] and nrows == len(groups) and joined == sum(c for _, c in groups)
        assert list(zip(*[c.cpu().tolist() for c in cols])) == host[1]
        assert all(x is None for x in db.last_device_nulls)
        lim = ways(db, sql[:-1] + " ORDER BY yb, xa LIMIT 5, 50;", monkeypatch)
        assert lim[1] == shape(groups, lim[0], XY, order=lambda k, n: (k[1], k[0]), limit=(5, 50))
        cnt = ways(db, f"SELECT COUNT(*) FROM A JOIN B ON {ON_XY};", monkeypatch)
        assert cnt[1] == [(sum(c for _, c in groups),)]
        db.results_on_device(False)
        db.groups_any_order(True)
        names, rows = ways(db, sql, monkeypatch, norm=sorted)
        assert sorted(rows) == sorted(shape(groups, names, XY))
        sqlite_check(tabs, sql, names, rows)
        assert ways(db, f"SELECT COUNT(*) FROM A JOIN B ON {ON_XY};", monkeypatch) == cnt
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 7. statements that must not take the plan

def test_statements_that_keep_the_general_plan(monkeypatch):
    """the counter stays and the rows are the restatement's (nested loop over Python lists, NULL = false)"""
    rng = np.random.default_rng(17)
    tabs = small_ab(17, extra=True)
    cc, cn = two_key_table(rng, 60, 4, 12, 9000, 0.08)
    tabs["C"] = ("xc INT, yc INT, tc INT", cc, cn)
    A, B, C = (rows_of(tabs, t) for t in "ABC")
    S = [[a] for a in A]
    on_xy = lambda t: eq(val(t[0], 0), val(t[1], 0)) and eq(val(t[0], 1), val(t[1], 1))	# noqa: E731
    xy_of = lambda t: (val(t[0], 0), val(t[0], 1))						# noqa: E731
    g = "GROUP BY A.xa, A.ya"
    cases = [
        (f"SELECT xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} AND A.va < B.wb {g};", nested_loop(S, B, lambda t: on_xy(t) and lt(val(t[0], 3), val(t[1], 3)), "JOIN"), xy_of),
        (f"SELECT xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} WHERE A.va < B.wb {g};", nested_loop(S, B, lambda t: on_xy(t) and lt(val(t[0], 3), val(t[1], 3)), "JOIN"), xy_of),
        (f"SELECT xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} AND A.da = B.db {g};", nested_loop(S, B, lambda t: on_xy(t) and eq(val(t[0], 4), val(t[1], 4)), "JOIN"), xy_of),
        (f"SELECT xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} JOIN C ON A.xa = C.xc AND A.ya = C.yc {g};",
         nested_loop(nested_loop(S, B, on_xy, "JOIN"), C, lambda t: eq(val(t[0], 0), val(t[2], 0)) and eq(val(t[0], 1), val(t[2], 1)), "JOIN", width=2), xy_of),
        (f"SELECT xa, ya, COUNT(*) FROM A LEFT JOIN B ON {ON_XY} {g};", nested_loop(S, B, on_xy, "LEFT JOIN"), xy_of),
        (f"SELECT xa, COUNT(*) FROM A JOIN B ON {ON_XY} GROUP BY A.xa;", nested_loop(S, B, on_xy, "JOIN"), lambda t: (t[0][0],)),
    ]
    db = make_db(tabs)
    try:
        for sql, J, key_of in cases:
            names, rows = ways(db, sql, monkeypatch, taken=0, knobs=False)
            groups = loop_groups(J, key_of)
            assert rows == shape(groups, names, XY) and len(rows) > 3, sql
        # count-only over a DOUBLE equality
        J = nested_loop(S, B, lambda t: eq(val(t[0], 0), val(t[1], 0)) and eq(val(t[0], 4), val(t[1], 4)), "JOIN")
        names, rows = ways(db, "SELECT COUNT(*) FROM A JOIN B ON A.xa = B.xb AND A.da = B.db;", monkeypatch, taken=0, knobs=False)
        assert rows == [(len(J),)] and len(J) > 10
        # a single-key fused statement on the same tables: what it always returned, the counter where it was
        names, rows = ways(db, "SELECT xa, COUNT(*) FROM A JOIN B ON A.xa = B.xb GROUP BY A.xa;", monkeypatch, taken=0, knobs=False)
        J = nested_loop(S, B, lambda t: eq(val(t[0], 0), val(t[1], 0)), "JOIN")
        assert rows == shape(loop_groups(J, lambda t: (t[0][0],)), names, XY) and len(rows) == 4
    finally:
        db.close()


def test_distinct_never_reaches_the_plan(monkeypatch):
    """DISTINCT beside GROUP BY or COUNT(*) is refused when the statement is checked, before any plan, as it always was; DISTINCT over the
    plain join keeps the general plan: the joined rows' distinct key tuples in first-occurrence order"""
    from midoridb_amd.query import QueryError
    tabs = small_ab(18, extra=True)
    (_, ac, an), (_, bc, bn) = tabs["A"], tabs["B"]
    db = make_db(tabs)
    try:
        f0 = db.composite_fused()
        for sql in (f"SELECT DISTINCT xa, ya FROM A JOIN B ON {ON_XY} GROUP BY xa, ya;", f"SELECT DISTINCT COUNT(*) FROM A JOIN B ON {ON_XY};"):
            with pytest.raises(QueryError, match="DISTINCT"):
                db.query(sql)
        assert db.composite_fused() == f0
        sql = f"SELECT DISTINCT xa, yb FROM A JOIN B ON {ON_XY};"
        names, rows = ways(db, sql, monkeypatch, taken=0, knobs=False)
        assert rows == shape(np_groups(ac, an, bc, bn, (0, 1)), names, XY) and len(rows) > 20
        sqlite_check(tabs, sql, names, rows)
    finally:
        db.close()


def test_two_columns_spread_over_2_to_the_40_do_not_fit(monkeypatch):
    """41 + 41 bits: no packed key, the general plan answers"""
    rng = np.random.default_rng(19)
    n = 400
    wide = np.array([-2**40, 2**40, -5, 0, 5, 2**39], dtype=np.int64)

    def tab(tag0):
        return [wide[rng.integers(0, 6, n)], wide[rng.integers(0, 6, n)], np.arange(tag0, tag0 + n, dtype=np.int64)], \
               [rng.random(n) < 0.05, rng.random(n) < 0.05, np.zeros(n, dtype=bool)]
    ac, an = tab(0)
    bc, bn = tab(10**6)
    tabs = {"A": ("xa INT, ya INT, ta INT", ac, an), "B": ("xb INT, yb INT, tb INT", bc, bn)}
    db = make_db(tabs)
    try:
        sql = f"SELECT xa, ya, COUNT(*) FROM A JOIN B ON {ON_XY} GROUP BY xa, ya;"
        names, rows = ways(db, sql, monkeypatch, taken=0, knobs=False)
        assert rows == shape(np_groups(ac, an, bc, bn, (0, 1)), names, XY) and len(rows) > 20
        sqlite_check(tabs, sql, names, rows)
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 8. beyond the pair operator's limit

def test_more_joined_rows_than_the_pair_join_addresses():
    """140 000 rows per table, x and y in {0, 1} dealt evenly: 35 000 rows per combination and side, 4 x 35 000^2 = 4.9 x 10^9 joined
    rows - more than the 2^32 - 1 pairs the pair join can write, so only the fused plan answers (never run with a knob off)"""
    rng = np.random.default_rng(23)
    n = 140_000
    z = [np.zeros(n, dtype=bool)] * 3

    def tab(tag0):
        i = rng.permutation(n)
        return [(i % 2).astype(np.int64), ((i // 2) % 2).astype(np.int64), np.arange(tag0, tag0 + n, dtype=np.int64)]
    ac, bc = tab(0), tab(10**6)
    db = make_db({"A": ("xa INT, ya INT, ta INT", ac, z), "B": ("xb INT, yb INT, tb INT", bc, z)})
    try:
        f0, j0 = db.composite_fused(), db.composite_joins()
        res = db.query(f"SELECT COUNT(*) FROM A JOIN B ON {ON_XY};")
        assert res.rows() == [(4 * 35_000**2,)] and res.joined_rows == 4_900_000_000
        res = db.query(f"SELECT A.xa, A.ya, COUNT(*) FROM A JOIN B ON {ON_XY} GROUP BY A.xa, A.ya;")
        assert db.composite_fused() == f0 + 2 and db.composite_joins() == j0
        ua, first, ca = np.unique(np.stack(ac[:2], axis=1), axis=0, return_index=True, return_counts=True)
        ub, cb = np.unique(np.stack(bc[:2], axis=1), axis=0, return_counts=True)
        assert np.array_equal(ua, ub)
        groups = [((int(ua[o][0]), int(ua[o][1])), int(ca[o]) * int(cb[o])) for o in np.argsort(first)]
        assert res.rows() == shape(groups, res.names, XY)
        assert [c for _, c in groups] == [1_225_000_000] * 4
    finally:
        db.close()
