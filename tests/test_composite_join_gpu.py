"""ON l.x = r.x AND l.y = r.y [AND ...] through DB.query: the equalities whose columns fit 63 bits together are joined as ONE packed key
(mdb_exec_join.c: composite_join_plan / composite_join_pack; mdb_dev_join_key_layout / mdb_dev_join_key_pack).

Every statement is compared row for row, ORDER INCLUDED, with
  - the same statement under MDB_COMPOSITE_JOIN=0 - the join on the first equality with the others as filters over its pairs -, and
  - an expectation computed here: `nested_loop` of tests/test_outer_join_gpu.py (SQL's rules over Python lists: a pair is in the result
    when the whole ON expression is true, NULL counting as false; preserved side major) for small tables, `np_equi` (numpy: the rows'
    key tuples numbered, sort + searchsorted) for 40 000-row tables - each checked against the other in test_the_two_restatements_agree -,
    plus SQLite as a multiset for the outer joins;
and mdb_database_composite_joins() must rise by one per statement with the knob on (by as many as the case says) and stay with it off.
"""
import numpy as np
import pytest

from tests.test_outer_join_gpu import check_sqlite, eq, lt, make_db, nested_loop, project, result_rows, table_rows, val

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ---------------------------------------------------------------------------------------------- helpers

def both_ways(db, sql, monkeypatch, taken=1, query=result_rows):
    """the statement with the knob off and on -> (names, rows) of the composite run; equal rows in equal order, counter as said"""
    monkeypatch.setenv("MDB_COMPOSITE_JOIN", "0")
    c0 = db.composite_joins()
    off = query(db, sql)
    assert db.composite_joins() == c0, sql
    monkeypatch.delenv("MDB_COMPOSITE_JOIN")
    on = query(db, sql)
    assert db.composite_joins() == c0 + taken, (sql, db.composite_joins() - c0)
    assert on[0] == off[0], sql
    assert on[1] == off[1], sql
    return on


def bulk_rows(db, sql):
    """whole columns at once (NULL cells read 0): for statements that select NOT NULL columns of 40 000-row tables"""
    res = db.query(sql)
    return res.names, list(zip(*[c.tolist() for c in res.columns])) if res.nrows else []


def np_equi(keys_a, nulls_a, keys_b, nulls_b):
    """inner join ON every key column equal (NULL equals nothing) -> (rows of A, rows of B), A-major, B-minor"""
    na, nb = len(keys_a[0]), len(keys_b[0])
    stacked = np.stack([np.concatenate([ka, kb]) for ka, kb in zip(keys_a, keys_b)], axis=1)
    _, ids = np.unique(stacked, axis=0, return_inverse=True)		# equal key tuples, equal ids
    ids = ids.reshape(-1)
    ia_null = np.zeros(na, dtype=bool)
    ib_null = np.zeros(nb, dtype=bool)
    for x in nulls_a:
        ia_null |= x
    for x in nulls_b:
        ib_null |= x
    ida, idb = ids[:na], ids[na:]
    vb = np.flatnonzero(~ib_null)
    order = vb[np.argsort(idb[vb], kind="stable")]
    sk = idb[order]
    lo = np.searchsorted(sk, ida, "left")
    hi = np.searchsorted(sk, ida, "right")
    deg = np.where(ia_null, 0, hi - lo)
    ia = np.repeat(np.arange(na), deg)
    start = np.cumsum(deg) - deg
    within = np.arange(len(ia)) - np.repeat(start, deg)
    return ia, order[np.repeat(lo, deg) + within]


def two_key_table(rng, n, xs, ys, tag0, null_frac=0.03, x_lo=0, y_lo=0):
    """columns: x, y (keys, null_frac NULLs each), tag (unique, never NULL)"""
    cols = [rng.integers(x_lo, x_lo + xs, n, dtype=np.int64), rng.integers(y_lo, y_lo + ys, n, dtype=np.int64), np.arange(tag0, tag0 + n, dtype=np.int64)]
    nulls = [rng.random(n) < null_frac, rng.random(n) < null_frac, np.zeros(n, dtype=bool)]
    return cols, nulls


AB = {"A.xa": (0, 0), "A.ya": (0, 1), "A.ta": (0, 2), "A.va": (0, 3), "A.da": (0, 4),
      "B.xb": (1, 0), "B.yb": (1, 1), "B.tb": (1, 2), "B.wb": (1, 3), "B.db": (1, 4),
      "C.xc": (2, 0), "C.yc": (2, 1), "C.tc": (2, 2)}


def on_xy(t):
    return eq(val(t[0], 0), val(t[1], 0)) and eq(val(t[0], 1), val(t[1], 1))


def small_ab(seed, na=150, nb=170, xs=4, ys=12, extra=False):
    """two small tables with many partners per x and few per (x, y); extra: + v / w INT and d DOUBLE columns"""
    rng = np.random.default_rng(seed)
    ac, an = two_key_table(rng, na, xs, ys, 1000, 0.08)
    bc, bn = two_key_table(rng, nb, xs, ys, 5000, 0.08)
    decl_a, decl_b = "xa INT, ya INT, ta INT", "xb INT, yb INT, tb INT"
    if extra:
        ac += [rng.integers(0, 10, na, dtype=np.int64), rng.integers(0, 3, na) / 2.0]
        bc += [rng.integers(0, 10, nb, dtype=np.int64), rng.integers(0, 3, nb) / 2.0]
        an += [rng.random(na) < 0.1, rng.random(na) < 0.1]
        bn += [rng.random(nb) < 0.1, rng.random(nb) < 0.1]
        decl_a += ", va INT, da DOUBLE"
        decl_b += ", wb INT, db DOUBLE"
    return {"A": (decl_a, ac, an), "B": (decl_b, bc, bn)}


def rows_of(tabs, name):
    return table_rows(tabs[name][1], tabs[name][2])


# ---------------------------------------------------------------------------------------------- the restatements

def test_the_two_restatements_agree():
    tabs = small_ab(1)
    A, B = rows_of(tabs, "A"), rows_of(tabs, "B")
    J = nested_loop([[a] for a in A], B, on_xy, "JOIN")
    (_, ac, an), (_, bc, bn) = tabs["A"], tabs["B"]
    ia, ib = np_equi(ac[:2], an[:2], bc[:2], bn[:2])
    assert [(A[i], B[j]) for i, j in zip(ia, ib)] == [(t[0], t[1]) for t in J] and len(J) > 50


# ---------------------------------------------------------------------------------------------- 1. the shape of the issue

def test_8_by_5000_values_at_40000_rows(monkeypatch):
    """x has 8 values, y 5000: 2 x 10^8 pairs on x alone, about 4 x 10^4 on (x, y); 3 % NULLs in every key column"""
    rng = np.random.default_rng(5)
    n = 40_000
    ac, an = two_key_table(rng, n, 8, 5000, 1)
    bc, bn = two_key_table(rng, n, 8, 5000, 10**6)
    db = make_db({"A": ("xa INT, ya INT, ta INT", ac, an), "B": ("xb INT, yb INT, tb INT", bc, bn)})
    try:
        names, rows = both_ways(db, "SELECT ta, tb FROM A JOIN B ON A.xa = B.xb AND A.ya = B.yb;", monkeypatch, query=bulk_rows)
        ia, ib = np_equi(ac[:2], an[:2], bc[:2], bn[:2])
        assert 30_000 < len(ia) < 50_000
        exp = {"A.ta": ac[2][ia].tolist(), "B.tb": bc[2][ib].tolist()}
        assert rows == list(zip(*[exp[nm] for nm in names]))
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 2. / 3. / 6. small tables, every ON shape

SHAPES = [
    ("A.xa = B.xb AND A.ya = B.yb", on_xy, 1),
    ("A.ya = B.yb AND A.xa = B.xb", on_xy, 1),						# the other order
    ("B.xb = A.xa AND B.yb = A.ya", on_xy, 1),						# table t on the left of the =
    ("xa = xb AND yb = ya", on_xy, 1),
    ("A.xa = B.xb AND A.ya = B.yb AND A.va < B.wb", lambda t: on_xy(t) and lt(val(t[0], 3), val(t[1], 3)), 1),	# a residual beside the key
    ("A.va < B.wb AND A.xa = B.xb AND A.ya = B.yb", lambda t: on_xy(t) and lt(val(t[0], 3), val(t[1], 3)), 1),
    ("A.xa = B.xb AND A.ya = B.yb AND A.da = B.db", lambda t: on_xy(t) and eq(val(t[0], 4), val(t[1], 4)), 1),	# a DOUBLE equality stays IEEE ==
    ("A.da = B.db AND A.xa = B.xb AND A.ya = B.yb", lambda t: on_xy(t) and eq(val(t[0], 4), val(t[1], 4)), 1),	# ... also as the first conjunct
    ("A.xa = B.xb AND A.ya = B.yb AND B.wb > 4", lambda t: on_xy(t) and val(t[1], 3) is not None and val(t[1], 3) > 4, 1),
    ("A.xa = B.xb AND A.da = B.db", lambda t: eq(val(t[0], 0), val(t[1], 0)) and eq(val(t[0], 4), val(t[1], 4)), 0),	# one qualifying equality: as before
]


@pytest.mark.parametrize("kind", ["JOIN", "LEFT JOIN", "RIGHT JOIN", "LEFT OUTER JOIN", "RIGHT OUTER JOIN"])
def test_every_on_shape_inner_left_right(kind, monkeypatch):
    """2., 3., 4.: conjunct order, `B.x = A.x`, residuals and a DOUBLE equality beside the key; outer joins with unmatched rows and NULL
    keys on both sides (8 % NULLs per key column; SQLite as a multiset for the shapes without DOUBLE)"""
    tabs = small_ab(20 + len(kind), extra=True)
    A, B = rows_of(tabs, "A"), rows_of(tabs, "B")
    db = make_db(tabs)
    try:
        for k, (on_sql, on, taken) in enumerate(SHAPES):
            sql = f"SELECT xa, ya, ta, va, xb, yb, tb, wb FROM A {kind} B ON {on_sql};"		# (not the DOUBLE columns: their cells read as bits)
            names, rows = both_ways(db, sql, monkeypatch, taken=taken)
            J = nested_loop([[a] for a in A], B, on, kind)
            assert rows == project(J, names, AB), sql
            if kind != "JOIN":
                assert any(r[names.index("A.ta" if kind.startswith("RIGHT") else "B.tb")] is None for r in rows)	# unmatched rows exist
                if "da" not in on_sql and k % 2 == 0:
                    check_sqlite(tabs, f"SELECT * FROM A {kind} B ON {on_sql};", names, rows)
    finally:
        db.close()


def test_where_conjunct_pushed_onto_the_joined_table(monkeypatch):
    """6.: B is filtered first and packed through its selection vector; A filtered too (the stream side through a row-id vector)"""
    tabs = small_ab(6, na=4000, nb=5000, xs=4, ys=300, extra=True)
    (_, ac, an), (_, bc, bn) = tabs["A"], tabs["B"]
    db = make_db(tabs)
    try:
        for where, keep_a, keep_b in (("wb > 4", None, ~bn[3] & (bc[3] > 4)), ("wb > 4 AND va < 7", ~an[3] & (ac[3] < 7), ~bn[3] & (bc[3] > 4))):
            names, rows = both_ways(db, f"SELECT ta, tb FROM A JOIN B ON xa = xb AND ya = yb WHERE {where};", monkeypatch, query=bulk_rows)
            ia, ib = np_equi(ac[:2], an[:2], bc[:2], bn[:2])
            keep = keep_b[ib] if keep_a is None else keep_b[ib] & keep_a[ia]
            exp = {"A.ta": ac[2][ia][keep].tolist(), "B.tb": bc[2][ib][keep].tolist()}
            assert rows == list(zip(*[exp[nm] for nm in names])) and len(rows) > 1000
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 5. three tables

@pytest.mark.parametrize("first", ["JOIN", "LEFT JOIN"])
def test_keys_from_two_earlier_tables(first, monkeypatch):
    """... JOIN C ON A.xa = C.xc AND B.yb = C.yc: the stream side is packed through two row-id vectors; behind A LEFT JOIN B the stream
    holds "no row" for B: such tuples match nothing in the inner join to C"""
    rng = np.random.default_rng(55 + len(first))
    ac, an = two_key_table(rng, 60, 3, 5, 100, 0.1)
    bc, bn = two_key_table(rng, 50, 3, 5, 200, 0.1)
    cc, cn = two_key_table(rng, 70, 3, 5, 300, 0.1)
    tabs = {"A": ("xa INT, ya INT, ta INT", ac, an), "B": ("xb INT, yb INT, tb INT", bc, bn), "C": ("xc INT, yc INT, tc INT", cc, cn)}
    A, B, C = (rows_of(tabs, t) for t in "ABC")
    S = nested_loop([[a] for a in A], B, lambda t: eq(val(t[0], 1), val(t[1], 1)), first)
    assert (first == "LEFT JOIN") == any(t[1] is None for t in S)
    db = make_db(tabs)
    try:
        for last in ("JOIN", "LEFT JOIN", "RIGHT JOIN"):
            T = nested_loop(S, C, lambda t: eq(val(t[0], 0), val(t[2], 0)) and eq(val(t[1], 1), val(t[2], 1)), last, width=2)
            sql = f"SELECT * FROM A {first} B ON A.ya = B.yb {last} C ON A.xa = C.xc AND B.yb = C.yc;"
            names, rows = both_ways(db, sql, monkeypatch)
            assert rows == project(T, names, AB), sql
            assert len(rows) > 50
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 7. other column types

def test_varchar_and_date_composites(monkeypatch):
    from midoridb_amd.query import DB
    rng = np.random.default_rng(7)
    names_pool = ["ann", "bob", "cy", "dee", None]
    dates = ["2023-06-02", "2024-01-31", "1999-12-31", None]

    def table(n, tag0):
        return [(names_pool[int(rng.integers(0, 5))], dates[int(rng.integers(0, 4))], int(rng.integers(0, 4)), tag0 + i) for i in range(n)]

    def lit(v):
        return "NULL" if v is None else (f"'{v}'" if isinstance(v, str) else str(v))
    A, B = table(50, 100), table(60, 500)
    lay = {"A.sa": (0, 0), "A.da": (0, 1), "A.ka": (0, 2), "A.ta": (0, 3), "B.sb": (1, 0), "B.db": (1, 1), "B.kb": (1, 2), "B.tb": (1, 3)}
    with DB() as db:
        db.execute("CREATE TABLE A (sa VARCHAR(8), da DATE, ka INT, ta INT);")
        db.execute("CREATE TABLE B (sb VARCHAR(8), db DATE, kb INT, tb INT);")
        for name, rows in (("A", A), ("B", B)):
            db.execute(f"INSERT INTO {name} VALUES " + ", ".join("(" + ", ".join(lit(v) for v in r) + ")" for r in rows) + ";")
        for on_sql, cols in (("sa = sb AND ka = kb", (0, 2)), ("da = db AND ka = kb", (1, 2)), ("ka = kb AND sa = sb AND da = db", (0, 1, 2))):
            for kind in ("JOIN", "LEFT JOIN"):
                J = nested_loop([[a] for a in A], B, lambda t: all(eq(val(t[0], c), val(t[1], c)) for c in cols), kind)
                names, rows = both_ways(db, f"SELECT sa, ka, ta, sb, tb FROM A {kind} B ON {on_sql};", monkeypatch)
                assert rows == project(J, names, lay), on_sql
                assert len(J) > 10


# ---------------------------------------------------------------------------------------------- 8. not taken / partly taken

def test_not_taken_when_the_first_key_of_the_joined_table_is_measured_distinct(monkeypatch):
    rng = np.random.default_rng(8)
    n = 3000
    ac = [rng.integers(0, n, n, dtype=np.int64), rng.integers(0, 4, n, dtype=np.int64), np.arange(n, dtype=np.int64)]
    bc = [rng.permutation(n).astype(np.int64), rng.integers(0, 4, n, dtype=np.int64), np.arange(n, dtype=np.int64) + 10**6]
    z = [np.zeros(n, dtype=bool)] * 3
    # (declared PRIMARY KEY: the catalog measures "no value twice" also for a table this small - the declaration itself is never trusted)
    db = make_db({"A": ("xa INT, ya INT, ta INT", ac, z), "B": ("xb INT PRIMARY KEY, yb INT, tb INT", bc, z)})
    try:
        names, rows = both_ways(db, "SELECT ta, tb FROM A JOIN B ON xa = xb AND ya = yb;", monkeypatch, taken=0, query=bulk_rows)
        ia, ib = np_equi(ac[:2], z[:2], bc[:2], z[:2])
        exp = {"A.ta": ac[2][ia].tolist(), "B.tb": bc[2][ib].tolist()}
        assert rows == list(zip(*[exp[nm] for nm in names])) and 500 < len(rows) < 1000
        # the other way round B's first key column is ya's partner, which repeats: taken
        both_ways(db, "SELECT ta, tb FROM A JOIN B ON ya = yb AND xa = xb;", monkeypatch, taken=1, query=bulk_rows)
    finally:
        db.close()


def test_columns_that_do_not_fit(monkeypatch):
    """two columns spread over +-2^62 do not fit 63 bits: as before, counter unchanged; with a third, narrow one, two fit and the
    wide one in the middle stays a residual"""
    rng = np.random.default_rng(9)
    n = 400
    wide = np.array([-2**62, 2**62, -5, 0, 5, 2**61], dtype=np.int64)

    def tab(tag0):
        cols = [wide[rng.integers(0, 6, n)], wide[rng.integers(0, 6, n)], rng.integers(0, 3, n, dtype=np.int64), np.arange(tag0, tag0 + n, dtype=np.int64)]
        return cols, [rng.random(n) < 0.05, rng.random(n) < 0.05, rng.random(n) < 0.05, np.zeros(n, dtype=bool)]
    ac, an = tab(0)
    bc, bn = tab(10**6)
    db = make_db({"A": ("xa INT, ya INT, za INT, ta INT", ac, an), "B": ("xb INT, yb INT, zb INT, tb INT", bc, bn)})
    try:
        for on_sql, kc, taken in (("xa = xb AND ya = yb", (0, 1), 0), ("za = zb AND xa = xb AND ya = yb", (0, 1, 2), 0),
                                  ("za = zb AND xa = xb AND ya = yb AND zb = za", (0, 1, 2), 1)):
            names, rows = both_ways(db, f"SELECT ta, tb FROM A JOIN B ON {on_sql};", monkeypatch, taken=taken, query=bulk_rows)
            ia, ib = np_equi([ac[c] for c in kc], [an[c] for c in kc], [bc[c] for c in kc], [bn[c] for c in kc])
            exp = {"A.ta": ac[3][ia].tolist(), "B.tb": bc[3][ib].tolist()}
            assert rows == list(zip(*[exp[nm] for nm in names])) and len(rows) > 100, on_sql
    finally:
        db.close()
    # three equalities of which two fit (the middle one is 2^63 wide): counted, and the third stays a residual
    ac[1], bc[1] = wide[rng.integers(0, 6, n)], wide[rng.integers(0, 6, n)]
    ac[0], bc[0] = rng.integers(-50, 50, n, dtype=np.int64), rng.integers(-50, 50, n, dtype=np.int64)
    ac[0][:200], bc[0][:200] = 7, 7
    db = make_db({"A": ("xa INT, ya INT, za INT, ta INT", ac, an), "B": ("xb INT, yb INT, zb INT, tb INT", bc, bn)})
    try:
        names, rows = both_ways(db, "SELECT ta, tb FROM A JOIN B ON xa = xb AND ya = yb AND za = zb;", monkeypatch, taken=1, query=bulk_rows)
        ia, ib = np_equi(ac[:3], an[:3], bc[:3], bn[:3])
        exp = {"A.ta": ac[3][ia].tolist(), "B.tb": bc[3][ib].tolist()}
        assert rows == list(zip(*[exp[nm] for nm in names])) and len(rows) > 100
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 9. disjoint ranges

def test_disjoint_ranges(monkeypatch):
    rng = np.random.default_rng(10)
    ac, an = two_key_table(rng, 300, 4, 10, 0, 0.05)
    bc, bn = two_key_table(rng, 200, 4, 10, 1000, 0.05, y_lo=50)		# yb in [50, 60): no ya
    tabs = {"A": ("xa INT, ya INT, ta INT", ac, an), "B": ("xb INT, yb INT, tb INT", bc, bn)}
    A, B = rows_of(tabs, "A"), rows_of(tabs, "B")
    db = make_db(tabs)
    try:
        names, rows = both_ways(db, "SELECT * FROM A JOIN B ON xa = xb AND ya = yb;", monkeypatch)
        assert rows == []
        for kind in ("LEFT JOIN", "RIGHT JOIN"):
            names, rows = both_ways(db, f"SELECT * FROM A {kind} B ON xa = xb AND ya = yb;", monkeypatch)
            assert rows == project(nested_loop([[a] for a in A], B, on_xy, kind), names, AB)
            assert len(rows) == (300 if kind == "LEFT JOIN" else 200)
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 10. after UPDATE and DELETE

def test_after_update_and_delete(monkeypatch):
    """the catalog's ranges follow the data: a key moved far outside the old range joins its partner, deleted rows are gone"""
    tabs = small_ab(11, na=300, nb=300, xs=4, ys=20)
    (_, ac, an), (_, bc, bn) = tabs["A"], tabs["B"]
    db = make_db(tabs)
    try:
        sql = "SELECT ta, tb FROM A JOIN B ON xa = xb AND ya = yb;"
        both_ways(db, sql, monkeypatch)
        for stmt in ("UPDATE A SET ya = 1000000 WHERE ta < 1010;", "UPDATE B SET yb = 1000000 WHERE tb < 5020;",
                     "UPDATE A SET xa = -70000 WHERE ta = 1100;", "UPDATE B SET xb = -70000 WHERE tb = 5100;",
                     "UPDATE A SET ya = 3 WHERE ta = 1100;", "UPDATE B SET yb = 3 WHERE tb = 5100;"):
            db.execute(stmt)
        ac[1][ac[2] < 1010], an[1][ac[2] < 1010] = 10**6, False
        bc[1][bc[2] < 5020], bn[1][bc[2] < 5020] = 10**6, False
        ac[0][100], an[0][100], ac[1][100], an[1][100] = -70000, False, 3, False
        bc[0][100], bn[0][100], bc[1][100], bn[1][100] = -70000, False, 3, False
        names, rows = both_ways(db, sql, monkeypatch)
        A, B = rows_of(tabs, "A"), rows_of(tabs, "B")
        J = nested_loop([[a] for a in A], B, on_xy, "JOIN")
        assert rows == project(J, names, AB)
        assert (1100, 5100) in [(r[names.index("A.ta")], r[names.index("B.tb")]) for r in rows]
        assert sum(1 for t in J if t[0][1] == 10**6) > 0
        db.execute("DELETE FROM B WHERE tb >= 5100 AND tb < 5200;")
        db.execute("DELETE FROM A WHERE ya = 1000000;")
        A = [a for a in A if a[1] != 10**6]
        B = [b for b in B if not 5100 <= b[2] < 5200]
        names, rows = both_ways(db, sql, monkeypatch)
        assert rows == project(nested_loop([[a] for a in A], B, on_xy, "JOIN"), names, AB) and len(rows) > 50
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------- 11. the live reference

@pytest.mark.parametrize("seed", range(3))
def test_differential_vs_reference_live(seed, monkeypatch):
    """the reference evaluates the whole ON expression per pair (executor_select.c:1128): the inner statement, at most 60 rows per table,
    int32 values"""
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref/libmidori_ref.so not present on this box")
    rng = np.random.default_rng(1100 + seed)
    na, nb = int(rng.integers(30, 61)), int(rng.integers(30, 61))
    a = [rng.integers(-2, 2, na), rng.integers(2**31 - 6, 2**31 - 1, na), rng.integers(-1000, 1000, na)]
    b = [rng.integers(-2, 2, nb), rng.integers(2**31 - 6, 2**31 - 1, nb), rng.integers(-1000, 1000, nb)]
    an = [rng.random(na) < 0.1, rng.random(na) < 0.1, None]
    bn = [rng.random(nb) < 0.1, rng.random(nb) < 0.1, None]
    ddl = ["CREATE TABLE A (id_a INT, ya INT, f1 INT);", "CREATE TABLE B (id_b INT, yb INT, f2 INT);"]
    from midoridb_amd.query import DB
    rdb = ref.RefDB()
    with DB() as db:
        for s in ddl:
            rdb.execute(s)
            db.execute(s)
        rdb.bulk_insert("A", a, an)
        rdb.bulk_insert("B", b, bn)
        db.append_columns("A", a, an)
        db.append_columns("B", b, bn)
        for q in ("SELECT * FROM A INNER JOIN B ON A.id_a = B.id_b AND A.ya = B.yb;",
                  "SELECT f1, f2 FROM A INNER JOIN B ON A.ya = B.yb AND A.id_a = B.id_b AND f1 < f2;"):
            names, rows = rdb.query(q)
            c0 = db.composite_joins()
            res = db.query(q)
            assert db.composite_joins() == c0 + 1
            assert res.names == names, q
            assert res.rows() == rows and len(rows) > 5, q
    rdb.close()
