"""UNION [ALL], INTERSECT and EXCEPT through query_execute(): rows AND their order against tests/setops_model.py.  A plain arm's rows come
from the arrays the tables were loaded from; the rows of an arm that is a join, a GROUP BY, a window function or a SELECT DISTINCT are
what that SELECT answers alone (its own tests pin that), so that the compound is checked as the model's combination of its arms."""
import struct

import numpy as np
import pytest

from tests import setops_model as M

pytestmark = pytest.mark.gpu

OPS = [M.UNION, M.UNIONALL, M.INTERSECT, M.EXCEPT]
N = 10_000
NAN1, NAN2 = 0x7FF8000000000000, 0x7FF8000000000001


def dbl(bits):
    return struct.unpack("<d", struct.pack("<Q", bits & (2 ** 64 - 1)))[0]


def make_table(rng, n, shift):
    """(INT, DOUBLE, VARCHAR, DATE, INT) over small domains that overlap between the tables (shift moves them), NULLs in every column -
    random bits under the NULL cells - and among the doubles +0.0, -0.0 and two NaNs"""
    k = rng.integers(shift, shift + 6, n).astype(np.int64)
    dvals = np.array([dbl(0), dbl(1 << 63), dbl(NAN1), dbl(NAN2), 1.5, -2.25])[rng.integers(0, 6, n)] if shift == 0 else \
        np.array([dbl(1 << 63), dbl(NAN2), 1.5, 7.0])[rng.integers(0, 4, n)]
    s = ["name%d" % x for x in rng.integers(shift, shift + 4, n)]
    t = 1577880000 + 86400 * rng.integers(shift, shift + 3, n).astype(np.int64)
    v = rng.integers(-3, 3, n).astype(np.int64)
    nulls = [rng.random(n) < 0.1 for _ in range(5)]
    k = np.where(nulls[0], rng.integers(-2 ** 40, 2 ** 40, n), k)
    s = [None if z else x for x, z in zip(s, nulls[2])]
    return [k, dvals, s, t, v], nulls


def table_rows(cols, nulls, which):
    out = []
    for i in range(len(cols[0])):
        out.append(tuple(None if nulls[c][i] else (cols[c][i] if c == 2 else float(cols[c][i]) if c == 1 else int(cols[c][i])) for c in which))
    return out


TABLES = (("A", "k, d, s, t, v", 0, N), ("B", "j, e, r, u, w", 2, N), ("C", "ck, cd, cs, ct, cv", 3, N // 2))


def world_data():
    rng = np.random.default_rng(2605)
    data = {name: make_table(rng, n, shift) for name, _, shift, n in TABLES}
    return data, rng


@pytest.fixture(scope="module")
def world(dev):
    """(behind the session's device context: torch has the device before the library's own context opens it, as in the whole suite)"""
    from midoridb_amd.query import DB
    data, rng = world_data()
    db = DB()
    for name, names, shift, n in TABLES:
        c = [x.strip() for x in names.split(",")]
        db.execute(f"CREATE TABLE {name} ({c[0]} INT, {c[1]} DOUBLE, {c[2]} VARCHAR(12), {c[3]} DATE, {c[4]} INT);")
        cols, nulls = data[name]
        db.append_columns(name, [cols[0], cols[1].view(np.int64), cols[2], cols[3], cols[4]], [x.astype(np.uint8) for x in nulls])
    db.execute("CREATE TABLE E (ek INT, ed DOUBLE, es VARCHAR(12), et DATE, ev INT);")
    db.execute("CREATE TABLE ONE (ok INT, od DOUBLE, os VARCHAR(12), ot DATE, ov INT);")
    db.execute("INSERT INTO ONE VALUES (3, 1.5, 'name3', '2020-01-03', NULL);")
    # two small tables for the arms that join: P's keys 0 .. 49 several times, Q's partly outside
    db.execute("CREATE TABLE P (pk INT, pv INT);")
    db.append_columns("P", [rng.integers(0, 50, 400).astype(np.int64), rng.integers(0, 4, 400).astype(np.int64)])
    db.execute("CREATE TABLE Q (qk INT, qv INT);")
    db.append_columns("Q", [rng.integers(30, 80, 300).astype(np.int64), rng.integers(0, 4, 300).astype(np.int64)])
    yield db, data
    db.close()


def sql_rows(db, sql, wanted=None):
    """-> the rows in order, their columns in `wanted` order (result column names; None: as they come): DOUBLE cells as floats of the
    cell's bits, NULL as None"""
    res = db.query(sql, step_cursor=True)
    idx = list(range(len(res.names))) if wanted is None else [res.names.index(w) for w in wanted]
    rows = []
    for i in range(res.nrows):
        rows.append(tuple(None if res.nulls[c][i] else dbl(int(res.columns[c][i])) if res.types[c] == 3 else
                          res.columns[c][i] if res.types[c] == 0 else int(res.columns[c][i]) for c in idx))
    return rows, res


COLSETS = {"k": ([0], "k", "j", ["A.k"]), "d": ([1], "d", "e", ["A.d"]), "s": ([2], "s", "r", ["A.s"]), "t": ([3], "t", "u", ["A.t"]),
           "all": ([3, 2, 0, 1], "t, s, k, d", "u, r, j, e", ["A.t", "A.s", "A.k", "A.d"])}


@pytest.mark.parametrize("cols", list(COLSETS))
@pytest.mark.parametrize("op", OPS)
def test_each_operator_over_every_column_type(world, op, cols):
    db, data = world
    which, la, lb, names = COLSETS[cols]
    want = M.OPS[op](table_rows(*data["A"], which), table_rows(*data["B"], which))
    c0 = db.setop_calls()
    got, res = sql_rows(db, f"SELECT {la} FROM A {op} SELECT {lb} FROM B;", names)
    assert db.setop_calls() - c0 == (1 if op in (M.INTERSECT, M.EXCEPT) else 0)
    assert sorted(res.names) == sorted(names)                      # the first arm's names
    assert [M.row_key(r) for r in got] == [M.row_key(r) for r in want]
    assert 0 < len(got) and (op == M.UNIONALL or len(got) < N // 4)         # duplicates and overlaps were plentiful
    types = {"A.k": 1, "A.d": 3, "A.s": 0, "A.t": 4}
    assert [res.types[res.names.index(n)] for n in names] == [types[n] for n in names]


def test_the_arms_correspond_by_their_select_lists(world):
    """... whatever order the reference gives the columns of a result: (k, v) meets (w, j) as written"""
    db, data = world
    want = M.intersect(table_rows(*data["A"], [0, 4]), table_rows(*data["B"], [4, 0]))
    got, res = sql_rows(db, "SELECT k, v FROM A INTERSECT SELECT w, j FROM B;", ["A.k", "A.v"])
    assert got == want and len(got) > 3
    want = M.except_(table_rows(*data["A"], [4, 0]), table_rows(*data["B"], [0, 4]))
    got, res = sql_rows(db, "SELECT v, k FROM A EXCEPT SELECT j, w FROM B;", ["A.v", "A.k"])
    assert got == want and len(got) > 3


ARMS = {"join": ("SELECT pk, qv FROM P INNER JOIN Q ON pk = qk", ["P.pk", "Q.qv"]),
        "group": ("SELECT pk, SUM(pv) FROM P GROUP BY pk", ["P.pk", "SUM(P.pv)"]),
        "window": ("SELECT pk, ROW_NUMBER() OVER (PARTITION BY pk ORDER BY pv) AS rn FROM P", ["P.pk", "rn"]),
        "distinct": ("SELECT DISTINCT qk, qv FROM Q", ["Q.qk", "Q.qv"]),
        "where": ("SELECT qk, qv FROM Q WHERE qk IN (SELECT pk FROM P)", ["Q.qk", "Q.qv"])}


@pytest.mark.parametrize("left,op,right", [("join", M.UNION, "group"), ("group", M.EXCEPT, "window"), ("window", M.INTERSECT, "join"),
                                           ("distinct", M.UNIONALL, "join"), ("join", M.EXCEPT, "distinct"), ("where", M.UNION, "group"),
                                           ("distinct", M.INTERSECT, "where")])
def test_arms_that_are_joins_groups_windows_and_distincts(world, left, op, right):
    db, _ = world
    l, _ = sql_rows(db, ARMS[left][0] + ";", ARMS[left][1])
    r, _ = sql_rows(db, ARMS[right][0] + ";", ARMS[right][1])
    got, res = sql_rows(db, f"{ARMS[left][0]} {op} {ARMS[right][0]};", ARMS[left][1])
    assert got == M.OPS[op](l, r) and len(l) > 40 and len(r) > 40
    if op != M.EXCEPT:
        assert len(got) > 10


@pytest.mark.parametrize("op", OPS)
def test_an_empty_arm_on_either_side(world, op):
    db, data = world
    a = table_rows(*data["A"], [0, 2])
    got, res = sql_rows(db, f"SELECT k, s FROM A {op} SELECT ek, es FROM E;", ["A.k", "A.s"])
    assert got == M.OPS[op](a, [])
    got, res = sql_rows(db, f"SELECT ek, es FROM E {op} SELECT k, s FROM A;", ["E.ek", "E.es"])
    assert got == M.OPS[op]([], a) and res.types[res.names.index("E.es")] == 0
    got, res = sql_rows(db, f"SELECT ek FROM E {op} SELECT ek FROM E;")
    assert got == [] and res.names == ["E.ek"]
    got, res = sql_rows(db, f"SELECT k, s FROM A WHERE k > 1000 {op} SELECT j, r FROM B WHERE j < -1000 ORDER BY k LIMIT 5;")
    assert got == []


def test_one_row_arms(world):
    """a result of one row stays on the host: SELECT COUNT(*) alone, or any statement that found one row"""
    db, data = world
    got, res = sql_rows(db, "SELECT COUNT(*) FROM A UNION ALL SELECT COUNT(*) FROM B;")
    assert got == [(N,), (N,)] and res.names == ["COUNT(*)"]
    got, _ = sql_rows(db, "SELECT COUNT(*) FROM A UNION SELECT COUNT(*) FROM B UNION ALL SELECT COUNT(*) FROM C;")
    assert got == [(N,), (N // 2,)]
    got, _ = sql_rows(db, "SELECT COUNT(*) FROM A EXCEPT SELECT COUNT(*) FROM B;")
    assert got == []
    one = [(3, 1.5, "name3", None)]
    a = table_rows(*data["A"], [0, 1, 2, 4])
    names = ["ONE.ok", "ONE.od", "ONE.os", "ONE.ov"]
    got, _ = sql_rows(db, "SELECT ok, od, os, ov FROM ONE INTERSECT SELECT k, d, s, v FROM A;", names)
    assert got == M.intersect(one, a) == one            # (3, 1.5, 'name3', NULL) occurs in A: NULL = NULL
    got, _ = sql_rows(db, "SELECT ok, od, os, ov FROM ONE EXCEPT SELECT k, d, s, v FROM A;", names)
    assert got == []
    got, _ = sql_rows(db, "SELECT k, d, s, v FROM A EXCEPT SELECT ok, od, os, ov FROM ONE;", ["A.k", "A.d", "A.s", "A.v"])
    assert [M.row_key(r) for r in got] == [M.row_key(r) for r in M.except_(a, one)]
    got, _ = sql_rows(db, "SELECT ov, ok FROM ONE UNION ALL SELECT ov, ok FROM ONE;", ["ONE.ov", "ONE.ok"])
    assert got == [(None, 3), (None, 3)]
    got, _ = sql_rows(db, "SELECT MAX(v) FROM A WHERE k > 1000 UNION ALL SELECT MIN(w) FROM B;")
    assert got == [(-3,)]                               # (an aggregate over no rows answers no row, as COUNT(*) does)


def test_chains_of_three_and_of_eight_arms(world):
    db, data = world
    a, b, c = (table_rows(*data[x], [0, 2]) for x in "ABC")
    for o1, o2 in [(M.UNION, M.EXCEPT), (M.INTERSECT, M.UNION), (M.EXCEPT, M.UNIONALL), (M.INTERSECT, M.EXCEPT), (M.UNIONALL, M.UNION)]:
        c0 = db.setop_calls()
        got, _ = sql_rows(db, f"SELECT k, s FROM A {o1} SELECT j, r FROM B {o2} SELECT ck, cs FROM C;", ["A.k", "A.s"])
        assert got == M.chain(a, [(o1, b), (o2, c)]), (o1, o2)
        assert db.setop_calls() - c0 == sum(o in (M.INTERSECT, M.EXCEPT) for o in (o1, o2))
    arms = [("A", "k, s", a), ("B", "j, r", b), ("C", "ck, cs", c), ("A", "k, s", a), ("C", "ck, cs", c), ("B", "j, r", b), ("ONE", "ok, os", [(3, "name3")]),
            ("A", "k, s", a)]
    ops = [M.INTERSECT, M.INTERSECT, M.UNION, M.EXCEPT, M.UNIONALL, M.EXCEPT, M.UNION]
    sql = f"SELECT {arms[0][1]} FROM {arms[0][0]}" + "".join(f" {o} SELECT {x[1]} FROM {x[0]}" for o, x in zip(ops, arms[1:]))
    got, _ = sql_rows(db, sql + ";", ["A.k", "A.s"])
    assert got == M.chain(a, [(o, x[2]) for o, x in zip(ops, arms[1:])]) and len(got) > 5
    from midoridb_amd.query import QueryError
    with pytest.raises(QueryError) as ei:
        db.query(sql + " UNION SELECT k, s FROM A;")
    assert "more than 8 arms" in str(ei.value)


def test_order_by_and_limit_over_the_compound(world):
    db, data = world
    a, b = table_rows(*data["A"], [0, 3, 2]), table_rows(*data["B"], [0, 3, 2])
    for op in OPS:
        rows = M.OPS[op](a, b)
        got, res = sql_rows(db, f"SELECT k AS kk, t AS day, s FROM A {op} SELECT j, u, r FROM B ORDER BY day DESC, kk LIMIT 3, 10;", ["kk", "day", "A.s"])
        assert got == M.order_limit(rows, [(1, True), (0, False)], (3, 10)) and len(got) == 10        # (ties keep the compound's row order)
        got, _ = sql_rows(db, f"SELECT k AS kk, t, s FROM A {op} SELECT j, u, r FROM B ORDER BY kk DESC, t;", ["kk", "A.t", "A.s"])
        assert got == M.order_limit(rows, [(0, True), (1, False)])                                       # a column by its own name beside an alias
        got, _ = sql_rows(db, f"SELECT k, t, s FROM A {op} SELECT j, u, r FROM B LIMIT 7, 5;", ["A.k", "A.t", "A.s"])
        assert got == rows[7:12]
        got, _ = sql_rows(db, f"SELECT k, t, s FROM A {op} SELECT j, u, r FROM B ORDER BY k LIMIT 0;")
        assert got == []
        got, _ = sql_rows(db, f"SELECT k, t, s FROM A {op} SELECT j, u, r FROM B LIMIT 1000000, 5;")
        assert got == []
    got, _ = sql_rows(db, "SELECT d FROM A UNION SELECT e FROM B ORDER BY d;")          # DOUBLE keys: mdb_dev_sort_perm's order, NULL first
    assert got[0] == (None,) and [M.row_key(r) for r in got[1:4]] == [M.row_key((x,)) for x in (-2.25, dbl(1 << 63), 0.0)]


def test_same_statement_same_bytes_and_results_on_device_or_host(world):
    db, data = world
    sql = "SELECT k, d, t FROM A INTERSECT SELECT j, e, u FROM B EXCEPT SELECT ck, cd, ct FROM C;"
    want = M.chain(table_rows(*data["A"], [0, 1, 3]), [(M.INTERSECT, table_rows(*data["B"], [0, 1, 3])), (M.EXCEPT, table_rows(*data["C"], [0, 1, 3]))])
    host1, host2 = db.query(sql), db.query(sql)
    assert host1.names == host2.names and all(a.tobytes() == b.tobytes() for a, b in zip(host1.columns, host2.columns))
    got, _ = sql_rows(db, sql, ["A.k", "A.d", "A.t"])
    assert [M.row_key(r) for r in got] == [M.row_key(r) for r in want] and len(want) > 3
    db.results_on_device(True)
    try:
        names, types, cols, nrows, joined, ms = db.query_device(sql)
        nulls = db.last_device_nulls
        kept, _ = sql_rows(db, sql, ["A.k", "A.d", "A.t"])             # ... and read through the cursor: fetched on first use
    finally:
        db.results_on_device(False)
    assert nrows == len(want) and names == host1.names and ms > 0
    order = [names.index(x) for x in ("A.k", "A.d", "A.t")]
    host_cols = [c.cpu().numpy().view(np.int64) for c in cols]             # (a DOUBLE column: its cells' bits)
    host_nulls = [None if x is None else x.cpu().numpy() for x in nulls]
    dev_rows = []
    for i in range(nrows):
        dev_rows.append(tuple(None if host_nulls[c] is not None and host_nulls[c][i] else
                              dbl(int(host_cols[c][i])) if types[c] == 3 else int(host_cols[c][i]) for c in order))
    assert [M.row_key(r) for r in dev_rows] == [M.row_key(r) for r in want]
    assert [M.row_key(r) for r in kept] == [M.row_key(r) for r in want]


def test_after_a_refusal_the_database_still_answers(world):
    db, data = world
    from midoridb_amd.query import QueryError
    for bad, msg in [("SELECT k FROM A UNION SELECT e FROM B;", "column 1 is INTEGER in the first SELECT ('A.k') and DOUBLE in SELECT 2 ('B.e')"),
                     ("SELECT k, s FROM A EXCEPT SELECT j FROM B;", "the first SELECT has 2 result columns, SELECT 2 has 1"),
                     ("SELECT k FROM A INTERSECT SELECT j FROM B WHERE r IN (SELECT ck FROM C);", "IN (SELECT ...)")]:
        with pytest.raises(QueryError) as ei:
            db.query(bad)
        assert msg in str(ei.value)
        got, _ = sql_rows(db, "SELECT k FROM A WHERE k < 3 INTERSECT SELECT j FROM B;")
        assert got == [(2,)]


def test_sharded_mode_refuses_set_operations():
    """at world 2 on one GPU (the test transport of tests/_dist_gpu_worker.py): every rank gets the refusal, before any exchange"""
    from tests.test_dist_gpu import _run
    out = _run("setops", 2, 29671, worker="_setops_dist_worker.py", timeout=300)
    assert "sharded set operations refused ok" in out
