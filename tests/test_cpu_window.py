"""Window functions without a GPU: what the front end emits for fn(...) OVER (...) (this project's own RPN words `WINORDER d` and
`WINDOW fn npart norder`), that no word became reserved for it, every refusal that is decided before a device is needed, with its
message, that the operator is exported - and the numpy model of the operator's contract (tests/window_model.py) against SQLite.
The sharded-mode refusal needs an exchange handle, which needs a device: tests/test_window_gpu.py."""
import sqlite3

import numpy as np
import pytest

from tests import window_model as M

RANKING = ["ROW_NUMBER", "RANK", "DENSE_RANK"]
FOLDING = ["SUM", "MIN", "MAX", "AVG"]


def _rpn(sql):
    from oracle.ref import sql_to_rpn		# (the product's own front end, mdb_sql.c, through its C entry point)
    return sql_to_rpn(sql).strip().split("\n")


def _syntax_error(sql):
    from oracle.ref import sql_to_rpn
    with pytest.raises(ValueError) as ei:
        sql_to_rpn(sql)
    return str(ei.value)


# ------------------------------------------------------------------ grammar

@pytest.mark.parametrize("fn", RANKING)
def test_rpn_of_the_ranking_functions(fn):
    assert _rpn(f"SELECT {fn}() OVER () FROM A;") == [f"WINDOW {fn} 0 0", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn(f"SELECT k, {fn.lower()}() over (partition by k order by o) AS rn FROM A;") == [
        "NAME k", "NAME k", "NAME o", "WINORDER 0", f"WINDOW {fn} 1 1", "ALIAS rn", "TABLE A", "SELECT 0 3", "STMT"]
    assert _rpn(f"SELECT {fn}() OVER (PARTITION BY A.k, j ORDER BY A.o DESC, v ASC) rn FROM A;") == [
        "FIELDNAME A.k", "NAME j", "FIELDNAME A.o", "WINORDER 1", "NAME v", "WINORDER 0", f"WINDOW {fn} 2 2", "ALIAS rn", "TABLE A",
        "SELECT 0 2", "STMT"]
    assert _rpn(f"SELECT {fn}() OVER (ORDER BY o DESC) FROM A;")[:3] == ["NAME o", "WINORDER 1", f"WINDOW {fn} 0 1"]
    assert _rpn(f"SELECT {fn}() OVER (PARTITION BY k) FROM A;")[:2] == ["NAME k", f"WINDOW {fn} 1 0"]


@pytest.mark.parametrize("fn", FOLDING)
def test_rpn_of_the_running_aggregates(fn):
    assert _rpn(f"SELECT {fn}(v) OVER () FROM A;") == ["NAME v", f"WINDOW {fn} 0 0", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn(f"SELECT {fn}(A.v) OVER (PARTITION BY k ORDER BY A.o DESC) AS run, k FROM A WHERE k > 1;") == [
        "FIELDNAME A.v", "NAME k", "FIELDNAME A.o", "WINORDER 1", f"WINDOW {fn} 1 1", "ALIAS run", "NAME k", "TABLE A", "NAME k",
        "NUMBER 1", "CMP 2", "WHERE", "SELECT 0 4", "STMT"]
    # the aggregate without OVER is what it was
    assert _rpn(f"SELECT {fn}(v) FROM A;") == ["NAME v", f"AGG {fn}", "TABLE A", "SELECT 0 2", "STMT"]


def test_rpn_of_count_over_and_of_several_items():
    assert _rpn("SELECT COUNT(*) OVER (PARTITION BY k) c FROM A;") == ["NAME k", "WINDOW COUNT 1 0", "ALIAS c", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn("SELECT COUNT(*) FROM A;") == ["COUNTALL", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn("SELECT k, ROW_NUMBER() OVER (PARTITION BY k ORDER BY o) AS rn, SUM(v) OVER (PARTITION BY k ORDER BY o) AS s FROM A "
                "HAVING rn <= 3 ORDER BY k, rn;") == [
        "NAME k", "NAME k", "NAME o", "WINORDER 0", "WINDOW ROW_NUMBER 1 1", "ALIAS rn", "NAME v", "NAME k", "NAME o", "WINORDER 0",
        "WINDOW SUM 1 1", "ALIAS s", "TABLE A", "NAME rn", "NUMBER 3", "CMP 5", "HAVING", "NAME k", "ORDERBYITEM 0", "NAME rn",
        "ORDERBYITEM 0", "ORDERBYLIST 2", "SELECT 0 6", "STMT"]


def test_no_word_became_reserved():
    """over, rank, partition and row_number (and dense_rank, rows, range, window) stay names: of columns, of tables, of aliases"""
    assert _rpn("SELECT over, rank, partition, row_number FROM T WHERE rank > 1 AND over = 2 GROUP BY partition ORDER BY row_number;") == [
        "NAME over", "NAME rank", "NAME partition", "NAME row_number", "TABLE T", "NAME rank", "NUMBER 1", "CMP 2", "NAME over", "NUMBER 2",
        "CMP 4", "AND", "WHERE", "NAME partition", "GROUPBYLIST 1", "NAME row_number", "ORDERBYITEM 0", "ORDERBYLIST 1", "SELECT 0 8", "STMT"]
    assert _rpn("SELECT SUM(v) over FROM A;") == ["NAME v", "AGG SUM", "ALIAS over", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn("SELECT COUNT(*) over, MAX(v) AS rank FROM A;")[:5] == ["COUNTALL", "ALIAS over", "NAME v", "AGG MAX", "ALIAS rank"]
    assert _rpn("SELECT k AS partition, v rank FROM A AS over;") == ["NAME k", "ALIAS partition", "NAME v", "ALIAS rank", "TABLE A", "ALIAS over",
                                                                      "SELECT 0 3", "STMT"]
    assert _rpn("SELECT over.rank, rank.over FROM over INNER JOIN rank ON over.rank = rank.over;") == [
        "FIELDNAME over.rank", "FIELDNAME rank.over", "TABLE over", "TABLE rank", "FIELDNAME over.rank", "FIELDNAME rank.over", "CMP 4",
        "ONEXPR", "JOIN 1", "SELECT 0 3", "STMT"]
    assert _rpn("CREATE TABLE rank(over INT, partition INT, row_number INT, dense_rank INT);")[-2] == "CREATE 0 4 rank"
    assert _rpn("INSERT INTO rank(over) VALUES (1);") == ["COLUMN over", "INSERTCOLS 1", "NUMBER 1", "VALUES 1", "INSERTVALS 1 1 rank", "STMT"]
    assert _rpn("UPDATE rank SET over = 1 WHERE partition = 2;") == ["NUMBER 1", "ASSIGN over", "NAME partition", "NUMBER 2", "CMP 4", "WHERE",
                                                                   "UPDATE rank 1 1", "STMT"]
    # ... and inside a window: a column called `partition` orders it, one called `over` partitions it
    assert _rpn("SELECT RANK() OVER (PARTITION BY over ORDER BY partition, rank) FROM A;")[:6] == [
        "NAME over", "NAME partition", "WINORDER 0", "NAME rank", "WINORDER 0", "WINDOW RANK 1 2"]


@pytest.mark.parametrize("bad,msg", [
    ("SELECT SUM(v) OVER w FROM A;", "named windows"),
    ("SELECT RANK() OVER w FROM A;", "named windows"),
    ("SELECT RANK() OVER (w ORDER BY o) FROM A;", "named windows are not supported"),
    ("SELECT k FROM A HAVING k > 1 WINDOW w AS (ORDER BY k);", "named windows"),
    ("SELECT SUM(v) OVER (ORDER BY o ROWS BETWEEN 1 PRECEDING AND CURRENT ROW) FROM A;", "window frame clauses"),
    ("SELECT RANK() OVER (PARTITION BY k RANGE UNBOUNDED PRECEDING) FROM A;", "window frame clauses"),
    ("SELECT COUNT(v) OVER () FROM A;", "COUNT(col) OVER is not supported"),
    ("SELECT COUNT(A.v) OVER (PARTITION BY k) FROM A;", "COUNT(col) OVER is not supported"),
    ("SELECT COUNT(DISTINCT v) OVER () FROM A;", "DISTINCT inside a window function"),
    ("SELECT SUM(DISTINCT v) OVER (PARTITION BY k) FROM A;", "DISTINCT inside a window function"),
    ("SELECT RANK() FROM A;", "RANK() needs its window"),
    ("SELECT ROW_NUMBER(k) OVER () FROM A;", "ROW_NUMBER() takes no argument"),
    ("SELECT RANK() OVER (PARTITION BY k + 1) FROM A;", "expecting ')'"),
    ("SELECT RANK() OVER (ORDER BY 1) FROM A;", "inside OVER take columns"),
    ("SELECT k FROM A WHERE ROW_NUMBER() OVER (ORDER BY k) < 3;", "allowed in the select list only"),
    ("SELECT k FROM A INNER JOIN B ON RANK() OVER () = kb;", "allowed in the select list only"),
    ("SELECT k FROM A GROUP BY SUM(v) OVER ();", "allowed in the select list only"),
    ("SELECT k FROM A ORDER BY DENSE_RANK() OVER (ORDER BY k);", "allowed in the select list only"),
    ("SELECT k FROM A WHERE k IN (SELECT kb FROM B WHERE RANK() OVER () = 1);", "allowed in the select list only"),
    ("DELETE FROM A WHERE ROW_NUMBER() OVER () > 1;", "window function ROW_NUMBER ... OVER can't be used in DELETE / UPDATE"),
    ("UPDATE A SET v = RANK() OVER ();", "window function RANK ... OVER can't be used in DELETE / UPDATE"),
])
def test_front_end_refusals(bad, msg):
    assert msg in _syntax_error(bad)


def test_rpn_words_pass_the_plan_builder_and_bad_ones_do_not():
    from midoridb_amd.query import DB, QueryError
    with DB() as db:
        db.execute("CREATE TABLE A (k INT, v INT);")
        for rpn, msg in [("NUMBER 3\nWINDOW SUM 0 0\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),
                         ("NAME v\nWINDOW MEDIAN 0 0\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),
                         ("WINDOW SUM 0 0\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),
                         ("NAME k\nWINDOW RANK 0 1\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),      # an order field without its WINORDER
                         ("NAME k\nWINORDER 0\nWINDOW RANK 1 0\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),
                         ("WINDOW RANK 0 3\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),
                         ("NAME nosuch\nWINORDER 1\nWINDOW RANK 0 1\nTABLE A\nSELECT 0 2\nSTMT\n", "no such column")]:
            with pytest.raises(QueryError) as ei:
                db.query(rpn, rpn=True)
            assert msg in str(ei.value), (rpn, str(ei.value))


# ------------------------------------------------------------------ semantic checks

@pytest.fixture()
def db():
    from midoridb_amd.query import DB
    with DB() as d:
        d.execute("CREATE TABLE A (k INT, o INT, v INT, d DOUBLE, s VARCHAR(8), t DATE, u DATETIME, b TINYINT);")
        d.execute("INSERT INTO A VALUES (1, 1, 2, 1.5, 'x', '2020-01-01', '2020-01-01 10:00:00', TRUE);")
        d.execute("CREATE TABLE B (kb INT, w INT);")
        yield d


def _error(db, sql):
    from midoridb_amd.query import QueryError
    with pytest.raises(QueryError) as ei:
        db.query(sql)
    return str(ei.value)


@pytest.mark.parametrize("fn", FOLDING)
def test_argument_types(db, fn):
    assert f"{fn} ... OVER over the VARCHAR column 'A.s' is not supported" in _error(db, f"SELECT {fn}(s) OVER (PARTITION BY k) FROM A;")
    if fn in ("SUM", "AVG"):
        assert f"{fn} ... OVER over the DOUBLE column 'A.d' is not supported" in _error(db, f"SELECT {fn}(d) OVER (ORDER BY o) FROM A;")
        assert f"{fn} ... OVER over the DATE column 'A.t' is not supported" in _error(db, f"SELECT {fn}(t) OVER () FROM A;")
        assert f"{fn} ... OVER over the DATETIME column 'A.u' is not supported" in _error(db, f"SELECT {fn}(A.u) OVER () AS z FROM A;")


def test_keys(db):
    assert "ORDER BY over the VARCHAR column 'A.s' inside OVER is not supported" in _error(db, "SELECT RANK() OVER (ORDER BY s) FROM A;")
    assert "no such column: 'nosuch'" in _error(db, "SELECT RANK() OVER (PARTITION BY nosuch) FROM A;")
    assert "table is not part of from clause: 'Z'" in _error(db, "SELECT SUM(v) OVER (ORDER BY Z.o) FROM A;")
    nine = ", ".join(["k", "o", "v", "d", "t", "u", "b", "k", "o"])
    assert "more than 16 PARTITION BY and ORDER BY fields together" in _error(db, f"SELECT RANK() OVER (PARTITION BY {nine} ORDER BY {nine}) FROM A;")


def test_statement_shape(db):
    nine = ", ".join(f"ROW_NUMBER() OVER (ORDER BY o) AS r{i}" for i in range(9))
    assert "more than 8 window functions in one select list" in _error(db, f"SELECT {nine} FROM A;")
    assert "a window function beside GROUP BY is not supported" in _error(db, "SELECT k, RANK() OVER (ORDER BY k) FROM A GROUP BY k;")
    assert "beside COUNT(*) or an aggregate without OVER" in _error(db, "SELECT COUNT(*), RANK() OVER (ORDER BY k) FROM A;")
    assert "beside COUNT(*) or an aggregate without OVER" in _error(db, "SELECT SUM(v) OVER (), MAX(v) FROM A;")
    assert "a window function inside an expression is not supported" in _error(db, "SELECT ROW_NUMBER() OVER (ORDER BY k) + 1 FROM A;")
    assert "a window function inside an expression is not supported" in _error(db, "SELECT -SUM(v) OVER () AS z FROM A;")
    assert "duplicate column name: 'ROW_NUMBER() OVER'" in _error(db, "SELECT ROW_NUMBER() OVER (ORDER BY k), ROW_NUMBER() OVER (ORDER BY o) FROM A;")
    assert "duplicate column name: 'SUM(A.v) OVER'" in _error(db, "SELECT SUM(v) OVER (), SUM(A.v) OVER (PARTITION BY k) FROM A;")
    assert "duplicate alias: 'rn'" in _error(db, "SELECT RANK() OVER () AS rn, DENSE_RANK() OVER () AS rn FROM A;")


def test_where_an_alias_may_be_named(db):
    assert "no such column: 'rn'" in _error(db, "SELECT k, ROW_NUMBER() OVER (ORDER BY o) AS rn FROM A WHERE rn <= 3;")
    assert "no such column: 'rn'" in _error(db, "SELECT k, RANK() OVER (ORDER BY o) AS rn FROM A INNER JOIN B ON rn = kb;")
    assert "comparison operands must have the same type" in _error(db, "SELECT AVG(v) OVER () AS a FROM A HAVING a > 1;")    # (AVG is DOUBLE)


def _reaches_the_device(db, sql):
    import torch
    if torch.cuda.is_available():
        db.query(sql)
    else:
        assert "no usable HIP device" in _error(db, sql), sql


def test_what_is_accepted_fails_only_for_lack_of_a_device(db):
    for sql in ["SELECT k, ROW_NUMBER() OVER (PARTITION BY k ORDER BY o) AS rn FROM A HAVING rn <= 3 ORDER BY k, rn;",
                "SELECT RANK() OVER (PARTITION BY s, d ORDER BY t DESC, u, b, d), DENSE_RANK() OVER (), COUNT(*) OVER (PARTITION BY s) FROM A;",
                "SELECT SUM(v) OVER (ORDER BY o), MIN(d) OVER (), MAX(t) OVER (), MIN(u) OVER (), AVG(b) OVER (), SUM(b) OVER (), AVG(v) OVER () a FROM A HAVING a > 1.0;",
                "SELECT DISTINCT DENSE_RANK() OVER (ORDER BY k) AS dr FROM A ORDER BY dr DESC LIMIT 2;",
                "SELECT k, w, SUM(w) OVER (PARTITION BY w ORDER BY k) FROM A LEFT JOIN B ON k = kb WHERE o > 0;"]:
        _reaches_the_device(db, sql)


def test_the_operator_is_exported_and_bound():
    from midoridb_amd.lib import load_library
    from midoridb_amd import dev, query
    lib = load_library()
    assert hasattr(lib, "mdb_dev_window") and hasattr(lib, "mdb_database_window_calls")
    assert "mdb_dev_window" in dev.DEV_SYMBOLS and "mdb_database_window_calls" in query.QUERY_SYMBOLS
    assert [name for name, _ in dev.WindowFn._fields_] == ["op", "type", "values", "nullbits", "rid", "out", "out_nullbits"]
    assert (dev.WIN_ROW_NUMBER, dev.WIN_RANK, dev.WIN_DENSE_RANK, dev.WIN_COUNT, dev.WIN_SUM, dev.WIN_MIN, dev.WIN_MAX, dev.WIN_AVG) == \
        (M.ROW_NUMBER, M.RANK, M.DENSE_RANK, M.COUNT, M.SUM, M.MIN, M.MAX, M.AVG) == tuple(range(1, 9))


# ------------------------------------------------------------------ the model against SQLite

def _sqlite_world():
    """~300 rows: NULL partition keys, NULL order keys, NULL cells, ties in the order keys, a partition whose cells are all NULL"""
    rng = np.random.default_rng(20)
    n = 307
    k = rng.integers(0, 7, n).astype(np.int64)
    kn = rng.random(n) < 0.08
    o = rng.integers(0, 12, n).astype(np.int64)                 # ties
    on = rng.random(n) < 0.1
    o2 = rng.integers(-3, 3, n).astype(np.int64)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    vn = (rng.random(n) < 0.15) | (k == 3)                      # partition 3: every cell NULL
    x = (rng.integers(-40, 40, n) / 8.0).astype(np.float64)     # (no +-0.0 in a key; as cells both compare equal in SQLite, so none either)
    x[x == 0.0] = 0.125
    xn = rng.random(n) < 0.15
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE A (k INTEGER, o INTEGER, o2 INTEGER, v INTEGER, x REAL)")
    con.executemany("INSERT INTO A VALUES (?, ?, ?, ?, ?)",
                    [(None if kn[i] else int(k[i]), None if on[i] else int(o[i]), int(o2[i]), None if vn[i] else int(v[i]),
                      None if xn[i] else float(x[i])) for i in range(n)])
    return con, n, dict(k=(k, kn), o=(o, on), o2=(o2, None), v=(v, vn), x=(x, xn))


WINDOWS = [("", [], []),
           ("PARTITION BY k", ["k"], []),
           ("ORDER BY o", [], [("o", False)]),
           ("PARTITION BY k ORDER BY o", ["k"], [("o", False)]),
           ("PARTITION BY k ORDER BY o DESC, o2", ["k"], [("o", True), ("o2", False)]),
           ("PARTITION BY k, o2 ORDER BY o DESC", ["k", "o2"], [("o", True)]),
           ("PARTITION BY x ORDER BY x DESC, o", ["x"], [("x", True), ("o", False)])]


@pytest.mark.parametrize("over,part,order", WINDOWS)
def test_model_against_sqlite(over, part, order):
    assert sqlite3.sqlite_version_info >= (3, 25), "SQLite without window functions"
    con, n, cols = _sqlite_world()
    pk = [(cols[c][0], cols[c][1], False) for c in part]
    ok = [(cols[c][0], cols[c][1], desc) for c, desc in order]
    fns = [(M.ROW_NUMBER,), (M.RANK,), (M.DENSE_RANK,), (M.COUNT,), (M.SUM,) + cols["v"], (M.MIN,) + cols["v"], (M.MAX,) + cols["v"],
           (M.AVG,) + cols["v"], (M.MIN,) + cols["x"], (M.MAX,) + cols["x"]]
    got = M.window_model(pk, ok, n, fns)
    # ROW_NUMBER: ties keep the stream order - rowid as SQLite's last order key
    rn_over = over + (", rowid" if order else " ORDER BY rowid")
    sql = (f"SELECT ROW_NUMBER() OVER ({rn_over}), RANK() OVER ({over}), DENSE_RANK() OVER ({over}), COUNT(*) OVER ({over}), SUM(v) OVER ({over}), "
           f"MIN(v) OVER ({over}), MAX(v) OVER ({over}), AVG(v) OVER ({over}), MIN(x) OVER ({over}), MAX(x) OVER ({over}) FROM A ORDER BY rowid")
    want = con.execute(sql).fetchall()
    assert len(want) == n
    assert _rpn(sql.replace(", rowid", "").replace(" ORDER BY rowid", "") + ";")[-1] == "STMT"     # (what SQLite answers here, the front end takes)
    for f in range(len(fns)):
        vals, nulls = got[f]
        mine = [None if nulls[i] else (float(vals[i]) if vals.dtype == np.float64 else int(vals[i])) for i in range(n)]
        assert mine == [r[f] for r in want], (over, f)


def test_model_small_streams_agree_with_the_sentences():
    """n <= 65: window_model() itself asserts that the vectorised evaluation and the sentence-by-sentence one agree - here over every
    function, both zeros in DOUBLE cells and keys, INT64_MIN / INT64_MAX (SUM wraps), DESC keys, NULLs everywhere"""
    from midoridb_amd import dev
    assert M.SMALL >= 65 and dev.WIN_MAX_FNS == 8
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 64, 65):
        k = rng.integers(0, 3, n).astype(np.int64)
        o = rng.choice(np.array([-0.0, 0.0, 1.5, -2.25]), n)
        v = rng.integers(-5, 5, n).astype(np.int64)
        v[rng.random(n) < 0.3] = np.iinfo(np.int64).max
        v[rng.random(n) < 0.2] = np.iinfo(np.int64).min
        x = rng.choice(np.array([-0.0, 0.0, 3.0, -1.0]), n)
        nl = lambda p: rng.random(n) < p
        fns = [(M.ROW_NUMBER,), (M.RANK,), (M.DENSE_RANK,), (M.COUNT,), (M.SUM, v, nl(0.2)), (M.AVG, v, nl(0.2)), (M.MIN, v, None),
               (M.MAX, v, nl(0.5)), (M.MIN, x, nl(0.2)), (M.MAX, x, nl(0.2))]
        for part, order in [([], []), ([(k, nl(0.2), False)], []), ([], [(o, nl(0.2), True)]), ([(k, nl(0.2), False)], [(o, nl(0.1), False), (v, None, True)])]:
            out = M.window_model(part, order, n, fns)
            assert len(out) == len(fns) and all(len(vals) == n and len(nulls) == n for vals, nulls in out)
    # -0.0 and +0.0 in a DOUBLE order key are different peers, -0.0 first ascending
    o = np.array([0.0, -0.0, 0.0, -0.0])
    (rank, _), (dense, _) = M.window_model([], [(o, None, False)], 4, [(M.RANK,), (M.DENSE_RANK,)])
    assert list(rank) == [3, 1, 3, 1] and list(dense) == [2, 1, 2, 1]
