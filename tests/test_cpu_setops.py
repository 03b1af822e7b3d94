"""Set operations without a GPU: what the front end emits for UNION [ALL] / INTERSECT / EXCEPT (this project's own RPN words `SETOP op`,
`SETORDER d`, `SETLIMIT n` and `COMPOUND narms norder nlimit`), that no word became reserved for them, every refusal that is decided
before a device is needed, with its message, that the operators are exported - and the model of the four operations
(tests/setops_model.py) against SQLite.  The sharded-mode refusal needs an exchange handle, which needs a device:
tests/test_setops_gpu.py."""
import sqlite3

import numpy as np
import pytest

from tests import setops_model as M


def _rpn(sql):
    from oracle.ref import sql_to_rpn		# (the product's own front end, mdb_sql.c, through its C entry point)
    return sql_to_rpn(sql).strip().split("\n")


def _syntax_error(sql):
    from oracle.ref import sql_to_rpn
    with pytest.raises(ValueError) as ei:
        sql_to_rpn(sql)
    return str(ei.value)


# ------------------------------------------------------------------ the model against SQLite

def _random_table(rng, n):
    """(k INTEGER, s VARCHAR) over small domains, NULLs in both"""
    ks = [None if rng.random() < 0.15 else int(rng.integers(0, 6)) for _ in range(n)]
    ss = [None if rng.random() < 0.15 else "abcd"[int(rng.integers(0, 4))] for _ in range(n)]
    return list(zip(ks, ss))


@pytest.fixture(scope="module")
def lite():
    rng = np.random.default_rng(20260)
    tables = {name: _random_table(rng, 200) for name in "ABC"}
    con = sqlite3.connect(":memory:")
    for name, rows in tables.items():
        con.execute(f"CREATE TABLE {name} (k INTEGER, s VARCHAR(8))")
        con.executemany(f"INSERT INTO {name} VALUES (?, ?)", rows)
    yield con, tables
    con.close()


def _canon(rows):
    return sorted(rows, key=lambda r: tuple((0, "") if v is None else (1, str(v)) for v in r))


@pytest.mark.parametrize("op", [M.UNION, M.UNIONALL, M.INTERSECT, M.EXCEPT])
@pytest.mark.parametrize("cols", ["k", "s", "k, s"])
def test_the_model_against_sqlite(lite, op, cols):
    con, t = lite
    pick = {"k": lambda r: (r[0],), "s": lambda r: (r[1],), "k, s": lambda r: r}[cols]
    got = M.OPS[op]([pick(r) for r in t["A"]], [pick(r) for r in t["B"]])
    want = con.execute(f"SELECT {cols} FROM A {op} SELECT {cols} FROM B").fetchall()
    assert _canon(got) == _canon(want)          # (SQLite sorts a compound's rows: compared as sorted lists)
    if op != M.UNIONALL:
        assert len(set(got)) == len(got)


@pytest.mark.parametrize("ops", [(M.UNION, M.UNION), (M.UNIONALL, M.UNION), (M.UNION, M.EXCEPT), (M.INTERSECT, M.INTERSECT), (M.INTERSECT, M.UNION),
                                 (M.INTERSECT, M.EXCEPT), (M.EXCEPT, M.EXCEPT), (M.EXCEPT, M.UNIONALL), (M.UNIONALL, M.UNIONALL)])
def test_chains_of_three_arms_against_sqlite(lite, ops):
    """the accepted grammar only (no INTERSECT behind a UNION or EXCEPT): there the standard's reading and SQLite's left-to-right one agree"""
    con, t = lite
    got = M.chain(t["A"], [(ops[0], t["B"]), (ops[1], t["C"])])
    want = con.execute(f"SELECT k, s FROM A {ops[0]} SELECT k, s FROM B {ops[1]} SELECT k, s FROM C").fetchall()
    assert _canon(got) == _canon(want)


def test_the_models_row_order():
    L = [(2, "b"), (1, None), (2, "b"), (None, None), (3, "c"), (1, None), (None, None)]
    R = [(3, "c"), (None, None), (9, "z"), (3, "c")]
    assert M.union_all(L, R) == L + R
    assert M.union(L, R) == [(2, "b"), (1, None), (None, None), (3, "c"), (9, "z")]                   # first occurrences, in the concatenation's order
    assert M.intersect(L, R) == [(None, None), (3, "c")]                                              # L's order, NULL = NULL
    assert M.except_(L, R) == [(2, "b"), (1, None)]
    assert M.intersect(R, L) == [(3, "c"), (None, None)]
    assert M.chain(L, [(M.EXCEPT, R), (M.UNIONALL, R)]) == [(2, "b"), (1, None)] + R
    assert M.order_limit(M.union(L, R), [(0, True)], (1, 3)) == [(3, "c"), (2, "b"), (1, None)]     # DESC: NULL last
    assert M.order_limit(M.union(L, R), [(0, False)]) == [(None, None), (1, None), (2, "b"), (3, "c"), (9, "z")]
    # doubles by their bits
    nan1, nan2 = np.uint64(0x7FF8000000000000).view(np.float64), np.uint64(0x7FF8000000000001).view(np.float64)
    assert M.intersect([(0.0,), (-0.0,), (nan1,), (nan2,)], [(-0.0,), (nan2,)]) == [(-0.0,), (nan2,)]
    assert M.rows_semi([(1, None), (2, 2), (None, None)], [(None, None), (1, None), (1, None)]) == ([0, 2], 2)
    assert M.rows_semi([(1, None), (2, 2), (None, None)], [(None, None), (1, None)], anti=True) == ([1], 2)
    v, w = M.concat64([(np.arange(63), np.ones(63, dtype=bool)), (np.arange(2), None), (np.arange(1), np.ones(1, dtype=bool))])
    assert len(v) == 66 and list(w) == [(1 << 63) - 1, 0b10]


# ------------------------------------------------------------------ grammar

def test_rpn_of_compound_statements():
    a, b = ["NAME k", "TABLE A", "SELECT 0 2"], ["NAME j", "TABLE B", "SELECT 0 2"]
    assert _rpn("SELECT k FROM A UNION SELECT j FROM B;") == a + b + ["SETOP UNION", "COMPOUND 2 0 0", "STMT"]
    assert _rpn("select k from A union distinct select j from B;") == a + b + ["SETOP UNION", "COMPOUND 2 0 0", "STMT"]
    assert _rpn("SELECT k FROM A UNION ALL SELECT j FROM B;") == a + b + ["SETOP UNIONALL", "COMPOUND 2 0 0", "STMT"]
    assert _rpn("SELECT k FROM A Intersect SELECT j FROM B;") == a + b + ["SETOP INTERSECT", "COMPOUND 2 0 0", "STMT"]
    assert _rpn("SELECT k FROM A INTERSECT DISTINCT SELECT j FROM B;") == a + b + ["SETOP INTERSECT", "COMPOUND 2 0 0", "STMT"]
    assert _rpn("SELECT k FROM A EXCEPT\n SELECT j FROM B;") == a + b + ["SETOP EXCEPT", "COMPOUND 2 0 0", "STMT"]
    assert _rpn("SELECT k FROM A EXCEPT DISTINCT SELECT j FROM B;") == a + b + ["SETOP EXCEPT", "COMPOUND 2 0 0", "STMT"]
    assert _rpn("SELECT k FROM A INTERSECT SELECT j FROM B EXCEPT SELECT k FROM A UNION ALL SELECT j FROM B ORDER BY k DESC, j LIMIT 2, 3;") == \
        a + b + ["SETOP INTERSECT"] + a + ["SETOP EXCEPT"] + b + ["SETOP UNIONALL", "NAME k", "SETORDER 1", "NAME j", "SETORDER 0", "NUMBER 2", "NUMBER 3",
                                                                      "SETLIMIT 2", "COMPOUND 4 2 1", "STMT"]
    assert _rpn("SELECT k FROM A UNION SELECT j FROM B LIMIT 5;")[-4:] == ["NUMBER 5", "SETLIMIT 1", "COMPOUND 2 0 1", "STMT"]
    # every arm is an ordinary SELECT: what it emits alone, then its operator
    arm = "SELECT DISTINCT A.k AS x, SUM(v) s FROM A INNER JOIN B ON k = j WHERE k IN (SELECT j FROM B ORDER BY j LIMIT 3) GROUP BY k HAVING s > 1"
    alone = _rpn(arm + ";")[:-1]
    assert _rpn(f"{arm} UNION {arm} ORDER BY x;") == alone + alone + ["SETOP UNION", "NAME x", "SETORDER 0", "COMPOUND 2 1 0", "STMT"]
    eight = " UNION ALL ".join(["SELECT k FROM A"] * 8)
    assert _rpn(eight + ";")[-2] == "COMPOUND 8 0 0"
    assert "more than 8 arms" in _syntax_error(eight + " UNION ALL SELECT k FROM A;")


def test_no_word_became_reserved():
    """union, intersect, except and all stay names: of columns, of tables, of aliases - wherever no SELECT stands behind them"""
    assert _rpn("SELECT union, except FROM intersect;") == ["NAME union", "NAME except", "TABLE intersect", "SELECT 0 3", "STMT"]
    assert _rpn("SELECT k union FROM A;") == ["NAME k", "ALIAS union", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn("SELECT k FROM A union;") == ["NAME k", "TABLE A", "ALIAS union", "SELECT 0 2", "STMT"]
    assert _rpn("CREATE TABLE union (all INT);") == ["STARTCOL", "COLUMNDEF 50000 all", "CREATE 0 1 union", "STMT"]
    assert _rpn("SELECT all, A.except AS intersect FROM A except WHERE all > 1 ORDER BY all;") == [
        "NAME all", "FIELDNAME A.except", "ALIAS intersect", "TABLE A", "ALIAS except", "NAME all", "NUMBER 1", "CMP 2", "WHERE", "NAME all",
        "ORDERBYITEM 0", "ORDERBYLIST 1", "SELECT 0 5", "STMT"]
    assert _rpn("SELECT k FROM A union INNER JOIN B all ON k = j;") == ["NAME k", "TABLE A", "ALIAS union", "TABLE B", "ALIAS all", "NAME k", "NAME j",
                                                                        "CMP 4", "ONEXPR", "JOIN 1", "SELECT 0 2", "STMT"]
    # ... and as an alias right in front of the operator: the second `union` is the operator
    assert _rpn("SELECT k FROM A union UNION SELECT j all FROM B;") == ["NAME k", "TABLE A", "ALIAS union", "SELECT 0 2", "NAME j", "ALIAS all", "TABLE B",
                                                                        "SELECT 0 2", "SETOP UNION", "COMPOUND 2 0 0", "STMT"]
    assert _rpn("INSERT INTO union (all) VALUES (1);") == ["COLUMN all", "INSERTCOLS 1", "NUMBER 1", "VALUES 1", "INSERTVALS 1 1 union", "STMT"]


@pytest.mark.parametrize("bad,msg", [
    ("SELECT k FROM A INTERSECT ALL SELECT j FROM B;", "INTERSECT ALL is not supported: multiset semantics are not built"),
    ("SELECT k FROM A EXCEPT ALL SELECT j FROM B;", "EXCEPT ALL is not supported: multiset semantics are not built"),
    ("SELECT k FROM A ORDER BY k UNION SELECT j FROM B;", "ORDER BY / LIMIT in an arm of a set operation that is not the last"),
    ("SELECT k FROM A LIMIT 3 UNION ALL SELECT j FROM B;", "ORDER BY / LIMIT in an arm of a set operation that is not the last"),
    ("SELECT k FROM A UNION SELECT j FROM B ORDER BY k EXCEPT SELECT j FROM B;", "ORDER BY / LIMIT in an arm of a set operation that is not the last"),
    ("SELECT k FROM A UNION SELECT j FROM B LIMIT 1 UNION SELECT j FROM B;", "ORDER BY / LIMIT in an arm of a set operation that is not the last"),
    ("SELECT k FROM A UNION (SELECT j FROM B);", "a parenthesised SELECT as an arm of a set operation is not supported"),
    ("SELECT k FROM A UNION ALL (SELECT j FROM B);", "a parenthesised SELECT as an arm of a set operation is not supported"),
    ("(SELECT k FROM A) UNION SELECT j FROM B;", "a parenthesised SELECT as an arm of a set operation is not supported"),
    ("SELECT k FROM A WHERE k IN (SELECT j FROM B UNION SELECT j FROM B);", "a set operation (UNION / INTERSECT / EXCEPT) inside IN (SELECT ...) is not supported"),
    ("DELETE FROM A WHERE k IN (SELECT j FROM B EXCEPT SELECT j FROM B);", "inside IN (SELECT ...) is not supported"),
    ("SELECT k FROM A UNION SELECT j FROM B INTERSECT SELECT k FROM A;", "the standard binds INTERSECT tighter, SQLite reads left to right"),
    ("SELECT k FROM A EXCEPT SELECT j FROM B INTERSECT SELECT k FROM A;", "INTERSECT behind UNION or EXCEPT in one chain is not supported"),
    ("SELECT k FROM A INTERSECT SELECT j FROM B UNION ALL SELECT j FROM B INTERSECT SELECT k FROM A;", "there are no parentheses to say which"),
    ("SELECT k FROM A UNION SELECT j FROM B ORDER BY A.k;", "by their bare names"),
    ("SELECT k FROM A UNION SELECT j FROM B ORDER BY k + 1;", "expecting ';'"),
    ("SELECT k FROM A UNION SELECT j FROM B ORDER BY 1;", "by their bare names"),
    ("SELECT k FROM A UNION j FROM B;", "expecting ';'"),                     # (no SELECT behind it: `union` is the table's alias)
])
def test_front_end_refusals(bad, msg):
    assert msg in _syntax_error(bad)


def test_rpn_words_pass_the_plan_builder_and_bad_ones_do_not():
    from midoridb_amd.query import DB, QueryError
    a, b = "NAME k\nTABLE A\nSELECT 0 2\n", "NAME j\nTABLE B\nSELECT 0 2\n"
    with DB() as db:
        db.execute("CREATE TABLE A (k INT, v INT);")
        db.execute("CREATE TABLE B (j INT, w INT);")
        for rpn, msg in [(a + b + "SETOP UNION\nSTMT\n", "syntax analysis"),                                  # a chain without its COMPOUND
                         (a + b + "SETOP MINUS\nCOMPOUND 2 0 0\nSTMT\n", "syntax analysis"),
                         (a + "SETOP UNION\nCOMPOUND 2 0 0\nSTMT\n", "syntax analysis"),                      # one SELECT on the stack
                         (a + b + "SETOP UNION\nCOMPOUND 3 0 0\nSTMT\n", "syntax analysis"),                  # the arm count does not match
                         (a + b + "SETOP UNION\nCOMPOUND 2 1 0\nSTMT\n", "syntax analysis"),                  # an order item that is not there
                         (a + b + "SETOP UNION\nNAME k\nCOMPOUND 2 1 0\nSTMT\n", "syntax analysis"),          # ... without its SETORDER
                         (a + b + "SETOP UNION\nNUMBER 1\nSETORDER 0\nCOMPOUND 2 1 0\nSTMT\n", "syntax analysis"),
                         (a + b + "SETOP UNION\nNUMBER 1\nCOMPOUND 2 0 1\nSTMT\n", "syntax analysis"),        # a limit without its SETLIMIT
                         (a + b + "SETOP UNION\nNUMBER 1\nSETLIMIT 3\nCOMPOUND 2 0 1\nSTMT\n", "syntax analysis"),
                         (a + b + "SETOP UNION\nNAME k\nSETLIMIT 1\nCOMPOUND 2 0 1\nSTMT\n", "LIMIT takes non-negative integer literals"),
                         (a + b + "SETOP UNION\nCOMPOUND 2 0 0\n" + b + "SETOP UNION\nCOMPOUND 3 0 0\nSTMT\n", "syntax analysis"),   # a closed chain goes on
                         (a + "NAME j\nTABLE B\nNAME j\nORDERBYITEM 0\nORDERBYLIST 1\nSELECT 0 3\nSETOP UNION\nCOMPOUND 2 0 0\nSTMT\n", "syntax analysis"),
                         ("NAME k\nTABLE A\nNUMBER 1\nLIMIT 1\nSELECT 0 3\n" + b + "SETOP UNION\nCOMPOUND 2 0 0\nSTMT\n", "syntax analysis"),
                         ("NAME k\nTABLE A\nNAME k\n" + b + b + "SETOP UNION\nCOMPOUND 2 0 0\nSUBQUERY\nISINSUB\nWHERE\nSELECT 0 3\nSTMT\n", "syntax analysis"),
                         (a + b + "SETOP UNION\n" + a + "SETOP INTERSECT\nCOMPOUND 3 0 0\nSTMT\n", "INTERSECT behind UNION or EXCEPT"),
                         (a + (b + "SETOP UNIONALL\n") * 8 + "COMPOUND 9 0 0\nSTMT\n", "more than 8 arms"),
                         (a + "NAME nosuch\nTABLE B\nSELECT 0 2\nSETOP EXCEPT\nCOMPOUND 2 0 0\nSTMT\n", "no such column")]:
            with pytest.raises(QueryError) as ei:
                db.query(rpn, rpn=True)
            assert msg in str(ei.value), (rpn, str(ei.value))
        # a well-formed one is accepted by the builder: it fails for lack of a device, or runs
        _reaches_the_device(db, a + b + "SETOP EXCEPT\nNAME k\nSETORDER 1\nNUMBER 0\nNUMBER 2\nSETLIMIT 2\nCOMPOUND 2 1 1\nSTMT\n", rpn=True)


# ------------------------------------------------------------------ semantic checks

@pytest.fixture()
def db():
    from midoridb_amd.query import DB
    with DB() as d:
        d.execute("CREATE TABLE A (k INT, v INT, d DOUBLE, s VARCHAR(8), t DATE);")
        d.execute("INSERT INTO A VALUES (1, 2, 1.5, 'x', '2020-01-01');")
        d.execute("CREATE TABLE B (j INT, w INT, e DOUBLE, r VARCHAR(12), u DATE, z DATETIME);")
        d.execute("CREATE TABLE W (" + ", ".join(f"c{i} INT" for i in range(17)) + ");")
        d.execute("CREATE TABLE X (" + ", ".join(f"x{i} INT" for i in range(17)) + ");")
        yield d


def _error(db, sql):
    from midoridb_amd.query import QueryError
    with pytest.raises(QueryError) as ei:
        db.query(sql)
    return str(ei.value)


def _reaches_the_device(db, sql, rpn=False):
    import torch
    from midoridb_amd.query import QueryError
    if torch.cuda.is_available():
        db.query(sql, rpn=rpn)
    else:
        with pytest.raises(QueryError) as ei:
            db.query(sql, rpn=rpn)
        assert "no usable HIP device" in str(ei.value), sql


def test_column_counts(db):
    assert "UNION: the first SELECT has 1 result columns, SELECT 2 has 2: all arms of a set operation must have the same number" in \
        _error(db, "SELECT k FROM A UNION SELECT j, w FROM B;")
    assert "EXCEPT: the first SELECT has 2 result columns, SELECT 3 has 1" in _error(db, "SELECT k, v FROM A INTERSECT SELECT j, w FROM B EXCEPT SELECT j FROM B;")
    assert "UNION ALL: the first SELECT has 5 result columns, SELECT 2 has 6" in _error(db, "SELECT * FROM A UNION ALL SELECT * FROM B;")


def test_column_types(db):
    """no coercion: the position in the select lists and both types are named"""
    assert "UNION: column 2 is INTEGER in the first SELECT ('A.v') and DOUBLE in SELECT 2 ('B.e'): both sides must have the same type" in \
        _error(db, "SELECT k, v FROM A UNION SELECT j, e FROM B;")
    assert "INTERSECT: column 1 is VARCHAR in the first SELECT ('A.s') and INTEGER in SELECT 2 ('B.j')" in _error(db, "SELECT s FROM A INTERSECT SELECT j FROM B;")
    assert "EXCEPT: column 1 is DATE in the first SELECT ('A.t') and DATETIME in SELECT 2 ('B.z')" in _error(db, "SELECT t FROM A EXCEPT SELECT z FROM B;")
    assert "UNION ALL: column 1 is INTEGER in the first SELECT ('A.k') and DOUBLE in SELECT 3 ('AVG(B.w)')" in \
        _error(db, "SELECT k FROM A UNION ALL SELECT j FROM B UNION ALL SELECT AVG(w) FROM B;")
    assert "column 1 is INTEGER in the first SELECT ('n') and VARCHAR in SELECT 2 ('B.r')" in _error(db, "SELECT COUNT(*) AS n FROM A UNION SELECT r FROM B;")
    # the arms correspond by their select lists, whatever order the reference gives a result's columns
    assert "column 1 is VARCHAR in the first SELECT ('A.s') and INTEGER in SELECT 2 ('B.j')" in _error(db, "SELECT s, k FROM A UNION SELECT j, r FROM B;")
    _reaches_the_device(db, "SELECT s, k FROM A UNION SELECT r, j FROM B;")
    _reaches_the_device(db, "SELECT k, s FROM A UNION SELECT j, r FROM B;")


def test_arms_are_resolved_on_their_own(db):
    assert "no such column: 'j'" in _error(db, "SELECT j FROM A UNION SELECT j FROM B;")
    assert "table doesn't exist: 'Nope'" in _error(db, "SELECT k FROM A EXCEPT SELECT k FROM Nope;")
    assert "SELECT list is not in GROUP BY clause" in _error(db, "SELECT k FROM A UNION SELECT j FROM B GROUP BY w;")
    _reaches_the_device(db, "SELECT k FROM A UNION SELECT k FROM A;")          # the same names in two arms do not clash


def test_too_many_columns(db):
    assert "UNION, INTERSECT and EXCEPT over more than 16 columns are not supported (UNION ALL takes any number): 17 result columns" in \
        _error(db, "SELECT * FROM W UNION SELECT * FROM X;")
    assert "over more than 16 columns" in _error(db, "SELECT * FROM W UNION ALL SELECT * FROM X EXCEPT SELECT * FROM X;")
    _reaches_the_device(db, "SELECT * FROM W UNION ALL SELECT * FROM X;")


def test_order_by_of_the_compound(db):
    assert "ORDER BY behind a set operation: 'j' is no result column of the first SELECT (a column's name or an alias)" in \
        _error(db, "SELECT k FROM A UNION SELECT j FROM B ORDER BY j;")
    assert "'v' is no result column of the first SELECT" in _error(db, "SELECT k FROM A UNION SELECT j FROM B ORDER BY v;")
    assert "'k' is no result column of the first SELECT" in _error(db, "SELECT k AS kk FROM A UNION SELECT j FROM B ORDER BY k;")
    assert "ORDER BY over the VARCHAR column 'A.s' is not supported on the MI355X path" in _error(db, "SELECT k, s FROM A UNION SELECT j, r FROM B ORDER BY k, s;")
    assert "ORDER BY over the VARCHAR column 'name' is not supported on the MI355X path" in _error(db, "SELECT s AS name FROM A EXCEPT SELECT r FROM B ORDER BY name;")


def test_what_is_accepted_fails_only_for_lack_of_a_device(db):
    for sql in ["SELECT k FROM A UNION SELECT j FROM B;",
                "SELECT k, s, d, t FROM A UNION ALL SELECT j, r, e, u FROM B ORDER BY k DESC, d LIMIT 1, 2;",
                "SELECT k AS x FROM A INTERSECT DISTINCT SELECT j FROM B EXCEPT SELECT w FROM B ORDER BY x;",
                "SELECT DISTINCT k FROM A EXCEPT SELECT SUM(w) FROM B GROUP BY j;",
                "SELECT k, ROW_NUMBER() OVER (PARTITION BY k ORDER BY v) AS rn FROM A UNION SELECT j, w FROM B ORDER BY rn;",
                "SELECT COUNT(*) FROM A UNION ALL SELECT COUNT(*) FROM B;",
                "SELECT k FROM A WHERE k IN (SELECT j FROM B) UNION SELECT j FROM B INNER JOIN A ON j = k WHERE w > 0 LIMIT 3;",
                " UNION ALL ".join(["SELECT k FROM A"] * 8) + ";"]:
        _reaches_the_device(db, sql)


def test_the_operators_are_exported_and_bound():
    from midoridb_amd.lib import load_library
    from midoridb_amd import dev, query
    lib = load_library()
    assert hasattr(lib, "mdb_dev_rows_semi") and hasattr(lib, "mdb_dev_concat64") and hasattr(lib, "mdb_database_setop_calls")
    assert {"mdb_dev_rows_semi", "mdb_dev_concat64"} <= set(dev.DEV_SYMBOLS) and "mdb_database_setop_calls" in query.QUERY_SYMBOLS
    assert [name for name, _ in dev.RowsInfo._fields_] == ["members", "log2_slots", "form"]
    assert [name for name, _ in dev.ConcatPart._fields_] == ["values", "nullbits", "n"]
    assert (dev.ROWS_MAX_COLS, dev.ROWS_MAX_BUILD) == (16, 1 << 30)
