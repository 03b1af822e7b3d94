"""x [NOT] IN (SELECT ...) without a GPU: what the front end emits for a nested SELECT (the inner statement's tokens in place, ending in its
own `SELECT d n`; `SUBQUERY` wraps it into one stack entry; `ISINSUB` / `ISNOTINSUB` pop the field and the subquery - this project's own
words), that the same words pass the plan builder when they come in through mdb_query_execute_rpn(), every refusal
that is decided before a device is needed, by its message, and that statements without a subquery parse to what they parsed to before."""
import pytest

INNER_B = ["NAME k", "TABLE B", "NAME v", "NUMBER 1", "CMP 2", "WHERE", "SELECT 0 3"]

STATEMENTS = {
    "SELECT k FROM A WHERE k IN (SELECT k FROM B WHERE v > 1);":
        ["NAME k", "TABLE A", "NAME k"] + INNER_B + ["SUBQUERY", "ISINSUB", "WHERE", "SELECT 0 3", "STMT"],
    "SELECT k FROM A WHERE k NOT IN (SELECT k FROM B WHERE v > 1);":
        ["NAME k", "TABLE A", "NAME k"] + INNER_B + ["SUBQUERY", "ISNOTINSUB", "WHERE", "SELECT 0 3", "STMT"],
    "SELECT k FROM A WHERE k NOT IN (SELECT k FROM B WHERE k IN (SELECT DISTINCT C.k FROM C));":
        ["NAME k", "TABLE A", "NAME k", "NAME k", "TABLE B", "NAME k", "FIELDNAME C.k", "TABLE C", "SELECT 2 2", "SUBQUERY", "ISINSUB", "WHERE",
         "SELECT 0 3", "SUBQUERY", "ISNOTINSUB", "WHERE", "SELECT 0 3", "STMT"],
    "DELETE FROM A WHERE k IN (SELECT k FROM B WHERE v > 1);":
        ["NAME k"] + INNER_B + ["SUBQUERY", "ISINSUB", "WHERE", "DELETEONE A", "STMT"],
    "UPDATE A SET v = 7 WHERE k NOT IN (SELECT k FROM B WHERE v > 1) AND v = 2;":
        ["NUMBER 7", "ASSIGN v", "NAME k"] + INNER_B + ["SUBQUERY", "ISNOTINSUB", "NAME v", "NUMBER 2", "CMP 4", "AND", "WHERE", "UPDATE A 1 1",
                                                         "STMT"],
}


def _rpn(sql):
    from oracle.ref import sql_to_rpn		# (the product's own front end, mdb_sql.c, through its C entry point)
    return sql_to_rpn(sql).strip().split("\n")


def _parse_error(sql):
    from oracle.ref import sql_to_rpn
    with pytest.raises(ValueError) as ei:
        sql_to_rpn(sql)
    return str(ei.value)


@pytest.mark.parametrize("sql", list(STATEMENTS))
def test_rpn_token_for_token(sql):
    assert _rpn(sql) == STATEMENTS[sql]


def test_inside_the_parentheses_the_grammar_is_selects_whatever_the_outer_statement_is():
    # a qualified name, COUNT( and arithmetic are refused in delete_expr / update_expr - and accepted in a SELECT nested there
    assert "SUM can't be used in DELETE / UPDATE" in _parse_error("DELETE FROM A WHERE SUM(v) > 1;")
    assert _rpn("DELETE FROM A WHERE k IN (SELECT MAX(B.v) FROM B);") == [
        "NAME k", "FIELDNAME B.v", "AGG MAX", "TABLE B", "SELECT 0 2", "SUBQUERY", "ISINSUB", "WHERE", "DELETEONE A", "STMT"]
    # ... and behind the closing parenthesis the outer statement's rules hold again
    assert "SUM can't be used" in _parse_error("DELETE FROM A WHERE k IN (SELECT k FROM B) AND SUM(v) > 1;")


def test_a_value_list_stays_a_value_list_and_like_stays_like():
    """statements without a subquery: the RPN they had before"""
    assert _rpn("SELECT k FROM A WHERE k IN (1, 2, 3, 4, 5, 6, 7, 8, 9) AND s LIKE 'a%';") == [
        "NAME k", "TABLE A", "NAME k"] + [f"NUMBER {i}" for i in range(1, 10)] + ["ISIN 9", "NAME s", "STRING 'a%'", "LIKE", "AND", "WHERE",
                                                                                   "SELECT 0 3", "STMT"]
    assert _rpn("DELETE FROM A WHERE k NOT IN (1, 2, 3, 4, 5, 6, 7, 8, 9);") == ["NAME k"] + [f"NUMBER {i}" for i in range(1, 10)] + [
        "ISNOTIN 9", "WHERE", "DELETEONE A", "STMT"]
    assert _rpn("UPDATE A SET v = 1 WHERE k IN (1, 2, 3, 4, 5, 6, 7, 8, 9);") == ["NUMBER 1", "ASSIGN v", "NAME k"] + [
        f"NUMBER {i}" for i in range(1, 10)] + ["ISIN 9", "WHERE", "UPDATE A 1 1", "STMT"]
    assert _rpn("SELECT k FROM A WHERE s NOT LIKE '_b' OR k IN ((1), 2);") == [
        "NAME k", "TABLE A", "NAME s", "STRING '_b'", "NOTLIKE", "NAME k", "NUMBER 1", "NUMBER 2", "ISIN 2", "OR", "WHERE", "SELECT 0 3", "STMT"]


def _nested(depth):
    return "SELECT k FROM A WHERE k IN (" * depth + "SELECT k FROM B" + ")" * depth + ";"


def test_nesting_depth():
    assert _rpn(_nested(8)).count("SUBQUERY") == 8
    assert "subqueries nested deeper than 8" in _parse_error(_nested(9))
    assert "subqueries nested deeper than 8" in _parse_error(_nested(20000))        # answered at the ninth, never descended into


def test_missing_closing_parenthesis():
    assert "expecting ')'" in _parse_error("SELECT k FROM A WHERE k IN (SELECT k FROM B;")
    assert "expecting ')'" in _parse_error("DELETE FROM A WHERE k NOT IN (SELECT k FROM B WHERE v > 1;")


@pytest.fixture()
def db():
    from midoridb_amd.query import DB
    with DB() as d:
        d.execute("CREATE TABLE A (k INT, v INT, d DOUBLE, s VARCHAR(8), t DATE);")
        d.execute("CREATE TABLE B (bk INT, bv INT, bd DOUBLE, bs VARCHAR(8), bt DATE);")
        d.execute("CREATE TABLE C (ck INT, cv INT);")
        d.execute("INSERT INTO A VALUES (1, 2, 1.5, 'x', '2020-01-01');")
        d.execute("INSERT INTO B VALUES (1, 2, 1.5, 'x', '2020-01-01');")
        d.execute("INSERT INTO C VALUES (1, 2);")
        yield d


def _error(db, sql, rpn=False):
    from midoridb_amd.query import QueryError
    with pytest.raises(QueryError) as ei:
        if sql.lstrip().upper().startswith("SELECT") or rpn:
            db.query(sql, rpn=rpn)
        else:
            db.execute(sql)
    return str(ei.value)


ONE_COLUMN = "a subquery must select one column"


@pytest.mark.parametrize("sql,msg", [
    ("SELECT k FROM A WHERE k IN (SELECT bk, bv FROM B);", ONE_COLUMN),
    ("SELECT k FROM A WHERE k NOT IN (SELECT * FROM B);", ONE_COLUMN),
    ("DELETE FROM A WHERE k IN (SELECT bk, COUNT(*) FROM B GROUP BY bk);", ONE_COLUMN),
    ("SELECT k FROM A WHERE k IN (SELECT bd FROM B);", "the column 'A.k' is INTEGER, the subquery's column is DOUBLE"),
    ("SELECT k FROM A WHERE s IN (SELECT bk FROM B);", "the column 'A.s' is VARCHAR, the subquery's column is INTEGER"),
    ("SELECT k FROM A WHERE d IN (SELECT COUNT(*) FROM B);", "the column 'A.d' is DOUBLE, the subquery's column is INTEGER"),
    ("SELECT k FROM A WHERE k IN (SELECT AVG(bv) FROM B);", "the column 'A.k' is INTEGER, the subquery's column is DOUBLE"),
    ("UPDATE A SET v = 1 WHERE t IN (SELECT bk FROM B);", "the column 'A.t' is DATE, the subquery's column is INTEGER"),
    ("SELECT k FROM A JOIN B ON k = bk AND k IN (SELECT ck FROM C);", "IN (SELECT ...) in JOIN ... ON is not supported"),
    # a correlated reference: the inner statement sees its own FROM tables only
    ("SELECT k FROM A WHERE k IN (SELECT bk FROM B WHERE bv = v);", "no such column: 'v'"),
    ("SELECT k FROM A WHERE k IN (SELECT bk FROM B WHERE bv = A.v);", "table is not part of from clause: 'A'"),
    ("DELETE FROM A WHERE k IN (SELECT bk FROM B WHERE bv = v);", "no such column: 'v'"),
    ("SELECT k FROM A WHERE k IN (SELECT nosuch FROM B);", "no such column: 'nosuch'"),
    ("SELECT k FROM A WHERE k IN (SELECT x FROM Nowhere);", "table doesn't exist: 'Nowhere'"),
    # the inner statement is checked like any statement, at any depth
    ("SELECT k FROM A WHERE k IN (SELECT bk FROM B WHERE bk IN (SELECT ck, cv FROM C));", ONE_COLUMN),
    ("SELECT k, COUNT(*) FROM A GROUP BY k HAVING k IN (SELECT bd FROM B);", "the subquery's column is DOUBLE"),
])
def test_refusals_by_message(db, sql, msg):
    assert msg in _error(db, sql)


def _reaches_the_device(db, sql, rpn=False):
    import torch
    from midoridb_amd.query import QueryError
    if torch.cuda.is_available():
        try:
            db.query(sql, rpn=rpn)
        except QueryError as e:
            assert "not a SELECT" in str(e)
    else:
        assert "no usable HIP device" in _error(db, sql, rpn)


ACCEPTED = [
    "SELECT k FROM A WHERE k IN (SELECT bk FROM B);",
    "SELECT k FROM A WHERE k NOT IN (SELECT bk FROM B WHERE bv > 1) AND v > 0;",
    "SELECT k, COUNT(*) FROM A GROUP BY k HAVING k IN (SELECT bk FROM B);",
    "DELETE FROM A WHERE k IN (SELECT bk FROM B);",
    "DELETE FROM A WHERE v NOT IN (SELECT v FROM A WHERE k > 3);",
    "UPDATE A SET v = 1 WHERE k NOT IN (SELECT bk FROM B) OR v = 3;",
    "SELECT k FROM A WHERE k IN (SELECT bk FROM B WHERE bv NOT IN (SELECT cv FROM C));",
    "SELECT k FROM A WHERE k IN (SELECT bk FROM B) OR v IN (SELECT ck FROM C);",
    "SELECT k FROM A WHERE k IN (SELECT bk FROM B GROUP BY bk HAVING COUNT(*) > 1);",
    "SELECT k FROM A WHERE k IN (SELECT DISTINCT bk FROM B ORDER BY bk LIMIT 3);",
    "SELECT k FROM A WHERE k IN (SELECT bk FROM B JOIN C ON bk = ck WHERE cv > 0);",
    "SELECT k FROM A WHERE k IN (SELECT COUNT(*) FROM B) AND v NOT IN (SELECT MAX(cv) FROM C);",
    "SELECT k FROM A WHERE s IN (SELECT bs FROM B) AND d IN (SELECT bd FROM B) AND t NOT IN (SELECT bt FROM B);",
    "SELECT k FROM A WHERE d IN (SELECT AVG(bv) FROM B);",
]


@pytest.mark.parametrize("sql", ACCEPTED)
def test_what_is_accepted_fails_only_for_lack_of_a_device(db, sql):
    _reaches_the_device(db, sql)


def _outcome(db, text, rpn):
    """what the statement comes to, through query_execute() (SQL text) or mdb_query_execute_rpn() (the token queue): the error's text,
    or the rows affected / the result's rows"""
    import ctypes
    fn = db.lib.mdb_query_execute_rpn if rpn else db.lib.query_execute
    out = fn(ctypes.byref(db.db), text.encode())
    assert out
    try:
        if out.contents.status == 2:        # ST_ERROR
            return out.contents.error.message.decode(errors="replace").strip()
        if out.contents.status == 1:        # executed: DELETE / UPDATE
            return ("rows affected", out.contents.n_rows_aff)
        return ("rows", int(db.lib.query_row_count(ctypes.byref(out.contents.results))))
    finally:
        db.lib.query_free(out)


REFUSED_BY_THE_RESOLVER = [
    "SELECT k FROM A WHERE k IN (SELECT bk, bv FROM B);",
    "SELECT k FROM A WHERE s IN (SELECT bk FROM B);",
    "SELECT k FROM A JOIN B ON k = bk AND k IN (SELECT ck FROM C);",
    "SELECT k FROM A WHERE k IN (SELECT bk FROM B WHERE bv = v);",
    "DELETE FROM A WHERE k IN (SELECT * FROM B);",
    "DELETE FROM A WHERE d IN (SELECT bk FROM B);",
    "UPDATE A SET v = 1 WHERE t IN (SELECT bk FROM B);",
    "UPDATE A SET v = 1 WHERE k NOT IN (SELECT bk FROM B WHERE bv = v);",
]


@pytest.mark.parametrize("sql", ACCEPTED + REFUSED_BY_THE_RESOLVER)
def test_the_same_words_as_hand_written_rpn_come_to_the_same(db, sql):
    """mdb_query_execute_rpn() takes the vocabulary the parser emits - SELECT, DELETE and UPDATE alike - and builds the plan the SQL
    text builds: the statement comes to the same end either way, error for error (without a device: the refusal, or "no usable HIP
    device" for what is accepted) and row count for row count (with one; each form on a database of its own, a DELETE changes it)"""
    from midoridb_amd.query import DB
    as_text = _outcome(db, sql, rpn=False)
    with DB() as other:
        for ddl in ("CREATE TABLE A (k INT, v INT, d DOUBLE, s VARCHAR(8), t DATE);", "CREATE TABLE B (bk INT, bv INT, bd DOUBLE, bs VARCHAR(8), bt DATE);",
                    "CREATE TABLE C (ck INT, cv INT);", "INSERT INTO A VALUES (1, 2, 1.5, 'x', '2020-01-01');",
                    "INSERT INTO B VALUES (1, 2, 1.5, 'x', '2020-01-01');", "INSERT INTO C VALUES (1, 2);"):
            other.execute(ddl)
        as_rpn = _outcome(other, "\n".join(_rpn(sql)) + "\n", rpn=True)
    assert as_rpn == as_text
    if sql in REFUSED_BY_THE_RESOLVER:
        assert isinstance(as_text, str) and "HIP device" not in as_text, as_text


@pytest.mark.parametrize("rpn", [
    "NAME k\nTABLE A\nNAME k\nSUBQUERY\nISINSUB\nWHERE\nSELECT 0 3\nSTMT\n",                                   # SUBQUERY without a SELECT under it
    "NAME k\nTABLE A\nNAME k\nNAME bk\nTABLE B\nSELECT 0 2\nISINSUB\nWHERE\nSELECT 0 3\nSTMT\n",              # ISINSUB without SUBQUERY
    "NAME k\nTABLE A\nNAME bk\nTABLE B\nSELECT 0 2\nSUBQUERY\nISNOTINSUB\nWHERE\nSELECT 0 3\nSTMT\n",          # no field under the subquery
    "NAME k\nTABLE A\nNAME k\nNAME bk\nTABLE B\nSELECT 0 2\nSUBQUERY\nWHERE\nSELECT 0 3\nSTMT\n",              # a subquery nobody consumes
    "NAME k\nTABLE A\nSELECT 0 2\nNAME bk\nTABLE B\nSELECT 0 2\nSTMT\n",                                        # two statements
    "NAME k\nTABLE A\nNAME k\nNAME bk\nTABLE B\nSELECT 0 2\nSUBQUERY\nISIN 1\nWHERE\nSELECT 0 3\nSTMT\n",      # a subquery as a list value
])
def test_malformed_rpn_is_refused_not_crashed_on(db, rpn):
    msg = _error(db, rpn, rpn=True)
    assert "syntax analysis" in msg or "must" in msg or "IN-clause" in msg, msg
