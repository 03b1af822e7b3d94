"""COUNT(DISTINCT col) without a GPU: what the front end emits for it (the column's NAME / FIELDNAME, then the RPN word `AGG COUNTD` - an
extension: upstream knows COUNT(*) and COUNT(expr) only, which keep their words) and every rejection that is decided before a device is
needed, with its message.  The sharded-mode rejection needs an exchange handle, which needs a device: tests/test_count_distinct_gpu.py."""
import pytest

ONE_COLUMN = "COUNT(DISTINCT col) takes one column"


def _rpn(sql):
    from oracle.ref import sql_to_rpn		# (the product's own front end, mdb_sql.c, through its C entry point)
    return sql_to_rpn(sql).strip().split("\n")


def test_rpn_of_the_new_form():
    assert _rpn("SELECT COUNT(DISTINCT v) FROM A;") == ["NAME v", "AGG COUNTD", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn("SELECT count( distinct A.v) FROM A;") == ["FIELDNAME A.v", "AGG COUNTD", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn("SELECT k, COUNT(DISTINCT A.v) AS d FROM A GROUP BY k HAVING COUNT(DISTINCT v) > 3 ORDER BY d DESC;") == [
        "NAME k", "FIELDNAME A.v", "AGG COUNTD", "ALIAS d", "TABLE A", "NAME k", "GROUPBYLIST 1", "NAME v", "AGG COUNTD", "NUMBER 3", "CMP 2",
        "HAVING", "NAME d", "ORDERBYITEM 1", "ORDERBYLIST 1", "SELECT 0 6", "STMT"]


def test_count_star_and_count_of_an_expression_emit_what_they_always_did():
    assert _rpn("SELECT COUNT(*) FROM A;") == ["COUNTALL", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn("SELECT COUNT(v) FROM A;") == ["NAME v", "COUNTFIELD", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn("SELECT k, COUNT(A.v + 1) FROM A GROUP BY k;") == ["NAME k", "FIELDNAME A.v", "NUMBER 1", "ADD", "COUNTFIELD", "TABLE A", "NAME k",
                                                                   "GROUPBYLIST 1", "SELECT 0 4", "STMT"]
    # a column called `distinct_v` is no keyword
    assert _rpn("SELECT COUNT(distinct_v) FROM A;") == ["NAME distinct_v", "COUNTFIELD", "TABLE A", "SELECT 0 2", "STMT"]


@pytest.mark.parametrize("bad,msg", [
    ("SELECT COUNT(DISTINCT *) FROM A;", ONE_COLUMN),
    ("SELECT COUNT(DISTINCT) FROM A;", ONE_COLUMN),
    ("SELECT COUNT(DISTINCT v + 1) FROM A;", ONE_COLUMN),
    ("SELECT COUNT(DISTINCT 3) FROM A;", ONE_COLUMN),
    ("SELECT COUNT(DISTINCT a, b) FROM A;", ONE_COLUMN),
    ("SELECT COUNT(DISTINCT (v)) FROM A;", ONE_COLUMN),
    ("SELECT COUNT(DISTINCT A.) FROM A;", "expecting column name"),
    ("SELECT SUM(DISTINCT v) FROM A;", "SUM takes one column"),
    ("SELECT AVG(DISTINCT v) FROM A;", "AVG takes one column"),
    ("DELETE FROM A WHERE COUNT(DISTINCT v) > 1;", "COUNT(DISTINCT) can't be used in DELETE / UPDATE"),
    ("UPDATE A SET v = COUNT(DISTINCT v);", "COUNT(DISTINCT) can't be used in DELETE / UPDATE"),
    ("UPDATE A SET v = 1 WHERE COUNT( distinct v) = 1;", "COUNT(DISTINCT) can't be used in DELETE / UPDATE"),
])
def test_front_end_rejections(bad, msg):
    from oracle.ref import sql_to_rpn
    with pytest.raises(ValueError) as ei:
        sql_to_rpn(bad)
    assert msg in str(ei.value), str(ei.value)


def test_deeply_nested_argument_is_answered_not_recursed_into():
    """the argument is one column: the parser answers COUNT(DISTINCT (((( ... at the first parenthesis, however many follow"""
    from oracle.ref import sql_to_rpn
    for tail in ("v" + ")" * 200000 + ") FROM A;", ""):
        with pytest.raises(ValueError) as ei:
            sql_to_rpn("SELECT COUNT(DISTINCT " + "(" * 200000 + tail)
        assert ONE_COLUMN in str(ei.value)


def test_rpn_word_passes_the_plan_builder_and_needs_its_column():
    from midoridb_amd.query import DB, QueryError
    with DB() as db:
        db.execute("CREATE TABLE A (k INT, v INT);")
        for rpn, msg in [("NUMBER 3\nAGG COUNTD\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),
                         ("AGG COUNTD\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),
                         ("NAME nosuch\nAGG COUNTD\nTABLE A\nSELECT 0 2\nSTMT\n", "no such column")]:
            with pytest.raises(QueryError) as ei:
                db.query(rpn, rpn=True)
            assert msg in str(ei.value), (rpn, str(ei.value))


@pytest.fixture()
def db():
    from midoridb_amd.query import DB
    with DB() as d:
        d.execute("CREATE TABLE A (k INT, v INT, d DOUBLE, s VARCHAR(8), t DATE, u DATETIME, b TINYINT);")
        d.execute("INSERT INTO A VALUES (1, 2, 1.5, 'x', '2020-01-01', '2020-01-01 10:00:00', TRUE);")
        yield d


def _error(db, sql):
    from midoridb_amd.query import QueryError
    with pytest.raises(QueryError) as ei:
        db.query(sql)
    return str(ei.value)


def test_every_column_type_is_accepted_and_fails_only_for_lack_of_a_device(db):
    from midoridb_amd.query import QueryError
    for sql in ["SELECT COUNT(DISTINCT s) FROM A;", "SELECT k, COUNT(DISTINCT A.s) AS z FROM A GROUP BY k;",
                "SELECT COUNT(DISTINCT v), COUNT(DISTINCT d), COUNT(DISTINCT t), COUNT(DISTINCT u), COUNT(DISTINCT b) FROM A;",
                "SELECT k, COUNT(DISTINCT v) AS z, COUNT(*), SUM(v) FROM A GROUP BY k HAVING z > 0 AND COUNT(DISTINCT v) < 9 ORDER BY z DESC LIMIT 2;",
                "SELECT DISTINCT COUNT(DISTINCT v) FROM A GROUP BY k;"]:
        try:                    # (where there is a device the statement runs: tests/test_count_distinct_gpu.py checks what it returns)
            db.query(sql)
        except QueryError as ex:
            assert "no usable HIP device" in str(ex), (sql, str(ex))


def test_named_only_in_having_or_order_by_is_rejected(db):
    assert "COUNT(DISTINCT A.v) in the HAVING clause must also stand in the select list" in _error(
        db, "SELECT k FROM A GROUP BY k HAVING COUNT(DISTINCT v) > 1;")
    assert "COUNT(DISTINCT A.d) in the HAVING clause must also stand in the select list" in _error(
        db, "SELECT k, COUNT(DISTINCT v) FROM A GROUP BY k HAVING COUNT(DISTINCT d) > 1;")
    assert "COUNT(DISTINCT A.v) in the ORDER BY clause must also stand in the select list" in _error(
        db, "SELECT k, SUM(v) FROM A GROUP BY k ORDER BY COUNT(DISTINCT v);")


def test_a_non_group_column_beside_it_is_rejected_as_beside_count(db):
    beside_count = _error(db, "SELECT k, COUNT(*) FROM A;")
    assert _error(db, "SELECT k, COUNT(DISTINCT v) FROM A;") == beside_count
    assert "requires a GROUP BY clause" in beside_count
    assert _error(db, "SELECT v, COUNT(DISTINCT v) FROM A GROUP BY k;") == _error(db, "SELECT v, COUNT(*) FROM A GROUP BY k;")


def test_it_counts_towards_the_eight_aggregates_of_a_select_list(db):
    assert "more than 8 SUM / MIN / MAX / AVG aggregates" in _error(
        db, "SELECT SUM(v), MIN(v), MAX(v), AVG(v), SUM(d), MIN(d), MAX(d), AVG(d), COUNT(DISTINCT v) FROM A;")
    assert "more than 8 SUM / MIN / MAX / AVG aggregates" in _error(
        db, "SELECT COUNT(DISTINCT k), COUNT(DISTINCT v), COUNT(DISTINCT d), COUNT(DISTINCT s), COUNT(DISTINCT t), COUNT(DISTINCT u), "
            "COUNT(DISTINCT b), SUM(v), MIN(v) FROM A;")


def test_it_is_no_predicate_operand_outside_having(db):
    assert "where clause" in _error(db, "SELECT COUNT(DISTINCT v) FROM A WHERE COUNT(DISTINCT v) > 1;")
    assert "no usable HIP device" not in _error(db, "SELECT A.k FROM A INNER JOIN A AS B ON COUNT(DISTINCT A.v) = B.k;")
    assert "HAVING over an ungrouped aggregate" in _error(db, "SELECT COUNT(DISTINCT v) FROM A HAVING COUNT(DISTINCT v) > 1;")
    assert "group-by clauses support only fields and aliases" in _error(db, "SELECT COUNT(DISTINCT v) FROM A GROUP BY COUNT(DISTINCT v);")
    # the result is INTEGER: a DOUBLE literal does not compare with it
    assert "comparison operands must have the same type" in _error(db, "SELECT k, COUNT(DISTINCT d) FROM A GROUP BY k HAVING COUNT(DISTINCT d) > 1.5;")


def test_use_in_update_and_delete_is_rejected(db):
    from midoridb_amd.query import QueryError
    for sql in ["DELETE FROM A WHERE COUNT(DISTINCT v) > 1;", "UPDATE A SET v = COUNT(DISTINCT v);", "UPDATE A SET v = 1 WHERE COUNT(DISTINCT k) = 1;"]:
        with pytest.raises(QueryError) as ei:
            db.execute(sql)
        assert "COUNT(DISTINCT) can't be used in DELETE / UPDATE" in str(ei.value)


def test_the_operators_limits_are_exported():
    from midoridb_amd.dev import _bind
    from midoridb_amd.lib import load_library
    lib = load_library()
    _bind(lib)
    assert lib.mdb_dev_count_distinct_bitmap_bits() == 1 << 30		# what DESIGN.md 2.3 states
    assert lib.mdb_dev_group_count_distinct_lds_groups() == 4096	# 8192 slots of 12 bytes at load <= 1/2: the largest table in 159 KiB of LDS
