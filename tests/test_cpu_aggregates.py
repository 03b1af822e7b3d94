"""SUM / MIN / MAX / AVG without a GPU: what the front end emits for them (the RPN words `AGG SUM | MIN | MAX | AVG` behind the argument's
NAME / FIELDNAME - an extension, upstream lexes COUNT( only), and every rejection that is decided before a device is needed, with its
message.  The sharded-mode rejection needs an exchange handle, which needs a device: tests/test_aggregate_gpu.py."""
import pytest

FUNCS = ["SUM", "MIN", "MAX", "AVG"]


def _rpn(sql):
    from oracle.ref import sql_to_rpn		# (the product's own front end, mdb_sql.c, through its C entry point)
    return sql_to_rpn(sql).strip().split("\n")


@pytest.mark.parametrize("fn", FUNCS)
def test_rpn_bare_qualified_and_aliased(fn):
    assert _rpn(f"SELECT {fn}(v) FROM A;") == ["NAME v", f"AGG {fn}", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn(f"SELECT {fn.lower()}(A.v) FROM A;") == ["FIELDNAME A.v", f"AGG {fn}", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn(f"SELECT k, {fn}(v) AS total, COUNT(*) FROM A GROUP BY k;") == [
        "NAME k", "NAME v", f"AGG {fn}", "ALIAS total", "COUNTALL", "TABLE A", "NAME k", "GROUPBYLIST 1", "SELECT 0 5", "STMT"]
    assert _rpn(f"SELECT k, {fn}(v) total FROM A GROUP BY k;")[:4] == ["NAME k", "NAME v", f"AGG {fn}", "ALIAS total"]


@pytest.mark.parametrize("fn", FUNCS)
def test_rpn_inside_having_and_order_by(fn):
    assert _rpn(f"SELECT k, {fn}(v) FROM A GROUP BY k HAVING {fn}(v) > 3 ORDER BY {fn}(A.v) DESC LIMIT 3;") == [
        "NAME k", "NAME v", f"AGG {fn}", "TABLE A", "NAME k", "GROUPBYLIST 1", "NAME v", f"AGG {fn}", "NUMBER 3", "CMP 2", "HAVING",
        "FIELDNAME A.v", f"AGG {fn}", "ORDERBYITEM 1", "ORDERBYLIST 1", "NUMBER 3", "LIMIT 1", "SELECT 0 7", "STMT"]


@pytest.mark.parametrize("name", ["sum", "min", "max", "avg", "SUM"])
def test_a_column_called_like_a_function_stays_a_column(name):
    # a function only with the parenthesis right behind the name, as COUNT
    assert _rpn(f"SELECT {name} FROM A WHERE {name} > 1;") == [f"NAME {name}", "TABLE A", f"NAME {name}", "NUMBER 1", "CMP 2", "WHERE",
                                                              "SELECT 0 3", "STMT"]
    assert _rpn(f"SELECT A.{name}, SUM({name}) FROM A GROUP BY {name};")[:3] == [f"FIELDNAME A.{name}", f"NAME {name}", "AGG SUM"]


@pytest.mark.parametrize("bad,msg", [
    ("SELECT SUM(v + 1) FROM A;", "SUM takes one column"),
    ("SELECT AVG(DISTINCT v) FROM A;", "AVG takes one column"),
    ("SELECT MIN(*) FROM A;", "MIN takes one column"),
    ("SELECT MAX() FROM A;", "MAX takes one column"),
    ("SELECT SUM(3) FROM A;", "SUM takes one column"),
    ("SELECT SUM(A.) FROM A;", "expecting column name"),
    ("DELETE FROM A WHERE SUM(v) > 1;", "SUM can't be used in DELETE / UPDATE"),
    ("UPDATE A SET v = MAX(v);", "MAX can't be used in DELETE / UPDATE"),
    ("UPDATE A SET v = 1 WHERE AVG(v) = 1;", "AVG can't be used in DELETE / UPDATE"),
])
def test_front_end_rejections(bad, msg):
    from oracle.ref import sql_to_rpn
    with pytest.raises(ValueError) as ei:
        sql_to_rpn(bad)
    assert msg in str(ei.value), str(ei.value)


def test_deeply_nested_argument_is_answered_not_recursed_into():
    """the argument of an aggregate is one column: the parser answers SUM(((( ... at the first parenthesis it does not expect, however
    many follow (it never descends into them)"""
    from oracle.ref import sql_to_rpn
    with pytest.raises(ValueError) as ei:
        sql_to_rpn("SELECT SUM(" + "(" * 200000 + "v" + ")" * 200000 + ") FROM A;")
    assert "SUM takes one column" in str(ei.value)


def test_rpn_words_pass_the_plan_builder_and_bad_ones_do_not():
    """through mdb_query_execute_rpn(): `AGG x` needs a column under it and a known function"""
    from midoridb_amd.query import DB, QueryError
    with DB() as db:
        db.execute("CREATE TABLE A (k INT, v INT);")
        for rpn, msg in [("NUMBER 3\nAGG SUM\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),
                         ("NAME v\nAGG MEDIAN\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),
                         ("AGG SUM\nTABLE A\nSELECT 0 2\nSTMT\n", "syntax analysis"),
                         ("NAME nosuch\nAGG SUM\nTABLE A\nSELECT 0 2\nSTMT\n", "no such column")]:
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


@pytest.mark.parametrize("fn", FUNCS)
def test_varchar_argument_is_rejected(db, fn):
    assert f"{fn} over the VARCHAR column 'A.s' is not supported" in _error(db, f"SELECT {fn}(s) FROM A;")
    assert f"{fn} over the VARCHAR column 'A.s' is not supported" in _error(db, f"SELECT k, {fn}(A.s) AS z FROM A GROUP BY k;")


@pytest.mark.parametrize("fn", ["SUM", "AVG"])
def test_sum_and_avg_over_points_in_time_are_rejected(db, fn):
    assert f"{fn} over the DATE column 'A.t' is not supported" in _error(db, f"SELECT {fn}(t) FROM A;")
    assert f"{fn} over the DATETIME column 'A.u' is not supported" in _error(db, f"SELECT k, {fn}(u) FROM A GROUP BY k;")


def _reaches_the_device(db, sql):
    import torch
    if torch.cuda.is_available():
        db.query(sql)
    else:
        assert "no usable HIP device" in _error(db, sql)


def test_what_is_accepted_fails_only_for_lack_of_a_device(db):
    for sql in ["SELECT MIN(t), MAX(u) FROM A;", "SELECT SUM(b), AVG(b), MIN(b), SUM(d), AVG(v) FROM A;",
                "SELECT k, SUM(v) AS z FROM A GROUP BY k HAVING z > 1 ORDER BY z DESC LIMIT 2;",
                "SELECT k, SUM(v), COUNT(*) FROM A GROUP BY k HAVING SUM(A.v) > 1 AND COUNT(*) > 0 ORDER BY SUM(v);",
                "SELECT DISTINCT SUM(v) FROM A GROUP BY k;",
                "SELECT SUM(v), MIN(v), MAX(v), AVG(v), SUM(d), MIN(d), MAX(d), AVG(d) FROM A;"]:
        _reaches_the_device(db, sql)


def test_an_aggregate_named_only_in_having_or_order_by_is_rejected(db):
    assert "SUM(A.v) in the HAVING clause must also stand in the select list" in _error(db, "SELECT k FROM A GROUP BY k HAVING SUM(v) > 1;")
    assert "MAX(A.v) in the HAVING clause must also stand in the select list" in _error(db, "SELECT k, SUM(v) FROM A GROUP BY k HAVING MAX(v) > 1;")
    assert "SUM(A.d) in the HAVING clause must also stand in the select list" in _error(db, "SELECT k, SUM(v) FROM A GROUP BY k HAVING SUM(d) > 1.0;")
    assert "MIN(A.v) in the ORDER BY clause must also stand in the select list" in _error(db, "SELECT k, SUM(v) FROM A GROUP BY k ORDER BY MIN(v);")
    assert "AVG(A.v) in the ORDER BY clause must also stand in the select list" in _error(db, "SELECT k FROM A GROUP BY k ORDER BY AVG(A.v) DESC;")


def test_a_non_group_column_beside_an_aggregate_is_rejected_as_beside_count(db):
    beside_count = _error(db, "SELECT k, COUNT(*) FROM A;")
    assert _error(db, "SELECT k, SUM(v) FROM A;") == beside_count
    assert "requires a GROUP BY clause" in beside_count
    assert _error(db, "SELECT v, SUM(v) FROM A GROUP BY k;") == _error(db, "SELECT v, COUNT(*) FROM A GROUP BY k;")
    assert "SELECT list is not in GROUP BY clause: 'A'.'v'" in _error(db, "SELECT v, SUM(v) FROM A GROUP BY k;")


def test_more_than_eight_aggregates_are_rejected(db):
    assert "more than 8 SUM / MIN / MAX / AVG aggregates" in _error(
        db, "SELECT SUM(v), MIN(v), MAX(v), AVG(v), SUM(d), MIN(d), MAX(d), AVG(d), SUM(b) FROM A;")


def test_aggregates_are_no_predicate_operands_outside_having(db):
    assert "where clause" in _error(db, "SELECT SUM(v) FROM A WHERE SUM(v) > 1;")
    assert "HAVING over an ungrouped aggregate" in _error(db, "SELECT SUM(v) FROM A HAVING SUM(v) > 1;")
    assert "comparison operands must have the same type" in _error(db, "SELECT k, AVG(v) FROM A GROUP BY k HAVING AVG(v) > 1;")
    assert "group-by clauses support only fields and aliases" in _error(db, "SELECT SUM(v) FROM A GROUP BY SUM(v);")


def test_use_in_update_and_delete_is_rejected(db):
    from midoridb_amd.query import QueryError
    for sql in ["DELETE FROM A WHERE SUM(v) > 1;", "UPDATE A SET v = SUM(v);", "UPDATE A SET v = 1 WHERE MIN(k) = 1;"]:
        with pytest.raises(QueryError) as ei:
            db.execute(sql)
        assert "can't be used in DELETE / UPDATE" in str(ei.value)


def test_lds_group_limit_is_exported_and_shrinks_with_the_aggregates():
    from midoridb_amd.lib import load_library
    import ctypes
    lib = load_library()
    lib.mdb_dev_group_aggregate_lds_groups.argtypes = [ctypes.c_int]
    lib.mdb_dev_group_aggregate_lds_groups.restype = ctypes.c_uint64
    got = [lib.mdb_dev_group_aggregate_lds_groups(k) for k in range(0, 10)]
    assert got[0] == 0 and got[9] == 0
    assert all(got[k] >= got[k + 1] > 0 for k in range(1, 8)), got
    budget = 160 * 1024
    for k in range(1, 9):		# key table at load <= 1/2 (8-byte key + 4-byte group number per slot) + 16 bytes per aggregate and group
        g = got[k]
        slots = 16
        while slots < 2 * g:
            slots *= 2
        assert slots * 12 + g * k * 16 <= budget, (k, g)
