"""FULL [OUTER] JOIN without a GPU: the front end knows the word (FULL JOIN is join number 6, FULL OUTER JOIN 12: LEFT 2 + RIGHT 4,
+ 6 with OUTER) instead of reading it as an alias of the left table, the resolver lets both numbers through - with no HIP device the
statement fails like every SELECT ("no usable HIP device") -, and a join number nobody emits is still refused."""
import pytest

SPELLINGS = [("FULL JOIN", 6), ("FULL OUTER JOIN", 12)]


def _tables(db):
    db.execute("CREATE TABLE A (id_a INT);")
    db.execute("CREATE TABLE B (id_b INT);")
    db.execute("INSERT INTO A VALUES (1), (3), (4), (9);")
    db.execute("INSERT INTO B VALUES (3), (4), (5), (6);")


def _no_device():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.parametrize("spelling,code", SPELLINGS)
def test_both_spellings_parse_to_their_join_numbers(spelling, code):
    from oracle.ref import sql_to_rpn	# (the product's own front end, mdb_sql.c, through its C entry point)
    lines = sql_to_rpn(f"SELECT * FROM A {spelling} B ON A.id_a = B.id_b;").strip().split("\n")
    assert f"JOIN {code}" in lines, lines
    assert "ALIAS FULL" not in lines and "JOIN 1" not in lines, lines	# (what the word used to be: an alias of A, on an inner join)


def test_full_joins_in_a_chain_keep_their_numbers():
    from oracle.ref import sql_to_rpn
    lines = sql_to_rpn("SELECT * FROM A FULL JOIN B ON A.id_a = B.id_b LEFT JOIN C ON id_b = id_c FULL OUTER JOIN D ON id_c = id_d;").strip().split("\n")
    assert [ln for ln in lines if ln.startswith("JOIN ")] == ["JOIN 6", "JOIN 2", "JOIN 12"], lines


@pytest.mark.parametrize("spelling,code", SPELLINGS)
def test_full_join_reaches_execution_and_fails_only_for_lack_of_a_device(spelling, code):
    from midoridb_amd.query import DB, QueryError
    with DB() as db:
        _tables(db)
        if _no_device():		# (with a device: tests/test_full_join_gpu.py)
            with pytest.raises(QueryError) as ei:
                db.query(f"SELECT * FROM A {spelling} B ON A.id_a = B.id_b;")
            assert "no usable HIP device" in str(ei.value), str(ei.value)
            assert "is not executed" not in str(ei.value)
        # the statement is still checked like an inner join's before it runs
        with pytest.raises(QueryError) as ei:
            db.query(f"SELECT * FROM A {spelling} NOSUCH ON A.id_a = NOSUCH.id_b;")
        assert "table doesn't exist" in str(ei.value)


def _rpn_join(number):
    from oracle.ref import sql_to_rpn
    rpn = sql_to_rpn("SELECT * FROM A LEFT JOIN B ON A.id_a = B.id_b;")
    assert rpn.count("JOIN 2") == 1
    return rpn.replace("JOIN 2", f"JOIN {number}")


@pytest.mark.parametrize("number", [6, 12])
def test_the_rpn_entry_accepts_the_full_join_numbers(number):
    """mdb_query_execute_rpn(): the parser's queue from anyone.  Accepted = past the resolver: with a device it runs (two rows match,
    two of either side do not), without one it fails for lack of it"""
    from midoridb_amd.query import DB, QueryError
    with DB() as db:
        _tables(db)
        if _no_device():
            with pytest.raises(QueryError) as ei:
                db.query(_rpn_join(number), rpn=True)
            assert "no usable HIP device" in str(ei.value) and "is not executed" not in str(ei.value), str(ei.value)
        else:
            assert db.query(_rpn_join(number), rpn=True).nrows == 6


@pytest.mark.parametrize("number", [7, 3, 14])
def test_an_unknown_join_number_is_still_refused_and_the_refusal_names_full(number):
    from midoridb_amd.query import DB, QueryError
    with DB() as db:
        _tables(db)
        with pytest.raises(QueryError) as ei:
            db.query(_rpn_join(number), rpn=True)
        assert f"join type {number} is not executed" in str(ei.value) and "FULL [OUTER]" in str(ei.value), str(ei.value)
