"""Navigation window functions without a GPU: LAG, LEAD, FIRST_VALUE, LAST_VALUE and NTILE ... OVER.  What the front end emits (the
literal arguments as the literals' own tokens, closed by `WINARG n`), that no word became reserved, every refusal that is decided before
a device is needed, by its message, the struct's mirror in dev.py - and the numpy model (tests/window_nav_model.py) against SQLite."""
import ctypes
import sqlite3

import numpy as np
import pytest

from tests import window_nav_model as N

NAV = ["LAG", "LEAD", "FIRST_VALUE", "LAST_VALUE"]


def _rpn(sql):
    from oracle.ref import sql_to_rpn		# (the product's own front end, mdb_sql.c, through its C entry point)
    return sql_to_rpn(sql).strip().split("\n")


def _syntax_error(sql):
    from oracle.ref import sql_to_rpn
    with pytest.raises(ValueError) as ei:
        sql_to_rpn(sql)
    return str(ei.value)


# ------------------------------------------------------------------ grammar

@pytest.mark.parametrize("fn", ["LAG", "LEAD"])
def test_rpn_of_lag_and_lead(fn):
    assert _rpn(f"SELECT {fn}(v) OVER () FROM A;") == ["NAME v", "WINARG 0", f"WINDOW {fn} 0 0", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn(f"SELECT k, {fn.lower()}(A.v, 2) over (partition by k order by o desc) AS prev FROM A;") == [
        "NAME k", "FIELDNAME A.v", "NUMBER 2", "WINARG 1", "NAME k", "NAME o", "WINORDER 1", f"WINDOW {fn} 1 1", "ALIAS prev", "TABLE A",
        "SELECT 0 3", "STMT"]
    assert _rpn(f"SELECT {fn}(v, 0, -7) OVER (ORDER BY o) FROM A;")[:6] == ["NAME v", "NUMBER 0", "NUMBER -7", "WINARG 2", "NAME o", "WINORDER 0"]
    assert _rpn(f"SELECT {fn}(d, 1, 1.5) OVER () FROM A;")[:4] == ["NAME d", "NUMBER 1", "FLOAT 1.5", "WINARG 2"]
    assert _rpn(f"SELECT {fn}(b, 1, TRUE) OVER () FROM A;")[:4] == ["NAME b", "NUMBER 1", "BOOL 1", "WINARG 2"]
    assert _rpn(f"SELECT {fn}(A.v, 2147483647, -2147483648) OVER () FROM A;")[:4] == ["FIELDNAME A.v", "NUMBER 2147483647", "NUMBER -2147483648", "WINARG 2"]
    assert _rpn(f"SELECT {fn}(v, 3, NULL) OVER () x FROM A;")[:6] == ["NAME v", "NUMBER 3", "NULL", "WINARG 2", f"WINDOW {fn} 0 0", "ALIAS x"]


def test_rpn_of_first_value_last_value_and_ntile():
    for fn in ("FIRST_VALUE", "LAST_VALUE"):
        assert _rpn(f"SELECT {fn}(v) OVER (PARTITION BY A.k ORDER BY o) f FROM A;") == [
            "NAME v", "FIELDNAME A.k", "NAME o", "WINORDER 0", f"WINDOW {fn} 1 1", "ALIAS f", "TABLE A", "SELECT 0 2", "STMT"]
    assert _rpn("SELECT NTILE(4) OVER (ORDER BY o) FROM A;") == ["NUMBER 4", "WINARG 1", "NAME o", "WINORDER 0", "WINDOW NTILE 0 1", "TABLE A",
                                                                "SELECT 0 2", "STMT"]
    # old and new functions side by side; HAVING by alias
    assert _rpn("SELECT ROW_NUMBER() OVER (ORDER BY o) rn, LAG(v) OVER (ORDER BY o) AS prev FROM A HAVING prev IS NULL;") == [
        "NAME o", "WINORDER 0", "WINDOW ROW_NUMBER 0 1", "ALIAS rn", "NAME v", "WINARG 0", "NAME o", "WINORDER 0", "WINDOW LAG 0 1", "ALIAS prev",
        "TABLE A", "NAME prev", "ISNULL", "HAVING", "SELECT 0 4", "STMT"]


def test_no_word_became_reserved():
    assert _rpn("SELECT lag, lead, ntile FROM first_value;") == ["NAME lag", "NAME lead", "NAME ntile", "TABLE first_value", "SELECT 0 4", "STMT"]
    assert _rpn("SELECT last_value, winarg FROM T WHERE lag > 1 ORDER BY ntile;")[:2] == ["NAME last_value", "NAME winarg"]
    assert _rpn("CREATE TABLE lag(lead INT, ntile INT, first_value INT, last_value INT);")[-2] == "CREATE 0 4 lag"
    assert _rpn("INSERT INTO lag(lead) VALUES (1);") == ["COLUMN lead", "INSERTCOLS 1", "NUMBER 1", "VALUES 1", "INSERTVALS 1 1 lag", "STMT"]
    assert _rpn("SELECT SUM(v) ignore, k AS respect, v nulls, k last FROM A;")[2] == "ALIAS ignore"
    assert _rpn("SELECT LAG(lag) OVER (PARTITION BY lead ORDER BY ntile) FROM A;")[:6] == [
        "NAME lag", "WINARG 0", "NAME lead", "NAME ntile", "WINORDER 0", "WINDOW LAG 1 1"]


@pytest.mark.parametrize("bad,msg", [
    ("SELECT LAG(v) IGNORE NULLS OVER (ORDER BY o) FROM A;", "IGNORE NULLS / RESPECT NULLS behind LAG is not supported"),
    ("SELECT LAST_VALUE(v) RESPECT NULLS OVER () FROM A;", "IGNORE NULLS / RESPECT NULLS behind LAST_VALUE is not supported"),
    ("SELECT FIRST_VALUE(v) FROM LAST OVER () FROM A;", "FROM FIRST / FROM LAST behind FIRST_VALUE is not supported"),
    ("SELECT LAG(v, o) OVER () FROM A;", "the offset of LAG must be a non-negative integer literal"),
    ("SELECT LEAD(v, 1 + 1) OVER () FROM A;", "the offset of LEAD must be a non-negative integer literal"),
    ("SELECT LAG(v, 1.5) OVER () FROM A;", "the offset of LAG must be a non-negative integer literal"),
    ("SELECT LAG(v, 1, o) OVER () FROM A;", "the default of LAG must be a literal or NULL"),
    ("SELECT LEAD(v, 1, 2 * 3) OVER () FROM A;", "the default of LEAD must be a literal or NULL"),
    ("SELECT LAG(v, -1) OVER () FROM A;", "a negative offset in LAG is not supported"),
    ("SELECT LEAD(v, -2, 0) OVER () FROM A;", "a negative offset in LEAD is not supported"),
    ("SELECT LAG(v, 2147483648) OVER () FROM A;", "the offset 2147483648 of LAG is not supported in a statement: integer literals are 32-bit"),
    ("SELECT LEAD(v, 4294967296) OVER () FROM A;", "the offset 4294967296 of LEAD is not supported in a statement"),
    ("SELECT LAG(v, 1, 5000000000) OVER () FROM A;", "the default 5000000000 of LAG is not supported: integer literals are 32-bit"),
    ("SELECT LAG(v, 1, -2147483649) OVER () FROM A;", "the default -2147483649 of LAG is not supported"),
    ("SELECT NTILE(4294967297) OVER () FROM A;", "NTILE(4294967297): more than 2147483647 buckets"),
    ("SELECT NTILE(0) OVER () FROM A;", "NTILE(0): the number of buckets must be at least 1"),
    ("SELECT NTILE(-3) OVER () FROM A;", "the number of buckets must be at least 1"),
    ("SELECT NTILE(k) OVER () FROM A;", "NTILE takes the number of buckets as a positive integer literal, not a column"),
    ("SELECT NTILE() OVER () FROM A;", "NTILE takes the number of buckets as a positive integer literal"),
    ("SELECT LAG() OVER () FROM A;", "LAG() needs a column"),
    ("SELECT FIRST_VALUE() OVER () FROM A;", "FIRST_VALUE() needs a column"),
    ("SELECT LAG(1) OVER () FROM A;", "LAG takes a column as its first argument"),
    ("SELECT FIRST_VALUE(v, 2) OVER () FROM A;", "FIRST_VALUE takes one column"),
    ("SELECT LAG(DISTINCT v) OVER () FROM A;", "DISTINCT inside a window function is not supported"),
    ("SELECT NTILE(DISTINCT 2) OVER () FROM A;", "DISTINCT inside a window function is not supported"),
    ("SELECT LAG(v) FROM A;", "LAG(...) needs its window"),
    ("SELECT LEAD(v) OVER w FROM A;", "named windows"),
    ("SELECT LAG(v) OVER (ORDER BY o ROWS 1 PRECEDING) FROM A;", "window frame clauses"),
    ("SELECT k FROM A WHERE LAG(v) OVER (ORDER BY o) < 3;", "allowed in the select list only"),
    ("SELECT k FROM A HAVING LEAD(v) OVER () = 1;", "allowed in the select list only"),
    ("SELECT k FROM A ORDER BY NTILE(2) OVER (ORDER BY k);", "allowed in the select list only"),
    ("SELECT k FROM A GROUP BY FIRST_VALUE(v) OVER ();", "allowed in the select list only"),
    ("DELETE FROM A WHERE LAG(v) OVER () > 1;", "window function LAG ... OVER can't be used in DELETE / UPDATE"),
    ("UPDATE A SET v = NTILE(2) OVER ();", "window function NTILE ... OVER can't be used in DELETE / UPDATE"),
])
def test_front_end_refusals(bad, msg):
    assert msg in _syntax_error(bad)


def test_rpn_words_pass_the_plan_builder_and_bad_ones_do_not():
    from midoridb_amd.query import DB, QueryError
    T = "TABLE A\nSELECT 0 2\nSTMT\n"
    with DB() as db:
        db.execute("CREATE TABLE A (k INT, v INT);")
        for rpn, msg in [("NAME v\nWINDOW LAG 0 0\n" + T, "syntax analysis"),                          # LAG without its WINARG
                         ("NAME v\nNUMBER 1\nNUMBER 2\nNUMBER 3\nWINARG 3\nWINDOW LAG 0 0\n" + T, "syntax analysis"),
                         ("NAME v\nNUMBER -1\nWINARG 1\nWINDOW LAG 0 0\n" + T, "syntax analysis"),
                         ("NAME v\nFLOAT 1.5\nWINARG 1\nWINDOW LEAD 0 0\n" + T, "syntax analysis"),
                         ("NAME v\nNAME k\nWINARG 1\nWINDOW LEAD 0 0\n" + T, "syntax analysis"),
                         ("NUMBER 1\nWINARG 1\nWINDOW LAG 0 0\n" + T, "syntax analysis"),               # no column
                         ("NUMBER 0\nWINARG 1\nWINDOW NTILE 0 0\n" + T, "syntax analysis"),
                         ("WINARG 0\nWINDOW NTILE 0 0\n" + T, "syntax analysis"),
                         ("NUMBER 1\nNUMBER 2\nWINARG 2\nWINDOW NTILE 0 0\n" + T, "syntax analysis"),
                         ("NAME v\nWINARG 0\nWINDOW FIRST_VALUE 0 0\n" + T, "syntax analysis"),
                         ("WINDOW LAST_VALUE 0 0\n" + T, "syntax analysis"),
                         ("NAME v\nWINARG 0\nWINDOW NTH_VALUE 0 0\n" + T, "syntax analysis"),
                         ("NAME nosuch\nWINARG 0\nWINDOW LAG 0 0\n" + T, "no such column")]:
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
        yield d


def _error(db, sql):
    from midoridb_amd.query import QueryError
    with pytest.raises(QueryError) as ei:
        db.query(sql)
    return str(ei.value)


def _reaches_the_device(db, sql):
    import torch
    if torch.cuda.is_available():
        return db.query(sql)
    assert "no usable HIP device" in _error(db, sql), sql
    return None


@pytest.mark.parametrize("fn", ["LAG", "LEAD"])
def test_default_types(db, fn):
    assert f"{fn} ... OVER: the default does not match the type of column 'A.v': it takes an integer" in _error(db, f"SELECT {fn}(v, 1, 1.5) OVER () FROM A;")
    assert "the default does not match the type of column 'A.v'" in _error(db, f"SELECT {fn}(v, 1, TRUE) OVER () FROM A;")
    assert "the default does not match the type of column 'A.v'" in _error(db, f"SELECT {fn}(v, 1, 'x') OVER () FROM A;")
    assert "the default does not match the type of column 'A.d': it takes a number with a decimal point" in _error(db, f"SELECT {fn}(d, 1, 1) OVER () FROM A;")
    assert "the default does not match the type of column 'A.b': it takes TRUE or FALSE" in _error(db, f"SELECT {fn}(b, 1, 1) OVER () FROM A;")
    assert f"{fn} ... OVER: UNKNOWN as a default is not supported: write NULL" in _error(db, f"SELECT {fn}(b, 1, UNKNOWN) OVER () FROM A;")
    for col, ty, lit in [("s", "VARCHAR", "'x'"), ("t", "DATE", "'2020-01-01'"), ("u", "DATETIME", "1"), ("s", "VARCHAR", "7")]:
        assert f"{fn} ... OVER: a default for the {ty} column 'A.{col}' is not supported" in _error(db, f"SELECT {fn}({col}, 1, {lit}) OVER () FROM A;")
    for sql in [f"SELECT {fn}(v, 1, -3) OVER (ORDER BY o), {fn}(d, 2, 0.5) OVER (ORDER BY o), {fn}(b, 1, FALSE) OVER (ORDER BY o) FROM A;",
                f"SELECT {fn}(s, 1, NULL) OVER (ORDER BY o), {fn}(t, 1, NULL) OVER (ORDER BY o), {fn}(u) OVER (ORDER BY o) FROM A;"]:
        _reaches_the_device(db, sql)


def test_statement_shape(db):
    mixed = ", ".join([f"ROW_NUMBER() OVER (ORDER BY o) AS r{i}" for i in range(4)] + [f"LAG(v, {i + 2}) OVER (ORDER BY o) AS l{i}" for i in range(4)] +
                      ["NTILE(2) OVER (ORDER BY o) AS nt"])
    assert "more than 8 window functions in one select list" in _error(db, f"SELECT {mixed} FROM A;")
    assert "duplicate column name: 'LAG(A.v) OVER'" in _error(db, "SELECT LAG(v) OVER (ORDER BY k), LAG(A.v, 1, 0) OVER (ORDER BY o) FROM A;")
    assert "duplicate column name: 'LEAD(A.v, 2) OVER'" in _error(db, "SELECT LEAD(v, 2) OVER (ORDER BY k), LEAD(v, 2) OVER (ORDER BY o) FROM A;")
    assert "duplicate column name: 'NTILE(3) OVER'" in _error(db, "SELECT NTILE(3) OVER (ORDER BY k), NTILE(3) OVER (ORDER BY o) FROM A;")
    assert "a window function beside GROUP BY is not supported" in _error(db, "SELECT k, LAG(k) OVER (ORDER BY k) FROM A GROUP BY k;")
    assert "a window function inside an expression is not supported" in _error(db, "SELECT v - LAG(v) OVER (ORDER BY o) FROM A;")
    assert "no such column: 'nosuch'" in _error(db, "SELECT LAG(nosuch) OVER () FROM A;")
    assert "no such column: 'prev'" in _error(db, "SELECT LAG(v) OVER (ORDER BY o) AS prev FROM A WHERE prev < v;")
    # the result has the argument's type: a DOUBLE column against an INT literal is a type error, against a FLOAT one it is not
    assert "comparison operands must have the same type" in _error(db, "SELECT LAG(d) OVER (ORDER BY o) AS p FROM A HAVING p > 1;")
    assert "comparison operands must have the same type" in _error(db, "SELECT FIRST_VALUE(s) OVER (ORDER BY o) AS p FROM A HAVING p > 1;")
    assert "comparison operands must have the same type" in _error(db, "SELECT NTILE(2) OVER (ORDER BY o) AS p FROM A HAVING p > 1.5;")
    # a VARCHAR result holds dictionary ids, which are not in string order: no ORDER BY over it, as over the column itself
    for fn in NAV:
        assert "ORDER BY over the VARCHAR column 'ps' is not supported" in _error(db, f"SELECT {fn}(s) OVER (ORDER BY o) AS ps FROM A ORDER BY ps;")
        assert "ORDER BY over the VARCHAR column 'ps' is not supported" in _error(db, f"SELECT k, {fn}(A.s) OVER () ps FROM A ORDER BY k, ps DESC LIMIT 3;")
    assert "ORDER BY over the VARCHAR column 'A.s' is not supported" in _error(db, "SELECT s FROM A ORDER BY s;")
    # IS NULL takes a window item's alias in HAVING, and nowhere else
    assert "no such column: 'prev'" in _error(db, "SELECT LAG(v) OVER (ORDER BY o) AS prev FROM A WHERE prev IS NULL;")
    for sql in ["SELECT LAG(d) OVER (ORDER BY o) AS p FROM A HAVING p > 1.0;",
                "SELECT v, LAG(v) OVER (PARTITION BY k ORDER BY o) AS prev FROM A HAVING prev < v;",
                "SELECT LAG(v) OVER (ORDER BY o) AS prev FROM A HAVING prev IS NULL;",
                "SELECT LAG(t) OVER (ORDER BY o) AS pt, LEAD(d) OVER (ORDER BY o) AS nd FROM A ORDER BY pt DESC, nd;",
                "SELECT LAG(b) OVER (ORDER BY o) AS pb FROM A HAVING pb < TRUE;",
                "SELECT ROW_NUMBER() OVER (ORDER BY o) AS rn FROM A HAVING rn IS NOT NULL;",
                "SELECT DISTINCT NTILE(2) OVER (ORDER BY o) AS nt, LAST_VALUE(t) OVER (ORDER BY o) FROM A ORDER BY nt DESC LIMIT 2;",
                "SELECT LAG(v, 0) OVER (), LAG(v, 2) OVER (), LEAD(A.v, 3, 0) OVER (), FIRST_VALUE(s) OVER (), LAST_VALUE(u) OVER (), NTILE(1) OVER (), "
                "ROW_NUMBER() OVER (), SUM(v) OVER () FROM A;"]:
        _reaches_the_device(db, sql)


def test_the_struct_and_the_constants_are_mirrored(tmp_path):
    import os
    import shutil
    import subprocess
    from midoridb_amd.lib import load_library
    from midoridb_amd import dev
    lib = load_library()
    assert hasattr(lib, "mdb_dev_window") and hasattr(lib, "mdb_dev_window_fn_size")
    assert "mdb_dev_window_fn_size" in dev.DEV_SYMBOLS
    assert (dev.WIN_LAG, dev.WIN_LEAD, dev.WIN_FIRST_VALUE, dev.WIN_LAST_VALUE, dev.WIN_NTILE) == \
        (N.LAG, N.LEAD, N.FIRST_VALUE, N.LAST_VALUE, N.NTILE) == tuple(range(16, 21))
    assert [name for name, _ in dev.WindowFnFull._fields_] == ["arg", "dflt", "dflt_null"] and issubclass(dev.WindowFnFull, dev.WindowFn)
    lib.mdb_dev_window_fn_size.restype = ctypes.c_uint64
    assert ctypes.sizeof(dev.WindowFnFull) == lib.mdb_dev_window_fn_size() == 72
    assert dev.WindowFnFull.arg.offset == ctypes.sizeof(dev.WindowFn) == 48
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:      # ... and what a C compiler makes of the header
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        src = tmp_path / "size.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mdb_dev.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", '
                       'sizeof(struct mdb_window_fn), offsetof(struct mdb_window_fn, arg), offsetof(struct mdb_window_fn, dflt), '
                       'offsetof(struct mdb_window_fn, dflt_null), (int)MDB_WIN_NTILE); return 0; }\n')
        subprocess.run([cc, "-I", os.path.join(root, "include"), "-o", str(tmp_path / "size"), str(src)], check=True)
        got = subprocess.run([str(tmp_path / "size")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
        assert [int(x) for x in got] == [ctypes.sizeof(dev.WindowFnFull), dev.WindowFnFull.arg.offset, dev.WindowFnFull.dflt.offset,
                                         dev.WindowFnFull.dflt_null.offset, dev.WIN_NTILE]


# ------------------------------------------------------------------ the model against SQLite

def _sqlite_world():
    rng = np.random.default_rng(21)
    n = 311
    k = rng.integers(0, 7, n).astype(np.int64)
    kn = rng.random(n) < 0.08
    o = rng.integers(0, 12, n).astype(np.int64)                 # ties
    on = rng.random(n) < 0.1
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    vn = (rng.random(n) < 0.15) | (k == 3)
    x = (rng.integers(-40, 40, n) / 8.0).astype(np.float64)
    xn = rng.random(n) < 0.15
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE A (k INTEGER, o INTEGER, v INTEGER, x REAL)")
    con.executemany("INSERT INTO A VALUES (?, ?, ?, ?)",
                    [(None if kn[i] else int(k[i]), None if on[i] else int(o[i]), None if vn[i] else int(v[i]), None if xn[i] else float(x[i]))
                     for i in range(n)])
    return con, n, dict(k=(k, kn), o=(o, on), v=(v, vn), x=(x, xn))


WINDOWS = [("", [], []),
           ("PARTITION BY k", ["k"], []),
           ("ORDER BY o", [], [("o", False)]),
           ("PARTITION BY k ORDER BY o", ["k"], [("o", False)]),
           ("PARTITION BY k ORDER BY o DESC", ["k"], [("o", True)])]


@pytest.mark.parametrize("over,part,order", WINDOWS)
def test_model_against_sqlite(over, part, order):
    assert sqlite3.sqlite_version_info >= (3, 25), "SQLite without window functions"
    con, n, cols = _sqlite_world()
    pk = [(cols[c][0], cols[c][1], False) for c in part]
    ok = [(cols[c][0], cols[c][1], desc) for c, desc in order]
    fns = [(N.LAG,) + cols["v"] + (1, None), (N.LAG,) + cols["v"] + (3, -5), (N.LAG,) + cols["x"] + (0, None), (N.LEAD,) + cols["v"] + (1, None),
           (N.LEAD,) + cols["x"] + (2, 0.25), (N.LEAD,) + cols["v"] + (400, 9), (N.FIRST_VALUE,) + cols["v"], (N.FIRST_VALUE,) + cols["x"],
           (N.LAST_VALUE,) + cols["v"], (N.NTILE, 1), (N.NTILE, 3), (N.NTILE, 7), (N.NTILE, 500)]
    got = N.nav_model(pk, ok, n, fns)
    # ties keep the stream order: rowid as SQLite's last order key.  LAST_VALUE looks at the row's last PEER: it keeps the window as written
    # (no order keys: the whole partition in SQLite too), but ties among the peers are then broken by ... nothing SQLite promises - so its
    # frame is spelled out over the stable order: up to the last row whose order keys equal the row's
    st = over + (", rowid" if order else " ORDER BY rowid")
    last = (f"LAST_VALUE(v) OVER ({over} ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING)" if not order else None)
    sql = (f"SELECT LAG(v) OVER ({st}), LAG(v, 3, -5) OVER ({st}), LAG(x, 0) OVER ({st}), LEAD(v) OVER ({st}), LEAD(x, 2, 0.25) OVER ({st}), "
           f"LEAD(v, 400, 9) OVER ({st}), FIRST_VALUE(v) OVER ({st}), FIRST_VALUE(x) OVER ({st}), "
           f"{last or 'NULL'}, NTILE(1) OVER ({st}), NTILE(3) OVER ({st}), NTILE(7) OVER ({st}), NTILE(500) OVER ({st}) FROM A ORDER BY rowid")
    want = [list(r) for r in con.execute(sql).fetchall()]
    assert len(want) == n
    if order:   # LAST_VALUE under the default frame with ties: the last row, in stable order, among the rows that share the order keys
        okeys = ", ".join(c for c, _ in order)
        pkeys = "".join(f" AND B.{c} IS A.{c}" for c in part)
        sub = (f"SELECT (SELECT B.v FROM A AS B WHERE B.{okeys} IS A.{okeys}{pkeys} ORDER BY B.rowid DESC LIMIT 1) FROM A ORDER BY rowid")
        for i, r in enumerate(con.execute(sub).fetchall()):
            want[i][8] = r[0]
    assert _rpn(sql.replace(", rowid", "").replace(" ORDER BY rowid", "").replace(f"{last or 'NULL'}, ", "") + ";")[-1] == "STMT"
    for f in range(len(fns)):
        vals, nulls = got[f]
        mine = [None if nulls[i] else (float(vals[i]) if vals.dtype == np.float64 else int(vals[i])) for i in range(n)]
        assert mine == [r[f] for r in want], (over, f)


def test_model_small_streams_agree_with_the_sentences():
    """n <= 65: nav_model() itself asserts that the vectorised evaluation and the sentence-by-sentence one agree"""
    from midoridb_amd import dev
    from tests import window_model as M
    assert M.SMALL >= 65
    # (the model speaks the library's function codes: what it is asked is what the operator is asked)
    assert (N.LAG, N.LEAD, N.FIRST_VALUE, N.LAST_VALUE, N.NTILE) == (dev.WIN_LAG, dev.WIN_LEAD, dev.WIN_FIRST_VALUE, dev.WIN_LAST_VALUE, dev.WIN_NTILE)
    rng = np.random.default_rng(6)
    i64 = np.iinfo(np.int64)
    for n in (1, 2, 7, 64, 65):
        k = rng.integers(0, 3, n).astype(np.int64)
        o = rng.integers(0, 4, n).astype(np.int64)
        v = rng.integers(-5, 5, n).astype(np.int64)
        v[rng.random(n) < 0.2] = i64.max
        v[rng.random(n) < 0.2] = i64.min
        x = rng.choice(np.array([-0.0, 0.0, 3.0, -1.0]), n)
        nl = lambda p: rng.random(n) < p
        fns = [(N.LAG, v, nl(0.2), 1, None), (N.LAG, x, nl(0.2), 0, -0.0), (N.LAG, v, None, 2, i64.min), (N.LEAD, v, nl(0.3), 1, 7),
               (N.LEAD, x, None, 3, None), (N.LEAD, v, None, 1 << 32, 1), (N.FIRST_VALUE, x, nl(0.3)), (N.LAST_VALUE, v, nl(0.3)),
               (N.NTILE, 1), (N.NTILE, 2), (N.NTILE, 3), (N.NTILE, 64), (N.NTILE, 1000)]
        for part, order in [([], []), ([(k, nl(0.2), False)], []), ([], [(o, nl(0.2), True)]), ([(k, nl(0.2), False)], [(o, nl(0.1), False)])]:
            out = N.nav_model(part, order, n, fns)
            assert len(out) == len(fns) and all(len(vals) == n and len(nulls) == n for vals, nulls in out)
    # four rows, one partition, ordered by o with a tie: LAST_VALUE is the last PEER, ties in stream order
    o = np.array([2, 1, 2, 1], dtype=np.int64)
    v = np.array([10, 20, 30, 40], dtype=np.int64)
    (lag, lagn), (last, _), (nt, _) = N.nav_model([], [(o, None, False)], 4, [(N.LAG, v, None, 1, None), (N.LAST_VALUE, v, None), (N.NTILE, 3)])
    assert list(lag) == [40, 0, 10, 20] and list(lagn) == [False, True, False, False]
    assert list(last) == [30, 40, 30, 40] and list(nt) == [2, 1, 3, 1]
