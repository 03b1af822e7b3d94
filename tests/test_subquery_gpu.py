"""k IN / NOT IN (SELECT ...) on the device.

The operator: mdb_dev_set_from_column (mdb_dev_setbuild.hip) builds a set image from a DEVICE column; every image is downloaded and held
against the one the host builder (mdb_set_build) makes of the same valid cells - words 0 and 1 equal, the same members in the slots, every
member found by the host probe (mdb_set_image_contains walks the kernels' hash and probe sequence) - and then probed through
DeviceCtx.filter against numpy.isin.  Cells: 0, 1, around a wave (64), around a tile (4096), 2^18 + 1 (several workgroups per CU);
distinct values: 1, 9, the largest LDS-staged set, one more, 10^5; members at the extremes and on the first patterns of the marker
sequence, so the EMPTY marker has to move on.

The statements: against Python's sqlite3 on the same rows, and against this engine's own result for the same statement with the subquery
replaced by the literal list of its values (same rows, same order)."""
import ctypes

import numpy as np
import pytest

from midoridb_amd import dev as D

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NO_ROW = -1          # MDB_NO_ROW in an int32 row-id vector
MASK = (1 << 64) - 1


def _marker_seq(k):
    """the first k candidates of the EMPTY marker (mdb_dev.h), as signed 64-bit values"""
    out, x = [], 0x8000000000000000
    for _ in range(k):
        out.append(x - (1 << 64) if x >> 63 else x)
        x = (x * 6364136223846793005 + 1442695040888963407) & MASK
    return out


SPECIAL = sorted(set([I64_MIN, -1, 0, I64_MAX] + _marker_seq(3)))     # (INT64_MIN is the first candidate itself)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


class _HostImage:
    """mdb_set_build over host values (the reference image)"""

    def __init__(self, dev, values, typ):
        self.lib = dev.lib
        a = np.ascontiguousarray(values).view(np.int64)
        self.img = D.SetImage()
        rc = self.lib.mdb_set_build(ctypes.c_void_p(a.ctypes.data) if a.size else None, a.size, typ, ctypes.byref(self.img))
        assert rc == 0, rc

    def words(self):
        return np.ctypeslib.as_array(self.img.words, shape=(2 + self.img.slots,)).copy()

    def close(self):
        self.lib.mdb_set_image_free(ctypes.byref(self.img))


def _download(dev, s):
    """the device image behind the set's instruction -> (uint64 words, log2)"""
    insn = s.insn(0)
    log2 = insn[4]
    words = np.empty(2 + (1 << log2), dtype=np.uint64)
    dev._chk(dev.lib.mdb_dev_d2h(dev.h, ctypes.c_void_p(words.ctypes.data), ctypes.c_void_p(insn[5]), words.nbytes), "d2h")
    return words, log2


def _prober(dev, words, log2, typ, members_n):
    """value -> mdb_set_image_contains(the downloaded image, value)"""
    img = D.SetImage(words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1 << log2, members_n, int(words[0]), 0, log2, typ)
    ref, fn = ctypes.byref(img), dev.lib.mdb_set_image_contains
    return lambda value: fn(ref, value)


def _contains(dev, words, log2, typ, members_n, value):
    return bool(_prober(dev, words, log2, typ, members_n)(int(value)))


def _check_against_host(dev, cells, valid, typ, expect_log2=None, expect_rebuilt=None, nulls=None, rid=None, n_nan=0):
    """cells: the base column (int64 bits); valid: which CELLS of the stream count (after rid / NULL bits / NaN); builds on the device and
    compares with mdb_set_build over exactly the valid cells"""
    import torch
    d_cells = dev.to_dev(cells) if len(cells) else torch.empty(0, dtype=torch.int64, device=dev.device)
    d_nulls = dev.nullbits_dev(nulls) if nulls is not None else None
    d_rid = dev.to_dev(rid) if rid is not None else None
    stream = cells[np.where(rid == NO_ROW, 0, rid)] if rid is not None else cells
    host_vals = stream[valid] if len(stream) else np.empty(0, dtype=np.int64)
    s = dev.make_set_from_column(d_cells, d_nulls, d_rid, typ)
    host = _HostImage(dev, host_vals, typ)
    try:
        hw = host.words()
        words, log2 = _download(dev, s)
        info = s.info
        assert (int(words[0]), int(words[1])) == (int(hw[0]), int(hw[1])), "words 0 and 1 differ from the host image's"
        assert log2 == host.img.log2_slots == info.log2_slots
        if expect_log2 is not None:
            assert log2 == expect_log2
        marker = words[0]
        got = np.sort(words[2:][words[2:] != marker])
        exp = np.sort(hw[2:][hw[2:] != hw[0]])
        assert np.array_equal(got, exp), "the occupied slots are not the host image's members"
        assert info.members == host.img.members == len(exp)
        n_stream = len(stream)
        assert info.cells_nan == n_nan
        assert info.cells_null == n_stream - int(valid.sum()) - n_nan
        if expect_rebuilt is not None:
            assert info.rebuilt == expect_rebuilt
        # EVERY member on its probe path (the host probe walks the kernels' hash and probe sequence over the downloaded image); every
        # neighbour (member +- 1) that is no member is none
        members = exp.view(np.int64)
        has = _prober(dev, words, log2, typ, len(members))
        missing = [v for v in members.tolist() if not has(v)]
        assert not missing, missing[:8]
        if typ == D.T_INT64:
            near = np.concatenate([members[members < I64_MAX] + 1, members[members > I64_MIN] - 1])
            near = near[~np.isin(near, members)]
            found = [w for w in near.tolist() if has(w)]
            assert not found, found[:8]
        return info
    finally:
        host.close()
        s.close()


def _cells_with(rng, n, distinct):
    """n cells over exactly min(n, distinct) distinct values, the special ones first"""
    k = min(n, distinct)
    pool = np.array(SPECIAL[:k], dtype=np.int64)
    while len(pool) < k:
        more = rng.integers(-(1 << 62), 1 << 62, k - len(pool), dtype=np.int64)
        pool = np.concatenate([pool, np.setdiff1d(more, pool)])
    cells = np.concatenate([pool, rng.choice(pool, n - k)]) if n else np.empty(0, dtype=np.int64)
    return rng.permutation(cells), k


ROWS = [0, 1, 63, 64, 65, 4097, (1 << 18) + 1]


@pytest.mark.parametrize("n", ROWS)
def test_operator_all_distinct_against_host_builder(dev, n):
    rng = np.random.default_rng(n + 1)
    cells, k = _cells_with(rng, n, n)
    info = _check_against_host(dev, cells, np.ones(n, dtype=bool), D.T_INT64, expect_rebuilt=0)
    assert info.members == n


def _distinct_cases(dev):
    lds = dev.in_set_lds_values()
    return {"1": (1, 4), "9": (9, 6), "lds": (lds, 12), "lds+1": (lds + 1, 13), "1e5": (100_000, 18)}


@pytest.mark.parametrize("size", ["1", "9", "lds", "lds+1", "1e5"])
def test_operator_distinct_counts_against_host_builder(dev, size):
    distinct, log2 = _distinct_cases(dev)[size]
    rng = np.random.default_rng(distinct)
    n = distinct + distinct // 4 + 3                      # a quarter of the values twice
    cells, k = _cells_with(rng, n, distinct)
    info = _check_against_host(dev, cells, np.ones(n, dtype=bool), D.T_INT64, expect_log2=log2)
    assert info.members == distinct
    if distinct >= len(SPECIAL):                           # the first three candidates are members: the marker is the fourth
        s = dev.make_set_from_column(dev.to_dev(cells))
        words, _ = _download(dev, s)
        s.close()
        assert int(words[0]) == _marker_seq(4)[3] & MASK


@pytest.mark.parametrize("size", ["9", "lds"])
def test_operator_duplicate_heavy_is_rebuilt_small(dev, size):
    distinct, log2 = _distinct_cases(dev)[size]
    rng = np.random.default_rng(7 + distinct)
    n = (1 << 18) + 1
    cells, k = _cells_with(rng, n, distinct)
    info = _check_against_host(dev, cells, np.ones(n, dtype=bool), D.T_INT64, expect_log2=log2, expect_rebuilt=1)
    assert info.members == distinct and (1 << info.log2_slots) <= 4096


@pytest.mark.parametrize("n", [1, 65, 4097, (1 << 18) + 1])
def test_operator_null_bits(dev, n):
    rng = np.random.default_rng(100 + n)
    cells, k = _cells_with(rng, n, max(1, n // 3))
    nulls = rng.random(n) < 0.3
    _check_against_host(dev, cells, ~nulls, D.T_INT64, nulls=nulls)


@pytest.mark.parametrize("n", [1, 65, 4097, (1 << 18) + 1])
def test_operator_row_id_vector_with_no_row(dev, n):
    rng = np.random.default_rng(200 + n)
    base_n = max(1, n // 2 + 5)
    cells, k = _cells_with(rng, base_n, max(1, base_n // 2))
    nulls = rng.random(base_n) < 0.2
    rid = rng.integers(0, base_n, n).astype(np.int32)
    rid[rng.random(n) < 0.1] = NO_ROW
    at = np.where(rid == NO_ROW, 0, rid)
    valid = (rid != NO_ROW) & ~nulls[at]
    _check_against_host(dev, cells, valid, D.T_INT64, nulls=nulls, rid=rid)


@pytest.mark.parametrize("n", [5, 65, 4097, (1 << 18) + 1])
def test_operator_doubles_zero_signs_and_nan(dev, n):
    rng = np.random.default_rng(300 + n)
    vals = rng.choice(rng.standard_normal(max(2, n // 3)), n)
    vals[0], vals[1], vals[2] = -0.0, 0.0, np.nan
    vals[rng.random(n) < 0.05] = np.nan
    vals[rng.random(n) < 0.05] = -0.0
    nan = np.isnan(vals)
    cells = vals.view(np.int64).copy()
    info = _check_against_host(dev, cells, ~nan, D.T_DOUBLE, n_nan=int(nan.sum()))
    s = dev.make_set_from_column(dev.to_dev(vals), typ=D.T_DOUBLE)
    words, log2 = _download(dev, s)
    s.close()
    zero_bits = int(np.float64(-0.0).view(np.int64))
    assert _contains(dev, words, log2, D.T_DOUBLE, info.members, zero_bits) and _contains(dev, words, log2, D.T_DOUBLE, info.members, 0)
    assert int(words[0]) == 1 << 63 and not (words[2:] != words[0]).sum() - info.members     # -0.0 is looked up as +0.0: its bits are the marker
    assert info.members == len(np.unique(np.where(vals[~nan] == 0, 0.0, vals[~nan])))


@pytest.mark.parametrize("size", ["lds", "lds+1"])
def test_probe_through_filter_equals_isin(dev, size):
    distinct, log2 = _distinct_cases(dev)[size]
    rng = np.random.default_rng(400 + distinct)
    cells, k = _cells_with(rng, distinct * 2, distinct)
    members = np.unique(cells)
    s = dev.make_set_from_column(dev.to_dev(cells))
    n = 4097
    col = np.where(rng.random(n) < 0.5, rng.choice(members, n), rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64))
    col[:4] = [I64_MIN, I64_MAX, 0, -1]
    nulls = rng.random(n) < 0.1
    d_col, d_nulls = dev.to_dev(col), dev.nullbits_dev(nulls)
    isin = np.isin(col, members)
    for negate in (False, True):
        prog = [s.insn(0, negate)]
        assert prog[0][0] == D.P_IN_SET and prog[0][4] == log2
        got = dev.filter(prog, [(d_col, None, None)], n).cpu().numpy().astype(np.int64)
        assert np.array_equal(got, np.nonzero(isin != negate)[0]), negate
        got = dev.filter(prog, [(d_col, d_nulls, None)], n).cpu().numpy().astype(np.int64)
        assert np.array_equal(got, np.nonzero(~nulls & (isin != negate))[0]), negate
    s.close()


def test_more_distinct_values_than_the_cap(dev):
    rng = np.random.default_rng(5)
    cells = rng.permutation(np.arange(5000, dtype=np.int64) * 7919)
    d = dev.to_dev(cells)
    with pytest.raises(D.DeviceError) as e:
        dev.make_set_from_column(d, max_members=1000)
    text = str(e.value)
    assert "a set takes at most 1000" in text and "distinct values" in text
    count = int(text.split("set_from_column:")[1].split("distinct values")[0])
    assert 1000 < count <= 5000            # the count at which the insertion stopped, and the limit
    s = dev.make_set_from_column(d, max_members=5000)      # the context is as usable as before
    assert s.info.members == 5000 and s.info.log2_slots == 14
    s.close()


# ---------------------------------------------------------------------------------------------- SQL

N_ROWS = 5000


def _make_rows(seed):
    """three tables of a few thousand rows with NULLs in keys and values -> {name: (ddl, column names, [column values with None])}"""
    rng = np.random.default_rng(seed)

    def ints(n, lo, hi, p_null=0.05):
        v = rng.integers(lo, hi, n).tolist()
        return [None if rng.random() < p_null else x for x in v]

    def halves(n, lo, hi):
        return [None if x is None else x / 2 for x in ints(n, lo, hi)]

    def texts(n, k):
        return [None if x is None else f"s{x}" for x in ints(n, 0, k)]

    def days(n, k):
        return [None if x is None else 86400 * x for x in ints(n, 18000, 18000 + k)]

    n = N_ROWS
    return {
        "A": ("k INT, v INT, d DOUBLE, s VARCHAR(8), t DATE", ["k", "v", "d", "s", "t"],
              [ints(n, -300, 300), ints(n, 0, 50), halves(n, -200, 200), texts(n, 40), days(n, 60)]),
        "B": ("bk INT, bv INT, bd DOUBLE, bs VARCHAR(8), bt DATE", ["bk", "bv", "bd", "bs", "bt"],
              [ints(n, -400, 200), ints(n, 0, 50), halves(n, -300, 100), texts(n, 60), days(n, 90)]),
        "C": ("ck INT, cv INT", ["ck", "cv"], [ints(3000, -100, 500), ints(3000, 0, 50)]),
    }


def _engine(rows):
    from midoridb_amd.query import DB
    db = DB()
    for name, (ddl, names, cols) in rows.items():
        db.execute(f"CREATE TABLE {name} ({ddl});")
        arrs, nulls = [], []
        for decl, c in zip(ddl.split(", "), cols):
            isnull = np.array([x is None for x in c], dtype=np.uint8)
            if "VARCHAR" in decl:
                arrs.append(list(c))
                nulls.append(None)          # (None cells are SQL NULL)
            elif "DOUBLE" in decl:
                arrs.append(np.array([0.0 if x is None else x for x in c], dtype=np.float64))
                nulls.append(isnull)
            else:
                arrs.append(np.array([0 if x is None else x for x in c], dtype=np.int64))
                nulls.append(isnull)
        db.append_columns(name, arrs, nulls)
    return db


def _sqlite(rows):
    import sqlite3
    con = sqlite3.connect(":memory:")
    for name, (ddl, names, cols) in rows.items():
        con.execute(f"CREATE TABLE {name} ({ddl});")
        con.executemany(f"INSERT INTO {name} VALUES ({', '.join('?' * len(cols))});", list(zip(*cols)))
    return con


@pytest.fixture(scope="module")
def world():
    rows = _make_rows(11)
    db, con = _engine(rows), _sqlite(rows)
    yield db, con
    db.close()
    con.close()


def _engine_rows(db, sql, select_names):
    """the result as tuples in the select list's order (the result's own column order is the reference's), None for a NULL cell, DOUBLE
    cells as floats"""
    r = db.query(sql, step_cursor=True)
    at = [[i for i, nm in enumerate(r.names) if nm == want or nm.endswith("." + want)][0] for want in select_names]
    out = []
    for i in range(r.nrows):
        row = []
        for c in at:
            v = r.columns[c][i]
            if r.nulls[c][i]:
                v = None
            elif r.types[c] == 3:
                v = float(np.int64(v).view(np.float64))
            elif r.types[c] != 0:
                v = int(v)
            row.append(v)
        out.append(tuple(row))
    return out


def _literal(vals):
    def one(v):
        if v is None:
            return "NULL"
        if isinstance(v, str):
            return f"'{v}'"
        return repr(v)
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(one(v))
    return ", ".join(out)


# (statement with {0}, {1} ... where the subqueries stand, the subqueries, the select list's names, literal-list comparison?)
# A statement with ORDER BY is compared with sqlite row for row: its order is total (rows that tie are equal rows) and its ORDER BY
# columns hold no NULL in the selected rows (where a NULL sorts is not what these cases are about)
SELECTS = {
    "in": ("SELECT k, v FROM A WHERE k IN ({0});", ["SELECT bk FROM B"], ["k", "v"], True),
    "not_in_null_inside": ("SELECT k, v FROM A WHERE k NOT IN ({0});", ["SELECT bk FROM B"], ["k", "v"], True),
    "not_in": ("SELECT k, v FROM A WHERE v IS NOT NULL AND k NOT IN ({0}) ORDER BY k, v;", ["SELECT bk FROM B WHERE bk IS NOT NULL AND bv < 25"],
               ["k", "v"], True),
    "in_ordered": ("SELECT k, v FROM A WHERE v IS NOT NULL AND k IN ({0}) ORDER BY v DESC, k;", ["SELECT bk FROM B WHERE bv < 20"], ["k", "v"], True),
    "where": ("SELECT k FROM A WHERE v < 40 AND k IN ({0});", ["SELECT bk FROM B WHERE bv > 44"], ["k"], True),
    "group_having": ("SELECT k, v FROM A WHERE k IN ({0});", ["SELECT bk FROM B GROUP BY bk HAVING COUNT(*) > 9"], ["k", "v"], True),
    "distinct": ("SELECT k, v FROM A WHERE k NOT IN ({0});", ["SELECT DISTINCT bk FROM B WHERE bk > 0"], ["k", "v"], True),
    "limit": ("SELECT k, v FROM A WHERE k IN ({0});", ["SELECT DISTINCT bk FROM B WHERE bk > -50 ORDER BY bk LIMIT 30"], ["k", "v"], True),
    "join_inside": ("SELECT k, v FROM A WHERE k IN ({0});", ["SELECT bk FROM B JOIN C ON bk = ck WHERE cv > 40"], ["k", "v"], True),
    "empty_in": ("SELECT k, v FROM A WHERE k IN ({0});", ["SELECT bk FROM B WHERE bv > 1000"], ["k", "v"], False),
    "empty_not_in": ("SELECT k, v FROM A WHERE k NOT IN ({0});", ["SELECT bk FROM B WHERE bv > 1000"], ["k", "v"], False),
    "count": ("SELECT k, v FROM A WHERE k IN ({0});", ["SELECT COUNT(*) FROM C WHERE cv = 7"], ["k", "v"], True),
    "max": ("SELECT k, v FROM A WHERE v NOT IN ({0});", ["SELECT MAX(cv) FROM C"], ["k", "v"], True),
    "having": ("SELECT k, COUNT(*) FROM A GROUP BY k HAVING k IN ({0});", ["SELECT bk FROM B WHERE bv < 10"], ["k", "COUNT(*)"], True),
    "and": ("SELECT k, v FROM A WHERE k IN ({0}) AND v NOT IN ({1});", ["SELECT bk FROM B WHERE bv < 30", "SELECT cv FROM C WHERE ck < 0 AND cv > 10"],
            ["k", "v"], True),
    "or": ("SELECT k, v FROM A WHERE k IN ({0}) OR v IN ({1});", ["SELECT bk FROM B WHERE bv < 3", "SELECT cv FROM C WHERE ck < -90"], ["k", "v"], True),
    "nested": ("SELECT k, v FROM A WHERE k IN ({0});", ["SELECT bk FROM B WHERE bv NOT IN (SELECT cv FROM C WHERE ck < 100 AND cv > 5)"], ["k", "v"],
               True),
    "varchar": ("SELECT k, s FROM A WHERE s IN ({0});", ["SELECT bs FROM B WHERE bv < 2"], ["k", "s"], True),
    "varchar_not": ("SELECT k, s FROM A WHERE s NOT IN ({0});", ["SELECT bs FROM B WHERE bs IS NOT NULL AND bv < 1 AND bk > 100"], ["k", "s"], True),
    "double": ("SELECT k, d FROM A WHERE d IN ({0});", ["SELECT bd FROM B WHERE bv < 5"], ["k", "d"], True),
    "double_not": ("SELECT k, d FROM A WHERE d NOT IN ({0});", ["SELECT bd FROM B WHERE bd IS NOT NULL AND bv < 30"], ["k", "d"], True),
    # (a DATE column takes no literal list in SELECT - raw strings are not boxed there -: against sqlite alone)
    "date": ("SELECT k, t FROM A WHERE t IN ({0});", ["SELECT bt FROM B WHERE bv < 2"], ["k", "t"], False),
    "date_not": ("SELECT k, t FROM A WHERE k IS NOT NULL AND t NOT IN ({0}) ORDER BY t, k;",
                 ["SELECT bt FROM B WHERE bt IS NOT NULL AND bv < 1 AND bk > 100"], ["k", "t"], False),
}


@pytest.mark.parametrize("name", list(SELECTS))
def test_sql_select_against_sqlite_and_against_the_literal_list(world, name):
    db, con = world
    template, subs, names, with_literal = SELECTS[name]
    sql = template.format(*[s for s in subs])
    n_sub = sql.count("(SELECT")
    sets, lookups = db.subquery_sets(), db.in_set_lookups()
    got = _engine_rows(db, sql, names)
    assert db.subquery_sets() == sets + n_sub and db.in_set_lookups() == lookups
    exp = [tuple(r) for r in con.execute(sql.replace("COUNT(*) FROM A", "COUNT(*) AS c FROM A")).fetchall()]
    if "ORDER BY" in template:
        assert got == exp, name
        assert len(got) > 100 and all(r[0] is not None and r[1] is not None for r in got)
    else:
        assert sorted(got, key=repr) == sorted(exp, key=repr), name
    if name in ("not_in_null_inside",):
        assert got == []
    if name == "empty_not_in":
        assert len(got) == N_ROWS and any(r[0] is None for r in got)
    if name in ("in", "where", "and", "or", "nested", "varchar", "double", "date", "having", "count", "limit", "join_inside", "group_having"):
        assert 0 < len(got) < N_ROWS, "the case selects nothing or everything"
    if with_literal:
        lists = [_literal([r[0] for r in con.execute(s).fetchall()]) for s in subs]
        if all(lists):
            same = _engine_rows(db, template.format(*lists), names)
            assert got == same, "not the rows, in the order, of the literal list's statement"


def test_sql_large_subquery_probes_in_global_memory():
    """10^5 distinct values over 2 * 10^5 rows: a table of 2^18 slots"""
    from midoridb_amd.query import DB
    rng = np.random.default_rng(3)
    g = rng.integers(0, 400_000, 300_000, dtype=np.int64)
    h = rng.permutation(np.repeat(rng.permutation(400_000)[:100_000].astype(np.int64), 2))
    with DB() as db:
        db.execute("CREATE TABLE G (gk INT, gv INT);")
        db.execute("CREATE TABLE H (hk INT);")
        db.append_columns("G", [g, np.arange(len(g), dtype=np.int64)])
        db.append_columns("H", [h])
        for neg in (False, True):
            sets, lookups = db.subquery_sets(), db.in_set_lookups()
            r = db.query(f"SELECT gk, gv FROM G WHERE gk {'NOT ' if neg else ''}IN (SELECT hk FROM H);")
            assert db.subquery_sets() == sets + 1 and db.in_set_lookups() == lookups
            keep = np.isin(g, h) != neg
            at = {nm.split(".")[-1]: i for i, nm in enumerate(r.names)}
            assert np.array_equal(r.columns[at["gk"]], g[keep]) and np.array_equal(r.columns[at["gv"]], np.nonzero(keep)[0]), neg
            assert 10_000 < keep.sum() < len(g) - 10_000


DML = [
    ("DELETE FROM A WHERE k IN (SELECT bk FROM B WHERE bv < 10);", 1),
    ("UPDATE A SET v = 77 WHERE k NOT IN (SELECT bk FROM B WHERE bk IS NOT NULL AND bv < 30);", 1),
    # over the statement's own table: the subquery sees the table as it was
    ("DELETE FROM A WHERE v NOT IN (SELECT v FROM A WHERE k > 297 AND v IS NOT NULL);", 1),
    ("UPDATE A SET v = 3 WHERE k IN (SELECT k FROM A WHERE v = 3 OR v IN (SELECT cv FROM C WHERE ck > 495));", 2),
    ("DELETE FROM A WHERE k NOT IN (SELECT bk FROM B);", 1),        # a NULL inside: nothing goes
    ("DELETE FROM A WHERE s IN (SELECT bs FROM B WHERE bv = 1) OR d IN (SELECT bd FROM B WHERE bv = 2);", 2),
    ("DELETE FROM A WHERE k NOT IN (SELECT bk FROM B WHERE bv > 1000);", 1),      # an empty subquery: everything goes, NULL keys too
]


def test_sql_delete_and_update_against_sqlite():
    rows = _make_rows(12)
    db, con = _engine(rows), _sqlite(rows)
    try:
        for sql, n_sub in DML:
            sets, lookups = db.subquery_sets(), db.in_set_lookups()
            affected = db.execute(sql)
            assert db.subquery_sets() == sets + n_sub and db.in_set_lookups() == lookups, sql
            assert affected == con.execute(sql).rowcount, sql
            exp = [tuple(r) for r in con.execute("SELECT k, v, d, s FROM A ORDER BY rowid;").fetchall()]
            if exp:
                assert _engine_rows(db, "SELECT k, v, d, s FROM A;", ["k", "v", "d", "s"]) == exp, sql
            else:
                assert db.query("SELECT k FROM A;").nrows == 0
        assert not exp, "the last statement empties the table"
    finally:
        db.close()
        con.close()


def test_sharded_mode_refuses_subqueries():
    """at world 2 on one GPU (the test transport of tests/_dist_gpu_worker.py): every rank gets the refusal, before any exchange"""
    from tests.test_dist_gpu import _run
    out = _run("subquery", 2, 29635, worker="_subquery_dist_worker.py", timeout=300)
    assert "sharded subqueries refused ok" in out
