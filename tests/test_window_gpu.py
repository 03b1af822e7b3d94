"""Window functions on the device: mdb_dev_window against the numpy model of its contract (tests/window_model.py) - every cell and
every NULL word, guard cells around every output - and fn(...) OVER (...) statements through query_execute() against SQLite."""
import sqlite3

import numpy as np
import pytest

from tests import window_model as M

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
CHUNK = 4096                    # sorted positions per workgroup of the scan passes (WIN_CHUNK, mdb_dev_window.hip)
ROWS = [1, 63, 64, 65, 4095, 4096, 4097, 2 ** 18 + 1]     # wave, word and chunk edges; 2^18 + 1: the sort changes form
GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def D():
    from midoridb_amd import dev as D
    return D


def partition_sizes(rng, n, P):
    """P partitions over n sorted positions whose heads sit where carries can go wrong: on the last and the first position of a 64-bit
    word (63, 64) and of a chunk (4095, 4096, 8191, 8192); the last partition of a large stream covers whole chunks without a head"""
    if P == 1:
        return [n]
    if P == n:
        return [1] * n
    wanted = [h for h in (CHUNK - 1, CHUNK, 63, 64, 2 * CHUNK - 1, 2 * CHUNK) if h < n][:P - 1]
    heads = set(wanted)
    while len(heads) < P - 1:
        heads.add(int(rng.integers(1, min(n, 3 * CHUNK))))
    heads = [0] + sorted(heads) + [n]
    return [heads[i + 1] - heads[i] for i in range(P)]


class KeyThroughRowIds:
    """the partition key as a column of a base table read through a row-id vector.  MDB_NO_ROW stands only in rows of partition 0, whose
    key is NULL anyway: a "no row" key is a NULL key, so no row changes its partition and the heads stay where partition_sizes() put them"""

    def __init__(self, dev, D, rng, cells, nulls, norow_among):
        n = len(cells)
        m = n + 7
        place = rng.permutation(m)[:n]                      # row of the base table that stream position i reads
        base = rng.integers(-9, 9, m).astype(np.int64)
        base_null = rng.random(m) < 0.5
        base[place] = cells
        base_null[place] = nulls
        rid = place.astype(np.uint32)
        norow = norow_among & (rng.random(n) < 0.5)
        rid[norow] = D.NO_ROW
        self.cells, self.valid = cells, ~nulls
        self.rid = dev.to_dev(rid)
        self.values = dev.to_dev(base)
        self.nullbits = dev.nullbits_dev(base_null)
        self.norows = int(norow.sum())


class Case:
    """a stream of n rows in random order: a partition key (NULL for the first partition when there are several), an order key in one
    of three shapes, and the cells of the four folding functions"""

    def __init__(self, dev, D, rng, n, P, shape):
        from tests.test_aggregate_gpu import Column
        self.sizes = partition_sizes(rng, n, P)
        pid = np.repeat(np.arange(P), self.sizes)                      # partition of every sorted position
        shuffle = rng.permutation(n)
        pid = pid[shuffle]
        self.n, self.P = n, P
        key = pid.astype(np.int64) * 1000003 - 5 * 10 ** 6            # ascending with the partition: the sort puts partition i at its place
        knull = (pid == 0) & (P > 1)                                   # ... and the NULL key first
        self.part = KeyThroughRowIds(dev, D, rng, key, knull, knull)
        if shape == "peers":                                           # all rows of a partition are peers
            o = np.full(n, 7, dtype=np.int64)
            onull = np.zeros(n, dtype=bool)
        elif shape == "unique":                                        # every row is its own peer group
            o = rng.permutation(n).astype(np.int64) - n // 2
            onull = np.zeros(n, dtype=bool)
        else:                                                          # ties: peer groups of many rows (they span chunk edges), a NULL order key
            o = rng.integers(-2, 3, n).astype(np.int64) * (2 ** 40)
            onull = rng.random(n) < 0.1
        self.order = Column(dev, D, rng, o, onull)
        self.desc = bool(rng.integers(0, 2))
        v = rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int64)
        v[rng.random(n) < 0.05] = I64_MAX                              # SUM wraps
        v[rng.random(n) < 0.05] = I64_MIN
        allnull = (pid == 1) & (P > 1)                                 # a partition whose cells are all NULL (never the only one)
        self.v = Column(dev, D, rng, v, (rng.random(n) < 0.1) | allnull)
        self.vr = Column(dev, D, rng, v, (rng.random(n) < 0.1) | allnull, through_rid=n > 1)       # read through row ids with MDB_NO_ROW
        self.vm = Column(dev, D, rng, v, (rng.random(n) < 0.1) | allnull, misaligned=True)        # 8 bytes off a 16-byte boundary
        x = rng.choice(np.array([-0.0, 0.0, 1.5, -2.25, 1e300, -1e-300]), n)                       # DOUBLE MIN / MAX with both zeros
        self.x = Column(dev, D, rng, x.view(np.int64), (rng.random(n) < 0.2) | allnull)
        self.x.cells = x
        z = rng.choice(np.array([-0.0, 0.0]), n)                       # nothing but the two zeros: which of them MIN / MAX return shows the order
        self.z = Column(dev, D, rng, z.view(np.int64), (rng.random(n) < 0.3) | allnull)
        self.z.cells = z

    def keys(self, D, npart=1, norder=1):
        part = [(self.part.values, self.part.nullbits, self.part.rid, D.T_INT64, False)][:npart]
        order = [(self.order.values, self.order.nullbits, self.order.rid, D.T_INT64, self.desc)][:norder]
        mpart = [(self.part.cells, ~self.part.valid, False)][:npart]
        morder = [(self.order.cells, ~self.order.valid, self.desc)][:norder]
        return part, order, mpart, morder

    def double_min_max(self, D):
        """MIN and MAX over the DOUBLE columns that hold both zeros - x among other values, z nothing else: -0.0 lies before +0.0"""
        cols = [(op, c) for c in (self.x, self.z) for op in (D.WIN_MIN, D.WIN_MAX)]
        return [(op, D.T_DOUBLE, c.values, c.nullbits, c.rid) for op, c in cols], [(op, c.cells, ~c.valid) for op, c in cols]

    def all_eight(self, D):
        """all eight functions, for ONE call, and what the model is asked"""
        cols = [(D.WIN_SUM, self.v, D.T_INT64), (D.WIN_MIN, self.vr, D.T_INT64), (D.WIN_MAX, self.x, D.T_DOUBLE), (D.WIN_AVG, self.vm, D.T_INT64)]
        fns = [(D.WIN_ROW_NUMBER,), (D.WIN_RANK,), (D.WIN_DENSE_RANK,), (D.WIN_COUNT,)] + [(op, ty, c.values, c.nullbits, c.rid) for op, c, ty in cols]
        model = [(M.ROW_NUMBER,), (M.RANK,), (M.DENSE_RANK,), (M.COUNT,)] + [(op, c.cells, ~c.valid) for op, c, _ in cols]
        return fns, model


def call_guarded(dev, D, part, order, n, fns):
    """one mdb_dev_window call into outputs with guard cells in front and behind -> (cells as uint64 arrays, NULL words, form)"""
    import torch
    words = (n + 63) // 64
    outs = [torch.full((n + 16,), GUARD, dtype=torch.int64, device=dev.device) for _ in fns]
    nbs = [torch.full((words + 4,), GUARD, dtype=torch.int64, device=dev.device) for _ in fns]
    as_double = lambda fn: fn[0] == D.WIN_AVG or (fn[0] in (D.WIN_MIN, D.WIN_MAX) and fn[1] == D.T_DOUBLE)
    views = [o[8:8 + n].view(torch.float64) if as_double(fn) else o[8:8 + n] for o, fn in zip(outs, fns)]
    res, nulls, form = dev.window(part, order, n, fns, outs=views, nulls=[b[2:2 + words] for b in nbs])
    cells, nwords = [], []
    for o, b in zip(outs, nbs):
        h, hb = o.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64)
        assert (h[:8] == GUARD).all() and (h[8 + n:] == GUARD).all(), "a cell outside out[0 .. n) was written"
        assert (hb[:2] == GUARD).all() and (hb[2 + words:] == GUARD).all(), "a word outside the (n + 63) / 64 NULL words was written"
        cells.append(h[8:8 + n].copy())
        nwords.append(hb[2:2 + words].copy())
    return cells, nwords, form


def check(D, cells, nwords, n, model_out):
    from midoridb_amd.dev import pack_nullbits
    for f, (vals, nulls) in enumerate(model_out):
        want = np.ascontiguousarray(vals).view(np.uint64)
        bad = np.flatnonzero(cells[f] != want)
        assert bad.size == 0, f"function {f}: {bad.size} cells differ, first at stream position {bad[0]}: {cells[f][bad[0]]:#x} != {want[bad[0]]:#x}"
        assert (nwords[f] == pack_nullbits(nulls)).all(), f"function {f}: NULL words differ"


SHAPES = ["ties", "peers", "unique"]
CASES = [(n, P, SHAPES[(i + j) % 3]) for i, n in enumerate(ROWS) for j, P in enumerate(sorted({1, 2, 3, 65, n})) if P <= n]


@pytest.mark.parametrize("n,P,shape", CASES)
def test_operator_all_eight_functions_in_one_call(dev, D, n, P, shape):
    rng = np.random.default_rng(n * 31 + P)
    case = Case(dev, D, rng, n, P, shape)
    part, order, mpart, morder = case.keys(D)
    fns, model = case.all_eight(D)
    cells, nwords, form = call_guarded(dev, D, part, order, n, fns)
    assert form == 2
    want = M.window_model(mpart, morder, n, model)
    check(D, cells, nwords, n, want)
    # the partitions are where partition_sizes() put them: COUNT(*) OVER (PARTITION BY k) of the model is the designed size of every row's partition
    sizes = M.window_model(mpart, [], n, [(M.COUNT,)])[0][0]
    assert sorted(set(sizes.tolist())) == sorted(set(case.sizes)) and int(sizes.sum()) == sum(s * s for s in case.sizes)
    # a second call: MIN and MAX over the DOUBLE cells with both zeros
    fns2, model2 = case.double_min_max(D)
    cells, nwords, form = call_guarded(dev, D, part, order, n, fns2)
    assert form == 2
    want2 = M.window_model(mpart, morder, n, model2)
    check(D, cells, nwords, n, want2)
    if n >= 4095 and P == 65 and shape == "unique":     # (dozens of partitions whose frames grow row by row: both zeros are results of MIN and of MAX over z)
        for vals, nulls in want2[2:]:
            assert set(vals.view(np.uint64)[~nulls].tolist()) == {0, 1 << 63}, "the expected MIN / MAX over z do not hold both zeros"


@pytest.mark.parametrize("n", [65, 4097, 2 ** 18 + 1])
def test_operator_forms_keys_alone_and_none(dev, D, n):
    rng = np.random.default_rng(n)
    case = Case(dev, D, rng, n, min(n, 65), "ties")
    fns, model = case.all_eight(D)
    for npart, norder, want_form in [(1, 0, 2), (0, 1, 2), (0, 0, 1)]:
        part, order, mpart, morder = case.keys(D, npart, norder)
        cells, nwords, form = call_guarded(dev, D, part, order, n, fns)
        assert form == want_form, (npart, norder)
        check(D, cells, nwords, n, M.window_model(mpart, morder, n, model))
    # two order keys, the second a DOUBLE in descending order with both zeros: -0.0 and +0.0 are different peers
    x = rng.choice(np.array([-0.0, 0.0, 2.5]), n)
    xd = dev.to_dev(x.view(np.int64))
    part, order, mpart, morder = case.keys(D)
    order = order + [(xd, None, None, D.T_DOUBLE, True)]
    morder = morder + [(x, None, True)]
    cells, nwords, form = call_guarded(dev, D, part, order, n, fns)
    assert form == 2
    check(D, cells, nwords, n, M.window_model(mpart, morder, n, model))


def test_operator_same_input_same_bytes_and_empty_stream(dev, D):
    n = 3 * CHUNK + 17
    rng = np.random.default_rng(77)
    case = Case(dev, D, rng, n, 3, "ties")
    part, order, mpart, morder = case.keys(D)
    fns, model = case.all_eight(D)
    first = call_guarded(dev, D, part, order, n, fns)
    second = call_guarded(dev, D, part, order, n, fns)
    for a, b in zip(first[0] + first[1], second[0] + second[1]):
        assert a.tobytes() == b.tobytes()
    # n == 0: nothing is written, the form is still reported
    import torch
    outs = [torch.full((2,), GUARD, dtype=torch.int64, device=dev.device) for _ in fns]
    nbs = [torch.full((2,), GUARD, dtype=torch.int64, device=dev.device) for _ in fns]
    res, nulls, form = dev.window(part, order, 0, fns, outs=outs, nulls=nbs)
    assert form == 2 and all(len(r) == 0 for r in res)
    assert all((t.cpu().numpy().view(np.uint64) == GUARD).all() for t in outs + nbs)


def test_operator_refusals(dev, D):
    from midoridb_amd.dev import DeviceError
    v = dev.to_dev(np.arange(8, dtype=np.int64))
    for fns, msg in [([(D.WIN_SUM, D.T_DOUBLE, v, None, None)], "SUM / AVG over DOUBLE"), ([(D.WIN_AVG, D.T_DOUBLE, v, None, None)], "SUM / AVG over DOUBLE"),
                     ([(9,)], "unknown function"), ([(D.WIN_RANK,)] * 9, "functions per call")]:
        with pytest.raises(DeviceError) as ei:
            dev.window([], [], 8, fns)
        assert msg in str(ei.value), str(ei.value)
    out, nulls, form = dev.window([], [], 8, [(D.WIN_ROW_NUMBER,)])      # the context stays usable
    assert out[0].cpu().tolist() == list(range(1, 9)) and form == 1


# ------------------------------------------------------------------ statements, compared with SQLite

@pytest.fixture(scope="module")
def world():
    """A: 700 rows - partition keys with NULLs, order keys with ties and NULLs, NULL cells, a VARCHAR and a DATE column, a unique pk;
    B: keys with and without partner in A; E: empty; ONE: one row.  The same rows in SQLite."""
    from midoridb_amd.query import DB
    rng = np.random.default_rng(11)
    n = 700
    k = rng.integers(0, 9, n).astype(np.int64)
    o = rng.integers(0, 15, n).astype(np.int64)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    d = rng.integers(-40, 40, n) / 8.0 + 0.0625
    s = [None if rng.random() < 0.1 else "name%d" % rng.integers(0, 5) for _ in range(n)]
    t = 1577880000 + 86400 * rng.integers(0, 30, n).astype(np.int64)
    pk = rng.permutation(n).astype(np.int64)
    nulls = [rng.random(n) < 0.06, rng.random(n) < 0.08, (rng.random(n) < 0.12) | (k == 4), rng.random(n) < 0.1, None, rng.random(n) < 0.05, np.zeros(n, dtype=bool)]
    db = DB()
    db.execute("CREATE TABLE A (k INT, o INT, v INT, d DOUBLE, s VARCHAR(12), t DATE, pk INT PRIMARY KEY);")
    zero = np.zeros(n, dtype=np.uint8)
    db.append_columns("A", [k, o, v, d.view(np.int64), s, t, pk], [zero if x is None else x.astype(np.uint8) for x in nulls])
    m = 40
    kb = np.arange(m, dtype=np.int64) % 13 - 2                  # -2, -1, 9, 10: no partner in A; some of A's keys have several
    w = np.arange(m, dtype=np.int64) * 3 - 50
    db.execute("CREATE TABLE B (kb INT, w INT);")
    db.append_columns("B", [kb, w])
    db.execute("CREATE TABLE E (k INT, v INT);")
    db.execute("CREATE TABLE ONE (k INT, v INT);")
    db.execute("INSERT INTO ONE VALUES (5, 6);")
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE A (k INTEGER, o INTEGER, v INTEGER, d REAL, s TEXT, t INTEGER, pk INTEGER)")
    cell = lambda c, i, x: None if (nulls[c] is not None and nulls[c][i]) else x
    con.executemany("INSERT INTO A VALUES (?, ?, ?, ?, ?, ?, ?)", [(cell(0, i, int(k[i])), cell(1, i, int(o[i])), cell(2, i, int(v[i])), cell(3, i, float(d[i])),
                                                                     s[i], cell(5, i, int(t[i])), int(pk[i])) for i in range(n)])
    con.execute("CREATE TABLE B (kb INTEGER, w INTEGER)")
    con.executemany("INSERT INTO B VALUES (?, ?)", [(int(kb[i]), int(w[i])) for i in range(m)])
    con.execute("CREATE TABLE E (k INTEGER, v INTEGER)")
    con.execute("CREATE TABLE ONE (k INTEGER, v INTEGER)")
    con.execute("INSERT INTO ONE VALUES (5, 6)")
    yield db, con
    db.close()


def ours(db, sql, wanted):
    from tests.test_aggregate_gpu import sql_rows, by_name
    names, types, rows = sql_rows(db, sql)
    return by_name(names, rows, wanted), names, types


def multiset(rows):
    return sorted(rows, key=lambda r: tuple((x is None, 0 if x is None else x) for x in r))


def same(db, con, sql, wanted, lite=None, total=False):
    got, names, types = ours(db, sql, wanted)
    want = [tuple(r) for r in con.execute(lite or sql.rstrip(";")).fetchall()]
    if total:
        assert got == want, sql
    else:
        assert multiset(got) == multiset(want), sql
    return names, types


def test_sql_each_function_over_a_single_table(world):
    db, con = world
    over = "PARTITION BY k ORDER BY o DESC"
    # ROW_NUMBER: ties keep the stream order - the table's row order, SQLite's rowid
    same(db, con, f"SELECT pk, ROW_NUMBER() OVER ({over}) AS x FROM A;", ["A.pk", "x"], lite=f"SELECT pk, ROW_NUMBER() OVER ({over}, rowid) FROM A")
    for fn in ["RANK()", "DENSE_RANK()", "COUNT(*)", "SUM(v)", "MIN(v)", "MAX(v)", "AVG(v)", "MIN(d)", "MAX(d)", "MIN(t)", "MAX(t)"]:
        names, types = same(db, con, f"SELECT pk, {fn} OVER ({over}) AS x FROM A;", ["A.pk", "x"])
        assert types[names.index("x")] == (3 if fn in ("AVG(v)", "MIN(d)", "MAX(d)") else 4 if fn in ("MIN(t)", "MAX(t)") else 1), fn
    # without an alias the result column is named by the function's text
    got, names, types = ours(db, "SELECT pk, SUM(v) OVER (PARTITION BY k), RANK() OVER (ORDER BY o), COUNT(*) OVER () FROM A;", ["A.pk"])
    assert sorted(names) == sorted(["A.pk", "SUM(A.v) OVER", "RANK() OVER", "COUNT(*) OVER"])
    same(db, con, "SELECT pk, SUM(v) OVER (PARTITION BY k), RANK() OVER (ORDER BY o), COUNT(*) OVER () FROM A;",
         ["A.pk", "SUM(A.v) OVER", "RANK() OVER", "COUNT(*) OVER"])
    # whole partition without ORDER BY, whole stream without keys, NULL keys on both sides
    same(db, con, "SELECT pk, SUM(v) OVER (PARTITION BY k) AS a, AVG(v) OVER () AS b, MAX(v) OVER (ORDER BY o, k) AS c FROM A;", ["A.pk", "a", "b", "c"])


def test_sql_windows_shared_and_not(world):
    db, con = world
    c0 = db.window_calls()
    same(db, con, "SELECT pk, RANK() OVER (PARTITION BY k ORDER BY o) AS a, SUM(v) OVER (PARTITION BY A.k ORDER BY A.o) AS b FROM A;", ["A.pk", "a", "b"])
    assert db.window_calls() == c0 + 1                 # equal field for field: one operator call
    same(db, con, "SELECT pk, RANK() OVER (PARTITION BY k ORDER BY o) AS a, SUM(v) OVER (PARTITION BY k ORDER BY o DESC) AS b, "
                  "DENSE_RANK() OVER (PARTITION BY k ORDER BY o) AS c, MIN(v) OVER (ORDER BY o) AS e FROM A;", ["A.pk", "a", "b", "c", "e"])
    assert db.window_calls() == c0 + 1 + 3             # three different windows among the four items


def test_sql_over_joins_and_where(world):
    db, con = world
    # unique order keys: the joined rows' order plays no part
    same(db, con, "SELECT pk, w, ROW_NUMBER() OVER (PARTITION BY kb ORDER BY pk, w) AS rn, SUM(w) OVER (PARTITION BY k ORDER BY pk DESC, w) AS sw "
                  "FROM A INNER JOIN B ON k = kb;", ["A.pk", "B.w", "rn", "sw"])
    # LEFT JOIN: the NULL-supplied column is the partition key and the summed column
    same(db, con, "SELECT pk, w, SUM(w) OVER (PARTITION BY kb ORDER BY o) AS sw, COUNT(*) OVER (PARTITION BY kb) AS c, RANK() OVER (PARTITION BY kb ORDER BY w) AS r "
                  "FROM A LEFT JOIN B ON k = kb;", ["A.pk", "B.w", "sw", "c", "r"])
    same(db, con, "SELECT pk, DENSE_RANK() OVER (PARTITION BY k ORDER BY o) AS dr, MAX(v) OVER (PARTITION BY k ORDER BY o) AS mx FROM A WHERE v > 0 AND o < 12;",
         ["A.pk", "dr", "mx"])


def test_sql_tail_clauses_over_window_columns(world):
    db, con = world
    # top 3 per partition: HAVING filters the ungrouped stream by the alias; SQLite gets the statement as a subquery
    same(db, con, "SELECT k, pk, ROW_NUMBER() OVER (PARTITION BY k ORDER BY v DESC, pk) AS rn FROM A HAVING rn <= 3 ORDER BY k, rn;", ["A.k", "A.pk", "rn"],
         lite="SELECT * FROM (SELECT k, pk, ROW_NUMBER() OVER (PARTITION BY k ORDER BY v DESC, pk) AS rn FROM A) WHERE rn <= 3 ORDER BY k, rn", total=True)
    same(db, con, "SELECT pk, SUM(v) OVER (PARTITION BY k ORDER BY pk) AS run FROM A ORDER BY run DESC, pk LIMIT 10;", ["A.pk", "run"], total=True)
    same(db, con, "SELECT DISTINCT DENSE_RANK() OVER (ORDER BY o) AS dr FROM A;", ["dr"])
    same(db, con, "SELECT DISTINCT k, COUNT(*) OVER (PARTITION BY k) AS c FROM A;", ["A.k", "c"])


def test_sql_key_types_and_tiny_streams(world):
    db, con = world
    same(db, con, "SELECT pk, COUNT(*) OVER (PARTITION BY s) AS c, RANK() OVER (PARTITION BY s ORDER BY t DESC) AS r, MIN(v) OVER (PARTITION BY d) AS m FROM A;",
         ["A.pk", "c", "r", "m"])
    for sql in ["SELECT k, ROW_NUMBER() OVER (ORDER BY k) AS rn, SUM(v) OVER () AS s FROM E;", "SELECT pk, RANK() OVER (ORDER BY o) AS r FROM A WHERE pk < 0;"]:
        got, names, types = ours(db, sql, [])
        assert got == [] and len(names) >= 2, sql
    same(db, con, "SELECT k, ROW_NUMBER() OVER (PARTITION BY k ORDER BY v) AS rn, SUM(v) OVER () AS s, AVG(v) OVER (ORDER BY k) AS a FROM ONE;", ["ONE.k", "rn", "s", "a"])


def test_sql_results_kept_on_the_device(world):
    db, con = world
    want = con.execute("SELECT pk, SUM(v) OVER (PARTITION BY k ORDER BY o) FROM A").fetchall()
    db.results_on_device(True)
    try:
        names, types, cols, nrows, joined, ms = db.query_device("SELECT pk, SUM(v) OVER (PARTITION BY k ORDER BY o) AS run FROM A;")
        nulls = db.last_device_nulls
    finally:
        db.results_on_device(False)
    a, b = names.index("A.pk"), names.index("run")
    got = [(int(cols[a][i]), None if nulls[b] is not None and bool(nulls[b][i]) else int(cols[b][i])) for i in range(nrows)]
    assert multiset(got) == multiset([tuple(r) for r in want])


def test_sharded_mode_refuses_window_functions():
    """at world 2 on one GPU (the test transport of tests/_dist_gpu_worker.py): every rank gets the refusal, before any exchange"""
    from tests.test_dist_gpu import _run
    out = _run("window", 2, 29637, worker="_window_dist_worker.py", timeout=300)
    assert "sharded window functions refused ok" in out
