"""Navigation window functions on the device: LAG, LEAD, FIRST_VALUE, LAST_VALUE and NTILE of mdb_dev_window against the numpy model of
their contract (tests/window_nav_model.py) - every cell and every NULL word, guard cells around every output - and the statements
through query_execute() against the same model."""
import numpy as np
import pytest

from tests import window_model as M
from tests import window_nav_model as N
from tests.test_window_gpu import CHUNK, GUARD, I64_MAX, I64_MIN, ROWS, Case, call_guarded, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    from midoridb_amd import dev as D
    return D


HEADS = [63, 64, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK]


class HeadsCase(Case):
    """Case's columns over partitions of random length whose heads stand exactly at the sorted positions HEADS (those below n): the
    sizes are given, nothing of Case's own layout is used"""

    def __init__(self, dev, D, rng, n, shape):
        from tests.test_aggregate_gpu import Column
        from tests.test_window_gpu import KeyThroughRowIds
        heads = {h for h in HEADS if h < n}
        while len(heads) < min(n - 1, 40):
            heads.add(int(rng.integers(1, n)))
        self.heads = [0] + sorted(heads)
        self.sizes = [t - h for h, t in zip(self.heads, self.heads[1:] + [n])]
        P = len(self.sizes)
        pid = np.repeat(np.arange(P), self.sizes)[rng.permutation(n)]
        self.n, self.P = n, P
        key = pid.astype(np.int64) * 1000003 - 5 * 10 ** 6             # ascending with the partition; partition 0 has the NULL key
        self.part = KeyThroughRowIds(dev, D, rng, key, pid == 0, pid == 0)
        o = rng.permutation(n).astype(np.int64) if shape == "unique" else np.full(n, 7, dtype=np.int64) if shape == "peers" else \
            rng.integers(-2, 3, n).astype(np.int64) * (2 ** 40)
        self.order = Column(dev, D, rng, o, (rng.random(n) < 0.1) & (shape == "ties"))
        self.desc = bool(rng.integers(0, 2))
        v = rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int64)
        v[rng.random(n) < 0.05] = I64_MAX
        v[rng.random(n) < 0.05] = I64_MIN
        self.v = Column(dev, D, rng, v, rng.random(n) < 0.1)
        self.vr = Column(dev, D, rng, v, rng.random(n) < 0.1, through_rid=True)
        self.vm = Column(dev, D, rng, v, rng.random(n) < 0.1, misaligned=True)
        x = rng.choice(np.array([-0.0, 0.0, 1.5, -2.25, 1e300, -1e-300]), n)
        self.x = Column(dev, D, rng, x.view(np.int64), rng.random(n) < 0.2)
        self.x.cells = x


def nav_calls(D, case, n):
    """the calls of one case, at most 8 functions each: (device functions, model functions)"""
    v, vr, vm, x = case.v, case.vr, case.vm, case.x
    col = lambda c: (D.T_DOUBLE if c is x else D.T_INT64, c.values, c.nullbits, c.rid)
    mcol = lambda c: (c.cells, ~c.valid)
    big = n + 5                                                     # larger than any partition
    lists = [
        [(N.LAG, v, 0, None), (N.LAG, vr, 1, None), (N.LAG, x, 63, -0.0), (N.LAG, vm, 64, I64_MIN),
         (N.LEAD, vr, 1, 7), (N.LEAD, v, 63, None), (N.LEAD, x, 64, None), (N.LEAD, vm, 0, I64_MAX)],
        [(N.LAG, v, 4096, None), (N.LAG, vr, 4097, -1), (N.LAG, x, 1 << 32, 1.5), (N.LAG, vm, big, None),
         (N.LEAD, vr, 4096, I64_MAX), (N.LEAD, v, 4097, None), (N.LEAD, x, 1 << 32, None), (N.LEAD, vm, big, 0)],
        [(N.FIRST_VALUE, v), (N.FIRST_VALUE, x), (N.LAST_VALUE, vr), (N.LAST_VALUE, x), (N.NTILE, 1), (N.NTILE, 2), (N.NTILE, 3), (N.NTILE, 7)],
        [(N.NTILE, 4096), (N.NTILE, big), (N.NTILE, 1 << 40), (N.LAST_VALUE, vm), (N.FIRST_VALUE, vr)],
    ]
    out = []
    for fl in lists:
        dfn, mfn = [], []
        for f in fl:
            if f[0] == N.NTILE:
                dfn.append((f[0], f[1]))
                mfn.append((f[0], f[1]))
            else:
                k, dflt = (f[2], f[3]) if len(f) > 2 else (1, None)
                dfn.append((f[0],) + col(f[1]) + (k, dflt))
                mfn.append((f[0],) + mcol(f[1]) + (k, dflt))
        out.append((dfn, mfn))
    return out


def run_case(dev, D, case, n, npart=1, norder=1, want_form=2):
    part, order, mpart, morder = case.keys(D, npart, norder)
    for dfn, mfn in nav_calls(D, case, n):
        cells, nwords, form = call_guarded(dev, D, part, order, n, dfn)
        assert form == want_form
        check(D, cells, nwords, n, N.nav_model(mpart, morder, n, mfn))


SHAPES = ["ties", "peers", "unique"]
CASES = [(n, P, SHAPES[(i + j) % 3]) for i, n in enumerate(ROWS) for j, P in enumerate(sorted({1, 3, 65, n})) if P <= n]


@pytest.mark.parametrize("n,P,shape", CASES)
def test_operator_navigation_against_the_model(dev, D, n, P, shape):
    """P = 1: one partition over the whole stream - chunks without a partition head, the carry crosses them; P = n: every row its own
    partition; the NULL partition key is partition 0; v holds I64_MIN / I64_MAX, x both zeros, vr is read through row ids with MDB_NO_ROW"""
    rng = np.random.default_rng(n * 37 + P)
    run_case(dev, D, Case(dev, D, rng, n, P, shape), n)


@pytest.mark.parametrize("n,shape", [(4097, "ties"), (4098, "unique"), (3 * CHUNK + 17, "ties"), (2 ** 18 + 1, "peers")])
def test_operator_partition_heads_at_the_chunk_edge(dev, D, n, shape):
    rng = np.random.default_rng(n)
    case = HeadsCase(dev, D, rng, n, shape)
    part, order, mpart, morder = case.keys(D)
    perm, b, pe, e = N.structure(mpart, morder, n)
    # the partitions begin where they were put: b is its own position at every head, and at no other
    assert np.flatnonzero(b == np.arange(n)).tolist() == case.heads and {h for h in HEADS if h < n} <= set(case.heads)
    assert all(b[h - 1] < h for h in case.heads[1:]) and pe[CHUNK - 1] == CHUNK and (n <= CHUNK + 1 or pe[CHUNK] == CHUNK + 1)
    run_case(dev, D, case, n)


@pytest.mark.parametrize("n", [65, 4097, 2 ** 18 + 1])
def test_operator_forms_keys_alone_and_none(dev, D, n):
    """no order keys: LAST_VALUE is the partition's last row; no keys at all (form 1, no sort): the stream is one partition of peers"""
    rng = np.random.default_rng(n + 1)
    case = Case(dev, D, rng, n, min(n, 65), "ties")
    for npart, norder, want_form in [(1, 0, 2), (0, 1, 2), (0, 0, 1)]:
        run_case(dev, D, case, n, npart, norder, want_form)


def test_operator_mixed_call_and_same_bytes(dev, D):
    """one call mixing old and new functions over one window: the old functions' cells are those of a call without the new ones"""
    n = 3 * CHUNK + 17
    rng = np.random.default_rng(78)
    case = Case(dev, D, rng, n, 3, "ties")
    part, order, mpart, morder = case.keys(D)
    v = (D.T_INT64, case.v.values, case.v.nullbits, case.v.rid)
    old = [(D.WIN_ROW_NUMBER,), (D.WIN_SUM,) + v, (D.WIN_COUNT,)]
    new = [(D.WIN_LAG,) + v + (1, None), (D.WIN_LEAD,) + v + (2, 0), (D.WIN_NTILE, 5)]
    mixed = [old[0], new[0], old[1], new[1], new[2], old[2]]
    alone = call_guarded(dev, D, part, order, n, old)
    first = call_guarded(dev, D, part, order, n, mixed)
    second = call_guarded(dev, D, part, order, n, mixed)
    for a, b in zip(first[0] + first[1], second[0] + second[1]):
        assert a.tobytes() == b.tobytes()
    for i, j in [(0, 0), (1, 2), (2, 5)]:
        assert alone[0][i].tobytes() == first[0][j].tobytes() and alone[1][i].tobytes() == first[1][j].tobytes()
    mv = (case.v.cells, ~case.v.valid)
    check(D, alone[0], alone[1], n, M.window_model(mpart, morder, n, [(M.ROW_NUMBER,), (M.SUM,) + mv, (M.COUNT,)]))
    check(D, [first[0][j] for j in (1, 3, 4)], [first[1][j] for j in (1, 3, 4)], n,
          N.nav_model(mpart, morder, n, [(N.LAG,) + mv + (1, None), (N.LEAD,) + mv + (2, 0), (N.NTILE, 5)]))


def test_operator_refusals_and_empty_stream(dev, D):
    import torch
    from midoridb_amd.dev import DeviceError
    v = dev.to_dev(np.arange(8, dtype=np.int64))
    guard = [torch.full((10,), GUARD, dtype=torch.int64, device=dev.device) for _ in range(4)]
    for fns, msg in [([(D.WIN_ROW_NUMBER,), (D.WIN_NTILE, 0)], "NTILE(0)"), ([(9,)], "unknown function"), ([(15,)], "unknown function"), ([(21,)], "unknown function"),
                     ([(D.WIN_LAG, D.T_INT64, None, None, None, 1, None)], "no cells")]:
        with pytest.raises(DeviceError) as ei:
            dev.window([], [], 8, fns, outs=[g[1:9] for g in guard[:len(fns)]], nulls=[g[1:2] for g in guard[2:2 + len(fns)]])
        assert msg in str(ei.value), str(ei.value)
    assert all((g.cpu().numpy().view(np.uint64) == GUARD).all() for g in guard), "a refused call wrote something"
    # n == 0: nothing is written
    fns = [(D.WIN_LAG, D.T_INT64, v, None, None, 1, 3), (D.WIN_NTILE, 2)]
    res, nulls, form = dev.window([], [], 0, fns, outs=guard[:2], nulls=guard[2:])
    assert form == 1 and all((g.cpu().numpy().view(np.uint64) == GUARD).all() for g in guard)
    # the context stays usable; the result's dtype follows the cells
    x = dev.to_dev(np.array([1.5, -0.0, 2.5]))
    (lag, lead, nt), (ln, _, _), form = dev.window([], [], 3, [(D.WIN_LAG, D.T_DOUBLE, x, None, None, 1, None), (D.WIN_LEAD, D.T_DOUBLE, x, None, None, 1, -0.0), (D.WIN_NTILE, 2)])
    assert lag.dtype == torch.float64 and nt.dtype == torch.int64
    assert lag.cpu().numpy().tobytes() == np.array([0.0, 1.5, -0.0]).tobytes() and int(ln[0]) == 1
    assert lead.cpu().numpy().tobytes() == np.array([-0.0, 2.5, -0.0]).tobytes() and nt.cpu().tolist() == [1, 1, 2]


# ------------------------------------------------------------------ statements

@pytest.fixture(scope="module")
def world():
    """R: 3000 readings - a sensor k (NULL for some), a unique time o, a value v with NULLs, a VARCHAR s, a DATE t, a unique pk; S: one
    row for some of the sensors"""
    from midoridb_amd.query import DB
    rng = np.random.default_rng(12)
    n = 3000
    k = rng.integers(0, 11, n).astype(np.int64)
    kn = rng.random(n) < 0.05
    o = rng.permutation(n).astype(np.int64)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    vn = rng.random(n) < 0.1
    names = [None if rng.random() < 0.1 else "name%d" % rng.integers(0, 7) for _ in range(n)]
    t = 1577880000 + 86400 * rng.integers(0, 300, n).astype(np.int64)
    tn = rng.random(n) < 0.05
    pk = np.arange(n, dtype=np.int64)
    db = DB()
    db.execute("CREATE TABLE R (k INT, o INT, v INT, s VARCHAR(12), t DATE, pk INT PRIMARY KEY);")
    zero = np.zeros(n, dtype=np.uint8)
    db.append_columns("R", [k, o, v, names, t, pk], [kn.astype(np.uint8), zero, vn.astype(np.uint8), zero, tn.astype(np.uint8), zero])
    ks = np.array([0, 2, 4, 6, 8, 20], dtype=np.int64)
    w = ks * 10 + 1
    db.execute("CREATE TABLE S (ks INT, w INT);")
    db.append_columns("S", [ks, w])
    yield db, dict(n=n, k=k, kn=kn, o=o, v=v, vn=vn, s=names, t=t, tn=tn, pk=pk, ks=ks, w=w)
    db.close()


def rows_of(db, sql):
    res = db.query(sql, step_cursor=True)
    rows = [tuple(None if res.nulls[c][i] else (res.columns[c][i] if isinstance(res.columns[c][i], str) else int(res.columns[c][i]))
                  for c in range(len(res.names))) for i in range(res.nrows)]
    return res.names, res.types, rows


def model_rows(w, fns, part=True):
    out = N.nav_model([(w["k"], w["kn"], False)] if part else [], [(w["o"], None, False)], w["n"], fns)
    return [[None if nl[i] else int(vals[i]) for i in range(w["n"])] for vals, nl in out]


def test_sql_previous_reading_per_partition(world):
    db, w = world
    c0 = db.window_calls()
    names, types, rows = rows_of(db, "SELECT pk, v, LAG(v) OVER (PARTITION BY k ORDER BY o) AS prev, LEAD(v, 2, -7) OVER (PARTITION BY k ORDER BY o) AS nxt, "
                                     "NTILE(4) OVER (PARTITION BY k ORDER BY o) AS q, FIRST_VALUE(v) OVER (PARTITION BY k ORDER BY o) AS f, "
                                     "LAST_VALUE(v) OVER (PARTITION BY k ORDER BY o) AS l, ROW_NUMBER() OVER (PARTITION BY k ORDER BY o) AS rn FROM R;")
    assert db.window_calls() == c0 + 1                 # one OVER clause: one operator call for old and new functions together
    assert len(rows) == w["n"] and all(types[names.index(c)] == 1 for c in ("prev", "nxt", "q", "f", "l", "rn"))
    cell = (w["v"], w["vn"])
    prev, nxt, q, f, l = model_rows(w, [(N.LAG,) + cell + (1, None), (N.LEAD,) + cell + (2, -7), (N.NTILE, 4), (N.FIRST_VALUE,) + cell, (N.LAST_VALUE,) + cell])
    ix = {c: names.index(c) for c in ("R.pk", "R.v", "prev", "nxt", "q", "f", "l")}
    for r in rows:
        i = r[ix["R.pk"]]
        assert (r[ix["prev"]], r[ix["nxt"]], r[ix["q"]], r[ix["f"]], r[ix["l"]]) == (prev[i], nxt[i], q[i], f[i], l[i]), i
        # the previous-reading delta, where both readings exist
        if r[ix["R.v"]] is not None and r[ix["prev"]] is not None:
            assert r[ix["R.v"]] - r[ix["prev"]] == int(w["v"][i]) - prev[i]
    # names without an alias carry the offset where it is not 1
    names, _, _ = rows_of(db, "SELECT LAG(v) OVER (ORDER BY o), LEAD(R.v, 3) OVER (ORDER BY o), NTILE(2) OVER (ORDER BY o), LAST_VALUE(s) OVER (ORDER BY o) FROM R LIMIT 1;")
    assert sorted(names) == sorted(["LAG(R.v) OVER", "LEAD(R.v, 3) OVER", "NTILE(2) OVER", "LAST_VALUE(R.s) OVER"])


def test_sql_varchar_and_date_cells_decoded(world):
    db, w = world
    names, types, rows = rows_of(db, "SELECT pk, LAG(s) OVER (PARTITION BY k ORDER BY o) AS ps, LEAD(t) OVER (PARTITION BY k ORDER BY o) AS nt, "
                                     "FIRST_VALUE(s) OVER (ORDER BY o) AS fs FROM R;")
    from midoridb_amd.query import CT_VARCHAR
    assert types[names.index("ps")] == types[names.index("fs")] == CT_VARCHAR and types[names.index("nt")] == 4      # ... and DATE
    ids = {s: j for j, s in enumerate(sorted({x for x in w["s"] if x is not None}))}
    sid = np.array([ids.get(x, 0) for x in w["s"]], dtype=np.int64)
    sn = np.array([x is None for x in w["s"]])
    back = {j: s for s, j in ids.items()}
    ps, nt = model_rows(w, [(N.LAG, sid, sn, 1, None), (N.LEAD, w["t"], w["tn"], 1, None)])
    first = w["s"][int(np.argmin(w["o"]))]
    for r in rows:
        i = r[names.index("R.pk")]
        assert r[names.index("ps")] == (None if ps[i] is None else back[ps[i]]), i
        assert r[names.index("nt")] == nt[i], i
        assert r[names.index("fs")] == first


def test_sql_having_order_limit_and_distinct(world):
    db, w = world
    prev, = model_rows(w, [(N.LAG, w["v"], w["vn"], 1, None)])
    perm, b, pe, e = N.structure([(w["k"], w["kn"], False)], [(w["o"], None, False)], w["n"])
    heads = sorted(int(perm[p]) for p in range(w["n"]) if b[p] == p)
    # a partition's head has no previous row - and a row behind a NULL reading has a NULL one
    names, _, rows = rows_of(db, "SELECT pk, LAG(pk) OVER (PARTITION BY k ORDER BY o) AS prev FROM R HAVING prev IS NULL;")
    assert sorted(r[names.index("R.pk")] for r in rows) == heads and len(heads) == 12
    names, _, rows = rows_of(db, "SELECT pk, LAG(v) OVER (PARTITION BY k ORDER BY o) AS prev FROM R HAVING prev IS NOT NULL;")
    assert sorted(r[names.index("R.pk")] for r in rows) == [i for i in range(w["n"]) if prev[i] is not None]
    names, _, rows = rows_of(db, "SELECT pk, v, LAG(v) OVER (PARTITION BY k ORDER BY o) AS prev FROM R HAVING prev < v ORDER BY prev DESC, pk LIMIT 25;")
    want = sorted([(i, int(w["v"][i]), prev[i]) for i in range(w["n"]) if prev[i] is not None and not w["vn"][i] and prev[i] < w["v"][i]],
                  key=lambda r: (-r[2], r[0]))[:25]
    assert [(r[names.index("R.pk")], r[names.index("R.v")], r[names.index("prev")]) for r in rows] == want
    names, _, rows = rows_of(db, "SELECT DISTINCT NTILE(7) OVER (ORDER BY o) AS q FROM R ORDER BY q DESC;")
    assert [r[0] for r in rows] == [7, 6, 5, 4, 3, 2, 1]


def test_sql_over_a_left_join(world):
    """the NULL-supplied side's cells are "no row" cells: NULL to LAG, and not the default"""
    db, w = world
    names, _, rows = rows_of(db, "SELECT pk, w, LAG(w, 1, -1) OVER (ORDER BY pk) AS pw, LEAD(w, 1, -1) OVER (PARTITION BY ks ORDER BY pk) AS nw FROM R LEFT JOIN S ON k = ks;")
    assert len(rows) == w["n"]
    wcol = np.array([int(w["w"][list(w["ks"]).index(k)]) if (not kn and k in w["ks"]) else 0 for k, kn in zip(w["k"], w["kn"])], dtype=np.int64)
    wn = np.array([kn or k not in w["ks"] for k, kn in zip(w["k"], w["kn"])])
    assert wn.any() and not wn.all()
    out = N.nav_model([], [(w["pk"], None, False)], w["n"], [(N.LAG, wcol, wn, 1, -1)])
    pw = [None if out[0][1][i] else int(out[0][0][i]) for i in range(w["n"])]
    ksc = np.where(wn, 0, w["k"])
    out = N.nav_model([(ksc, wn, False)], [(w["pk"], None, False)], w["n"], [(N.LEAD, wcol, wn, 1, -1)])
    nw = [None if out[0][1][i] else int(out[0][0][i]) for i in range(w["n"])]
    for r in rows:
        i = r[names.index("R.pk")]
        assert (r[names.index("pw")], r[names.index("nw")]) == (pw[i], nw[i]), i
    assert pw[0] == -1 and None in pw



def test_sql_tinyint_cells_know_only_equal_and_not_equal():
    """a TINYINT column's cells through LAG compare as the column itself does: =, <> - every other operator is false for every row"""
    from midoridb_amd.query import DB
    with DB() as db:
        db.execute("CREATE TABLE T (o INT, b TINYINT);")
        db.execute("INSERT INTO T VALUES (1, FALSE), (2, TRUE), (3, FALSE), (4, TRUE);")
        def rows(sql):
            names, _, got = rows_of(db, sql)
            return sorted(r[names.index("T.o")] for r in got)
        assert rows("SELECT o, LAG(b) OVER (ORDER BY o) AS pb FROM T HAVING pb = FALSE;") == rows("SELECT o FROM T WHERE o = 2 OR o = 4;") == [2, 4]
        assert rows("SELECT o FROM T WHERE b < TRUE;") == [] == rows("SELECT o, LAG(b) OVER (ORDER BY o) AS pb FROM T HAVING pb < TRUE;")
        assert rows("SELECT o, LEAD(b, 1, FALSE) OVER (ORDER BY o) AS nb FROM T HAVING nb <> TRUE;") == [2, 4]
