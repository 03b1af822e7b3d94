"""LEFT / RIGHT [OUTER] JOIN on the device: the completion operator, "no row" (MDB_NO_ROW) in every operator that reads through a
row-id vector, and whole statements - rows AND their order.

There is no reference behaviour to compare with (upstream aborts on these join types): the expected rows come from the
restatement in this file - `nested_loop` (SQL's rules over Python lists: a pair is in the result when the whole ON expression is
true, NULL counting as false; a preserved row without pair appears once with the other side NULL; preserved side major) for
small tables, `np_left_equi` (numpy sort / searchsorted) for large ones, each checked against the other - and, for the small
two-table cases, from SQLite as a multiset of rows (its row order is unspecified; RIGHT JOIN needs SQLite 3.39, older ones get
the mirrored LEFT JOIN).
"""
import sqlite3

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_ROW = -1		# MDB_NO_ROW (0xFFFFFFFF) as it reads in an int32 tensor
KINDS = ["JOIN", "LEFT JOIN", "RIGHT JOIN", "LEFT OUTER JOIN", "RIGHT OUTER JOIN"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ---------------------------------------------------------------------------------------------- the restatement

def val(row, c):
    """cell c of a table's row in a joined tuple; a tuple without a row of that table (None) has NULL cells"""
    return None if row is None else row[c]


def lt(a, b):
    return a is not None and b is not None and a < b


def gt(a, b):
    return a is not None and b is not None and a > b


def eq(a, b):
    return a is not None and b is not None and a == b		# (floats: IEEE ==, so NaN equals nothing and -0.0 equals 0.0)


def nested_loop(S, T, on, kind, width=1):
    """S: list of tuples (each a list of `width` per-table rows or None), T: rows of the new table, on(tuple) -> bool"""
    out = []
    if kind.startswith("RIGHT"):
        for t in T:
            hit = [s + [t] for s in S if on(s + [t])]
            out += hit if hit else [[None] * width + [t]]
        return out
    for s in S:
        hit = [s + [t] for t in T if on(s + [t])]
        out += hit if hit else ([s + [None]] if kind.startswith("LEFT") else [])
    return out


def np_left_equi(ka, na, kb, nb):
    """LEFT JOIN ON ka = kb over integer keys (na / nb: NULL flags) -> (rows of A, rows of B or -1), A-major, B-minor"""
    vb = np.flatnonzero(~nb)
    order = vb[np.argsort(kb[vb], kind="stable")]
    sk = kb[order]
    lo = np.searchsorted(sk, ka, "left")
    hi = np.searchsorted(sk, ka, "right")
    deg = np.where(na, 0, hi - lo)
    reps = np.maximum(deg, 1)
    ia = np.repeat(np.arange(len(ka)), reps)
    start = np.cumsum(reps) - reps
    within = np.arange(len(ia)) - np.repeat(start, reps)
    pos = np.repeat(lo, reps) + within
    matched = np.repeat(deg > 0, reps)
    ib = np.full(len(ia), -1, dtype=np.int64)
    ib[matched] = order[pos[matched]]
    return ia, ib


def table_rows(cols, nulls):
    n = len(cols[0])
    return [tuple(None if nulls[c][i] else (cols[c][i].item() if hasattr(cols[c][i], "item") else cols[c][i]) for c in range(len(cols)))
            for i in range(n)]


def make_db(tables):
    """tables: {name: (ddl columns 'ka INT, xa INT', [numpy columns], [bool NULL flags])}"""
    from midoridb_amd.query import DB
    db = DB()
    for name, (decl, cols, nulls) in tables.items():
        db.execute(f"CREATE TABLE {name} ({decl});")
        if len(cols[0]):
            db.append_columns(name, cols, [np.asarray(x, dtype=np.uint8) for x in nulls])
    return db


def result_rows(db, sql):
    res = db.query(sql, step_cursor=True)
    rows = []
    for i in range(res.nrows):
        rows.append(tuple(None if res.nulls[c][i] else (res.columns[c][i] if isinstance(res.columns[c][i], str) else int(res.columns[c][i]))
                          for c in range(len(res.names))))
    return res.names, rows


def project(tuples, names, layout):
    """layout: {'A.ka': (table index in the tuple, column index)}; 'COUNT(*)' is not handled here"""
    return [tuple(val(tp[layout[n][0]], layout[n][1]) for n in names) for tp in tuples]


LAYOUT = {"A.ka": (0, 0), "A.xa": (0, 1), "B.kb": (1, 0), "B.xb": (1, 1), "C.kc": (2, 0), "C.xc": (2, 1)}


def rand_table(rng, n, domain, null_frac=0.2):
    k = rng.integers(0, domain, n, dtype=np.int64)
    x = rng.integers(0, 10, n, dtype=np.int64)
    return [k, x], [rng.random(n) < null_frac, rng.random(n) < null_frac]


def check_sqlite(tabs, sql, names, rows):
    """the same statement in SQLite, as a multiset of rows (two-table statements without GROUP BY / ORDER BY / LIMIT)"""
    con = sqlite3.connect(":memory:")
    for name, (decl, cols, nulls) in tabs.items():
        con.execute(f"CREATE TABLE {name} ({decl})")
        con.executemany(f"INSERT INTO {name} VALUES ({','.join('?' * len(cols))})", table_rows(cols, nulls))
    q = sql.replace(" OUTER ", " ")
    if " RIGHT JOIN " in q and sqlite3.sqlite_version_info < (3, 39):
        q = q.replace("FROM A RIGHT JOIN B", "FROM B LEFT JOIN A")
    sel = ", ".join(n.split(".")[1] for n in names)
    got = con.execute(q.replace("SELECT *", f"SELECT {sel}").rstrip(";")).fetchall()
    con.close()
    key = lambda r: tuple((0, 0) if v is None else (1, v) for v in r)	# noqa: E731
    assert sorted(got, key=key) == sorted(rows, key=key), sql


# ---------------------------------------------------------------------------------------------- 1. fails without the feature

def test_readme_tables_left_join_keeps_the_row_without_partner():
    from midoridb_amd.query import DB
    with DB() as db:
        db.execute("CREATE TABLE A (id_a INT);")
        db.execute("CREATE TABLE B (id_b INT);")
        db.execute("INSERT INTO A VALUES (1), (3), (4), (9);")
        db.execute("INSERT INTO B VALUES (3), (4), (5), (6);")
        names, rows = result_rows(db, "SELECT * FROM A LEFT JOIN B ON A.id_a = B.id_b;")
        assert sorted(names) == ["A.id_a", "B.id_b"]
        a, b = names.index("A.id_a"), names.index("B.id_b")
        assert [(r[a], r[b]) for r in rows] == [(1, None), (3, 3), (4, 4), (9, None)]
        names, rows = result_rows(db, "SELECT * FROM A RIGHT OUTER JOIN B ON A.id_a = B.id_b;")
        a, b = names.index("A.id_a"), names.index("B.id_b")
        assert [(r[a], r[b]) for r in rows] == [(3, 3), (4, 4), (None, 5), (None, 6)]
        # NULL cells read 0 through query_column_int64 / the bulk columns, as NULL cells always did
        bulk = db.query("SELECT * FROM A LEFT JOIN B ON A.id_a = B.id_b;")
        assert [int(v) for v in bulk.columns[bulk.names.index("B.id_b")]] == [0, 3, 4, 0]
        assert bulk.joined_rows == 4


# ---------------------------------------------------------------------------------------------- 2. the operator against numpy

def np_outer_complete(pp, po, n_p):
    un = np.setdiff1d(np.arange(n_p, dtype=np.int64), pp)
    allp = np.concatenate([pp.astype(np.int64), un])
    allo = np.concatenate([po.astype(np.int64), np.full(len(un), NO_ROW, dtype=np.int64)])
    order = np.argsort(allp, kind="stable")		# (a position is matched or unmatched, never both: the pairs keep their order)
    return allp[order], allo[order]


def run_outer_complete(dev, pp, po, n_p):
    d_p = dev.to_dev(pp.astype(np.int32)) if len(pp) else None
    d_o = dev.to_dev(po.astype(np.int32)) if len(pp) else None
    op, oo = dev.outer_complete(d_p, d_o, n_p)
    ep, eo = np_outer_complete(pp, po, n_p)
    assert np.array_equal(op.cpu().numpy().astype(np.int64), ep)
    assert np.array_equal(oo.cpu().numpy().astype(np.int64), eo)


def pairs_from_degrees(rng, deg):
    pp = np.repeat(np.arange(len(deg), dtype=np.int64), deg)
    return pp, rng.integers(0, 2**31 - 1, len(pp), dtype=np.int64)


@pytest.mark.parametrize("n_p", [1, 63, 64, 65, 4095, 4097, 2**20 + 1])
def test_outer_complete_sizes_and_boundaries(dev, n_p):
    rng = np.random.default_rng(n_p)
    e = np.zeros(0, dtype=np.int64)
    run_outer_complete(dev, e, e, n_p)						# J = 0: every row unmatched
    run_outer_complete(dev, *pairs_from_degrees(rng, np.ones(n_p, dtype=np.int64)), n_p)	# U = 0
    run_outer_complete(dev, *pairs_from_degrees(rng, np.arange(n_p) % 2), n_p)		# alternating
    run_outer_complete(dev, *pairs_from_degrees(rng, rng.integers(0, 4, n_p)), n_p)	# degrees 0 .. 3
    deg = np.zeros(n_p, dtype=np.int64)
    deg[n_p - 1] = 3										# one matched row at the very end
    run_outer_complete(dev, *pairs_from_degrees(rng, deg), n_p)


def test_outer_complete_runs_across_tile_boundaries(dev):
    rng = np.random.default_rng(7)
    n_p = 3 * 8192 + 100
    for lo, hi in ((60, 70), (4090, 4100), (1020, 1030), (8190, 8200), (0, 8192), (100, n_p)):	# unmatched runs over 64-, 1024-, 4096-, 8192-row bounds
        deg = rng.integers(1, 3, n_p)
        deg[lo:hi] = 0
        run_outer_complete(dev, *pairs_from_degrees(rng, deg), n_p)
    deg = np.zeros(5000, dtype=np.int64)
    deg[1234] = 10**6										# one row with 10^6 partners
    run_outer_complete(dev, *pairs_from_degrees(rng, deg), 5000)


def test_outer_complete_refuses_positions_that_are_not_ascending_or_out_of_range(dev):
    from midoridb_amd.dev import DeviceError
    for pp, n_p in (([3, 2, 5], 10), ([1, 2, 10], 10)):
        with pytest.raises(DeviceError):
            dev.outer_complete(dev.to_dev(np.array(pp, dtype=np.int32)), dev.to_dev(np.zeros(3, dtype=np.int32)), n_p)


def test_outer_complete_1e7_random_degrees(dev):
    rng = np.random.default_rng(11)
    n_p = 10**7
    run_outer_complete(dev, *pairs_from_degrees(rng, rng.integers(0, 4, n_p)), n_p)


def test_outer_complete_1e8_on_the_device(dev):
    """n_p = 10^8, J = 10^8: of every four rows one has two partners, two have one, one has none - compared on the device"""
    import torch
    n_p = 10**8
    i = torch.arange(n_p, dtype=torch.int32, device=dev.device)
    deg = torch.tensor([2, 1, 1, 0], dtype=torch.int64, device=dev.device).repeat(n_p // 4)
    pp = torch.repeat_interleave(i, deg)
    del deg, i
    J = pp.numel()
    assert J == n_p
    po = torch.arange(J, dtype=torch.int32, device=dev.device)
    op, oo = dev.outer_complete(pp, po, n_p)
    del pp, po
    k = torch.arange(J + n_p // 4, dtype=torch.int64, device=dev.device)
    g, w = k // 5, k % 5
    del k
    exp_p = (4 * g + torch.clamp(w - 1, min=0)).to(torch.int32)
    assert torch.equal(op, exp_p)
    del exp_p
    exp_o = torch.where(w == 4, torch.full_like(g, NO_ROW), 4 * g + w).to(torch.int32)
    assert torch.equal(oo, exp_o)


# ---------------------------------------------------------------------------------------------- 3. "no row" in every consumer

@pytest.mark.parametrize("with_bitmap", [False, True])
@pytest.mark.parametrize("absent", [False, True])
def test_no_row_in_every_operator_that_reads_through_row_ids(dev, with_bitmap, absent):
    from midoridb_amd import dev as D
    rng = np.random.default_rng(5 + with_bitmap + 2 * absent)
    n_src, n = 1000, 5000			# (5000 > 2048: the gathers' full-block form and their tail form both run)
    src = rng.integers(-50, 50, n_src, dtype=np.int64)
    src2 = rng.integers(0, 3, n_src, dtype=np.int64)
    srcd = rng.standard_normal(n_src)
    srcd[::7] = -0.0
    srcd[::11] = np.nan
    snull = rng.random(n_src) < 0.2 if with_bitmap else np.zeros(n_src, dtype=bool)
    idx = rng.integers(0, n_src, n, dtype=np.int64)
    gone = np.zeros(n, dtype=bool)
    if absent:
        gone[[0, 63, 64, 2047, 2048, n - 1]] = True
        gone[rng.integers(0, n, 40)] = True
    idx32 = np.where(gone, NO_ROW, idx).astype(np.int32)
    safe = np.where(gone, 0, idx)
    e_null = gone | snull[safe]
    e_val = np.where(gone, 0, src[safe])
    d_src, d_src2, d_srcd = dev.to_dev(src), dev.to_dev(src2), dev.to_dev(srcd)
    d_nb = dev.nullbits_dev(snull) if with_bitmap else None
    d_idx = dev.to_dev(idx32)

    v, nb = dev.gather64(d_src, d_nb, d_idx, n, dst_nulls=True)
    assert np.array_equal(v.cpu().numpy(), e_val)
    assert np.array_equal(D.unpack_nullbits(nb.cpu().numpy().view(np.uint64), n), e_null)
    (v, nb), (v2, nb2) = dev.gather_cols([(d_src, d_nb, d_idx), (d_src2, None, d_idx)], n, dst_nulls=True)
    assert np.array_equal(v.cpu().numpy(), e_val) and np.array_equal(v2.cpu().numpy(), np.where(gone, 0, src2[safe]))
    assert np.array_equal(D.unpack_nullbits(nb.cpu().numpy().view(np.uint64), n), e_null)
    assert np.array_equal(D.unpack_nullbits(nb2.cpu().numpy().view(np.uint64), n), gone)
    if not absent:		# the existing forms: no destination bitmap without a source bitmap
        v, nb = dev.gather64(d_src, d_nb, d_idx, n)
        assert np.array_equal(v.cpu().numpy(), src[idx]) and (nb is None) == (not with_bitmap)
    src32 = rng.integers(0, 2**31 - 1, n_src, dtype=np.int64).astype(np.int32)
    assert np.array_equal(dev.gather32(dev.to_dev(src32), d_idx).cpu().numpy(), np.where(gone, NO_ROW, src32[safe]))

    kv, kn = dev.double_join_keys(d_srcd, d_nb, d_idx)
    dv = srcd[safe]
    e_kn = e_null | np.isnan(dv)
    assert np.array_equal(D.unpack_nullbits(kn.cpu().numpy().view(np.uint64), n), e_kn)
    e_bits = np.where(gone, 0.0, np.where(dv == 0, 0.0, dv)).view(np.int64)
    assert np.array_equal(kv.cpu().numpy()[~e_kn], e_bits[~e_kn])

    sel = dev.filter([(D.P_ISNULL, 0, D.T_INT64, 0, 0, 0)], [(d_src, d_nb, d_idx)], n)
    assert np.array_equal(sel.cpu().numpy(), np.flatnonzero(e_null))
    sel = dev.filter([(D.P_CMP_COL_CONST, D.CMP_GE, D.T_INT64, 0, 0, 0)], [(d_src, d_nb, d_idx)], n)
    assert np.array_equal(sel.cpu().numpy(), np.flatnonzero(~e_null & (e_val >= 0)))

    # ORDER BY: NULL (and "no row") before every value ASC, behind every value DESC; ties keep the stream order
    for desc in (False, True):
        rank = np.where(e_null, -10**6, e_val)
        e_perm = np.argsort(-rank if desc else rank, kind="stable")
        perm = dev.sort_perm([(d_src, d_nb, d_idx, D.T_INT64, desc)], n)
        assert np.array_equal(perm.cpu().numpy(), e_perm)
        top, _ = dev.topk_perm([(d_src, d_nb, d_idx, D.T_INT64, desc)], n, 9)
        assert np.array_equal(top.cpu().numpy(), e_perm[:9])
    # DISTINCT / GROUP BY over two columns: NULL = NULL, first occurrences ascending
    keys2 = [(None if e_null[i] else int(e_val[i]), None if gone[i] else int(src2[safe[i]])) for i in range(n)]
    first, count = {}, {}
    for i, k in enumerate(keys2):
        first.setdefault(k, i)
        count[k] = count.get(k, 0) + 1
    e_first = sorted(first.values())
    two = [(d_src, d_nb, d_idx, D.T_INT64, False), (d_src2, None, d_idx, D.T_INT64, False)]
    assert dev.distinct_sel(two, n).cpu().numpy().tolist() == e_first
    f, c = dev.group_count_multi(two, n)
    assert f.cpu().numpy().tolist() == e_first
    assert c.cpu().numpy().tolist() == [count[keys2[i]] for i in e_first]


# ---------------------------------------------------------------------------------------------- 4. statements

ON_SHAPES = [
    ("ka = kb", lambda t: eq(val(t[0], 0), val(t[1], 0))),
    ("ka = kb AND xb > 5", lambda t: eq(val(t[0], 0), val(t[1], 0)) and gt(val(t[1], 1), 5)),
    ("ka = kb AND xa > 5", lambda t: eq(val(t[0], 0), val(t[1], 0)) and gt(val(t[0], 1), 5)),
    ("ka = kb AND xa < xb", lambda t: eq(val(t[0], 0), val(t[1], 0)) and lt(val(t[0], 1), val(t[1], 1))),
    ("1 = 1", lambda t: True),
    ("xa < xb", lambda t: lt(val(t[0], 1), val(t[1], 1))),
]


def two_table_statements(db, tabs, A, B, kind, on_sql, on, sqlite_too):
    S = [[a] for a in A]
    J = nested_loop(S, B, on, kind)
    base = f"FROM A {kind} B ON {on_sql}"
    names, rows = result_rows(db, f"SELECT * {base};")
    assert rows == project(J, names, LAYOUT), base
    if sqlite_too:
        check_sqlite(tabs, f"SELECT * {base};", names, rows)
    null_side = "ka" if kind.startswith("RIGHT") else "kb"
    nidx = LAYOUT["A.ka" if null_side == "ka" else "B.kb"]
    # WHERE runs after the join: the anti-join, and a conjunct over the NULL-supplied table that must not go below the join
    names, rows = result_rows(db, f"SELECT * {base} WHERE {null_side} IS NULL;")
    assert rows == project([t for t in J if val(t[nidx[0]], 0) is None], names, LAYOUT), base
    xcol, xi = ("xa", 0) if kind.startswith("RIGHT") else ("xb", 1)
    names, rows = result_rows(db, f"SELECT * {base} WHERE {xcol} = 3;")
    assert rows == project([t for t in J if eq(val(t[xi], 1), 3)], names, LAYOUT), base
    if sqlite_too:
        check_sqlite(tabs, f"SELECT * {base} WHERE {xcol} = 3;", names, rows)
    # GROUP BY a column + COUNT(*): groups in first-occurrence order, NULL one group; HAVING
    for gcol, gi in (("ka", (0, 0)), ("kb", (1, 0))):
        first, cnt = [], {}
        for t in J:
            k = val(t[gi[0]], gi[1])
            if k not in cnt:
                first.append(k)
            cnt[k] = cnt.get(k, 0) + 1
        names, rows = result_rows(db, f"SELECT {gcol}, COUNT(*) {base} GROUP BY {gcol};")
        ci, ki = names.index("COUNT(*)"), 1 - names.index("COUNT(*)")
        assert [(r[ki], r[ci]) for r in rows] == [(k, cnt[k]) for k in first], (base, gcol)
        names, rows = result_rows(db, f"SELECT {gcol}, COUNT(*) {base} GROUP BY {gcol} HAVING COUNT(*) > 1;")
        assert [(r[ki], r[ci]) for r in rows] == [(k, cnt[k]) for k in first if cnt[k] > 1], (base, gcol)
    # DISTINCT: first occurrences in order
    names, rows = result_rows(db, f"SELECT DISTINCT xa, xb {base};")
    seen, exp = set(), []
    for r in project(J, names, LAYOUT):
        if r not in seen:
            seen.add(r)
            exp.append(r)
    assert rows == exp, base
    # ORDER BY a NULL-supplied column: NULL first ASC, last DESC, ties in stream order; with LIMIT
    for desc in (False, True):
        names, rows = result_rows(db, f"SELECT * {base} ORDER BY {xcol}{' DESC' if desc else ''} LIMIT 7;")
        rank = [(-1 if val(t[xi], 1) is None else val(t[xi], 1)) for t in J]
        order = sorted(range(len(J)), key=lambda i: -rank[i] if desc else rank[i])
        assert rows == project([J[i] for i in order[:7]], names, LAYOUT), (base, desc)


@pytest.mark.parametrize("seed", range(40))
def test_random_small_tables_every_shape(seed):
    rng = np.random.default_rng(1000 + seed)
    big = seed % 10 == 9
    na, nb_ = (int(rng.integers(100, 201)), int(rng.integers(100, 201))) if big else (int(rng.integers(0, 40)), int(rng.integers(0, 40)))
    if seed == 3:
        na = 0		# empty S
    if seed == 4:
        nb_ = 0		# empty T
    dom = int(rng.integers(3, 51))
    ac, an = rand_table(rng, na, dom)
    bc, bn = rand_table(rng, nb_, dom)
    tabs = {"A": ("ka INT, xa INT", ac, an), "B": ("kb INT, xb INT", bc, bn)}
    A, B = table_rows(ac, an), table_rows(bc, bn)
    # the numpy restatement against the nested loop
    ia, ib = np_left_equi(ac[0], an[0], bc[0], bn[0])
    J = nested_loop([[a] for a in A], B, ON_SHAPES[0][1], "LEFT JOIN")
    assert [(A[i], B[j] if j >= 0 else None) for i, j in zip(ia, ib)] == [(t[0], t[1]) for t in J]
    db = make_db(tabs)
    try:
        kind = KINDS[1 + seed % 4]
        shapes = ON_SHAPES if not big else ON_SHAPES[:4]
        for k, (on_sql, on) in enumerate(shapes):
            if (k + seed) % 2 == 0 or k == 0:
                two_table_statements(db, tabs, A, B, kind, on_sql, on, sqlite_too=True)
            else:
                names, rows = result_rows(db, f"SELECT * FROM A {kind} B ON {on_sql};")
                assert rows == project(nested_loop([[a] for a in A], B, on, kind), names, LAYOUT), (kind, on_sql)
        if seed < 20:
            # 5. inner joins are untouched: where every A row has a partner, A LEFT JOIN B is A JOIN B row for row
            full_b = [np.arange(dom, dtype=np.int64).repeat(2), rng.integers(0, 10, 2 * dom, dtype=np.int64)]
            a2 = [ac[0], ac[1]]
            db.execute("CREATE TABLE D (kd INT, xd INT);")
            db.execute("CREATE TABLE E (ke INT, xe INT);")
            if na:
                db.append_columns("D", a2, [np.zeros(na, dtype=np.uint8), np.asarray(an[1], dtype=np.uint8)])
            db.append_columns("E", full_b, None)
            _, inner = result_rows(db, "SELECT * FROM D JOIN E ON kd = ke;")
            _, outer = result_rows(db, "SELECT * FROM D LEFT JOIN E ON kd = ke;")
            assert inner == outer and len(inner) == 2 * na
    finally:
        db.close()


@pytest.mark.parametrize("j1,j2", [(a, b) for a in KINDS[:3] for b in KINDS[:3] if (a, b) != ("JOIN", "JOIN")])
def test_three_tables_mixing_join_types(j1, j2):
    rng = np.random.default_rng(KINDS.index(j1) * 3 + KINDS.index(j2))
    cols = {n: rand_table(rng, int(rng.integers(5, 25)), 8) for n in "ABC"}
    tabs = {"A": ("ka INT, xa INT",) + cols["A"], "B": ("kb INT, xb INT",) + cols["B"], "C": ("kc INT, xc INT",) + cols["C"]}
    A, B, C = (table_rows(*cols[n]) for n in "ABC")
    S = nested_loop([[a] for a in A], B, lambda t: eq(val(t[0], 0), val(t[1], 0)), j1)
    # (a key cell that an earlier outer join NULL-supplied never matches)
    S = nested_loop(S, C, lambda t: eq(val(t[1], 0), val(t[2], 0)), j2, width=2)
    db = make_db(tabs)
    try:
        names, rows = result_rows(db, f"SELECT * FROM A {j1} B ON ka = kb {j2} C ON kb = kc;")
        assert rows == project(S, names, LAYOUT)
        names, rows = result_rows(db, f"SELECT * FROM A {j1} B ON ka = kb {j2} C ON kb = kc WHERE xa > 2 AND xc < 8;")
        assert rows == project([t for t in S if gt(val(t[0], 1), 2) and lt(val(t[2], 1), 8)], names, LAYOUT)
    finally:
        db.close()


def test_double_and_varchar_keys():
    da = np.array([0.0, -0.0, 1.5, np.nan, 2.5, 7.0])
    dbv = np.array([-0.0, 1.5, 1.5, np.nan, 3.0])
    tabs = {"A": ("ka DOUBLE, xa INT", [da, np.arange(6, dtype=np.int64)], [np.zeros(6, bool), np.zeros(6, bool)]),
            "B": ("kb DOUBLE, xb INT", [dbv, np.arange(5, dtype=np.int64)], [np.array([0, 0, 0, 0, 1], bool), np.zeros(5, bool)])}
    db = make_db(tabs)
    try:
        for kind in KINDS[1:]:
            A = [(float(da[i]), i) for i in range(6)]
            B = [(None if i == 4 else float(dbv[i]), i) for i in range(5)]
            J = nested_loop([[a] for a in A], B, ON_SHAPES[0][1], kind)
            names, rows = result_rows(db, f"SELECT xa, xb FROM A {kind} B ON ka = kb;")
            assert rows == project(J, names, LAYOUT), kind
    finally:
        db.close()
    from midoridb_amd.query import DB
    with DB() as db:
        db.execute("CREATE TABLE A (ka VARCHAR(8), xa INT);")
        db.execute("CREATE TABLE B (kb VARCHAR(8), xb INT);")
        db.execute("INSERT INTO A VALUES ('x', 1), ('y', 2), (NULL, 3), ('z', 4), ('y', 5);")
        db.execute("INSERT INTO B VALUES ('y', 10), ('w', 11), (NULL, 12), ('y', 13);")
        A = [("x", 1), ("y", 2), (None, 3), ("z", 4), ("y", 5)]
        B = [("y", 10), ("w", 11), (None, 12), ("y", 13)]
        for kind in KINDS[1:]:
            J = nested_loop([[a] for a in A], B, ON_SHAPES[0][1], kind)
            names, rows = result_rows(db, f"SELECT * FROM A {kind} B ON ka = kb;")
            assert rows == project(J, names, LAYOUT), kind


def test_inner_join_plans_are_what_they_were():
    """the inner join's shortcuts are still taken, and only by it: a primary key joined to a complete primary key, only the key
    columns read, is not joined at all (tests/test_query_gpu.py, join elimination, case key_columns_only); the same statement
    as a LEFT JOIN may not assume a partner - it runs the join and gives the same rows"""
    from midoridb_amd.query import DB
    rng = np.random.default_rng(4242)
    n = 50_000
    ka, kb = rng.permutation(n).astype(np.int64) + 7, rng.permutation(n).astype(np.int64) + 7
    with DB() as db:
        db.execute("CREATE TABLE A (id_a INT, fa INT);")
        db.execute("CREATE TABLE B (id_b INT PRIMARY KEY, fb INT);")
        db.append_columns("A", [ka, ka * 2])
        db.append_columns("B", [kb, kb * 3])
        before = db.joins_eliminated()
        inner = db.query("SELECT id_a, id_b FROM A INNER JOIN B ON A.id_a = B.id_b;")
        assert db.joins_eliminated() == before + 1
        outer = db.query("SELECT id_a, id_b FROM A LEFT JOIN B ON A.id_a = B.id_b;")
        assert db.joins_eliminated() == before + 1
        assert inner.names == outer.names and outer.joined_rows == n
        for c in range(2):
            assert np.array_equal(inner.columns[c], outer.columns[c]) and np.array_equal(inner.columns[c], ka)


def test_left_join_1e7_rows_half_of_the_left_keys_without_partner():
    n = 10**7
    ka = np.arange(n, dtype=np.int64)
    ka[1::2] += 3 * n				# every second key lies outside B's range
    kb = np.arange(n, dtype=np.int64) + 1	# (no key 0: a 0 in the bulk column is a NULL cell)
    z = np.zeros(n, dtype=bool)
    ia, ib = np_left_equi(ka, z, kb, z)
    db = make_db({"A": ("ka INT", [ka], [z]), "B": ("kb INT", [kb], [z])})
    try:
        res = db.query("SELECT ka, kb FROM A LEFT JOIN B ON ka = kb;")
        assert res.joined_rows == n
        assert np.array_equal(res.columns[res.names.index("A.ka")], ka[ia])
        assert np.array_equal(res.columns[res.names.index("B.kb")], np.where(ib >= 0, kb[np.maximum(ib, 0)], 0))
    finally:
        db.close()


def test_sharded_mode_refuses_outer_joins():
    """at world 2 on one GPU (the test transport of tests/_dist_gpu_worker.py): every rank gets the refusal, before any exchange"""
    from tests.test_dist_gpu import _run
    out = _run("outer", 2, 29631, worker="_outer_join_dist_worker.py", timeout=300)
    assert "sharded outer join refused ok" in out
