"""FULL [OUTER] JOIN on the device: the completion operator's second half (mdb_dev_outer_complete_full: the other side's positions that
no pair names, behind the LEFT completion) and whole statements - rows AND their order.

The expected rows come from the restatement in this file: `join` is SQL's rule over Python lists (a pair is in the result when the
whole ON expression is true, NULL counting as false; S-major; a row of S without a pair once with T absent; for FULL, T's rows without
a pair follow in T's row order with S absent).  Three more witnesses for the two-table cases: the same statement as LEFT JOIN followed
by the A-less rows of the RIGHT JOIN (the product's own, older paths), SQLite from 3.39 on as a multiset of rows, and numpy for the
large case."""
import sqlite3

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_ROW = -1		# MDB_NO_ROW (0xFFFFFFFF) as it reads in an int32 tensor
SPELLINGS = ["FULL JOIN", "FULL OUTER JOIN"]
OUTER_CHUNK = 8192	# pairs per workgroup of the kernels that read the pairs (mdb_dev_outer.hip)
OUTER_SPAN = 16384	# positions of the other side per workgroup of outer_unmatched / outer_tail


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ---------------------------------------------------------------------------------------------- 1. the operator against numpy

def run_full(dev, pp, po, n_p, n_o, offset=0):
    """offset: the pair columns start that many elements into their buffers (1: not 16-byte aligned, the scalar-load path)"""
    import torch
    J = len(pp)
    d_p = d_o = None
    if J:
        d_p = dev.to_dev(np.concatenate([np.zeros(offset, np.int64), pp]).astype(np.int32))[offset:]
        d_o = dev.to_dev(np.concatenate([np.zeros(offset, np.int64), po]).astype(np.int32))[offset:]
        assert d_p.data_ptr() % 16 == (4 * offset) % 16
    op, oo, uo = dev.outer_complete_full(d_p, d_o, n_p, n_o)
    un = np.setdiff1d(np.arange(n_o, dtype=np.int64), po)
    assert uo == len(un)
    if n_p:
        lp, lo = dev.outer_complete(d_p, d_o, n_p)
    else:
        lp = lo = torch.empty(0, dtype=torch.int32, device=dev.device)
    head = lp.numel()
    assert op.numel() == oo.numel() == head + len(un)
    assert torch.equal(op[:head], lp) and torch.equal(oo[:head], lo)		# the LEFT completion, byte for byte
    assert np.array_equal(oo[head:].cpu().numpy().astype(np.int64), un)
    assert bool((op[head:] == NO_ROW).all())
    return uo


def some_pairs(rng, n_p, J, o_values):
    """J pairs over n_p preserved positions (ascending, repeats and gaps), partners drawn from o_values in no order"""
    pp = np.sort(rng.integers(0, n_p, J, dtype=np.int64))
    return pp, rng.choice(np.asarray(o_values, dtype=np.int64), J)


@pytest.mark.parametrize("n_o", [0, 1, 63, 64, 65])
def test_no_pairs_every_position_of_both_sides_is_unmatched(dev, n_o):
    e = np.zeros(0, dtype=np.int64)
    assert run_full(dev, e, e, 37, n_o) == n_o


def test_empty_preserved_side_gives_the_tail_alone(dev):
    e = np.zeros(0, dtype=np.int64)
    assert run_full(dev, e, e, 0, 5) == 5
    op, oo, uo = dev.outer_complete_full(None, None, 0, 0)
    assert op.numel() == 0 and oo.numel() == 0 and uo == 0


@pytest.mark.parametrize("n_o", [63, 64, 65, 4095, 4097, OUTER_SPAN + 1])
def test_sizes_at_the_word_tile_and_span_boundaries(dev, n_o):
    rng = np.random.default_rng(n_o)
    n_p = 1000
    evens = np.arange(0, n_o, 2, dtype=np.int64)
    po = rng.permutation(np.concatenate([evens, rng.choice(evens, 100)]))
    assert run_full(dev, np.sort(rng.integers(0, n_p, len(po), dtype=np.int64)), po, n_p, n_o) == n_o // 2	# every second position named
    run_full(dev, *some_pairs(rng, n_p, 500, np.arange(n_o)), n_p, n_o)					# random
    pp = np.sort(rng.integers(0, n_p, n_o, dtype=np.int64))
    assert run_full(dev, pp, rng.permutation(n_o).astype(np.int64), n_p, n_o) == 0				# every o matched
    assert run_full(dev, pp[:9], np.full(9, n_o - 1, dtype=np.int64), n_p, n_o) == n_o - 1			# all pairs name one o: the last
    assert run_full(dev, pp[:9], np.zeros(9, dtype=np.int64), n_p, n_o) == n_o - 1				# ... the first
    # no o matched that a larger other side has: the pairs name the lower half only
    assert run_full(dev, *some_pairs(rng, n_p, 2 * n_o, np.arange(n_o)), n_p, 2 * n_o) >= n_o


def test_one_pair_more_than_a_workgroups_chunk_and_unaligned_pair_columns(dev):
    rng = np.random.default_rng(8193)
    n_p, n_o = 5000, 3 * OUTER_SPAN + 17
    pp, po = some_pairs(rng, n_p, OUTER_CHUNK + 1, np.arange(n_o))
    po[-1] = n_o - 1							# (the pair of the second workgroup names the last position)
    po[:-1] = np.minimum(po[:-1], n_o - 2)
    uo = run_full(dev, pp, po, n_p, n_o)
    assert uo == n_o - len(np.unique(po))
    assert run_full(dev, pp, po, n_p, n_o, offset=1) == uo		# a view one element into its buffer: 4-byte loads
    assert run_full(dev, pp[:5], po[:5], n_p, n_o, offset=1) == n_o - len(np.unique(po[:5]))


def test_a_partner_position_outside_the_other_side_is_refused(dev):
    from midoridb_amd.dev import DeviceError
    n_p, n_o = 10, 7
    for po in ([0, 7, 1], [2**31 - 1, 0, 0], [0, 0, -1]):	# n_o itself, far outside, MDB_NO_ROW
        with pytest.raises(DeviceError) as ei:
            dev.outer_complete_full(dev.to_dev(np.array([1, 2, 5], dtype=np.int32)), dev.to_dev(np.array(po, dtype=np.int32)), n_p, n_o)
        assert "not below 7" in str(ei.value), str(ei.value)
    with pytest.raises(DeviceError):				# pairs over an empty other side
        dev.outer_complete_full(dev.to_dev(np.array([1], dtype=np.int32)), dev.to_dev(np.array([0], dtype=np.int32)), n_p, 0)
    for pp in ([3, 2, 5], [1, 2, 10]):				# what the LEFT completion refuses is refused here too
        with pytest.raises(DeviceError):
            dev.outer_complete_full(dev.to_dev(np.array(pp, dtype=np.int32)), dev.to_dev(np.zeros(3, dtype=np.int32)), n_p, n_o)
    e = np.zeros(0, dtype=np.int64)
    assert run_full(dev, e, e, n_p, n_o) == n_o			# the context works on


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


def join(S, T, on, kind, width=1):
    """S: list of tuples (each a list of `width` per-table rows or None), T: rows of the new table, on(tuple) -> bool"""
    out = []
    if kind.startswith("RIGHT"):
        for t in T:
            hit = [s + [t] for s in S if on(s + [t])]
            out += hit if hit else [[None] * width + [t]]
        return out
    matched = [False] * len(T)
    for s in S:
        hit = [j for j, t in enumerate(T) if on(s + [t])]
        for j in hit:
            matched[j] = True
        out += [s + [T[j]] for j in hit]
        if not hit and kind != "JOIN":
            out.append(s + [None])
    if kind.startswith("FULL"):
        out += [[None] * width + [t] for j, t in enumerate(T) if not matched[j]]
    return out


def table_rows(cols, nulls):
    n = len(cols[0])
    return [tuple(None if nulls[c][i] else (cols[c][i].item() if hasattr(cols[c][i], "item") else cols[c][i]) for c in range(len(cols)))
            for i in range(n)]


def make_db(tables):
    """tables: {name: (ddl columns 'ka INT, xa INT, ia INT', [numpy columns], [bool NULL flags])}"""
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


# every table: a key k?, a value x?, and i? = its row number, never NULL (a tuple has no row of the table exactly where i? is NULL)
LAYOUT = {f"{T}.{c}{T.lower()}": (ti, ci) for ti, T in enumerate("ABC") for ci, c in enumerate("kxi")}


def project(tuples, names):
    return [tuple(val(tp[LAYOUT[n][0]], LAYOUT[n][1]) for n in names) for tp in tuples]


def rand_table(rng, n, domain, null_frac=0.2):
    k = rng.integers(0, domain, n, dtype=np.int64)
    x = rng.integers(0, 10, n, dtype=np.int64)
    z = np.zeros(n, dtype=bool)
    return [k, x, np.arange(n, dtype=np.int64)], [rng.random(n) < null_frac, rng.random(n) < null_frac, z]


def int_tables(rng, sizes, domain):
    cols = {T: rand_table(rng, n, domain) for T, n in zip("ABC", sizes)}
    tabs = {T: (f"k{T.lower()} INT, x{T.lower()} INT, i{T.lower()} INT",) + cols[T] for T in cols}
    return tabs, [table_rows(*cols[T]) for T in cols]


def check_sqlite(tabs, sql, names, rows):
    """the same statement in SQLite, as a multiset of rows (FULL JOIN: from SQLite 3.39 on; older ones skip this comparison only)"""
    if sqlite3.sqlite_version_info < (3, 39):
        return
    con = sqlite3.connect(":memory:")
    for name, (decl, cols, nulls) in tabs.items():
        con.execute(f"CREATE TABLE {name} ({decl})")
        con.executemany(f"INSERT INTO {name} VALUES ({','.join('?' * len(cols))})", table_rows(cols, nulls))
    sel = ", ".join(n.split(".")[1] for n in names)
    got = con.execute("SELECT " + sel + " " + sql[sql.index("FROM"):].rstrip(";")).fetchall()
    con.close()
    key = lambda r: tuple((0, 0) if v is None else (1, v) for v in r)	# noqa: E731
    assert sorted(got, key=key) == sorted(rows, key=key), sql


def check_two_tables(db, tabs, A, B, on_sql, on, sel="*", sqlite_too=True):
    """both spellings against the restatement, rows and order; the identity with the LEFT and RIGHT joins; SQLite"""
    J = join([[a] for a in A], B, on, "FULL")
    for spelling in SPELLINGS:
        names, rows = result_rows(db, f"SELECT {sel} FROM A {spelling} B ON {on_sql};")
        assert rows == project(J, names), (spelling, on_sql)
    _, left = result_rows(db, f"SELECT {sel} FROM A LEFT JOIN B ON {on_sql};")
    rnames, right = result_rows(db, f"SELECT {sel} FROM A RIGHT JOIN B ON {on_sql};")
    assert rnames == names
    assert rows == left + [r for r in right if r[names.index("A.ia")] is None], on_sql
    if sqlite_too:
        check_sqlite(tabs, f"SELECT {sel} FROM A FULL JOIN B ON {on_sql};", names, rows)
    return J


ON_SHAPES = [
    ("ka = kb", lambda t: eq(val(t[0], 0), val(t[1], 0))),
    # conjuncts over one side alone decide matching: they make rows unmatched - on BOTH sides - and drop none
    ("ka = kb AND xa > 4 AND xb < 6", lambda t: eq(val(t[0], 0), val(t[1], 0)) and gt(val(t[0], 1), 4) and lt(val(t[1], 1), 6)),
    ("ka = kb AND xb > 5", lambda t: eq(val(t[0], 0), val(t[1], 0)) and gt(val(t[1], 1), 5)),
    ("ka < kb", lambda t: lt(val(t[0], 0), val(t[1], 0))),
    ("ka = kb AND xa = xb", lambda t: eq(val(t[0], 0), val(t[1], 0)) and eq(val(t[0], 1), val(t[1], 1))),		# a composite key
    ("1 = 1", lambda t: True),
]


# ---------------------------------------------------------------------------------------------- 2. statements

def test_readme_tables_full_join_keeps_the_rows_of_both_sides():
    from midoridb_amd.query import DB
    with DB() as db:
        db.execute("CREATE TABLE A (id_a INT);")
        db.execute("CREATE TABLE B (id_b INT);")
        db.execute("INSERT INTO A VALUES (1), (3), (4), (9);")
        db.execute("INSERT INTO B VALUES (3), (4), (5), (6);")
        for spelling in SPELLINGS:
            names, rows = result_rows(db, f"SELECT * FROM A {spelling} B ON A.id_a = B.id_b;")
            a, b = names.index("A.id_a"), names.index("B.id_b")
            assert [(r[a], r[b]) for r in rows] == [(1, None), (3, 3), (4, 4), (9, None), (None, 5), (None, 6)]
        bulk = db.query("SELECT * FROM A FULL JOIN B ON A.id_a = B.id_b;")
        assert bulk.joined_rows == 6


@pytest.mark.parametrize("seed,sizes", [(0, (23, 31)), (1, (40, 17)), (2, (0, 12)), (3, (12, 0)), (4, (0, 0)), (5, (1, 1)), (6, (300, 260))])
def test_two_tables_every_on_shape(seed, sizes):
    rng = np.random.default_rng(600 + seed)
    big = max(sizes) > 100
    tabs, (A, B) = int_tables(rng, sizes, 40 if big else int(rng.integers(3, 12)))
    db = make_db(tabs)
    try:
        for on_sql, on in ON_SHAPES[:5] if big else ON_SHAPES:		# (no 300 x 260 cross pairs through the Python loop and seven statements)
            check_two_tables(db, tabs, A, B, on_sql, on)
    finally:
        db.close()


def test_where_runs_after_the_join_on_either_side():
    """the push-down trap: a WHERE conjunct that reads one table filters the JOINED rows - below a FULL join it would turn the other
    side's partners into unmatched rows instead of dropping them"""
    rng = np.random.default_rng(77)
    tabs, (A, B) = int_tables(rng, (60, 50), 9)
    db = make_db(tabs)
    try:
        on_sql, on = ON_SHAPES[0]
        J = join([[a] for a in A], B, on, "FULL")
        for where, keep in [("xa = 3", lambda t: eq(val(t[0], 1), 3)), ("xb = 3", lambda t: eq(val(t[1], 1), 3)),
                            ("xa > 2 AND xb < 8", lambda t: gt(val(t[0], 1), 2) and lt(val(t[1], 1), 8)),
                            ("ka IS NULL", lambda t: val(t[0], 0) is None), ("ib IS NULL", lambda t: val(t[1], 2) is None),
                            ("ia IS NULL", lambda t: val(t[0], 2) is None)]:
            sql = f"SELECT * FROM A FULL JOIN B ON {on_sql} WHERE {where};"
            names, rows = result_rows(db, sql)
            assert rows == project([t for t in J if keep(t)], names), where
            check_sqlite(tabs, sql, names, rows)
        assert any(val(t[0], 2) is None for t in J) and any(val(t[1], 2) is None for t in J)	# (both kinds of unmatched rows are there)
    finally:
        db.close()


def test_group_by_order_by_distinct_and_count_over_a_full_join():
    rng = np.random.default_rng(78)
    tabs, (A, B) = int_tables(rng, (80, 70), 12)
    db = make_db(tabs)
    try:
        on_sql, on = ON_SHAPES[0]
        base = f"FROM A FULL JOIN B ON {on_sql}"
        J = join([[a] for a in A], B, on, "FULL")
        names, rows = result_rows(db, f"SELECT COUNT(*) {base};")
        assert rows == [(len(J),)]
        # GROUP BY a column that can be absent: groups in first-occurrence order, NULL cells and absent rows one group; the aggregates
        # skip NULL cells, a group without a value has NULL
        for gcol, (gt_, gc), acol, (at_, ac) in (("kb", (1, 0), "xa", (0, 1)), ("ka", (0, 0), "xb", (1, 1))):
            first, cells = [], {}
            for t in J:
                k = val(t[gt_], gc)
                if k not in cells:
                    first.append(k)
                cells.setdefault(k, []).append(val(t[at_], ac))
            exp = []
            for k in first:
                v = [c for c in cells[k] if c is not None]
                exp.append((k, len(cells[k]), sum(v) if v else None, min(v) if v else None))
            tab = "A" if acol == "xa" else "B"
            names, rows = result_rows(db, f"SELECT {gcol}, COUNT(*), SUM({acol}), MIN({acol}) {base} GROUP BY {gcol};")
            want = [f"{'B' if gcol == 'kb' else 'A'}.{gcol}", "COUNT(*)", f"SUM({tab}.{acol})", f"MIN({tab}.{acol})"]
            assert [tuple(r[names.index(w)] for w in want) for r in rows] == exp, gcol
        # ORDER BY a column that can be absent: NULL first ASC, last DESC, ties in stream order; with LIMIT
        for col, (ti, ci) in (("xa", (0, 1)), ("xb", (1, 1))):
            for desc in (False, True):
                names, rows = result_rows(db, f"SELECT * {base} ORDER BY {col}{' DESC' if desc else ''} LIMIT 9;")
                rank = [(-1 if val(t[ti], ci) is None else val(t[ti], ci)) for t in J]
                order = sorted(range(len(J)), key=lambda i: -rank[i] if desc else rank[i])
                assert rows == project([J[i] for i in order[:9]], names), (col, desc)
        names, rows = result_rows(db, f"SELECT DISTINCT xa, xb {base};")
        seen, exp = set(), []
        for r in project(J, names):
            if r not in seen:
                seen.add(r)
                exp.append(r)
        assert rows == exp
    finally:
        db.close()


@pytest.mark.parametrize("j1,j2", [("FULL JOIN", "LEFT JOIN"), ("LEFT JOIN", "FULL JOIN"), ("FULL JOIN", "FULL OUTER JOIN"), ("RIGHT JOIN", "FULL JOIN"),
                                   ("FULL OUTER JOIN", "RIGHT JOIN"), ("JOIN", "FULL JOIN"), ("FULL JOIN", "JOIN")])
def test_three_tables_full_joins_in_a_chain(j1, j2):
    rng = np.random.default_rng(len(j1) * 31 + len(j2))
    tabs, (A, B, C) = int_tables(rng, [int(rng.integers(5, 25)) for _ in range(3)], 8)
    S = join([[a] for a in A], B, lambda t: eq(val(t[0], 0), val(t[1], 0)), j1)
    # (a key cell that an earlier outer join NULL-supplied never matches)
    S2 = join(S, C, lambda t: eq(val(t[1], 0), val(t[2], 0)), j2, width=2)
    db = make_db(tabs)
    try:
        names, rows = result_rows(db, f"SELECT * FROM A {j1} B ON ka = kb {j2} C ON kb = kc;")
        assert rows == project(S2, names)
        names, rows = result_rows(db, f"SELECT * FROM A {j1} B ON ka = kb {j2} C ON kb = kc WHERE xa > 2 AND xc < 8;")
        assert rows == project([t for t in S2 if gt(val(t[0], 1), 2) and lt(val(t[2], 1), 8)], names)
        # the second ON reads all three tables, one conjunct per table besides the key
        S3 = join(S, C, lambda t: eq(val(t[0], 0), val(t[2], 0)) and gt(val(t[1], 1), 2) and lt(val(t[2], 1), 8), j2, width=2)
        names, rows = result_rows(db, f"SELECT * FROM A {j1} B ON ka = kb {j2} C ON ka = kc AND xb > 2 AND xc < 8;")
        assert rows == project(S3, names)
    finally:
        db.close()


def test_double_and_varchar_keys():
    da = np.array([0.0, -0.0, 1.5, np.nan, 2.5, 7.0])
    dbv = np.array([-0.0, 1.5, 1.5, np.nan, 3.0, 8.0])
    ia, ib = np.arange(6, dtype=np.int64), np.arange(6, dtype=np.int64)
    z = np.zeros(6, bool)
    tabs = {"A": ("ka DOUBLE, xa INT, ia INT", [da, ia + 10, ia], [z, z, z]),
            "B": ("kb DOUBLE, xb INT, ib INT", [dbv, ib + 20, ib], [np.array([0, 0, 0, 0, 1, 0], bool), z, z])}
    db = make_db(tabs)
    try:
        A = [(float(da[i]), i + 10, i) for i in range(6)]
        B = [(None if i == 4 else float(dbv[i]), i + 20, i) for i in range(6)]
        J = check_two_tables(db, tabs, A, B, "ka = kb", ON_SHAPES[0][1], sel="xa, xb, ia, ib", sqlite_too=False)
        assert len(J) == 4 + 3 + 3		# 0.0 and -0.0 with -0.0, 1.5 with 1.5 twice; NaN, 2.5, 7.0 of A and NaN, NULL, 8.0 of B without partner
    finally:
        db.close()
    from midoridb_amd.query import DB
    with DB() as db:
        db.execute("CREATE TABLE A (ka VARCHAR(8), xa INT, ia INT);")
        db.execute("CREATE TABLE B (kb VARCHAR(8), xb INT, ib INT);")
        db.execute("INSERT INTO A VALUES ('x', 1, 0), ('y', 2, 1), (NULL, 3, 2), ('z', 4, 3), ('y', 5, 4);")
        db.execute("INSERT INTO B VALUES ('y', 10, 0), ('w', 11, 1), (NULL, 12, 2), ('y', 13, 3);")
        A = [("x", 1, 0), ("y", 2, 1), (None, 3, 2), ("z", 4, 3), ("y", 5, 4)]
        B = [("y", 10, 0), ("w", 11, 1), (None, 12, 2), ("y", 13, 3)]
        J = check_two_tables(db, None, A, B, "ka = kb", ON_SHAPES[0][1], sqlite_too=False)
        assert len(J) == 4 + 3 + 2


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


def test_two_hundred_thousand_rows_a_side_against_numpy():
    """the operator's chunk, span and word boundaries through the SQL path: duplicates and NULL keys on both sides, rows of either
    side without partner"""
    rng = np.random.default_rng(200)
    na, nb = 200_003, 199_999
    ka, kb = rng.integers(0, 150_000, na, dtype=np.int64), rng.integers(50_000, 200_000, nb, dtype=np.int64)
    za, zb = rng.random(na) < 0.2, rng.random(nb) < 0.2
    ia, ib = np_left_equi(ka, za, kb, zb)
    small = np_left_equi(ka[:50], za[:50], kb[:60], zb[:60])	# the numpy restatement against the nested loop
    A, B = table_rows([ka[:50]], [za[:50]]), table_rows([kb[:60]], [zb[:60]])
    loop = join([[(a[0], None, i)] for i, a in enumerate(A)], [(b[0], None, j) for j, b in enumerate(B)], ON_SHAPES[0][1], "LEFT")
    assert [(t[0][2], -1 if t[1] is None else t[1][2]) for t in loop] == list(zip(small[0].tolist(), small[1].tolist()))
    un = np.setdiff1d(np.arange(nb), ib)
    ea = np.concatenate([ia + 1, np.zeros(len(un), dtype=np.int64)])		# row numbers from 1: a 0 in the bulk column is a NULL cell
    eb = np.concatenate([ib + 1, un + 1])
    f = lambda n: np.zeros(n, dtype=bool)	# noqa: E731
    db = make_db({"A": ("ka INT, ia INT", [ka, np.arange(na, dtype=np.int64) + 1], [za, f(na)]),
                  "B": ("kb INT, ib INT", [kb, np.arange(nb, dtype=np.int64) + 1], [zb, f(nb)])})
    try:
        res = db.query("SELECT ia, ib FROM A FULL JOIN B ON ka = kb;")
        assert res.joined_rows == len(ea) and len(un) > 1000 and int((ib < 0).sum()) > 1000
        assert np.array_equal(res.columns[res.names.index("A.ia")], ea)
        assert np.array_equal(res.columns[res.names.index("B.ib")], eb)
    finally:
        db.close()


def test_the_plan_record_names_the_full_join():
    """mdb_dev_plan_info.outer_form: 1 after a LEFT / RIGHT completion, 2 after a FULL one"""
    rng = np.random.default_rng(9)
    tabs, _ = int_tables(rng, (30, 30), 6)
    db = make_db(tabs)
    try:
        for kind, form in (("LEFT JOIN", 1), ("FULL JOIN", 2), ("RIGHT OUTER JOIN", 1), ("FULL OUTER JOIN", 2)):
            db.query(f"SELECT * FROM A {kind} B ON ka = kb;")
            assert db.last_plan()["outer_form"] == form, kind
    finally:
        db.close()


def test_sharded_mode_refuses_full_joins():
    """at world 2 on one GPU (the test transport of tests/_dist_gpu_worker.py): every rank gets the refusal, before any exchange"""
    from tests.test_dist_gpu import _run
    out = _run("full", 2, 29633, worker="_full_join_dist_worker.py", timeout=300)
    assert "sharded full join refused ok" in out
