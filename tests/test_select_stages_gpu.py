"""The SELECT executor's corners that no other test drives, pinned before the driver was split into plan stages (they pass unchanged on
the commit before the split):

  - the executor's own chain of fused join + GROUP BY + COUNT(*) calls for FIVE and SIX tables on one key (three and four tables are
    answered by one mdb_dev_join_group_count_multi call: test_query_gpu.py::test_chained_fused_plan_three_and_four_tables);
  - the projection's gather batch flushed in the middle of the column loop: more than MDB_GATHER_MAX_COLS = 16 gathered columns, more
    than MDB_GATHER_MAX_RIDS = 8 row-id vectors - with the result on the host and kept on the device;
  - one statement per arm of the plan dispatch, the arm asserted by what can be observed: mdb_dev_counters().operator_calls (the
    join / GROUP BY operators count themselves: the fused plan is ONE call where the general plan is a join and a GROUP BY),
    mdb_dev_last_plan, joined_rows, the catalog's counters.

Arms that existing tests assert already, not repeated here:
  - composite fused plan, by the mdb_database_composite_fused() delta: test_composite_fused_gpu.py (every statement of _check);
  - keys-only plan in the reference's order (the pre-step): test_query_gpu.py::test_join_of_two_key_columns_in_the_references_order_takes_the_primary_key_plan;
  - keys-only plan in any order, by its leaf order at 2.4 * 10^6 rows: test_query_gpu.py::test_join_of_two_key_columns_in_any_order_is_the_ordered_result_as_a_multiset
    (here: the same statement at a few hundred rows, results only);
  - GROUP BY on one field in its any-order keys form at 2.6 * 10^6 rows: test_query_gpu.py::test_single_table_group_by_in_any_order (here: small, results only);
  - the filter + project plan has nothing to observe but its rows: results only, beside the neighbour that LIMIT keeps out of it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")


def _calls(db):
    return db.counters()["operator_calls"]


# ---------------------------------------------------------------------------------------------- chained fused plan, 5 and 6 tables

def _chain_tables(db, ntabs, seed):
    """tables A, B, ... of 40-80 rows, key id_<t> in [0, 12) with about 5 % NULLs; D has a second column f in [-3, 6)"""
    rng = np.random.default_rng(seed)
    tabs = {}
    for t in "ABCDEF"[:ntabs]:
        n = int(rng.integers(40, 81))
        k = rng.integers(0, 12, n)
        nl = rng.random(n) < 0.05
        if t == "D":
            f = rng.integers(-3, 6, n)
            db.execute("CREATE TABLE D (id_d INT, f INT);")
            db.append_columns("D", [k, f], [nl, np.zeros(n, dtype=bool)])
            tabs[t] = (k, nl, f)
        else:
            db.execute(f"CREATE TABLE {t} (id_{t.lower()} INT);")
            db.append_columns(t, [k], [nl])
            tabs[t] = (k, nl, None)
    return tabs


def _chain_closed_form(tabs, keep_d=None):
    """[(key, COUNT)] in the order of the keys' first occurrence in A: a group's COUNT is the product of the per-table multiplicities
    of its key, NULL keys join nothing; keep_d: the rows of D that pass its WHERE conjunct"""
    mult = {}
    for t, (k, nl, _) in tabs.items():
        ok = ~nl if not (t == "D" and keep_d is not None) else (~nl & keep_d)
        mult[t] = np.bincount(k[ok], minlength=12)
    ka, na, _ = tabs["A"]
    out, seen = [], set()
    for i in range(len(ka)):
        key = int(ka[i])
        if na[i] or key in seen:
            continue
        seen.add(key)
        c = 1
        for t in tabs:
            c *= int(mult[t][key])
        if c:
            out.append((key, c))
    return out


def _chain_from(ntabs, on_other_tables=False):
    on = {"B": "A.id_a = B.id_b", "C": "A.id_a = C.id_c", "D": "A.id_a = D.id_d", "E": "E.id_e = A.id_a", "F": "A.id_a = F.id_f"}
    if on_other_tables:
        on.update({"C": "C.id_c = B.id_b", "D": "D.id_d = B.id_b", "E": "C.id_c = E.id_e", "F": "F.id_f = D.id_d"})
    return "A " + " ".join(f"INNER JOIN {t} ON {on[t]}" for t in "BCDEF"[:ntabs - 1])


@pytest.mark.parametrize("ntabs", [5, 6])
def test_chained_fused_plan_five_and_six_tables(ntabs):
    """the executor chains the two-table operator itself: one call per further table, COUNTs multiplied (mdb_dev_combine_counts)"""
    from midoridb_amd.query import DB
    with DB() as db:
        tabs = _chain_tables(db, ntabs, 500 + ntabs)
        want = _chain_closed_form(tabs)
        assert len(want) >= 6, want
        total = sum(c for _, c in want)
        for other in (False, True):
            frm = _chain_from(ntabs, other)
            c0 = _calls(db)
            r = db.query(f"SELECT id_a, COUNT(*) FROM {frm} GROUP BY id_a;")
            assert _calls(db) - c0 == ntabs - 1, "one fused operator call per joined table, no materialising join"
            assert r.names == ["A.id_a", "COUNT(*)"] and r.rows() == want, frm
            assert r.joined_rows == total
            one = db.query(f"SELECT COUNT(*) FROM {frm};")
            assert one.names == ["COUNT(*)"] and one.rows() == [(total,)] and one.joined_rows == total
        frm = _chain_from(ntabs)
        # a pushed single-table conjunct on the fourth table
        keep = tabs["D"][2] >= 0
        want_f = _chain_closed_form(tabs, keep)
        assert want_f != want and want_f
        c0 = _calls(db)
        r = db.query(f"SELECT id_a, COUNT(*) FROM {frm} WHERE f >= 0 GROUP BY id_a;")
        assert _calls(db) - c0 == ntabs - 1
        assert r.rows() == want_f and r.joined_rows == sum(c for _, c in want_f)
        assert db.query(f"SELECT COUNT(*) FROM {frm} WHERE f >= 0;").rows() == [(sum(c for _, c in want_f),)]
        # ... and one that empties it: no group, no row
        none = db.query(f"SELECT COUNT(*) FROM {frm} WHERE f < -100;")
        assert none.names == ["COUNT(*)"] and none.nrows == 0 and none.joined_rows == 0
        assert db.query(f"SELECT id_a, COUNT(*) FROM {frm} WHERE f < -100 GROUP BY id_a;").nrows == 0
        # the tail clauses over the chained stream
        cut = sorted(c for _, c in want)[len(want) // 2]
        r = db.query(f"SELECT id_a, COUNT(*) FROM {frm} GROUP BY id_a HAVING COUNT(*) > {cut} ORDER BY id_a DESC;")
        assert r.rows() == sorted([g for g in want if g[1] > cut], reverse=True) and 0 < r.nrows < len(want)


# ---------------------------------------------------------------------------------------------- projection gather batch overflow

def _wide_tables(db):
    """A (ka, a1 .. a11), B (kb, b1 .. b11), 200 and 190 rows, keys in [0, 60) on both sides, NULLs in a3, a7, b2, b9"""
    rng = np.random.default_rng(2024)
    data = {}
    for t, n in (("A", 200), ("B", 190)):
        p = t.lower()
        names = [f"k{p}"] + [f"{p}{i}" for i in range(1, 12)]
        cols = [rng.integers(0, 60, n)] + [rng.integers(-1000, 1000, n) for _ in range(11)]
        nulls = [np.zeros(n, dtype=bool) for _ in names]
        for nm in ("a3", "a7", "b2", "b9"):
            if nm in names:
                nulls[names.index(nm)] = rng.random(n) < 0.1
        db.execute(f"CREATE TABLE {t} ({', '.join(nm + ' INT' for nm in names)});")
        db.append_columns(t, cols, nulls)
        for nm, c, nl in zip(names, cols, nulls):
            data[f"{t}.{nm}"] = (np.asarray(c, dtype=np.int64), nl)
    return data


def _wide_expected(data, residual):
    """nested loop, A-major: {column name: (cells with 0 for NULL, NULL flags)}"""
    ka, kb = data["A.ka"][0], data["B.kb"][0]
    ia, ib = [], []
    for i in range(len(ka)):
        for j in range(len(kb)):
            if ka[i] == kb[j] and (not residual or data["A.a1"][0][i] < data["B.b1"][0][j]):
                ia.append(i)
                ib.append(j)
    ia, ib = np.array(ia), np.array(ib)
    out = {}
    for nm, (c, nl) in data.items():
        at = ia if nm.startswith("A.") else ib
        out[nm] = (np.where(nl[at], 0, c[at]), nl[at])
    return out


def _many_tables(db, ntabs):
    """TA (k_a, v_a), TB (k_b, v_b), ...: 8 rows each, keys 0 .. 5 once and two of them twice (one NULL payload cell per table)"""
    rng = np.random.default_rng(900 + ntabs)
    data, letters = {}, "abcdefghij"[:ntabs]
    for p in letters:
        k = rng.permutation(np.concatenate([np.arange(6), rng.integers(0, 6, 2)]))
        v = rng.integers(0, 100, 8)
        nl = np.zeros(8, dtype=bool)
        nl[int(rng.integers(0, 8))] = True
        db.execute(f"CREATE TABLE T{p.upper()} (k_{p} INT, v_{p} INT);")
        db.append_columns(f"T{p.upper()}", [k, v], [np.zeros(8, dtype=bool), nl])
        data[p] = (k.astype(np.int64), v.astype(np.int64), nl)
    return data, letters


def _many_sql(letters, where=""):
    return "SELECT * FROM TA " + " ".join(f"INNER JOIN T{p.upper()} ON TA.k_a = T{p.upper()}.k_{p}" for p in letters[1:]) + where + ";"


def _many_expected(data, letters, v0_min=None):
    """nested loop, table by table: the joined tuples so far x the next table's rows in its row order"""
    k0, v0, n0 = data["a"]
    tuples = [(i,) for i in range(8) if v0_min is None or (not n0[i] and v0[i] >= v0_min)]
    for p in letters[1:]:
        k = data[p][0]
        tuples = [tp + (j,) for tp in tuples for j in range(8) if k[j] == k0[tp[0]]]
    out = {}
    for x, p in enumerate(letters):
        k, v, nl = data[p]
        at = np.array([tp[x] for tp in tuples], dtype=np.int64)
        out[f"T{p.upper()}.k_{p}"] = (k[at], np.zeros(len(at), dtype=bool))
        out[f"T{p.upper()}.v_{p}"] = (np.where(nl[at], 0, v[at]), nl[at])
    return out


def _check_host(db, sql, want):
    r = db.query(sql, step_cursor=True)
    assert sorted(r.names) == sorted(want) and len(r.names) == len(want), sql
    rows = len(next(iter(want.values()))[0])
    assert r.nrows == rows and r.joined_rows == rows
    for c, nm in enumerate(r.names):
        assert np.array_equal(r.columns[c], want[nm][0]), (sql, nm)
        assert np.array_equal(r.nulls[c], want[nm][1]), (sql, nm)
    return rows


def _check_device(db, sql, want, key_names):
    db.results_on_device(True)
    try:
        names, _, cols, nrows, joined, _ = db.query_device(sql)
        nulls = db.last_device_nulls
    finally:
        db.results_on_device(False)
    rows = len(next(iter(want.values()))[0])
    assert sorted(names) == sorted(want) and nrows == rows and joined == rows
    for c, nm in enumerate(names):
        assert cols[c] is not None, (sql, nm)
        got = cols[c].cpu().numpy()
        flags = nulls[c].cpu().numpy() if nulls[c] is not None else np.zeros(rows, dtype=bool)
        assert np.array_equal(flags, want[nm][1]), (sql, nm)
        assert np.array_equal(got[~flags], want[nm][0][~flags]), (sql, nm)     # (a NULL's cell holds what the table stored)
    for nm in key_names:    # both sides' key columns of the equi-join are served, neither with a NULL
        c = names.index(nm)
        assert np.array_equal(cols[c].cpu().numpy(), want[nm][0]) and (nulls[c] is None or not bool(nulls[c].any())), nm


@pytest.fixture(scope="module")
def wide():
    from midoridb_amd.query import DB
    with DB() as db:
        data = _wide_tables(db)
        yield db, {False: _wide_expected(data, False), True: _wide_expected(data, True)}


@pytest.mark.parametrize("residual", [False, True], ids=["equi_join", "with_residual"])
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "kept_on_device"])
def test_projection_gathers_more_columns_than_one_batch_holds(wide, residual, on_device):
    """SELECT * over A JOIN B, twelve columns each: 23 columns gathered through two row-id vectors (B's key column is A's): the batch of
    MDB_GATHER_MAX_COLS = 16 is flushed once in the middle of the column loop"""
    db, want = wide
    sql = "SELECT * FROM A INNER JOIN B ON A.ka = B.kb" + (" AND A.a1 < B.b1;" if residual else ";")
    rows = len(want[residual]["A.ka"][0])
    assert len(want[residual]) == 24 and (rows > 400 if not residual else 100 < rows < len(want[False]["A.ka"][0]))
    if on_device:
        _check_device(db, sql, want[residual], ["A.ka", "B.kb"])
    else:
        _check_host(db, sql, want[residual])


@pytest.mark.parametrize("ntabs", [9, 10])
@pytest.mark.parametrize("shape", ["select_star", "first_table_filtered"])
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "kept_on_device"])
def test_projection_gathers_through_more_row_id_vectors_than_one_batch_holds(ntabs, shape, on_device):
    """nine and ten tables joined on the first one's key: every table has a row-id vector of its own, the batch of MDB_GATHER_MAX_RIDS = 8
    is flushed when the ninth comes; with a WHERE conjunct on the first table that one is read through row ids from the start"""
    from midoridb_amd.query import DB
    with DB() as db:
        data, letters = _many_tables(db, ntabs)
        v0_min = 30 if shape == "first_table_filtered" else None
        want = _many_expected(data, letters, v0_min)
        rows = len(want["TA.k_a"][0])
        assert 8 < rows < 5000, rows
        sql = _many_sql(letters, " WHERE v_a >= 30" if v0_min is not None else "")
        if on_device:
            _check_device(db, sql, want, ["TA.k_a", f"T{letters[-1].upper()}.k_{letters[-1]}"])
        else:
            _check_host(db, sql, want)


# ---------------------------------------------------------------------------------------------- one statement per arm of the dispatch

@pytest.fixture(scope="module")
def arms():
    from midoridb_amd.query import DB
    rng = np.random.default_rng(31)
    with DB() as db:
        n = 300
        ka, fa = rng.integers(0, 40, n), rng.integers(0, 10, n)
        kb = rng.integers(0, 50, 260)
        db.execute("CREATE TABLE A (id_a INT, fa INT);")
        db.execute("CREATE TABLE B (id_b INT);")
        db.append_columns("A", [ka, fa])
        db.append_columns("B", [kb])
        u = rng.permutation(n).astype(np.int64) * 7
        db.execute("CREATE TABLE U (u INT PRIMARY KEY, w INT);")      # (declared unique: measured whatever the table's size)
        db.append_columns("U", [u, fa])
        yield db, ka.astype(np.int64), fa.astype(np.int64), kb.astype(np.int64), u


def _first_occurrence_groups(*cols):
    seen, out = {}, []
    for row in zip(*(c.tolist() for c in cols)):
        if row not in seen:
            seen[row] = len(out)
            out.append([row, 0])
        out[seen[row]][1] += 1
    return [tuple(k) + (c,) for k, c in out]


def test_arm_single_key_fused_plan(arms):
    db, ka, fa, kb, _ = arms
    mb = np.bincount(kb, minlength=50)
    want = [(k, c * int(mb[k])) for k, c in _first_occurrence_groups(ka) if mb[k]]
    c0 = _calls(db)
    r = db.query("SELECT id_a, COUNT(*) FROM A INNER JOIN B ON A.id_a = B.id_b GROUP BY id_a;")
    p = db.last_plan()
    assert _calls(db) - c0 == 1 and p["small_form"] == 1 and p["group_form"] == 0, (p, "the fused operator alone, in its one-workgroup form")
    assert r.rows() == want and r.joined_rows == sum(c for _, c in want)
    # a conjunct over both tables has to see the joined rows: the general plan, a join and a GROUP BY
    c0 = _calls(db)
    r2 = db.query("SELECT id_a, COUNT(*) FROM A INNER JOIN B ON A.id_a = B.id_b WHERE fa < id_b GROUP BY id_a;")
    assert _calls(db) - c0 == 2
    pairs = [(int(k), int(f)) for k, f in zip(ka, fa) if f < k]
    want2 = [(k, c * int(mb[k])) for k, c in _first_occurrence_groups(np.array([k for k, _ in pairs])) if mb[k]]
    assert r2.rows() == want2 and r2.joined_rows == r.joined_rows      # (the rows the joins produced: WHERE runs after them)


def test_arm_keys_only_plan_in_any_order(arms):
    db, ka, _, kb, _ = arms
    mb = np.bincount(kb, minlength=50)
    want = sorted(int(k) for k in ka for _ in range(int(mb[k])))
    db.groups_any_order(True)
    try:
        r = db.query("SELECT id_a, id_b FROM A INNER JOIN B ON A.id_a = B.id_b;")
    finally:
        db.groups_any_order(False)
    assert r.names == ["A.id_a", "B.id_b"] and np.array_equal(r.columns[0], r.columns[1])
    assert sorted(r.columns[0].tolist()) == want and r.joined_rows == len(want)


def test_arm_filter_project_and_its_neighbour_with_limit(arms):
    db, ka, fa, _, _ = arms
    sel = (fa < 4) & (ka >= 10)
    r = db.query("SELECT fa, id_a FROM A WHERE fa < 4 AND id_a >= 10;")
    cols = dict(zip(r.names, r.columns))
    assert np.array_equal(cols["A.id_a"], ka[sel]) and np.array_equal(cols["A.fa"], fa[sel]) and 0 < r.nrows < len(ka)
    lim = db.query("SELECT fa, id_a FROM A WHERE fa < 4 AND id_a >= 10 LIMIT 7;")
    cols = dict(zip(lim.names, lim.columns))
    assert lim.names == r.names and np.array_equal(cols["A.id_a"], ka[sel][:7]) and np.array_equal(cols["A.fa"], fa[sel][:7])


def test_arm_general_plan_group_by_one_field(arms):
    db, ka, fa, _, u = arms
    # the identity form: the catalog measured that U.u holds no value twice
    c0 = _calls(db)
    r = db.query("SELECT u, COUNT(*) FROM U GROUP BY u;")
    p = db.last_plan()
    assert _calls(db) - c0 == 1 and p["group_form"] == 3, p
    assert np.array_equal(r.columns[r.names.index("U.u")], u) and bool((r.columns[r.names.index("COUNT(*)")] == 1).all())
    # a key with duplicates: groups in the order of their first rows
    r = db.query("SELECT id_a, COUNT(*) FROM A GROUP BY id_a;")
    assert db.last_plan()["group_form"] != 3 and r.rows() == _first_occurrence_groups(ka)
    # the any-order keys form (or, where the operator does not serve it, the ordered one): the same groups as a set
    db.groups_any_order(True)
    try:
        anyo = db.query("SELECT id_a, COUNT(*) FROM A GROUP BY id_a;")
    finally:
        db.groups_any_order(False)
    assert anyo.names == r.names and sorted(anyo.rows()) == sorted(r.rows())


def test_arm_general_plan_group_by_several_fields(arms):
    db, ka, fa, _, _ = arms
    r = db.query("SELECT id_a, fa, COUNT(*) FROM A GROUP BY id_a, fa;")
    want = _first_occurrence_groups(ka, fa)
    at = [r.names.index(nm) for nm in ("A.id_a", "A.fa", "COUNT(*)")]
    assert [tuple(row[i] for i in at) for row in r.rows()] == want and len(want) > 40


def test_arm_general_plan_aggregates_without_group_by(arms):
    db, ka, fa, _, _ = arms
    a0 = sum(db.aggregate_calls())
    r = db.query("SELECT SUM(fa), COUNT(*) FROM A WHERE id_a >= 10;")
    cols = dict(zip(r.names, r.columns))
    assert r.nrows == 1 and int(cols["SUM(A.fa)"][0]) == int(fa[ka >= 10].sum()) and int(cols["COUNT(*)"][0]) == int((ka >= 10).sum())
    assert sum(db.aggregate_calls()) == a0 + 1
    empty = db.query("SELECT SUM(fa), COUNT(*) FROM A WHERE id_a < -5;")     # an empty stream: no row, the operator is not called
    assert sorted(empty.names) == ["COUNT(*)", "SUM(A.fa)"] and empty.nrows == 0
    assert sum(db.aggregate_calls()) == a0 + 1
