"""IN / NOT IN lists of any length on the device: the predicate instruction MDB_P_IN_SET (a hash-set probe; mdb_dev.h "device sets")
through DeviceCtx.filter / filter_project against numpy.isin - the one-instruction kernel with the table in LDS and in global memory,
and the interpreters -, and the SQL statements that compile to it (mdb_exec_pred.c), against numpy.

Row counts: 1, around a ballot word (64), around a row block (4096 = FILT_TUPLES_PER_BLOCK), around mdb_dev_filter's 2^18 switch, odd
counts for the two-row loads' tail.  Set sizes: 9, the largest list staged in LDS, one more (global memory), 10^5."""
import numpy as np
import pytest

from midoridb_amd import dev as D

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ROWS = [1, 63, 64, 65, 4095, 4096, 4097, (1 << 18) - 1, (1 << 18) + 1]
NMAX = max(ROWS)
NO_ROW = -1          # MDB_NO_ROW in an int32 row-id vector


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(t):
    return t.cpu().numpy()


def _set_sizes(dev):
    lds = dev.in_set_lds_values()
    return {"9": 9, "lds": lds, "lds+1": lds + 1, "1e5": 100_000}


# log2 of the slot count each size must get (the instruction's b field): "lds" is the largest table the one-instruction kernel stages in
# LDS - 2048 DISTINCT values in 4096 slots, load 1/2 -, "lds+1" the first it probes in global memory
SLOTS_LOG2 = {"9": 6, "lds": 12, "lds+1": 13, "1e5": 18}


@pytest.fixture(scope="module")
def world(dev):
    """per set size: the members, the device set, and ONE column of NMAX cells (half of them members) with its NULL flags, a second
    column and a row-id vector with MDB_NO_ROW entries - every test takes prefixes of them; built once, never changed"""
    rng = np.random.default_rng(20)
    out = {}
    for name, k in _set_sizes(dev).items():
        members = rng.permutation(np.unique(rng.integers(-(1 << 62), 1 << 62, 2 * k, dtype=np.int64)))[: k - 2]
        members = np.unique(np.concatenate([members, [I64_MIN, -1]]))    # members at the extremes; I64_MAX and 0 are none
        assert len(members) == k                                  # exactly k DISTINCT values ...
        listed = rng.permutation(np.concatenate([members, members[: k // 4]]))     # ... in a list that repeats a quarter of them
        cells = np.where(rng.random(NMAX) < 0.5, rng.choice(members, NMAX), rng.integers(-(1 << 62), 1 << 62, NMAX, dtype=np.int64))
        near = rng.choice(members[2:], NMAX) + 1                  # non-members next to members
        cells = np.where(rng.random(NMAX) < 0.1, near, cells)
        cells[rng.integers(0, NMAX, 64)] = I64_MAX
        cells[rng.integers(0, NMAX, 64)] = 0
        cells[rng.integers(0, NMAX, 64)] = I64_MIN
        cells[rng.integers(0, NMAX, 64)] = -1
        cells[:8] = [I64_MIN, I64_MAX, 0, -1, members[2], members[2] + 1, I64_MAX, I64_MIN]
        nulls = rng.random(NMAX) < 0.1
        other = rng.integers(-1000, 1000, NMAX, dtype=np.int64)
        rid = rng.integers(0, NMAX, NMAX).astype(np.int32)
        rid[rng.random(NMAX) < 0.05] = NO_ROW
        # the same cells one 8-byte step off a 16-byte boundary: torch allocations are at least 16-byte aligned
        shifted = dev.to_dev(np.concatenate([[0], cells]))
        assert shifted.data_ptr() % 16 == 0
        out[name] = dict(members=members, set=dev.make_set(listed), cells=cells, nulls=nulls, other=other, rid=rid,
                         d_cells=dev.to_dev(cells), d_nulls=dev.nullbits_dev(nulls), d_other=dev.to_dev(other), d_rid=dev.to_dev(rid),
                         d_shifted=shifted[1:])
        assert out[name]["d_cells"].data_ptr() % 16 == 0 and out[name]["d_shifted"].data_ptr() % 16 == 8
        # which side of the LDS switch the size lands on (MDB_SET_LDS_SLOTS = 2^12 slots): the table is sized by the distinct values
        assert out[name]["set"].insn(0)[4] == SLOTS_LOG2[name], (name, out[name]["set"].insn(0)[4])
    yield out
    for w in out.values():
        w["set"].close()


def _expect(member, valid, negate):
    return np.nonzero(valid & (member != negate))[0]


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("size", ["9", "lds", "lds+1", "1e5"])
def test_in_set_operator_forms(dev, world, size, n):
    w = world[size]
    s, cells = w["set"], w["cells"][:n]
    member = np.isin(cells, w["members"])
    if n >= 8:
        assert member[:8].tolist() == [True, False, False, True, True, False, False, True]      # the extremes, both ways
    everything = np.ones(n, dtype=bool)
    for negate in (False, True):
        prog = [s.insn(0, negate)]
        assert prog[0][0] == D.P_IN_SET and prog[0][4] == SLOTS_LOG2[size] and (prog[0][4] <= 12) == (size in ("9", "lds"))
        # a direct column: the one-instruction kernel (table in LDS up to in_set_lds_values(), in global memory beyond)
        got = _np(dev.filter(prog, [(w["d_cells"], None, None)], n)).astype(np.int64)
        assert np.array_equal(got, _expect(member, everything, negate)), ("direct", negate)
        # ... with NULL bits: a NULL cell fails IN and NOT IN
        got = _np(dev.filter(prog, [(w["d_cells"], w["d_nulls"], None)], n)).astype(np.int64)
        assert np.array_equal(got, _expect(member, ~w["nulls"][:n], negate)), ("nulls", negate)
        # the same cells at an 8-byte-misaligned address: the one-row interpreter
        got = _np(dev.filter(prog, [(w["d_shifted"], None, None)], n)).astype(np.int64)
        assert np.array_equal(got, _expect(member, everything, negate)), ("misaligned", negate)
        # through a row-id vector with MDB_NO_ROW entries (such a cell is NULL), the column with NULL bits
        rid = w["rid"][:n].astype(np.int64)
        present = rid != NO_ROW
        at = np.where(present, rid, 0)
        m_rid = np.isin(w["cells"][at], w["members"])
        got = _np(dev.filter(prog, [(w["d_cells"], w["d_nulls"], w["d_rid"])], n)).astype(np.int64)
        assert np.array_equal(got, _expect(m_rid, present & ~w["nulls"][at], negate)), ("rid", negate)
        # combined with a comparison on a second column: the two-row interpreter
        lt = w["other"][:n] < 0
        for op, comb in ((D.P_AND, np.logical_and), (D.P_OR, np.logical_or)):
            prog2 = [s.insn(0, negate), (D.P_CMP_COL_CONST, D.CMP_LT, D.T_INT64, 1, 0, 0), (op, 0, 0, 0, 0, 0)]
            got = _np(dev.filter(prog2, [(w["d_cells"], w["d_nulls"], None), (w["d_other"], None, None)], n)).astype(np.int64)
            exp = np.nonzero(comb(~w["nulls"][:n] & (member != negate), lt))[0]
            assert np.array_equal(got, exp), ("combined", op, negate)
        # scan + WHERE + projection in one call
        keep = _expect(member, ~w["nulls"][:n], negate)
        m, outs = dev.filter_project(prog, [(w["d_cells"], w["d_nulls"], None)], n, [(w["d_other"], None), (w["d_cells"], w["d_nulls"])])
        assert m == len(keep), ("project", negate)
        assert np.array_equal(_np(outs[0][0]), w["other"][:n][keep]) and np.array_equal(_np(outs[1][0]), cells[keep])
        if m:
            assert not D.unpack_nullbits(_np(outs[1][1]).view(np.uint64), m).any()


@pytest.mark.parametrize("n", [65, 4097, (1 << 18) + 1])
@pytest.mark.parametrize("k", [9, 2048, 3000])
def test_in_set_double_compares_like_ieee_equality(dev, n, k):
    """-0.0 and +0.0 are one member, inf is a value like any other, a NaN cell is a member of nothing: IN false, NOT IN true"""
    rng = np.random.default_rng(n + k)
    members = np.concatenate([[-0.0, np.inf, np.nan], rng.integers(-10**6, 10**6, k - 3) + 0.5])
    pool = np.concatenate([members, [0.0, -np.inf, np.nan, 1.25], rng.integers(-10**6, 10**6, k) + 0.25])
    cells = rng.choice(pool, n)
    cells[:7] = [0.0, -0.0, np.inf, -np.inf, np.nan, members[3], 1.25][: min(7, n)]
    real = members[~np.isnan(members)]
    member = np.isin(np.where(cells == 0, 0.0, cells).view(np.int64), np.where(real == 0, 0.0, real).view(np.int64)) & ~np.isnan(cells)
    assert member[:7].tolist() == [True, True, True, False, False, True, False]
    s = dev.make_set(members, D.T_DOUBLE)
    assert s.insn(0)[4] == {9: 5, 2048: 12, 3000: 13}[k]      # 32 slots / the largest LDS table (the NaN and any repeat do not count) / global
    d_cells = dev.to_dev(cells)
    nulls = rng.random(n) < 0.1
    d_nulls = dev.nullbits_dev(nulls)
    shifted = dev.to_dev(np.concatenate([[0.0], cells]))[1:]
    for negate in (False, True):
        prog = [s.insn(0, negate)]
        assert prog[0][2] == D.T_DOUBLE
        got = _np(dev.filter(prog, [(d_cells, d_nulls, None)], n)).astype(np.int64)
        assert np.array_equal(got, _expect(member, ~nulls, negate)), negate
        got = _np(dev.filter(prog, [(shifted, None, None)], n)).astype(np.int64)
        assert np.array_equal(got, _expect(member, np.ones(n, dtype=bool), negate)), ("interpreter", negate)
    s.close()


@pytest.mark.parametrize("k", [12, 2040, 3000])
def test_in_set_extremes_as_members_and_as_non_members(dev, k):
    """INT64_MIN / INT64_MAX / 0 / -1: each of them a member of one set and none of the other, in the one-instruction kernel (table
    in LDS, table in global memory) and in the interpreter; the builder's EMPTY marker is none of the members either way"""
    rng = np.random.default_rng(k)
    ext = np.array([I64_MIN, I64_MAX, 0, -1], dtype=np.int64)
    filler = rng.integers(-(1 << 40), 1 << 40, k, dtype=np.int64)
    filler = filler[~np.isin(filler, ext)]
    n = 4097
    cells = rng.choice(np.concatenate([ext, filler, filler + 1, ext + np.array([1, -1, 1, -1])]), n)
    cells[:4] = ext
    d_cells, shifted = dev.to_dev(cells), dev.to_dev(np.concatenate([[0], cells]))[1:]
    for members in (np.concatenate([ext, filler]), np.concatenate([ext[:1], filler]), np.concatenate([ext[1:], filler]), filler):
        s = dev.make_set(members)
        assert (s.insn(0)[4] <= 12) == (k < 3000)               # table in LDS (k = 2040: 4096 slots, load 1/2) / in global memory
        member = np.isin(cells, members)
        assert member[:4].tolist() == np.isin(ext, members).tolist()
        for negate in (False, True):
            for col in (d_cells, shifted):
                got = _np(dev.filter([s.insn(0, negate)], [(col, None, None)], n)).astype(np.int64)
                assert np.array_equal(got, np.nonzero(member != negate)[0]), (len(members), negate)
        s.close()


def test_in_set_program_is_validated(dev, world):
    w = world["9"]
    op, cmp_, typ, a, b, imm = w["set"].insn(0)
    cols = [(w["d_cells"], None, None)]
    for bad in [(op, cmp_, typ, 1, b, imm), (op, cmp_, typ, 0, b, 0), (op, cmp_, typ, 0, b, imm + 8), (op, cmp_, typ, 0, 2, imm),
                (op, cmp_, typ, 0, 40, imm), (op, cmp_, 5, 0, b, imm),
                (op, cmp_, typ, 0, b + 3, imm)]:        # a size field that promises more slots than the library's buffer holds
        with pytest.raises(D.DeviceError):
            dev.filter([bad], cols, 100)
    with pytest.raises(D.DeviceError):
        w["set"].insn(99)


# ---------------------------------------------------------------------------------------------- SQL

def _db(tables):
    from midoridb_amd.query import DB
    db = DB()
    for name, ddl, cols, nulls in tables:
        db.execute(f"CREATE TABLE {name} ({ddl});")
        db.append_columns(name, cols, nulls)
    return db


def _col(r, name):
    """a result column by its name: the result's column order is the reference's, not the select list's"""
    return r.columns[[i for i, nm in enumerate(r.names) if nm == name or nm.endswith("." + name)][0]]


def _rows(r, *names):
    return sorted(zip(*[_col(r, nm).tolist() for nm in names]))


def _lst(vals):
    return ", ".join("NULL" if v is None else (f"'{v}'" if isinstance(v, str) else str(int(v))) for v in vals)


@pytest.fixture(scope="module")
def table_t():
    rng = np.random.default_rng(7)
    n = 100_000
    k = rng.integers(-20_000, 20_000, n, dtype=np.int64)
    v = rng.integers(0, 100, n, dtype=np.int64)
    knull = rng.random(n) < 0.05
    db = _db([("T", "k INT, v INT", [k, v], [knull.astype(np.uint8), None])])
    yield db, k, v, knull
    db.close()


def test_sql_where_list_of_1000_values(table_t):
    """the statement the parent refuses as "predicate too large"; the list is pushed down to the table: the one-instruction kernel"""
    db, k, v, knull = table_t
    rng = np.random.default_rng(8)
    lst = rng.choice(np.arange(-25_000, 25_000), 1000, replace=False)
    for neg in (False, True):
        c0 = db.in_set_lookups()
        r = db.query(f"SELECT v, k FROM T WHERE k {'NOT ' if neg else ''}IN ({_lst(lst)});")
        assert db.in_set_lookups() == c0 + 1
        keep = ~knull & (np.isin(k, lst) != neg)
        assert np.array_equal(_col(r, "k"), k[keep]) and np.array_equal(_col(r, "v"), v[keep]), neg
        assert 500 < keep.sum() < len(k) - 500


def test_sql_list_of_100000_values(table_t):
    """front end and executor on a list of 10^5 values (a table of 2^18 slots, probed in global memory); a type error in its last value
    is named, not reported as a program that is too large"""
    from midoridb_amd.query import QueryError
    db, k, v, knull = table_t
    lst = np.arange(100_000, dtype=np.int64) * 7 - 350_000
    for neg in (False, True):
        c0 = db.in_set_lookups()
        r = db.query(f"SELECT k FROM T WHERE k {'NOT ' if neg else ''}IN ({_lst(lst)});")
        assert db.in_set_lookups() == c0 + 1
        keep = ~knull & (np.isin(k, lst) != neg)
        assert np.array_equal(_col(r, "k"), k[keep]) and 1000 < keep.sum() < len(k) - 1000, neg
    with pytest.raises(QueryError) as ei:
        db.query(f"SELECT k FROM T WHERE k IN ({_lst(lst)}, 'x');")
    assert "requires an VARCHAR() column" in str(ei.value)


def test_sql_lists_of_8_and_9_values(table_t):
    db, k, v, knull = table_t
    for size, rise in ((8, 0), (9, 1)):
        lst = np.arange(size) * 3 - 5
        c0 = db.in_set_lookups()
        r = db.query(f"SELECT k FROM T WHERE k IN ({_lst(lst)}) AND v < 50;")
        assert db.in_set_lookups() == c0 + rise, size
        assert np.array_equal(r.columns[0], k[~knull & np.isin(k, lst) & (v < 50)])


def test_sql_null_among_50_values(table_t):
    db, k, v, knull = table_t
    lst = [int(x) for x in np.arange(49) * 11 - 200]
    with_null = lst[:20] + [None] + lst[20:]
    r = db.query(f"SELECT k FROM T WHERE k IN ({_lst(with_null)});")
    assert np.array_equal(r.columns[0], k[~knull & np.isin(k, lst)]) and r.nrows > 0
    r = db.query(f"SELECT k FROM T WHERE k NOT IN ({_lst(with_null)});")        # x <> NULL is never true
    assert r.nrows == 0
    r = db.query(f"SELECT v FROM T WHERE k NOT IN ({_lst(with_null)}) OR v = 3;")
    assert r.nrows == int((v == 3).sum()) and (r.columns[0] == 3).all()


def test_sql_knob_expands_every_list_as_before(table_t, monkeypatch):
    from midoridb_amd.query import QueryError
    db, k, v, knull = table_t
    big, small = np.arange(1000) * 7, np.arange(20) * 7
    monkeypatch.setenv("MDB_IN_SET", "0")
    c0 = db.in_set_lookups()
    with pytest.raises(QueryError) as ei:
        db.query(f"SELECT k FROM T WHERE k IN ({_lst(big)});")
    assert "predicate too large" in str(ei.value)
    r = db.query(f"SELECT k FROM T WHERE k IN ({_lst(small)});")
    assert db.in_set_lookups() == c0
    monkeypatch.delenv("MDB_IN_SET")
    r2 = db.query(f"SELECT k FROM T WHERE k IN ({_lst(small)});")
    assert db.in_set_lookups() == c0 + 1
    assert np.array_equal(r.columns[0], r2.columns[0]) and np.array_equal(r2.columns[0], k[~knull & np.isin(k, small)])


def test_sql_list_in_a_joins_where_and_as_on_residual():
    rng = np.random.default_rng(9)
    na, nb = 3000, 2000
    ak, av = rng.integers(0, 1500, na, dtype=np.int64), rng.integers(0, 5000, na, dtype=np.int64)
    bk, bw = rng.integers(0, 1500, nb, dtype=np.int64), rng.integers(0, 5000, nb, dtype=np.int64)
    db = _db([("A", "k INT, v INT", [ak, av], None), ("B", "k2 INT, w INT", [bk, bw], None)])
    lst = rng.choice(5000, 600, replace=False)
    ia, ib = np.nonzero(ak[:, None] == bk[None, :])
    try:
        c0 = db.in_set_lookups()
        r = db.query(f"SELECT v, w FROM A INNER JOIN B ON A.k = B.k2 WHERE v IN ({_lst(lst)});")
        keep = np.isin(av[ia], lst)
        assert _rows(r, "v", "w") == sorted(zip(av[ia][keep].tolist(), bw[ib][keep].tolist())) and keep.sum() > 100
        r = db.query(f"SELECT v, w FROM A INNER JOIN B ON A.k = B.k2 AND w NOT IN ({_lst(lst)});")
        keep = ~np.isin(bw[ib], lst)
        assert _rows(r, "v", "w") == sorted(zip(av[ia][keep].tolist(), bw[ib][keep].tolist())) and keep.sum() > 100
        # over both tables' columns at once: evaluated on the joined pairs, through row-id vectors
        r = db.query(f"SELECT v, w FROM A INNER JOIN B ON A.k = B.k2 WHERE v IN ({_lst(lst)}) OR w IN ({_lst(lst[:300])});")
        keep = np.isin(av[ia], lst) | np.isin(bw[ib], lst[:300])
        assert _rows(r, "v", "w") == sorted(zip(av[ia][keep].tolist(), bw[ib][keep].tolist()))
        assert db.in_set_lookups() == c0 + 4
    finally:
        db.close()


def test_sql_delete_and_update_with_a_500_value_list():
    rng = np.random.default_rng(10)
    n = 20_000
    k, v = rng.integers(0, 3000, n, dtype=np.int64), np.arange(n, dtype=np.int64)
    db = _db([("T", "k INT, v INT", [k, v], None)])
    try:
        lst = rng.choice(3000, 500, replace=False)
        c0 = db.in_set_lookups()
        gone = np.isin(k, lst)
        assert db.execute(f"DELETE FROM T WHERE k IN ({_lst(lst)});") == int(gone.sum())
        k, v = k[~gone], v[~gone]
        r = db.query("SELECT k, v FROM T;")
        assert np.array_equal(_col(r, "k"), k) and np.array_equal(_col(r, "v"), v)
        lst2 = rng.choice(3000, 500, replace=False)
        hit = ~np.isin(k, lst2)
        assert db.execute(f"UPDATE T SET v = -7 WHERE k NOT IN ({_lst(lst2)});") == int(hit.sum())
        v = np.where(hit, -7, v)
        r = db.query("SELECT k, v FROM T;")
        assert np.array_equal(_col(r, "k"), k) and np.array_equal(_col(r, "v"), v)
        assert db.in_set_lookups() == c0 + 2 and 0 < hit.sum() < len(k)
    finally:
        db.close()


def test_sql_varchar_list_of_300_strings():
    """a bit per dictionary id (MDB_P_IN_BITS, as LIKE): a third of the strings are in no cell"""
    rng = np.random.default_rng(11)
    n = 5000
    words = [f"w{i:04d}" for i in range(400)]
    s = [None if rng.random() < 0.05 else words[int(i)] for i in rng.integers(0, 400, n)]
    ids = np.arange(n, dtype=np.int64)
    db = _db([("S", "id INT, s VARCHAR(12)", [ids, s], None)])
    try:
        lst = [words[int(i)] for i in rng.choice(400, 200, replace=False)] + [f"absent{i}" for i in range(100)]
        c0 = db.in_set_lookups()
        r = db.query(f"SELECT id FROM S WHERE s IN ({_lst(lst)});")
        want = np.array([x is not None and x in set(lst) for x in s])
        assert np.array_equal(r.columns[0], ids[want]) and want.sum() > 1000
        r = db.query(f"SELECT id FROM S WHERE s NOT IN ({_lst(lst)});")
        want = np.array([x is not None and x not in set(lst) for x in s])
        assert np.array_equal(r.columns[0], ids[want]) and want.sum() > 1000
        assert db.in_set_lookups() == c0 + 2
        r = db.query(f"SELECT id FROM S WHERE s IN ({_lst([f'absent{i}' for i in range(40)])});")
        assert r.nrows == 0
    finally:
        db.close()
