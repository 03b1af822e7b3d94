"""mdb_dev_rows_semi and mdb_dev_concat64 (midoridb_amd/csrc/mdb_dev_rowset.hip) against tests/setops_model.py, at the smallest shapes
where the kernels can go wrong: the bitmap-word, wave and workgroup edges of the probe side, the edges of the slot-count rule on the
build side, rows that collide on purpose, NULLs in every position, row-id vectors, DOUBLE cells by their bits, and every refusal."""
import numpy as np
import pytest

from midoridb_amd import dev as D
from tests import setops_model as M

pytestmark = pytest.mark.gpu

NO_ROW = D.NO_ROW
I64, F64 = 0, 1                       # MDB_T_INT64, MDB_T_DOUBLE
PROBE_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4097]
BUILD_SIZES = [0, 1, 7, 8, 9, 2 ** 16 - 1, 2 ** 16, 2 ** 16 + 1]


class Side:
    """the columns of one side: cells[c] uint64 bit patterns of the base rows, nulls[c] bool or None, one optional row-id vector"""

    def __init__(self, dev, cells, nulls=None, rid=None, types=None):
        self.cells = [np.asarray(c, dtype=np.uint64) for c in cells]
        self.nulls = [None] * len(cells) if nulls is None else [None if x is None else np.asarray(x, dtype=bool) for x in nulls]
        self.rid = None if rid is None else np.asarray(rid, dtype=np.uint32)
        self.types = [I64] * len(cells) if types is None else list(types)
        self.n = len(self.cells[0]) if self.rid is None else len(self.rid)
        self._keep, self._rows = [], None
        d_rid = None if self.rid is None else dev.to_dev(self.rid.view(np.int32))
        self.keys = []
        for c, nb, ty in zip(self.cells, self.nulls, self.types):
            dv = dev.to_dev(c if len(c) else np.zeros(1, dtype=np.uint64))
            dn = None if nb is None else dev.to_dev(D.pack_nullbits(nb) if len(nb) else np.zeros(1, dtype=np.uint64))
            self._keep += [dv, dn]
            self.keys.append((dv, dn, d_rid, ty, 0))

    def rows(self):
        """what the operator must see: tuples of ints (the 64 bits; a DOUBLE compares by them) and None"""
        if self._rows is None:
            cols = []
            for c, nb in zip(self.cells, self.nulls):
                r = np.arange(self.n) if self.rid is None else self.rid.astype(np.int64)
                absent = r == NO_ROW
                r = np.where(absent, 0, r)
                isnull = absent | (nb[r] if nb is not None and len(nb) else False)
                vals = c[r].tolist() if len(c) else [0] * self.n
                cols.append([None if z else v for v, z in zip(vals, np.broadcast_to(isnull, (self.n,)).tolist())])
            self._rows = list(zip(*cols)) if self.n else []
        return self._rows


def check(dev, probe, build, members=True):
    """both ways round against the model; returns the semi-join's positions"""
    got = None
    for anti in (False, True):
        want, nmembers = M.rows_semi(probe.rows(), build.rows(), anti)
        sel, info = dev.rows_semi(probe.keys, probe.n, build.keys, build.n, anti=anti)
        pos = sel.cpu().numpy().view(np.uint32).tolist()
        assert pos == want, (anti, probe.n, build.n, len(pos), len(want))
        if members:
            assert info["members"] == nmembers
        assert info["form"] == 1
        if build.n:
            assert info["log2_slots"] == max(4, int(np.ceil(np.log2(2 * build.n))))
        got = pos if not anti else got
    return got


def random_side(dev, rng, n, ncols, domain, null_rate=0.1):
    cells = [rng.integers(0, domain, n).astype(np.uint64) for _ in range(ncols)]
    nulls = [rng.random(n) < null_rate for _ in range(ncols)]
    return Side(dev, cells, nulls)


@pytest.fixture(scope="module")
def build_sides(dev):
    """one build side per size, shared by the probe sizes: two columns over a domain that makes about half of the probe rows members"""
    rng = np.random.default_rng(7)
    return {n: random_side(dev, rng, n, 2, max(2, int(np.sqrt(max(n, 1) * 2)) + 1)) for n in BUILD_SIZES}


@pytest.mark.parametrize("n_build", BUILD_SIZES)
@pytest.mark.parametrize("n_probe", PROBE_SIZES)
def test_sizes_at_word_wave_workgroup_and_slot_rule_edges(dev, build_sides, n_probe, n_build):
    rng = np.random.default_rng(1000 * n_probe + n_build)
    build = build_sides[n_build]
    probe = random_side(dev, rng, n_probe, 2, max(2, int(np.sqrt(max(n_build, 1) * 2)) + 1))
    hits = check(dev, probe, build)
    if n_build >= 7 and n_probe >= 63:
        assert 0 < len(hits) < n_probe          # (the case means something: members and non-members)


def test_all_build_rows_equal(dev):
    """one member, every insert on one slot"""
    n = 2 ** 16
    build = Side(dev, [np.full(n, 42, dtype=np.uint64), np.full(n, 7, dtype=np.uint64)], [None, np.zeros(n, dtype=bool)])
    probe = Side(dev, [np.array([42, 42, 41, 42], dtype=np.uint64), np.array([7, 8, 7, 7], dtype=np.uint64)])
    assert check(dev, probe, build) == [0, 3]
    sel, info = dev.rows_semi(probe.keys, 4, build.keys, n)
    assert info["members"] == 1
    nulls = Side(dev, [np.arange(n, dtype=np.uint64)], [np.ones(n, dtype=bool)])       # ... and 2^16 NULL rows over different garbage are one row too
    sel, info = dev.rows_semi(nulls.keys, n, nulls.keys, n)
    assert info["members"] == 1 and sel.numel() == n


def test_rows_that_differ_only_in_bit_63_or_only_in_the_last_of_16_columns(dev):
    n = 2 ** 16
    low = np.arange(n // 2, dtype=np.uint64)
    build = Side(dev, [np.concatenate([low, low | np.uint64(1 << 63)])])                # pairs that differ in bit 63 alone
    probe = Side(dev, [np.array([5, 5 | (1 << 63), n // 2, (n // 2) | (1 << 63), (1 << 63) - 1], dtype=np.uint64)])
    assert check(dev, probe, build) == [0, 1]
    only_high = Side(dev, [np.arange(n, dtype=np.uint64) << np.uint64(48)])             # 2^16 rows that differ in bits 48..63 alone
    assert check(dev, Side(dev, [np.array([3 << 48, 3, 0, 1 << 47], dtype=np.uint64)]), only_high) == [0, 2]
    same = [np.full(n, 1000 + c, dtype=np.uint64) for c in range(15)]
    build16 = Side(dev, same + [np.arange(n, dtype=np.uint64)])
    p = 6
    probe16 = Side(dev, [np.full(p, 1000 + c, dtype=np.uint64) for c in range(15)] + [np.array([0, n - 1, n, 77, 2 ** 40, 12345], dtype=np.uint64)])
    assert check(dev, probe16, build16) == [0, 1, 3, 5]
    first_differs = Side(dev, [np.array([999] + [1000] * (p - 1), dtype=np.uint64)] + [np.full(p, 1000 + c, dtype=np.uint64) for c in range(1, 15)] +
                         [np.arange(p, dtype=np.uint64)])
    assert check(dev, first_differs, build16) == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("ncols", [1, 2, 5, 16])
def test_nulls_in_every_column_position(dev, ncols):
    """row r of the build side has its NULL in column r % ncols (and different garbage under it than the probe side has); the probe side
    holds those rows, rows with the NULL moved one column on, and a row of all NULLs"""
    rng = np.random.default_rng(ncols)
    n = 4 * ncols + 3
    base = [rng.integers(1, 4, n).astype(np.uint64) for _ in range(ncols)]
    b_nulls = [np.array([r % ncols == c or r == n - 1 for r in range(n)]) for c in range(ncols)]        # the last row: all NULL
    p_nulls = [np.array([(r % ncols == c) if r < n // 2 else ((r + 1) % ncols == c) for r in range(n - 1)] + [True]) for c in range(ncols)]
    garbage = lambda nulls, salt: [np.where(nb, np.uint64(salt) + np.arange(n, dtype=np.uint64), v) for v, nb in zip(base, nulls)]
    build = Side(dev, garbage(b_nulls, 0xDEAD0000), b_nulls)
    probe = Side(dev, garbage(p_nulls, 0xBEEF0000), p_nulls)
    hits = check(dev, probe, build)
    assert n - 1 in hits and set(range(n // 2)) <= set(hits)         # the all-NULL row; the rows whose NULL stands where the build row's does


def test_rid_vectors_with_repeats_and_no_row(dev):
    rng = np.random.default_rng(11)
    nb, np_ = 300, 500
    bcells = [rng.integers(0, 12, nb).astype(np.uint64), rng.integers(0, 3, nb).astype(np.uint64)]
    pcells = [rng.integers(0, 12, np_).astype(np.uint64), rng.integers(0, 3, np_).astype(np.uint64)]
    brid = rng.integers(0, nb, 257).astype(np.uint32)
    brid[[3, 100, 256]] = NO_ROW
    prid = rng.integers(0, np_, 1025).astype(np.uint32)
    prid[[0, 64, 1024]] = NO_ROW
    bn = [rng.random(nb) < 0.1, None]
    pn = [None, rng.random(np_) < 0.1]
    build, probe = Side(dev, bcells, bn, brid), Side(dev, pcells, pn, prid)
    hits = check(dev, probe, build)
    assert {0, 64, 1024} <= set(hits)            # a row of "no row" cells is the all-NULL row, which the build side holds too
    check(dev, Side(dev, pcells, pn, prid), Side(dev, bcells, bn))          # a row-id vector on one side only
    check(dev, Side(dev, pcells, pn), Side(dev, bcells, bn, brid))


def test_double_cells_compare_by_their_bits(dev):
    nan1, nan2 = 0x7FF8000000000000, 0x7FF8000000000001
    f = lambda *xs: np.array(xs, dtype=np.float64).view(np.uint64)
    build = Side(dev, [np.concatenate([f(0.0, 1.5), np.array([nan1], dtype=np.uint64)])], types=[F64])
    probe = Side(dev, [np.concatenate([f(0.0, -0.0, 1.5, 2.5), np.array([nan1, nan2], dtype=np.uint64)])], types=[F64])
    assert check(dev, probe, build) == [0, 2, 4]
    build = Side(dev, [np.concatenate([f(-0.0), np.array([nan2], dtype=np.uint64)])], types=[F64])
    assert check(dev, probe, build) == [1, 5]


def test_refusals_and_a_correct_call_after_each(dev):
    rng = np.random.default_rng(5)
    good_b, good_p = random_side(dev, rng, 100, 2, 8), random_side(dev, rng, 200, 2, 8)
    wide = Side(dev, [np.arange(4, dtype=np.uint64)] * 17)
    dbl = Side(dev, [np.arange(100, dtype=np.uint64)] * 2, types=[I64, F64])
    for call, msg in [(lambda: dev.rows_semi(good_p.keys, 200, good_b.keys, 100, ncols=0), "0 columns, a row has 1 to 16"),
                      (lambda: dev.rows_semi(wide.keys, 4, wide.keys, 4), "17 columns, a row has 1 to 16"),
                      (lambda: dev.rows_semi(good_p.keys, 200, dbl.keys, 100), "column 1 is of type 0 on the probe side and of type 1 on the build side"),
                      (lambda: dev.lib.mdb_dev_rows_semi(dev.h, dev._sort_keys(good_p.keys), 2 ** 32 - 1, dev._sort_keys(good_b.keys), 100, 2, 0,
                                                         good_p.keys[0][0].data_ptr(), D.byref(D.c_uint64(0)), None), "probe rows"),
                      (lambda: dev.lib.mdb_dev_rows_semi(dev.h, dev._sort_keys(good_p.keys), 200, dev._sort_keys(good_b.keys), 2 ** 30 + 1, 2, 0,
                                                         good_p.keys[0][0].data_ptr(), D.byref(D.c_uint64(0)), None), "build rows")]:
        try:
            rc = call()
            assert rc == -1, rc                     # (the raw calls return -MIDORIDB_ERROR; the wrapper raises)
            assert msg in dev.lib.mdb_dev_last_error(dev.h).decode()
        except D.DeviceError as ex:
            assert "(-1)" in str(ex) and msg in str(ex), str(ex)
        check(dev, good_p, good_b)


def test_general_case_three_columns_and_same_bytes(dev):
    """2 * 10^5 probe rows x 10^5 build rows over 3 columns, about half of the probe rows members"""
    rng = np.random.default_rng(2026)
    build = random_side(dev, rng, 100_000, 3, 52, null_rate=0.02)
    probe = random_side(dev, rng, 200_000, 3, 52, null_rate=0.02)
    hits = check(dev, probe, build)
    assert 0.35 * probe.n < len(hits) < 0.65 * probe.n
    a, ia = dev.rows_semi(probe.keys, probe.n, build.keys, build.n)
    b, ib = dev.rows_semi(probe.keys, probe.n, build.keys, build.n)
    assert ia == ib and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------ mdb_dev_concat64

@pytest.mark.parametrize("sizes", [(63, 64, 65, 1, 0), (0, 1, 65, 64, 63), (64, 0, 63, 1, 65), (1, 1, 0, 0, 1), (65, 63), (0, 0), (5000, 333)])
@pytest.mark.parametrize("bitmaps", ["all", "none", "alternating"])
def test_concat64_every_word(dev, sizes, bitmaps):
    rng = np.random.default_rng(sum(sizes) + len(bitmaps))
    parts, model_parts, keep = [], [], []
    for k, n in enumerate(sizes):
        v = rng.integers(0, 2 ** 63, n, dtype=np.int64)
        has = bitmaps == "all" or (bitmaps == "alternating" and k % 2 == 0)
        nb = (rng.random(n) < 0.4) if has else None
        dv = dev.to_dev(v) if n else None
        dn = dev.to_dev(D.pack_nullbits(nb) if n else np.zeros(1, dtype=np.uint64)) if has else None
        keep += [dv, dn]
        parts.append((dv, dn, n))
        model_parts.append((v, nb))
    want_v, want_w = M.concat64(model_parts)
    got_v, got_w = dev.concat64(parts)              # (the NULL words start as all ones: a word left unwritten, or a bit behind the last row, shows)
    assert np.array_equal(got_v.cpu().numpy(), want_v)
    assert np.array_equal(got_w.cpu().numpy().view(np.uint64), want_w)
    if bitmaps == "none":
        got_v, none = dev.concat64(parts, want_nulls=False)
        assert none is None and np.array_equal(got_v.cpu().numpy(), want_v)


def test_concat64_refusals(dev):
    v = dev.to_dev(np.arange(4, dtype=np.int64))
    nb = dev.to_dev(np.zeros(1, dtype=np.uint64))
    for parts, kw, msg in [([(v, None, 4)] * 17, {}, "17 parts, a call takes at most 16"), ([(None, None, 4)], {}, "part 0 has 4 rows and no values"),
                           ([(v, nb, 4)], {"want_nulls": False}, "part 0 has a NULL bitmap, the destination has none")]:
        with pytest.raises(D.DeviceError) as ei:
            dev.concat64(parts, **kw)
        assert msg in str(ei.value)
    got_v, got_w = dev.concat64([(v, None, 4), (v, nb, 4)])
    assert got_v.cpu().numpy().tolist() == [0, 1, 2, 3] * 2 and got_w.cpu().numpy().tolist() == [0]
