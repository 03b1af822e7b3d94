"""The row primitives of midoridb_amd/csrc/mdb_dev_core.hip - gather64, gather32, iota32, scatter_set64, map_ids, combine_counts,
key_range, distinct_scan, widen32to64, cross_pairs, double_join_keys - and the allocator's bookkeeping, each against
tests/rowops_model.py at the block and word edges.

Every test calls the C ABI (dev.lib / dev.h) with buffers it allocates itself.  Every output is a view into a larger tensor with 64
sentinel elements on either side (0xA5A5... for values, all-ones for NULL words; the view starts 16-byte aligned) and is itself
prefilled with the sentinel, so that after the call

    the payload must equal the model bit for bit             (an element left unwritten still holds the sentinel),
    both guard regions must be untouched                     (a write past n),
    every NULL word 0 .. ceil(n / 64) - 1 must equal the model  (a word left unwritten or a stray bit above n is all-ones / a 1).

Safe by construction: index vectors hold valid row ids or MDB_NO_ROW only, and every output buffer is at least as large as the routine
may write.  mdb_dev_gather32 has no identity form (its idx is required): "identity" there is an explicit 0 .. n-1 vector.
"""
from ctypes import byref, c_int, c_int64, c_size_t, c_uint64, c_void_p

import numpy as np
import pytest

from midoridb_amd import dev as D
from oracle import np_oracle as orc
from tests import rowops_model as rm

pytestmark = pytest.mark.gpu

GUARD = 64
VAL = 0xA5A5A5A5A5A5A5A5
ONES = (1 << 64) - 1
BIG = 333_333                        # 162 full blocks and a ragged tail of 1557 = 24 waves + 21 lanes
SIZES = rm.SIZES + (BIG,)
SRC_ROWS = 5000
ERR = -1                             # -MIDORIDB_ERROR
I64_MIN, I64_MAX = rm.I64_MIN, rm.I64_MAX


class Guarded:
    """n elements of an unsigned numpy dtype between two guards of GUARD sentinel elements, on the device.  `init` fills the payload
    (default: the sentinel too)."""

    def __init__(self, dev, n, dtype=np.uint64, sentinel=VAL, init=None):
        self.n, self.dtype = n, np.dtype(dtype)
        self.sentinel = sentinel & ((1 << (8 * self.dtype.itemsize)) - 1)
        host = np.full(n + 2 * GUARD, self.sentinel, dtype=self.dtype)
        if init is not None:
            host[GUARD:GUARD + n] = np.asarray(init).view(self.dtype)
        self.whole = dev.to_dev(host)
        self.ptr = c_void_p(self.whole.data_ptr() + GUARD * self.dtype.itemsize)
        assert self.ptr.value % 16 == 0

    def read(self):
        """the payload, after asserting that neither guard was written"""
        host = self.whole.cpu().numpy().view(self.dtype)
        for name, g in (("front", host[:GUARD]), ("back", host[GUARD + self.n:])):
            bad = np.flatnonzero(g != self.sentinel)
            assert not len(bad), f"{name} guard written at {bad[:8].tolist()}"
        return host[GUARD:GUARD + self.n]

    def check(self, want, what=""):
        got = self.read()
        want = np.ascontiguousarray(want).view(self.dtype)
        assert len(want) == self.n
        bad = np.flatnonzero(got != want)
        assert not len(bad), f"{what}: {len(bad)} of {self.n} differ, first at {bad[0]}: got {int(got[bad[0]]):#x}, want {int(want[bad[0]]):#x}"

    def untouched(self, what=""):
        self.check(np.full(self.n, self.sentinel, dtype=self.dtype), what)


def nullwords(dev, n, init=None):
    """ceil(n / 64) NULL words prefilled with all-ones (or `init`), guards all-ones"""
    return Guarded(dev, rm.words_for(n), np.uint64, ONES, init)


def ok(dev, rc, what):
    assert rc == 0, f"{what}: {rc}: {dev.lib.mdb_dev_last_error(dev.h).decode()}"


def refused(dev, rc, text):
    assert rc == ERR, rc
    assert text in dev.lib.mdb_dev_last_error(dev.h).decode()


def P(t):
    """the device address of a tensor the CALLER keeps alive (a temporary's memory is handed to the next tensor at once)"""
    return None if t is None else c_void_p(t.data_ptr())


def words64(rng, rows):
    return rng.integers(0, 1 << 64, size=rows, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------------ gather64

@pytest.mark.parametrize("shape", ["identity", "repeats", "perm", "norow"])
@pytest.mark.parametrize("n", SIZES)
def test_gather64(dev, n, shape):
    rng = np.random.default_rng(n * 4 + len(shape))
    src_n = n if shape == "perm" else max(n, SRC_ROWS)
    src = words64(rng, src_n)
    _, snull = rm.make_nulls(rng, src_n)
    idx = None if shape == "identity" else rm.make_idx(rng, shape, n, src_n)
    d_src, d_snull, d_idx = dev.to_dev(src), dev.to_dev(snull), (None if idx is None else dev.to_dev(idx))
    for with_src_null, with_dst_null in ((False, False), (False, True), (True, True)):
        what = f"gather64 n={n} {shape} src_null={with_src_null} dst_null={with_dst_null}"
        want, want_null = rm.gather64(src, snull if with_src_null else None, idx, n, with_dst_null)
        dst, dnull = Guarded(dev, n), (nullwords(dev, n) if with_dst_null else None)
        ok(dev, dev.lib.mdb_dev_gather64(dev.h, P(d_src), P(d_snull) if with_src_null else None, P(d_idx), n, dst.ptr,
                                         dnull.ptr if dnull else None), what)
        dst.check(want, what)
        if dnull:
            dnull.check(want_null, what + " NULL words")
        if shape == "norow":
            at = rm.norow_positions(n)
            assert not want[at].any()                                   # a MDB_NO_ROW output is value 0 ...
            if with_dst_null:
                assert rm.bit_is_set(want_null, at).all()               # ... with its NULL bit set
                if not with_src_null:                                   # and without source NULL bits nothing else is NULL
                    assert np.array_equal(np.flatnonzero(D.unpack_nullbits(want_null, n)), at)


def test_gather64_source_nulls_need_destination_nulls(dev):
    rng = np.random.default_rng(1)
    src, (_, snull) = words64(rng, 300), rm.make_nulls(rng, 300)
    dst = Guarded(dev, 300)
    d_src, d_snull = dev.to_dev(src), dev.to_dev(snull)
    rc = dev.lib.mdb_dev_gather64(dev.h, P(d_src), P(d_snull), None, 300, dst.ptr, None)
    refused(dev, rc, "source has NULL bits but no destination NULL bits given")
    dst.untouched("nothing is launched")


# ------------------------------------------------------------------------------------------------------------------ gather32 / iota32 / widen32

@pytest.mark.parametrize("shape", ["identity", "repeats", "perm", "norow"])
@pytest.mark.parametrize("n", SIZES)
def test_gather32(dev, n, shape):
    rng = np.random.default_rng(n * 4 + len(shape) + 1)
    src_n = n if shape == "perm" else max(n, SRC_ROWS)
    src = rng.integers(0, 1 << 32, size=src_n, dtype=np.uint64).astype(np.uint32)
    src[rng.integers(0, src_n, size=max(src_n // 50, 1))] = rm.NO_ROW           # (a composed stream holds MDB_NO_ROW as a value too)
    idx = rm.make_idx(rng, shape, n, src_n)
    dst = Guarded(dev, n, np.uint32)
    d_src, d_idx = dev.to_dev(src), dev.to_dev(idx)
    ok(dev, dev.lib.mdb_dev_gather32(dev.h, P(d_src), P(d_idx), n, dst.ptr), "gather32")
    want = rm.gather32(src, idx, n)
    dst.check(want, f"gather32 n={n} {shape}")
    if shape == "norow":
        assert (want[rm.norow_positions(n)] == rm.NO_ROW).all()


@pytest.mark.parametrize("n", SIZES)
def test_iota32(dev, n):
    dst = Guarded(dev, n, np.uint32)
    ok(dev, dev.lib.mdb_dev_iota32(dev.h, dst.ptr, n), "iota32")
    dst.check(rm.iota32(n), f"iota32 n={n}")


@pytest.mark.parametrize("n", SIZES)
def test_widen32to64(dev, n):
    rng = np.random.default_rng(n)
    src = rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64).astype(np.int32)
    edge = np.array([-(1 << 31), -1, (1 << 31) - 1, 0], dtype=np.int32)
    src[:min(n, 4)] = edge[:min(n, 4)]
    src[n - min(n, 4):] = edge[:min(n, 4)][::-1]
    dst = Guarded(dev, n)
    d_src = dev.to_dev(src)
    ok(dev, dev.lib.mdb_dev_widen32to64(dev.h, P(d_src), n, dst.ptr), "widen32to64")
    dst.check(rm.widen32to64(src, n), f"widen32to64 n={n}")


# ------------------------------------------------------------------------------------------------------------------ scatter_set64

SCATTER_VALUE = -0x0123456789ABCDEF


def _scatter_idx(rng, shape, m):
    if shape == "all":
        return None
    k = max(1, m // 3)
    sub = rng.choice(m, size=k, replace=False)
    sub[0] = m - 1
    if k > 1:
        sub[1] = 0
    sub = np.unique(sub)
    if shape == "sorted":
        return sub.astype(np.uint32)
    if shape == "shuffled":
        return rng.permutation(sub).astype(np.uint32)
    if shape == "repeats":
        return rng.permutation(np.concatenate([sub, sub[:max(1, k // 2)], sub[:1].repeat(70)])).astype(np.uint32)
    assert shape == "words"      # every row of a few NULL words, shuffled: up to 64 threads of one wave on one word
    ws = sorted({0, (m - 1) >> 6, (m >> 7), max(((m - 1) >> 6) - 1, 0)})
    rows = np.concatenate([np.arange(w * 64, min(w * 64 + 64, m)) for w in ws])
    return rng.permutation(rows).astype(np.uint32)


@pytest.mark.parametrize("shape", ["all", "sorted", "shuffled", "repeats", "words"])
@pytest.mark.parametrize("m", [1, 64, 65, 5000, 300_001])
def test_scatter_set64(dev, m, shape):
    rng = np.random.default_rng(m + len(shape))
    col = words64(rng, m)
    _, bitmap = rm.make_nulls(rng, m, 0.5)
    if m & 63:
        assert int(bitmap[-1]) >> (m & 63), "bits behind m to preserve"
    idx = _scatter_idx(rng, shape, m)
    n = m if idx is None else len(idx)
    d_idx = None if idx is None else dev.to_dev(idx)
    for set_null, with_bitmap in ((0, True), (1, True), (0, False)):
        what = f"scatter_set64 m={m} {shape} set_null={set_null} bitmap={with_bitmap}"
        want, want_null = rm.scatter_set64(col, bitmap if with_bitmap else None, idx, n, SCATTER_VALUE, set_null)
        dst = Guarded(dev, m, init=col)
        dnull = nullwords(dev, m, init=bitmap) if with_bitmap else None
        ok(dev, dev.lib.mdb_dev_scatter_set64(dev.h, dst.ptr, dnull.ptr if dnull else None, P(d_idx), n, SCATTER_VALUE, set_null), what)
        dst.check(want, what)
        if dnull:
            dnull.check(want_null, what + " NULL words")
        if set_null:
            assert np.array_equal(want, col)                      # SET NULL changes no value
    # SET NULL without a bitmap is refused and writes nothing
    dst = Guarded(dev, m, init=col)
    refused(dev, dev.lib.mdb_dev_scatter_set64(dev.h, dst.ptr, None, P(d_idx), n, SCATTER_VALUE, 1), "SET NULL needs a NULL bitmap")
    dst.check(col, "refused call")


def test_scatter_set64_drops_what_the_operators_remember(dev):
    """the operators remember a key column's range by its address; an UPDATE far outside that range must not meet a stale verdict"""
    rng = np.random.default_rng(99)
    n = 100_000
    keys = rng.integers(0, 1000, size=n, dtype=np.int64)
    right = np.arange(0, 1000, 3, dtype=np.int64)
    d_keys, d_right = dev.to_dev(keys), dev.to_dev(right)

    def both():
        f, c = dev.group_count(d_keys, None)
        ef, ec = orc.group_count(keys, None)
        assert np.array_equal(f.cpu().numpy().astype(np.int64), ef) and np.array_equal(c.cpu().numpy(), ec)
        k, c, f, j = dev.join_group_count(d_keys, None, d_right, None)
        ek, ec, ef, ej = orc.join_group_count(keys, None, right, None)
        assert j == ej and np.array_equal(k.cpu().numpy(), ek) and np.array_equal(c.cpu().numpy(), ec)
        assert np.array_equal(f.cpu().numpy().astype(np.int64), ef)

    both()
    both()                                                          # (verdicts are remembered after a use)
    far = 1 << 50
    rows = rng.choice(n, size=777, replace=False).astype(np.uint32)
    d_rows = dev.to_dev(rows)
    ok(dev, dev.lib.mdb_dev_scatter_set64(dev.h, P(d_keys), None, P(d_rows), len(rows), far, 0), "scatter_set64")
    keys[rows.astype(np.int64)] = far
    right = np.append(right, far)
    d_right = dev.to_dev(right)
    assert np.array_equal(d_keys.cpu().numpy(), keys)
    both()
    both()


# ------------------------------------------------------------------------------------------------------------------ map_ids

def _map_case(rng, n, table_n):
    pool = np.array([-1, I64_MIN, 0, table_n - 1, table_n, table_n + 1, I64_MAX], dtype=np.int64)
    cells = np.where(rng.random(n) < 0.5, rng.integers(0, table_n, size=n, dtype=np.int64), pool[rng.integers(0, len(pool), size=n)])
    cells[:min(n, len(pool))] = pool[:min(n, len(pool))]
    cells[n - 1] = pool[n % len(pool)]
    table = rng.integers(I64_MIN, I64_MAX, size=table_n, dtype=np.int64) | 1     # (never 0: a mapped cell differs from a refused one)
    return cells, table


@pytest.mark.parametrize("n", SIZES + (16384 * 256 + 257,))      # the last: past the grid cap of 16384 blocks, the grid-stride loop
def test_map_ids(dev, n):
    rng = np.random.default_rng(n)
    cells, table = _map_case(rng, n, 1000)
    out = Guarded(dev, n)
    d_cells, d_table = dev.to_dev(cells), dev.to_dev(table)
    ok(dev, dev.lib.mdb_dev_map_ids(dev.h, P(d_cells), n, P(d_table), len(table), out.ptr), "map_ids")
    out.check(rm.map_ids(cells, table), f"map_ids n={n}")


def test_map_ids_in_place_and_empty(dev):
    rng = np.random.default_rng(4)
    cells, table = _map_case(rng, 2049, 17)
    buf = Guarded(dev, 2049, init=cells)
    d_table = dev.to_dev(table)
    ok(dev, dev.lib.mdb_dev_map_ids(dev.h, buf.ptr, 2049, P(d_table), len(table), buf.ptr), "map_ids in place")
    buf.check(rm.map_ids(cells, table), "map_ids in place")
    ok(dev, dev.lib.mdb_dev_map_ids(dev.h, None, 0, None, 0, None), "map_ids n=0")
    assert dev.map_ids(dev.to_dev(cells), d_table).cpu().numpy().tolist() == rm.map_ids(cells, table).tolist()


# ------------------------------------------------------------------------------------------------------------------ combine_counts

@pytest.mark.parametrize("n", SIZES)
def test_combine_counts(dev, n):
    rng = np.random.default_rng(n)
    g1 = 3000
    cnt1 = rng.integers(1 << 17, 1 << 20, size=g1, dtype=np.int64)          # every product >= 2^34: the sum passes 2^32 at n = 1
    cnt2 = rng.integers(1 << 17, 1 << 20, size=n, dtype=np.int64)           # and stays below 2^59
    first1 = rng.integers(0, 1 << 32, size=g1, dtype=np.uint64).astype(np.uint32)
    idx = rng.integers(0, g1, size=n, dtype=np.int64).astype(np.uint32)     # (with repeats)
    idx[0], idx[n - 1] = g1 - 1, 0
    d = [dev.to_dev(a) for a in (cnt1, first1, idx, cnt2)]
    for with_first1, with_out_first in ((True, True), (False, True), (True, False)):
        what = f"combine_counts n={n} first1={with_first1} out_first={with_out_first}"
        want, want_first, want_sum = rm.combine_counts(cnt1, first1 if with_first1 else None, idx, cnt2, n)
        exact = sum(int(cnt1[int(g)]) * int(c) for g, c in zip(idx, cnt2))
        assert 1 << 32 < exact < 1 << 63 and exact == want_sum
        out, outf, tot = Guarded(dev, n), Guarded(dev, n, np.uint32), c_uint64(VAL)
        ok(dev, dev.lib.mdb_dev_combine_counts(dev.h, P(d[0]), P(d[1]) if with_first1 else None, P(d[2]), P(d[3]), n, out.ptr,
                                               outf.ptr if with_out_first else None, byref(tot)), what)
        out.check(want, what)
        if with_out_first:
            outf.check(want_first, what + " first rows")
        else:
            outf.untouched(what)
        assert tot.value == exact, what


# ------------------------------------------------------------------------------------------------------------------ key_range

def _key_range(dev, keys, nulls):
    lo, hi = c_int64(123), c_int64(456)
    d_keys, d_nulls = dev.to_dev(keys), (None if nulls is None else dev.to_dev(nulls))
    ok(dev, dev.lib.mdb_dev_key_range(dev.h, P(d_keys), P(d_nulls), len(keys), byref(lo), byref(hi)), "key_range")
    return lo.value, hi.value


@pytest.mark.parametrize("with_nulls", [False, True])
@pytest.mark.parametrize("n", SIZES + (4096 * 2048 + 2049,))     # the last: past the grid cap of 4096 blocks
def test_key_range(dev, n, with_nulls):
    rng = np.random.default_rng(n + with_nulls)
    keys = rng.integers(-(1 << 40), 1 << 40, size=n, dtype=np.int64)
    nulls = None
    if with_nulls:
        nulls = words64(rng, rm.words_for(n))                      # half the rows NULL; the padding bits random too
        stale = np.flatnonzero(rm.bit_is_set(nulls, np.arange(n)))
        keys[stale[::2]], keys[stale[1::2]] = I64_MIN, I64_MAX     # NULL rows hold more extreme stale values than any live row
    assert _key_range(dev, keys, nulls) == rm.key_range(keys, nulls, n)
    if n >= 2:                                                     # the extremes themselves, at the last and the first row
        keys[n - 1], keys[0] = I64_MIN, I64_MAX
        if nulls is not None:
            nulls[0] &= ~np.uint64(1)
            nulls[(n - 1) >> 6] &= ~np.uint64(1 << ((n - 1) & 63))
        assert _key_range(dev, keys, nulls) == (I64_MIN, I64_MAX) == rm.key_range(keys, nulls, n)


@pytest.mark.parametrize("n", [1, 64, 200, 2049])
def test_key_range_all_null(dev, n):
    keys = np.arange(n, dtype=np.int64)
    assert _key_range(dev, keys, D.pack_nullbits(np.ones(n, dtype=bool))) == (I64_MAX, I64_MIN)


@pytest.mark.parametrize("row", [0, 63, 127, 4095, 4159])           # row 0, last rows of a NULL word, row n-1
def test_key_range_one_live_row(dev, row):
    n = 4160
    keys = np.where(np.arange(n) & 1, I64_MIN, I64_MAX).astype(np.int64)      # stale values of the NULL rows
    flags = np.ones(n, dtype=bool)
    flags[row] = False
    for v in (42, -42, I64_MIN, I64_MAX):
        keys[row] = v
        assert _key_range(dev, keys, D.pack_nullbits(flags)) == (v, v) == rm.key_range(keys, D.pack_nullbits(flags), n)


# ------------------------------------------------------------------------------------------------------------------ distinct_scan

def _column(n, lo):
    """n distinct keys lo .. lo + n - 1 in a fixed shuffled order"""
    return (np.random.default_rng(n).permutation(n) + lo).astype(np.int64)


def _distinct_cases():
    n = 3000
    base = _column(n, 0)
    cases = {"no duplicate": (base, None, 0, n)}
    k = base.copy()
    k[n - 1] = k[0]
    cases["one pair at the two ends"] = (k, None, 0, n)
    k = base.copy()
    k[n - 1] = k[0]
    flags = np.zeros(n, dtype=bool)
    flags[[0, n - 1]] = True
    cases["a pair among NULL rows only"] = (k, D.pack_nullbits(flags), 0, n)
    flags = np.zeros(n, dtype=bool)
    flags[n - 1] = True
    cases["one of a pair NULL"] = (k, D.pack_nullbits(flags), 0, n)
    cases["a key just below the window"] = (_column(n, -1), None, 0, n)
    cases["a key just above the window"] = (_column(n, 0), None, 0, n - 1)
    k = base.copy()
    flags = np.zeros(n, dtype=bool)
    flags[int(np.flatnonzero(k == n - 1)[0])] = True
    cases["the key above the window is NULL"] = (k, D.pack_nullbits(flags), 0, n - 1)
    cases["negative lo"] = (_column(n, -1777), None, -1777, n)
    cases["lo = INT64_MIN"] = ((_column(n, 0) + I64_MIN).astype(np.int64), None, I64_MIN, n)
    cases["lo = INT64_MIN, key INT64_MAX outside"] = (np.append((_column(n, 0) + I64_MIN).astype(np.int64), np.int64(I64_MAX)), None, I64_MIN, n)
    cases["window_bits = 3001, no multiple of 32"] = (_column(3001, 5), None, 5, 3001)
    cases["window_bits = 33, last bit used"] = (_column(33, -16), None, -16, 33)
    cases["wide sparse window"] = (_column(n, 0) * 37 - 50_000, None, -50_000, 37 * n)
    return cases


DISTINCT = _distinct_cases()
DISTINCT_TWICE = {"one pair at the two ends", "a key just below the window", "a key just above the window", "lo = INT64_MIN, key INT64_MAX outside"}


@pytest.mark.parametrize("name", list(DISTINCT))
def test_distinct_scan(dev, name):
    keys, nulls, lo, bits = DISTINCT[name]
    n = len(keys)
    words = (bits + 31) // 32
    want_twice, want_seen = rm.distinct_scan(keys, nulls, n, lo, bits, np.zeros(words, dtype=np.uint32))
    assert want_twice == (1 if name in DISTINCT_TWICE else 0)
    seen = Guarded(dev, words, np.uint32, init=np.zeros(words, dtype=np.uint32))          # the caller clears the bitmap
    tw = c_int(-1)
    d_keys, d_nulls = dev.to_dev(keys), (None if nulls is None else dev.to_dev(nulls))
    ok(dev, dev.lib.mdb_dev_distinct_scan(dev.h, P(d_keys), P(d_nulls), n, lo, bits, seen.ptr, byref(tw)), name)
    assert tw.value == want_twice, name
    seen.check(want_seen, name)          # (the bits do not depend on the order of the rows, so they are exact in every case)
    if not want_twice:                   # the rows again into the kept bitmap: every key is there twice now
        ok(dev, dev.lib.mdb_dev_distinct_scan(dev.h, P(d_keys), P(d_nulls), n, lo, bits, seen.ptr, byref(tw)), name)
        assert tw.value == rm.distinct_scan(keys, nulls, n, lo, bits, want_seen)[0] == (1 if len(np.flatnonzero(want_seen)) else 0)
        seen.check(want_seen, name + ", second scan")


# ------------------------------------------------------------------------------------------------------------------ cross_pairs

@pytest.mark.parametrize("n_l,n_r", [(1, 1), (1, 2049), (2049, 1), (3, 683), (47, 131), (2048, 2)])
def test_cross_pairs(dev, n_l, n_r):
    out_l, out_r = Guarded(dev, n_l * n_r, np.uint32), Guarded(dev, n_l * n_r, np.uint32)
    ok(dev, dev.lib.mdb_dev_cross_pairs(dev.h, n_l, n_r, out_l.ptr, out_r.ptr), "cross_pairs")
    want_l, want_r = rm.cross_pairs(n_l, n_r)
    out_l.check(want_l, f"cross_pairs {n_l} x {n_r} left")
    out_r.check(want_r, f"cross_pairs {n_l} x {n_r} right")
    assert want_l.tolist() == sorted(want_l.tolist()) and want_r[:n_r].tolist() == list(range(n_r))      # row-major


@pytest.mark.parametrize("n_l,n_r", [(0, 5), (5, 0), (0, 0)])
def test_cross_pairs_of_an_empty_side_writes_nothing(dev, n_l, n_r):
    out_l, out_r = Guarded(dev, 64, np.uint32), Guarded(dev, 64, np.uint32)
    ok(dev, dev.lib.mdb_dev_cross_pairs(dev.h, n_l, n_r, out_l.ptr, out_r.ptr), "cross_pairs")
    out_l.untouched()
    out_r.untouched()


@pytest.mark.parametrize("n_l,n_r", [(1 << 16, 1 << 16), (1 << 32, 1), (1, 1 << 32),
                                     ((1 << 63) + 1, 2),             # the 64-bit product wraps to 2
                                     (1 << 32, 1 << 32)])            # ... and to 0
def test_cross_pairs_too_large_is_refused(dev, n_l, n_r):
    out_l, out_r = Guarded(dev, 64, np.uint32), Guarded(dev, 64, np.uint32)      # (room for what a wrapped product of 2 would write)
    rc = dev.lib.mdb_dev_cross_pairs(dev.h, n_l, n_r, out_l.ptr, out_r.ptr)
    out_l.untouched()
    out_r.untouched()
    refused(dev, rc, "is too large")


# ------------------------------------------------------------------------------------------------------------------ double_join_keys

@pytest.mark.parametrize("shape", ["identity", "repeats", "norow"])
@pytest.mark.parametrize("n", SIZES)
def test_double_join_keys(dev, n, shape):
    rng = np.random.default_rng(n * 4 + len(shape) + 2)
    src_n = max(n, SRC_ROWS)
    sp = rm.double_specials()
    src = np.where(rng.random(src_n) < 0.5, rng.standard_normal(src_n).view(np.uint64), words64(rng, src_n))
    at = rng.permutation(src_n)[:4 * len(sp)].reshape(4, len(sp))
    for rows in at:
        src[rows] = sp
    src[:min(n, len(sp))] = sp[:min(n, len(sp))]
    src[n - 1] = sp[-1 - (n % len(sp))]
    _, snull = rm.make_nulls(rng, src_n, 0.2)
    idx = None if shape == "identity" else rm.make_idx(rng, shape, n, src_n)
    if idx is not None and n > 400:
        idx[200:200 + len(sp)] = at[0]                               # every special value is gathered ...
        idx[300:300 + len(sp)] = at[1]
    d_src, d_snull, d_idx = dev.to_dev(src), dev.to_dev(snull), (None if idx is None else dev.to_dev(idx))
    for with_src_null in (False, True):
        what = f"double_join_keys n={n} {shape} src_null={with_src_null}"
        want, want_null = rm.double_join_keys(src, snull if with_src_null else None, idx, n)
        dst, dnull = Guarded(dev, n), nullwords(dev, n)
        ok(dev, dev.lib.mdb_dev_double_join_keys(dev.h, P(d_src), P(d_snull) if with_src_null else None, P(d_idx), n, dst.ptr, dnull.ptr), what)
        dst.check(want, what)
        dnull.check(want_null, what + " NULL words")


def test_double_join_keys_special_values(dev):
    """the whole table on its own: +-inf keep their words and are no NULL, every NaN is NULL, -0.0 becomes +0.0"""
    sp = rm.double_specials()
    n = len(sp)
    want, want_null = rm.double_join_keys(sp, None, None, n)
    dst, dnull = Guarded(dev, n), nullwords(dev, n)
    d_sp = dev.to_dev(sp)
    ok(dev, dev.lib.mdb_dev_double_join_keys(dev.h, P(d_sp), None, None, n, dst.ptr, dnull.ptr), "double_join_keys")
    dst.check(want)
    dnull.check(want_null)
    vals = sp.view(np.float64)
    assert np.array_equal(D.unpack_nullbits(want_null, n), np.isnan(vals))
    assert np.isinf(vals).sum() == 2 and np.isnan(vals).sum() == 12
    assert np.array_equal(want[vals == 0.0], np.zeros(2, dtype=np.uint64))


def test_double_join_keys_needs_destination_nulls(dev):
    dst = Guarded(dev, 64)
    d_src = dev.to_dev(np.zeros(64))
    rc = dev.lib.mdb_dev_double_join_keys(dev.h, P(d_src), None, None, 64, dst.ptr, None)
    refused(dev, rc, "destination values and NULL bits are both required")
    dst.untouched()


# ------------------------------------------------------------------------------------------------------------------ allocator bookkeeping

def test_allocator_bookkeeping(dev):
    """Every pointer is freed exactly as often as it was acquired (one alloc + its retains): a surplus mdb_dev_free would fall through to a
    plain hipFree."""
    lib, h = dev.lib, dev.h
    size = 3 * 4096 + 8
    acquired = {}

    def alloc():
        p = c_void_p()
        ok(dev, lib.mdb_dev_alloc(h, c_size_t(size), byref(p)), "alloc")
        assert p.value and p.value not in acquired
        acquired[p.value] = 1
        return p

    def free(p):
        assert acquired.get(p.value, 0) > 0, "never free a pointer more often than it was acquired"
        acquired[p.value] -= 1
        ok(dev, lib.mdb_dev_free(h, p), "free")

    buf = alloc()
    live = lib.mdb_dev_alloc_size(h, buf)
    assert size <= live <= 2 * size + 4096                         # (a released buffer of up to twice the size may serve)
    assert lib.mdb_dev_holders(h, buf) == 0
    inside = c_void_p(buf.value + 8)
    assert lib.mdb_dev_alloc_size(h, inside) == 0 and lib.mdb_dev_alloc_size(h, None) == 0
    assert lib.mdb_dev_retain(h, inside) == ERR and lib.mdb_dev_retain(h, None) == ERR
    assert lib.mdb_dev_holders(h, inside) == 0

    for _ in range(2):
        ok(dev, lib.mdb_dev_retain(h, buf), "retain")
        acquired[buf.value] += 1
    assert lib.mdb_dev_holders(h, buf) == 2
    pattern = np.random.default_rng(8).integers(0, 256, size=size, dtype=np.uint8)
    ok(dev, lib.mdb_dev_h2d(h, buf, c_void_p(pattern.ctypes.data), c_size_t(size)), "h2d")

    free(buf)                                                       # one holder gone: still live
    assert lib.mdb_dev_alloc_size(h, buf) == live and lib.mdb_dev_holders(h, buf) == 1
    others = [alloc() for _ in range(3)]                            # same size: none of them may be the retained buffer
    for i, o in enumerate(others):
        junk = np.full(size, 0x11 * (i + 1), dtype=np.uint8)
        ok(dev, lib.mdb_dev_h2d(h, o, c_void_p(junk.ctypes.data), c_size_t(size)), "h2d")
    back = np.zeros(size, dtype=np.uint8)
    ok(dev, lib.mdb_dev_d2h(h, c_void_p(back.ctypes.data), buf, c_size_t(size)), "d2h")
    assert np.array_equal(back, pattern)

    free(buf)                                                       # the other holder
    assert lib.mdb_dev_alloc_size(h, buf) == live and lib.mdb_dev_holders(h, buf) == 0
    ok(dev, lib.mdb_dev_d2h(h, c_void_p(back.ctypes.data), buf, c_size_t(size)), "d2h")
    assert np.array_equal(back, pattern)
    free(buf)                                                       # the owner
    assert lib.mdb_dev_alloc_size(h, buf) == 0 and lib.mdb_dev_holders(h, buf) == 0
    assert lib.mdb_dev_retain(h, buf) == ERR                        # released: unknown again
    for o in others:
        free(o)
        assert lib.mdb_dev_alloc_size(h, o) == 0
    assert not any(acquired.values())
