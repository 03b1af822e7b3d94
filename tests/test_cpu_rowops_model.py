"""tests/rowops_model.py (the reference of tests/test_row_primitives_gpu.py) against independent restatements: loops over Python ints,
math / struct for the DOUBLE cases, and midoridb_amd.dev's pack_nullbits / unpack_nullbits.  Small inputs, no GPU."""
import math
import struct

import numpy as np
import pytest

from midoridb_amd import dev as D
from tests import rowops_model as rm

M64 = (1 << 64) - 1


def _bit(words, i):
    return (int(words[i >> 6]) >> (i & 63)) & 1


def _src(rng, rows):
    return rng.integers(0, 1 << 64, size=rows, dtype=np.uint64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 257])
def test_pack_bits_is_pack_nullbits(n):
    rng = np.random.default_rng(n)
    flags = rng.random(n) < 0.5
    words = rm.pack_bits(flags)
    assert np.array_equal(words, D.pack_nullbits(flags))
    assert np.array_equal(D.unpack_nullbits(words, n), flags)
    assert np.array_equal(rm.bit_is_set(words, np.arange(n)), flags)
    if n & 63:
        assert int(words[-1]) >> (n & 63) == 0


def test_make_nulls_sets_word_edges_and_stale_tail():
    flags, words = rm.make_nulls(np.random.default_rng(1), 200)
    assert flags[0] and flags[63] and flags[191] and flags[128]
    assert np.array_equal(D.unpack_nullbits(words, 200), flags)
    assert len(words) == 4


@pytest.mark.parametrize("shape", ["identity", "repeats", "perm", "norow"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300, 2500])
def test_make_idx(shape, n):
    src_n = n if shape == "perm" else max(n, 500)
    idx = rm.make_idx(np.random.default_rng(n), shape, n, src_n)
    assert idx.dtype == np.uint32 and len(idx) == n
    live = idx[idx != rm.NO_ROW]
    assert (live < src_n).all()                          # only valid row ids or MDB_NO_ROW
    if shape != "norow":
        assert len(live) == n
    if shape == "perm":
        assert len(set(idx.tolist())) == n
    if shape == "identity":
        assert idx.tolist() == list(range(n))
    if shape in ("repeats", "perm") and n >= 4:
        assert 0 in idx and src_n - 1 in idx
    if shape == "norow":
        pos = set(rm.norow_positions(n).tolist())
        assert {0, n - 1} <= pos
        assert pos == set(np.flatnonzero(idx == rm.NO_ROW).tolist())
        if n >= 192:
            assert set(range(128, 192)) <= pos and {63, 64, 127} <= pos


@pytest.mark.parametrize("shape", [None, "repeats", "norow"])
@pytest.mark.parametrize("with_src_null", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_gather64(shape, with_src_null, n):
    rng = np.random.default_rng(n + 7)
    src_n = 300
    src = _src(rng, src_n)
    flags, words = rm.make_nulls(rng, src_n)
    idx = None if shape is None else rm.make_idx(rng, shape, n, src_n)
    dst, nw = rm.gather64(src, words if with_src_null else None, idx, n, True)
    assert len(nw) == (n + 63) // 64
    for k in range(n):
        row = k if idx is None else int(idx[k])
        if row == rm.NO_ROW:
            assert int(dst[k]) == 0 and _bit(nw, k) == 1
        else:
            assert int(dst[k]) == int(src[row])
            assert _bit(nw, k) == (int(flags[row]) if with_src_null else 0)
    for k in range(n, len(nw) * 64):
        assert _bit(nw, k) == 0
    if not with_src_null:
        d2, none = rm.gather64(src, None, idx, n, False)
        assert none is None and np.array_equal(d2, dst)
    else:
        with pytest.raises(ValueError):
            rm.gather64(src, words, idx, n, False)


@pytest.mark.parametrize("shape", ["identity", "repeats", "perm", "norow"])
def test_gather32(shape):
    rng = np.random.default_rng(3)
    n, src_n = 200, 200
    src = rng.integers(0, 1 << 32, size=src_n, dtype=np.uint64).astype(np.uint32)
    idx = rm.make_idx(rng, shape, n, src_n)
    out = rm.gather32(src, idx, n)
    assert out.dtype == np.uint32
    assert out.tolist() == [rm.NO_ROW if int(i) == rm.NO_ROW else int(src[int(i)]) for i in idx]


def test_iota32_widen32_map_ids():
    assert rm.iota32(5).tolist() == [0, 1, 2, 3, 4] and rm.iota32(5).dtype == np.uint32
    src = np.array([-(1 << 31), -1, 0, 1, (1 << 31) - 1], dtype=np.int32)
    w = rm.widen32to64(src, 5)
    assert w.dtype == np.int64 and w.tolist() == [-(1 << 31), -1, 0, 1, (1 << 31) - 1]
    table = np.array([11, -22, 33], dtype=np.int64)
    cells = np.array([-1, rm.I64_MIN, 0, 2, 3, 4, rm.I64_MAX, 1], dtype=np.int64)
    assert rm.map_ids(cells, table).tolist() == [0, 0, 11, 33, 0, 0, 0, -22]
    assert rm.map_ids(cells, np.zeros(0, dtype=np.int64)).tolist() == [0] * 8


@pytest.mark.parametrize("set_null", [0, 1])
@pytest.mark.parametrize("with_null", [False, True])
@pytest.mark.parametrize("shape", [None, "sorted", "repeats"])
def test_scatter_set64(set_null, with_null, shape):
    rng = np.random.default_rng(11)
    m = 150
    dst = _src(rng, m)
    _, words = rm.make_nulls(rng, m, 0.5)
    idx = None if shape is None else (np.array([0, 5, 63, 64, 149], dtype=np.uint32) if shape == "sorted" else
                                      np.array([149, 7, 7, 64, 0, 7, 64], dtype=np.uint32))
    n = m if idx is None else len(idx)
    value = -0x123456789ABCDEF
    if set_null and not with_null:
        with pytest.raises(ValueError):
            rm.scatter_set64(dst, None, idx, n, value, set_null)
        return
    d2, w2 = rm.scatter_set64(dst, words if with_null else None, idx, n, value, set_null)
    chosen = set(range(m)) if idx is None else set(int(i) for i in idx)
    for r in range(m):
        if r in chosen and not set_null:
            assert int(d2[r]) == value & M64
        else:
            assert int(d2[r]) == int(dst[r])
    if not with_null:
        assert w2 is None
        return
    for b in range(len(words) * 64):            # the bits behind m included
        if b in chosen:
            assert _bit(w2, b) == (1 if set_null else 0)
        else:
            assert _bit(w2, b) == _bit(words, b)
    assert int(words[-1]) >> (m & 63), "the starting bitmap has bits behind m to preserve"


def test_combine_counts():
    rng = np.random.default_rng(5)
    g1, n = 40, 100
    cnt1 = rng.integers(1 << 17, 1 << 20, size=g1, dtype=np.int64)
    cnt2 = rng.integers(1 << 17, 1 << 20, size=n, dtype=np.int64)
    first1 = rng.integers(0, 1 << 32, size=g1, dtype=np.uint64).astype(np.uint32)
    idx = rng.integers(0, g1, size=n).astype(np.uint32)
    out, first, total = rm.combine_counts(cnt1, first1, idx, cnt2, n)
    want = [int(cnt1[int(i)]) * int(c) for i, c in zip(idx, cnt2)]
    assert out.tolist() == want and total == sum(want)
    assert 1 << 32 < total < 1 << 63
    assert first.tolist() == [int(first1[int(i)]) for i in idx]
    assert rm.combine_counts(cnt1, None, idx, cnt2, n)[1].tolist() == idx.tolist()
    # one row alone already passes 2^32
    assert rm.combine_counts(cnt1, None, idx, cnt2, 1)[2] == want[0] > 1 << 32


def test_key_range():
    keys = np.array([5, rm.I64_MIN, -3, rm.I64_MAX, 9], dtype=np.int64)
    assert rm.key_range(keys, None, 5) == (rm.I64_MIN, rm.I64_MAX)
    nulls = D.pack_nullbits([0, 1, 0, 1, 0])
    assert rm.key_range(keys, nulls, 5) == (-3, 9)              # the stale extremes of NULL rows do not count
    assert rm.key_range(keys, D.pack_nullbits([1] * 5), 5) == (rm.I64_MAX, rm.I64_MIN)
    assert rm.key_range(keys, D.pack_nullbits([1, 1, 1, 1, 0]), 5) == (9, 9)
    assert rm.key_range(keys, None, 1) == (5, 5)


def test_distinct_scan():
    z = np.zeros(2, dtype=np.uint32)
    keys = np.array([-3, 0, 36, 5], dtype=np.int64)
    tw, seen = rm.distinct_scan(keys, None, 4, -3, 40, z)
    assert tw == 0 and int(seen[0]) == (1 << 0) | (1 << 3) | (1 << 8) and int(seen[1]) == 1 << 7 and not z.any()
    assert rm.distinct_scan(np.array([7, 1, 7], dtype=np.int64), None, 3, 0, 8, z)[0] == 1
    # a duplicate among NULL rows only is no duplicate, and NULL rows set no bit
    tw, seen = rm.distinct_scan(np.array([7, 7, 1], dtype=np.int64), D.pack_nullbits([1, 1, 0]), 3, 0, 8, z)
    assert tw == 0 and seen.tolist() == [2, 0]
    # just below / just above the window: "twice", and nothing is set for that key
    for k in (-1, 8):
        tw, seen = rm.distinct_scan(np.array([k, 3], dtype=np.int64), None, 2, 0, 8, z)
        assert tw == 1 and seen.tolist() == [8, 0]
    # a window from INT64_MIN; a bit set by earlier rows counts
    tw, seen = rm.distinct_scan(np.array([rm.I64_MIN, rm.I64_MIN + 33], dtype=np.int64), None, 2, rm.I64_MIN, 34, z)
    assert tw == 0 and seen.tolist() == [1, 2]
    assert rm.distinct_scan(np.array([rm.I64_MIN + 33], dtype=np.int64), None, 1, rm.I64_MIN, 34, seen)[0] == 1
    assert rm.distinct_scan(np.array([rm.I64_MAX], dtype=np.int64), None, 1, rm.I64_MIN, 34, z)[0] == 1


@pytest.mark.parametrize("n_l,n_r", [(1, 1), (1, 7), (7, 1), (3, 5), (0, 4), (4, 0)])
def test_cross_pairs(n_l, n_r):
    left, right = rm.cross_pairs(n_l, n_r)
    want = [(a, b) for a in range(n_l) for b in range(n_r)]
    assert list(zip(left.tolist(), right.tolist())) == want
    assert left.dtype == right.dtype == np.uint32


def test_cross_pairs_too_large():
    for n_l, n_r in ((1 << 16, 1 << 16), ((1 << 63) + 1, 2), (1 << 32, 1)):
        with pytest.raises(ValueError):
            rm.cross_pairs(n_l, n_r)


def test_double_specials_table():
    words = rm.double_specials()
    assert len(set(words.tolist())) == len(words) == 26
    vals = [struct.unpack("<d", struct.pack("<Q", int(w)))[0] for w in words]
    assert sum(math.isnan(v) for v in vals) == 12 and sum(math.isinf(v) for v in vals) == 2
    assert sum(v == 0.0 for v in vals) == 2 and 5e-324 in vals and -5e-324 in vals
    for frac in (1, 1 << 50, 1 << 51, (1 << 51) | 1):       # lowest / highest mantissa bits, signalling and quiet, both signs
        for sign in (0, 1 << 63):
            assert sign | 0x7FF0000000000000 | frac in words.tolist()


@pytest.mark.parametrize("shape", [None, "norow"])
def test_double_join_keys(shape):
    rng = np.random.default_rng(17)
    sp = rm.double_specials()
    src = np.concatenate([sp, rng.standard_normal(200 - len(sp)).view(np.uint64)])
    flags, words = rm.make_nulls(rng, 200, 0.2)
    n = 200
    idx = None if shape is None else rm.make_idx(rng, shape, n, 200)
    for nulls in (None, words):
        dst, nw = rm.double_join_keys(src, nulls, idx, n)
        assert len(nw) == 4 and int(nw[-1]) >> (n & 63) == 0
        for k in range(n):
            row = k if idx is None else int(idx[k])
            if row == rm.NO_ROW:
                assert int(dst[k]) == 0 and _bit(nw, k) == 1
                continue
            x = struct.unpack("<d", struct.pack("<Q", int(src[row])))[0]
            if x == 0.0:
                assert int(dst[k]) == 0                     # -0.0 and +0.0 are one key
            else:
                assert int(dst[k]) == int(src[row])         # everything else keeps its bits, NaN payloads included
            assert _bit(nw, k) == int(math.isnan(x) or (nulls is not None and bool(flags[row])))
