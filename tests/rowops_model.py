"""The row primitives of midoridb_amd/csrc/mdb_dev_core.hip (include/mdb_dev.h) restated in plain numpy: the reference that
tests/test_row_primitives_gpu.py holds every kernel against, and that tests/test_cpu_rowops_model.py checks on the CPU.

Values are 64-bit words (uint64 arrays: an INT64 or DOUBLE cell by its bits), row-id vectors are uint32, NULL bitmaps are uint64
words with bit (i & 63) of word (i >> 6) standing for row i.  Every function returns the COMPLETE output buffers a caller sees after
the call, the last NULL word with its bits at positions >= n included:

    gather64 / double_join_keys   write whole NULL words (one wave ballot each): bits >= n of the last word are 0
    scatter_set64                 touches single bits: every bit it does not select, bits >= m included, keeps its old value

Nothing here is fast or clever on purpose.
"""
import numpy as np

NO_ROW = 0xFFFFFFFF
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BLOCK = 2048            # STREAM_THREADS * STREAM_ROUNDS: outputs per workgroup of the stream-shaped kernels
# every size at which a stream-shaped kernel changes its path: one lane, a wave's last lane / a whole wave / one lane more, a
# workgroup round (256), a full block (the gather kernels' "full block" path starts there), three full blocks plus 65
SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 6209)
M64 = (1 << 64) - 1


def words_for(n):
    return (n + 63) // 64


def pack_bits(flags):
    """bool array -> uint64 words, the padding bits of the last word 0"""
    flags = np.asarray(flags, dtype=bool)
    return _mask_words(np.flatnonzero(flags), words_for(len(flags)))


def _mask_words(rows, words):
    """uint64[words] with the bits of `rows` set"""
    rows = np.asarray(rows, dtype=np.uint64)
    out = np.zeros(words, dtype=np.uint64)
    np.bitwise_or.at(out, (rows >> np.uint64(6)).astype(np.int64), np.uint64(1) << (rows & np.uint64(63)))
    return out


def bit_is_set(words, rows):
    """the bits of `rows` (an integer array) in `words` as a bool array"""
    rows = np.asarray(rows, dtype=np.uint64)
    return ((np.asarray(words, dtype=np.uint64)[(rows >> np.uint64(6)).astype(np.int64)] >> (rows & np.uint64(63))) & np.uint64(1)).astype(bool)


def _rows(idx, n):
    """(source rows with 0 in place of MDB_NO_ROW, absent flags) of an n-row output"""
    if idx is None:
        return np.arange(n, dtype=np.int64), np.zeros(n, dtype=bool)
    idx = np.asarray(idx, dtype=np.uint32)[:n]
    absent = idx == np.uint32(NO_ROW)
    return np.where(absent, 0, idx.astype(np.int64)), absent


def gather64(src, src_null, idx, n, want_null):
    """mdb_dev_gather64 -> (dst uint64[n], NULL words or None).  want_null: the caller gave dst_nullbits.  A MDB_NO_ROW output is
    0 with its NULL bit set; the source's NULL bits are carried."""
    if src_null is not None and not want_null:
        raise ValueError("gather64: source has NULL bits but no destination NULL bits given")
    src = np.asarray(src, dtype=np.uint64)
    rows, absent = _rows(idx, n)
    dst = np.where(absent, np.uint64(0), src[rows]) if n else np.zeros(0, dtype=np.uint64)
    if not want_null:
        return dst.astype(np.uint64), None
    isnull = absent.copy()
    if src_null is not None and n:
        isnull |= ~absent & bit_is_set(src_null, rows)
    return dst.astype(np.uint64), pack_bits(isnull)


def gather32(src, idx, n):
    """mdb_dev_gather32: dst[k] = src[idx[k]], MDB_NO_ROW where idx[k] is MDB_NO_ROW (idx is required)"""
    src = np.asarray(src, dtype=np.uint32)
    rows, absent = _rows(idx, n)
    return np.where(absent, np.uint32(NO_ROW), src[rows]).astype(np.uint32)


def iota32(n):
    return np.arange(n, dtype=np.uint32)


def scatter_set64(dst, nullwords, idx, n, value, set_null):
    """mdb_dev_scatter_set64 over copies of the buffers -> (dst, NULL words or None).  Selected rows: idx[0..n), or 0..n-1.
    set_null == 0: the value is written and the bits are cleared; set_null != 0: the bits are set and NO value changes."""
    if set_null and nullwords is None:
        raise ValueError("scatter_set64: SET NULL needs a NULL bitmap")
    dst = np.array(dst, dtype=np.uint64)
    nw = None if nullwords is None else np.array(nullwords, dtype=np.uint64)
    rows = np.arange(n, dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.uint32)[:n].astype(np.int64)
    if not set_null:
        dst[rows] = np.uint64(int(value) & M64)
    if nw is not None:
        mask = _mask_words(rows, len(nw))
        nw = (nw | mask) if set_null else (nw & ~mask)
    return dst, nw


def map_ids(cells, table):
    """mdb_dev_map_ids: out[i] = table[cells[i]] for 0 <= cells[i] < len(table), else 0"""
    cells = np.asarray(cells, dtype=np.int64)
    table = np.asarray(table, dtype=np.int64)
    ok = (cells >= 0) & (cells < len(table))
    out = np.zeros(len(cells), dtype=np.int64)
    if len(table):
        out[ok] = table[cells[ok]]
    return out


def combine_counts(cnt1, first1, idx, cnt2, n):
    """mdb_dev_combine_counts -> (out_cnt int64[n], out_first uint32[n], sum modulo 2^64 as a Python int)"""
    cnt1 = np.asarray(cnt1, dtype=np.int64)
    cnt2 = np.asarray(cnt2, dtype=np.int64)[:n]
    g = np.asarray(idx, dtype=np.uint32)[:n].astype(np.int64)
    with np.errstate(over="ignore"):
        out = cnt1[g] * cnt2
    first = g.astype(np.uint32) if first1 is None else np.asarray(first1, dtype=np.uint32)[g]
    total = 0
    for c in out.view(np.uint64).tolist():
        total = (total + c) & M64
    return out, first, total


def key_range(keys, nullwords, n):
    """mdb_dev_key_range: (min, max) of the non-NULL keys, (INT64_MAX, INT64_MIN) when there is none"""
    keys = np.asarray(keys, dtype=np.int64)[:n]
    live = np.ones(n, dtype=bool) if nullwords is None else ~bit_is_set(nullwords, np.arange(n))
    if not live.any():
        return I64_MAX, I64_MIN
    return int(keys[live].min()), int(keys[live].max())


def distinct_scan(keys, nullwords, n, window_lo, window_bits, seen):
    """mdb_dev_distinct_scan over a copy of `seen` (uint32 words) -> (twice 0 / 1, seen).  Every non-NULL key inside the window sets
    bit (key - window_lo); twice = a bit was set before, or a key lies outside the window.  The bitmap afterwards does not depend on
    the order of the rows."""
    seen = np.array(seen, dtype=np.uint32)
    twice = 0
    for i in range(n):
        if nullwords is not None and (int(nullwords[i >> 6]) >> (i & 63)) & 1:
            continue
        b = (int(keys[i]) - int(window_lo)) & M64
        if b >= window_bits:
            twice = 1
            continue
        m = 1 << (b & 31)
        if int(seen[b >> 5]) & m:
            twice = 1
        seen[b >> 5] = np.uint32(int(seen[b >> 5]) | m)
    return twice, seen


def widen32to64(src, n):
    return np.asarray(src, dtype=np.int32)[:n].astype(np.int64)


def cross_pairs(n_l, n_r):
    """mdb_dev_cross_pairs: all pairs, row-major ((0, 0), (0, 1) ...) -> (left uint32, right uint32)"""
    if n_l and n_r and n_l * n_r >= 1 << 32:
        raise ValueError("cross join is too large")
    k = np.arange(n_l * n_r, dtype=np.int64)
    if not len(k):
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    return (k // n_r).astype(np.uint32), (k % n_r).astype(np.uint32)


def double_join_keys(src, src_null, idx, n):
    """mdb_dev_double_join_keys -> (dst uint64[n], NULL words): the key words with -0.0 rewritten to +0.0; a NaN row, a source NULL and a
    MDB_NO_ROW row (word 0) have their NULL bit set"""
    src = np.asarray(src, dtype=np.uint64)
    rows, absent = _rows(idx, n)
    v = np.where(absent, np.uint64(0), src[rows]).astype(np.uint64) if n else np.zeros(0, dtype=np.uint64)
    drop = absent.copy()
    if src_null is not None and n:
        drop |= ~absent & bit_is_set(src_null, rows)
    mag = v & np.uint64(0x7FFFFFFFFFFFFFFF)             # the word without its sign
    v = np.where(mag == 0, np.uint64(0), v)
    drop |= mag > np.uint64(0x7FF0000000000000)         # exponent all ones, mantissa non-zero
    return v.astype(np.uint64), pack_bits(drop)


# ---- inputs shared by the CPU and the GPU tests -------------------------------------------------------------------------------

def double_specials():
    """the words of the special DOUBLE values: +-0, +-min subnormal, +-max subnormal, +-min normal, +-1, +-max finite, +-inf, quiet and
    signalling NaNs of both signs with the lowest and the highest mantissa bits"""
    pos = [0x0000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x3FF0000000000000, 0x7FEFFFFFFFFFFFFF,
           0x7FF0000000000000,
           0x7FF0000000000001,      # signalling NaN, lowest mantissa bit
           0x7FF4000000000000,      # signalling NaN, highest payload bit below the quiet bit
           0x7FF7FFFFFFFFFFFF,      # signalling NaN, every payload bit
           0x7FF8000000000000,      # quiet NaN
           0x7FF8000000000001, 0x7FFFFFFFFFFFFFFF]
    return np.array(pos + [w | (1 << 63) for w in pos], dtype=np.uint64)


def norow_positions(n):
    """where the index vectors of the tests hold MDB_NO_ROW: the first and the last output, the first and the last lane of a wave, whole
    64-row waves (one inside the first block, one inside the second, the last whole one), clipped to n"""
    pos = {0, n - 1, 63, 64, 127, 2047, 2048}
    pos.update(range(128, 192))
    pos.update(range(BLOCK + 256, BLOCK + 320))
    last = ((n - 1) // 64) * 64 - 64
    if last >= 0:
        pos.update(range(last, last + 64))
    return np.array(sorted(p for p in pos if 0 <= p < n), dtype=np.int64)


def make_idx(rng, shape, n, src_n):
    """an index vector of n entries over src_n source rows.  shape: "identity" (0 .. n-1), "repeats" (random, both ends of the source
    named), "perm" (distinct rows, both ends named), "norow" ("repeats" with MDB_NO_ROW at norow_positions())"""
    if shape == "identity":
        assert n <= src_n
        return np.arange(n, dtype=np.uint32)
    if shape == "perm":
        assert n <= src_n
        idx = rng.permutation(src_n)[:n].astype(np.uint32)
        for want in (0, src_n - 1):
            if n >= 2 and want not in idx:
                idx[int(rng.integers(0, n))] = want
                if len(np.unique(idx)) != n:      # (the swap hit the other end: redo deterministically)
                    idx = np.arange(n, dtype=np.uint32)
                    idx[-1] = src_n - 1
                    idx = idx[rng.permutation(n)]
        return idx
    idx = rng.integers(0, src_n, size=n, dtype=np.int64).astype(np.uint32)
    if n >= 4:
        idx[1], idx[n - 2] = 0, src_n - 1
    if n >= 70:       # rows whose NULL bits are bit 0 and bit 63 of a word
        idx[2], idx[3], idx[66], idx[67] = 63 % src_n, 64 % src_n, ((src_n // 64) * 64 - 1) % src_n, ((src_n // 64 - 1) * 64) % src_n
    if shape == "norow":
        idx[norow_positions(n)] = NO_ROW
    else:
        assert shape == "repeats", shape
    return idx


def make_nulls(rng, rows, frac=0.3):
    """a random NULL bitmap over `rows` rows as (flags, words), bit 0 and bit 63 of the first and of the last whole word set; the bits
    behind `rows` in the last word are random, as a bitmap that was longer once has them"""
    flags = rng.random(rows) < frac
    for r in (0, 63, (rows // 64) * 64 - 1, (rows // 64 - 1) * 64):
        if 0 <= r < rows:
            flags[r] = True
    words = pack_bits(flags)
    if rows & 63:
        words[-1] |= np.uint64((int(rng.integers(0, 1 << 62)) << (rows & 63)) & M64)
    return flags, words
