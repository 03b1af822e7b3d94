"""A pure-Python / numpy model of the set operations (UNION ALL, UNION, INTERSECT, EXCEPT over rows with NULL = NULL, in the row order
DESIGN.md 2.5 defines) and of the two device operators behind them (mdb_dev_rows_semi, mdb_dev_concat64).

Rows are tuples, None is NULL.  A float cell is compared by its 64 bits (-0.0 is not +0.0, a NaN equals the NaN of the same bits), as
the operators compare DOUBLE cells; every other cell by ==."""
import struct

import numpy as np

UNION, UNIONALL, INTERSECT, EXCEPT = "UNION", "UNION ALL", "INTERSECT", "EXCEPT"


def _cell_key(v):
    if isinstance(v, (float, np.floating)):
        return ("f", struct.unpack("<Q", struct.pack("<d", float(v)))[0])
    if isinstance(v, np.integer):
        return int(v)
    return v


def row_key(row):
    return tuple(_cell_key(v) for v in row)


def distinct(rows):
    """the first occurrences, in order"""
    seen, out = set(), []
    for r in rows:
        k = row_key(r)
        if k not in seen:
            seen.add(k)
            out.append(r)
    return out


def union_all(left, right):
    return list(left) + list(right)


def union(left, right):
    return distinct(union_all(left, right))


def intersect(left, right):
    members = {row_key(r) for r in right}
    return [r for r in distinct(left) if row_key(r) in members]


def except_(left, right):
    members = {row_key(r) for r in right}
    return [r for r in distinct(left) if row_key(r) not in members]


OPS = {UNION: union, UNIONALL: union_all, INTERSECT: intersect, EXCEPT: except_}


def chain(first, steps):
    """first OP1 rows1 OP2 rows2 ..., evaluated left to right; steps = [(op, rows), ...]"""
    cur = list(first)
    for op, rows in steps:
        cur = OPS[op](cur, rows)
    return cur


def order_limit(rows, order=(), limit=None):
    """ORDER BY over result columns - order = [(column index, desc), ...]: NULL before every value (ASC: first, DESC: last), ties keep the
    order of the rows - then LIMIT (off, cnt)"""
    out = list(rows)
    for col, desc in reversed(list(order)):
        out.sort(key=lambda r: (r[col] is not None, r[col] if r[col] is not None else 0), reverse=bool(desc))
    if limit is not None:
        off, cnt = limit
        out = out[off:off + cnt]
    return out


def rows_semi(probe, build, anti=False):
    """-> (ascending probe positions with (anti: without) an equal build row, number of distinct build rows)"""
    members = {row_key(r) for r in build}
    return [i for i, r in enumerate(probe) if (row_key(r) in members) != bool(anti)], len(members)


def concat64(parts):
    """parts = [(values: uint64/int64 array, nulls: bool array or None)] -> (cells, NULL words: every one of the (n + 63) // 64, the
    bits behind the last row zero)"""
    vals = np.concatenate([np.asarray(v).view(np.int64) for v, _ in parts]) if parts else np.zeros(0, dtype=np.int64)
    nulls = np.concatenate([np.zeros(len(v), dtype=bool) if nb is None else np.asarray(nb, dtype=bool) for v, nb in parts]) if parts else np.zeros(0, dtype=bool)
    n = len(vals)
    words = (n + 63) // 64
    padded = np.zeros(words * 64, dtype=np.uint8)
    padded[:n] = nulls
    return vals, np.packbits(padded.reshape(words, 64), axis=1, bitorder="little").view(np.uint64).reshape(words)
