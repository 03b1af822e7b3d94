"""The contract of mdb_dev_window's navigation functions (include/mdb_dev.h: LAG, LEAD, FIRST_VALUE, LAST_VALUE, NTILE) in plain numpy,
built on tests/window_model.py's sorted positions and heads.  It is what the GPU tests compare every cell with; itself it is checked
against SQLite (tests/test_cpu_window_nav.py) and, for n <= 65, against the contract read sentence by sentence over Python lists.

Columns in STREAM order as in window_model: a key is (cells, nulls or None, desc); a function is (LAG | LEAD, cells, nulls or None,
offset, default or None), (FIRST_VALUE | LAST_VALUE, cells, nulls or None) or (NTILE, buckets).  nav_model() returns one (values, nulls)
pair per function in stream order: values have the cells' dtype (int64 for NTILE), 0 under a NULL."""
import numpy as np

from tests import window_model as M

LAG, LEAD, FIRST_VALUE, LAST_VALUE, NTILE = 16, 17, 18, 19, 20     # enum mdb_win_op: 9 ... 15 are no functions


def structure(part, order, n):
    """perm, and per sorted position: b (partition start), pe (behind the partition), e (behind the peer group)"""
    part = [(k[0], k[1], False) for k in part]
    perm = M.sorted_positions(part, order, n)
    idx = np.arange(n)
    phead = M._heads(part, perm, n)
    phead[0] = True
    ghead = M._heads(order, perm, n) | phead
    b = np.maximum.accumulate(np.where(phead, idx, 0))
    pstart = np.flatnonzero(phead)
    pe = np.append(pstart, n)[np.cumsum(phead)]
    gstart = np.flatnonzero(ghead)
    e = np.append(gstart, n)[np.cumsum(ghead)]
    return perm, b, pe, e


def nav_model(part, order, n, fns):
    if n == 0:
        return [(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)) for _ in fns]
    perm, b, pe, e = structure(part, order, n)
    p = np.arange(n)
    out = []
    for fn in fns:
        op = fn[0]
        if op == NTILE:
            nb = int(fn[1])
            assert nb >= 1
            s, r = pe - b, p - b
            q, m = s // nb, s % nb
            big = m * (q + 1)
            val = np.where(r < big, r // (q + 1) + 1, m + (r - big) // np.maximum(q, 1) + 1).astype(np.int64)
            nulls = np.zeros(n, dtype=bool)
        else:
            cells = np.asarray(fn[1])
            cnull = np.zeros(n, dtype=bool) if len(fn) < 3 or fn[2] is None else np.asarray(fn[2], dtype=bool)
            k = int(fn[3]) if len(fn) > 3 else 1
            dflt = fn[4] if len(fn) > 4 else None
            if op == LAG:
                inside = (p - b) >= k                     # (Python ints and int64: k up to 2^63 - 1)
                q = np.where(inside, p - min(k, n), 0)
            elif op == LEAD:
                inside = (pe - p) > k
                q = np.where(inside, p + min(k, n), 0)
            elif op == FIRST_VALUE:
                inside, q = np.ones(n, dtype=bool), b
            else:
                inside, q = np.ones(n, dtype=bool), e - 1
            q = np.where(inside, q, 0)
            src = perm[q]
            val = np.where(inside, cells[src], cells.dtype.type(0 if dflt is None else dflt))
            nulls = np.where(inside, cnull[src], dflt is None)
            val = np.where(nulls, cells.dtype.type(0), val)
        sv = np.zeros(n, dtype=val.dtype)
        sn = np.zeros(n, dtype=bool)
        sv[perm] = val
        sn[perm] = nulls
        out.append((sv, sn))
    if n <= M.SMALL:
        slow = nav_by_sentences(part, order, n, fns)
        for (v, nl), (sv, snl) in zip(out, slow):
            assert list(nl) == snl
            assert [x.tobytes() for x in v] == [np.asarray(y, dtype=v.dtype).tobytes() for y in sv], (v, sv)
    return out


def nav_by_sentences(part, order, n, fns):
    """the contract, sentence by sentence, over Python lists"""
    part = [(k[0], k[1], False) for k in part]

    def cell(key, i):
        cells, nulls, _ = key
        if nulls is not None and nulls[i]:
            return None
        return int(M.image(np.asarray(cells)[i:i + 1])[0])

    def cmp_key(i):
        k = []
        for key in part:
            c = cell(key, i)
            k.append((0, 0) if c is None else (1, c))
        for key in order:
            c = cell(key, i)
            if key[2]:
                k.append((1, 0) if c is None else (0, -c))
            else:
                k.append((0, 0) if c is None else (1, c))
        return k

    rows = sorted(range(n), key=lambda i: (cmp_key(i), i))
    same_part = lambda i, j: [cell(k, i) for k in part] == [cell(k, j) for k in part]
    same_peer = lambda i, j: same_part(i, j) and [cell(k, i) for k in order] == [cell(k, j) for k in order]
    res = [([0] * n, [False] * n) for _ in fns]
    for p, i in enumerate(rows):
        b = p
        while b > 0 and same_part(rows[b - 1], i):
            b -= 1
        pe = p + 1
        while pe < n and same_part(rows[pe], i):
            pe += 1
        e = p + 1
        while e < n and same_peer(rows[e], i):
            e += 1
        for f, fn in enumerate(fns):
            op = fn[0]
            if op == NTILE:
                nb = int(fn[1])
                s, r = pe - b, p - b
                # the first s % nb buckets hold s // nb + 1 rows, the others s // nb: walk the buckets
                sizes = [s // nb + (1 if t < s % nb else 0) for t in range(min(nb, s))]
                bucket, seen = 0, 0
                while seen + sizes[bucket] <= r:
                    seen += sizes[bucket]
                    bucket += 1
                res[f][0][i] = bucket + 1
                continue
            cells = np.asarray(fn[1])
            cnull = fn[2] if len(fn) > 2 else None
            k = int(fn[3]) if len(fn) > 3 else 1
            dflt = fn[4] if len(fn) > 4 else None
            q = p - k if op == LAG else p + k if op == LEAD else b if op == FIRST_VALUE else e - 1
            if b <= q < pe:
                j = rows[q]
                if cnull is not None and cnull[j]:
                    res[f][1][i] = True
                else:
                    res[f][0][i] = cells[j]
            elif dflt is None:
                res[f][1][i] = True
            else:
                res[f][0][i] = dflt
    return res
