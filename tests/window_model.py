"""The contract of mdb_dev_window (include/mdb_dev.h) in plain numpy - the reference the GPU tests compare every cell with, itself
checked against SQLite (tests/test_cpu_window.py) and, for n <= 65, against the contract read sentence by sentence over Python lists.

Columns are given in STREAM order, row ids resolved by the caller: a key is (cells, nulls or None, desc), a function
(op,) or (op, cells, nulls or None); cells are int64 or float64 arrays, nulls bool arrays (True = NULL: the NULL bit, or "no row").
window_model() returns one (values, nulls) pair per function, in stream order: values int64, or float64 for AVG and MIN / MAX over
float64 cells (0 under a NULL); SUM wraps in int64, AVG is (double)wrapped sum / (double)cells."""
import numpy as np

ROW_NUMBER, RANK, DENSE_RANK, COUNT, SUM, MIN, MAX, AVG = 1, 2, 3, 4, 5, 6, 7, 8
SMALL = 65      # up to here window_model() also evaluates the contract over Python lists and asserts that both agree

_TOP = np.uint64(1) << np.uint64(63)


def image(cells):
    """the order-preserving uint64 image mdb_dev_sort_perm sorts by: int64 with the sign bit flipped, float64 by the IEEE total-order
    trick (-0.0 before +0.0)"""
    cells = np.asarray(cells)
    bits = cells.view(np.uint64)
    if cells.dtype == np.float64:
        return np.where(bits >> np.uint64(63) != 0, ~bits, bits ^ _TOP)
    return bits ^ _TOP


def unimage(u, is_double):
    u = np.asarray(u, dtype=np.uint64)
    if is_double:
        return np.where(u >> np.uint64(63) != 0, u ^ _TOP, ~u).view(np.float64)
    return (u ^ _TOP).view(np.int64)


def _key_columns(key, n):
    cells, nulls, desc = key
    nulls = np.zeros(n, dtype=bool) if nulls is None else np.asarray(nulls, dtype=bool)
    img = np.where(nulls, np.uint64(0), image(cells))       # NULL equals NULL whatever lies under it
    return img, nulls, bool(desc)


def sorted_positions(part, order, n):
    """perm[p] = stream position of the row at sorted position p: partition keys ascending, then the order keys with their desc; NULL
    before every value ascending (after every value descending); ties keep the stream order"""
    lex = [np.arange(n)]                                     # np.lexsort: the LAST key is the primary one
    for key in list(reversed(order)) + [(c, nl, False) for c, nl, _ in reversed(part)]:
        img, nulls, desc = _key_columns(key, n)
        rank = (~nulls).astype(np.uint8)                     # ascending: NULL (0) first
        if desc:
            img, rank = ~img, 1 - rank
        lex += [img, rank]
    return np.lexsort(lex) if n else np.zeros(0, dtype=np.int64)


def _heads(keys, perm, n):
    """head[p] = some key differs between sorted positions p - 1 and p (NULL = NULL, values by their bits)"""
    head = np.zeros(n, dtype=bool)
    for key in keys:
        img, nulls, _ = _key_columns(key, n)
        img, nulls = img[perm], nulls[perm]
        head[1:] |= (img[1:] != img[:-1]) | (nulls[1:] != nulls[:-1])
    return head


def window_model(part, order, n, fns):
    part = [(k[0], k[1], False) for k in part]
    if n == 0:
        return [(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)) for _ in fns]
    perm = sorted_positions(part, order, n)
    idx = np.arange(n)
    phead = _heads(part, perm, n)
    phead[0] = True
    ghead = _heads(order, perm, n) | phead
    b = np.maximum.accumulate(np.where(phead, idx, 0))      # first position of the partition
    g = np.maximum.accumulate(np.where(ghead, idx, 0))      # ... of the peer group
    gstart = np.flatnonzero(ghead)                          # the peer groups, in sorted order
    gid = np.cumsum(ghead) - 1                              # peer group of every position
    e = np.append(gstart, n)[gid + 1]                       # the position behind the peer group
    pgid = gid[b]                                           # first peer group of every position's partition
    out = []
    for fn in fns:
        op = fn[0]
        nulls = np.zeros(n, dtype=bool)
        if op == ROW_NUMBER:
            val = idx - b + 1
        elif op == RANK:
            val = g - b + 1
        elif op == DENSE_RANK:
            val = gid - pgid + 1
        elif op == COUNT:
            val = e - b
        else:
            cells = np.asarray(fn[1])
            is_double = cells.dtype == np.float64
            cnull = np.zeros(n, dtype=bool) if len(fn) < 3 or fn[2] is None else np.asarray(fn[2], dtype=bool)
            valid = ~cnull[perm]
            # per peer group, then running over the peer groups of a partition: the frame is [b, e)
            gcnt = np.add.reduceat(valid.astype(np.int64), gstart)
            ccnt = np.cumsum(gcnt)
            first = pgid[gstart]                             # the partition's first peer group, per peer group
            run_cnt = ccnt - np.where(first > 0, ccnt[first - 1], 0)
            if op in (SUM, AVG):
                assert not is_double, "SUM / AVG over DOUBLE cells are outside the operator's contract"
                gsum = np.add.reduceat(np.where(valid, cells[perm], 0).astype(np.int64), gstart)     # (int64 adds wrap)
                csum = np.cumsum(gsum)
                run = csum - np.where(first > 0, csum[first - 1], 0)
                if op == SUM:
                    gval = run
                else:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        gval = run.astype(np.float64) / run_cnt.astype(np.float64)
            else:
                img = image(cells)[perm]
                if op == MIN:
                    red = np.minimum.reduceat(np.where(valid, img, ~np.uint64(0)), gstart)
                else:
                    red = np.maximum.reduceat(np.where(valid, img, np.uint64(0)), gstart)
                run = red.copy()
                pstart = np.flatnonzero(first == np.arange(len(gstart)))        # peer groups that begin a partition
                pend = np.append(pstart[1:], len(gstart))
                for s, t in zip(pstart[pend - pstart > 1], pend[pend - pstart > 1]):
                    run[s:t] = (np.minimum if op == MIN else np.maximum).accumulate(red[s:t])
                gval = unimage(run, is_double)
            gnull = run_cnt == 0
            gval = np.where(gnull, 0, gval)
            val, nulls = gval[gid], gnull[gid]
        stream_val = np.zeros(n, dtype=val.dtype)
        stream_null = np.zeros(n, dtype=bool)
        stream_val[perm] = val
        stream_null[perm] = nulls
        out.append((stream_val, stream_null))
    if n <= SMALL:
        slow = window_by_sentences(part, order, n, fns)
        for (v, nl), (sv, snl) in zip(out, slow):
            assert list(nl) == snl
            assert [x.tobytes() for x in v] == [np.asarray(y, dtype=v.dtype).tobytes() for y in sv], (v, sv)
    return out


def window_by_sentences(part, order, n, fns):
    """the contract, sentence by sentence, over Python lists; -> [(values, nulls)] with Python numbers"""
    def cell(key, i):
        cells, nulls, _ = key
        if nulls is not None and nulls[i]:
            return None
        x = np.asarray(cells)[i:i + 1]
        return int(image(x)[0])                              # (ordered and compared as the sort does: by the image)

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

    rows = sorted(range(n), key=lambda i: (cmp_key(i), i))  # ties keep the stream order
    same_part = lambda i, j: [cell(k, i) for k in part] == [cell(k, j) for k in part]
    same_peer = lambda i, j: same_part(i, j) and [cell(k, i) for k in order] == [cell(k, j) for k in order]
    res = [([0] * n, [False] * n) for _ in fns]
    for p, i in enumerate(rows):
        b = p
        while b > 0 and same_part(rows[b - 1], i):
            b -= 1
        g = p
        while g > b and same_peer(rows[g - 1], i):
            g -= 1
        e = p + 1
        while e < n and same_peer(rows[e], i):
            e += 1
        for f, fn in enumerate(fns):
            op = fn[0]
            if op == ROW_NUMBER:
                v = p - b + 1
            elif op == RANK:
                v = g - b + 1
            elif op == DENSE_RANK:
                v = 1 + sum(1 for q in range(b + 1, p + 1) if not same_peer(rows[q - 1], rows[q]))
            elif op == COUNT:
                v = e - b
            else:
                cells = np.asarray(fn[1])
                cnull = fn[2] if len(fn) > 2 else None
                frame = [cells[rows[q]] for q in range(b, e) if cnull is None or not cnull[rows[q]]]
                if not frame:
                    res[f][1][i] = True
                    v = 0
                elif op in (SUM, AVG):
                    s = sum(int(x) for x in frame)
                    s = (s + 2 ** 63) % 2 ** 64 - 2 ** 63    # wraps in int64
                    v = s if op == SUM else float(s) / float(len(frame))
                else:
                    pick = min if op == MIN else max
                    v = pick(frame, key=lambda x: int(image(np.asarray([x]))[0]))
            res[f][0][i] = v
    return res
