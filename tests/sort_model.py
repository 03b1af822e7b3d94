"""ORDER BY, ORDER BY ... LIMIT k, SELECT DISTINCT and GROUP BY over several columns (mdb_dev_sort_perm, mdb_dev_topk_perm,
mdb_dev_distinct_sel, mdb_dev_group_count_multi: include/mdb_dev.h, midoridb_amd/csrc/mdb_dev_sort.hip) restated in vectorised numpy:
the reference that tests/test_sort_forms_gpu.py holds every kernel form of the sort family against, and that
tests/test_cpu_sort_model.py checks on the CPU.  Besides the results the module says what the device has to LAUNCH for a given input
(expected_pass_widths, packed_words, topk_form): those three are white-box on purpose - they restate the conditions written in
mdb_dev_sort.hip and mdb_dev_partition.hip, so that a shape can state its own premise ("the fullest bucket holds exactly 1024 words")
and have it asserted before the device is called.  The module also builds what both test files share: the case lists.

A key is (values, nulls, rid, is_double, desc): values an int64 or float64 array read by its bits, nulls a bool array over the BASE
rows or None, rid a row-id vector over the stream or None (identity).

Semantics (the header of mdb_dev_sort.hip):
    cell        NULL when its row id is MDB_NO_ROW (the base column is then not indexed at all) or its NULL bit is set
    image       INT64: the sign bit flipped; DOUBLE: the IEEE total-order trick (negative: all bits complemented, otherwise the sign
                bit set), so -0.0 sorts before +0.0, NaNs with the sign bit before -inf and the others after +inf, each by its bits;
                DESC: the image complemented
    NULL        before every value under ASC, after every value under DESC; NULL rows tie with each other whatever bytes lie under
                the NULL bit
    ties        of all keys keep the stream order (the permutation is the stable one)
    equality    (DISTINCT, GROUP BY) NULL equals NULL, values are compared by their 64 bits: -0.0 and +0.0 differ, so do two NaN payloads
"""
import collections

import numpy as np

NO_ROW = 0xFFFFFFFF
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SIGN = np.uint64(1 << 63)

# constants of the device code the white-box functions restate
TILE = 4096                     # MDB_TILE: rows per tile of a radix pass / of the packed path's first level
SCAN_SMALL = 16384              # MDB_SCAN_SMALL: a histogram up to here is scanned by one workgroup
SORT_TINY_ROWS = 2048           # SORT_TINY_ROWS
SORT_PACK_MIN_ROWS = 1 << 18    # SORT_PACK_MIN_ROWS
SORT_PACK_MAX_KEYS = 4          # SORT_PACK_MAX_KEYS
SORT_MAX_KEYS = 8               # MDB_SORT_MAX_KEYS
SORT_LEAF_CAP = 4096            # SORT_LEAF_CAP
SORT_BUCKET_MAX = 1024          # SORT_BUCKET_MAX
PART_NSUB = 8                   # PART_NSUB: sub-regions per first-level digit
MAX_RADIX_BITS = 9              # MDB_MAX_RADIX_BITS
TOPK_SAMPLE = 2048              # TOPK_SAMPLE


# ------------------------------------------------------------------------------------------------ cells and images

def _bits(values):
    a = np.ascontiguousarray(values)
    assert a.dtype.itemsize == 8, a.dtype
    return a.view(np.uint64)


def has_no_row(key, n):
    return key[2] is not None and bool(((np.asarray(key[2])[:n].astype(np.int64) & NO_ROW) == NO_ROW).any())


def load(key, n, raw=False):
    """-> (bits uint64[n], isnull bool[n]) of the first n stream positions; a NULL cell's bits are 0 (raw: the bytes under a NULL bit are
    kept - what k_topk_sample reads; a cell without a row is 0 either way)"""
    values, nulls, rid = key[0], key[1], key[2]
    bits = _bits(values)
    if rid is None:
        v = bits[:n]
        isnull = np.zeros(n, dtype=bool) if nulls is None else np.asarray(nulls, dtype=bool)[:n].copy()
    else:
        r = np.asarray(rid)[:n].astype(np.int64) & NO_ROW
        present = r != NO_ROW
        row = np.where(present, r, 0)          # MDB_NO_ROW never indexes the base column
        v = bits[row] if n else bits[:0]
        isnull = ~present
        if nulls is not None:
            isnull = isnull | (present & np.asarray(nulls, dtype=bool)[row])
    if raw:
        return (v if rid is None else np.where(present, v, np.uint64(0))), isnull
    return np.where(isnull, np.uint64(0), v), isnull


def image(bits, is_double, desc):
    bits = np.asarray(bits, dtype=np.uint64)
    if is_double:
        u = np.where((bits >> np.uint64(63)).astype(bool), ~bits, bits ^ SIGN)
    else:
        u = bits ^ SIGN
    return ~u if desc else u


def flags_images(keys, n):
    """per key (flag uint8[n], image uint64[n]): rows order by (flag, image); flag 0 = NULL under ASC, 1 = NULL under DESC; a NULL
    cell's image is 0"""
    out = []
    for key in keys:
        bits, isnull = load(key, n)
        img = np.where(isnull, np.uint64(0), image(bits, key[3], key[4]))
        out.append(((isnull == bool(key[4])).astype(np.uint8), img))
    return out


def can_hold_nulls(key, n):
    """what the device decides by `nullbits != NULL` once resolve_absent_keys has run: a bitmap is bound, or the row-id vector holds
    MDB_NO_ROW (the column is then gathered WITH NULL bits)"""
    return key[1] is not None or has_no_row(key, n)


# ------------------------------------------------------------------------------------------------ the four operators

def _lexsort(fi):
    """stable order by (flag_0, image_0, flag_1, image_1, ...): np.lexsort sorts by its LAST key first and is stable"""
    cols = []
    for flag, img in fi:
        cols += [flag, img]
    return np.lexsort(tuple(reversed(cols)))


def sort_perm(keys, n):
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    return _lexsort(flags_images(keys, n)).astype(np.uint32)


def topk(keys, n, k):
    """sort_perm(keys, n)[:k] without the full sort: the rows at or before the k-th smallest (flag, image) of the FIRST key (np.partition),
    then the stable sort of those"""
    k = min(k, n)
    if k == 0:
        return np.zeros(0, dtype=np.uint32)
    fi = flags_images(keys, n)
    flag, img = fi[0]
    zero = flag == 0
    n0 = int(zero.sum())
    if k <= n0:
        thr = np.partition(img[zero], k - 1)[k - 1]
        cand = zero & (img <= thr)
    else:
        thr = np.partition(img[~zero], k - n0 - 1)[k - n0 - 1]
        cand = zero | (img <= thr)
    pos = np.flatnonzero(cand)                      # ascending stream positions: the stable order among them is the stream's
    order = _lexsort([(f[pos], i[pos]) for f, i in fi])
    return pos[order][:k].astype(np.uint32)


def _groups(keys, n):
    """-> (first positions ascending int64, counts int64) of the groups of rows equal in every key (NULL = NULL, values by their bits)"""
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    cols = []
    for key in keys:
        bits, isnull = load(key, n)
        cols += [isnull.astype(np.uint8), bits]        # (a NULL cell's bits are 0 already)
    order = np.lexsort(tuple(reversed(cols)))          # stable: a group's first sorted row is its first stream row
    head = np.zeros(n, dtype=bool)
    head[0] = True
    for c in cols:
        s = c[order]
        head[1:] |= s[1:] != s[:-1]
    at = np.flatnonzero(head)
    first = order[at].astype(np.int64)
    count = np.diff(np.append(at, n)).astype(np.int64)
    by_first = np.argsort(first, kind="stable")
    return first[by_first], count[by_first]


def distinct_sel(keys, n):
    return _groups(keys, n)[0].astype(np.uint32)


def group_count_multi(keys, n):
    return _groups(keys, n)


# ------------------------------------------------------------------------------------------------ the general path's launches

def differing_bits(key, n):
    """position of the highest bit in which the smallest and the largest non-NULL image differ (0: equal, or no non-NULL row)"""
    bits, isnull = load(key, n)
    img = image(bits, key[3], key[4])[~isnull]
    if img.size == 0:
        return 0
    return (int(img.min()) ^ int(img.max())).bit_length()


def expected_pass_widths(keys, n):
    """the digit widths of the mdb_sort_pass calls of sort_perm_impl's general path, in launch order: last key first, per key 8-bit
    digits from bit 0 up (the last one narrower), then the 1-bit NULL pass when the key's stream holds a NULL.  A later key's passes
    do not depend on the earlier ones: every pass is a permutation of the same cells."""
    out = []
    for key in reversed(keys):
        b = differing_bits(key, n)
        out += [min(8, b - s) for s in range(0, b, 8)]
        if load(key, n)[1].any():
            out.append(1)
    return out


def expected_passes(keys, n):
    return len(expected_pass_widths(keys, n))


def null_passes(keys, n):
    return sum(1 for key in keys if load(key, n)[1].any())


def expected_scans(keys, n):
    """(one-workgroup scans, reduce / spine / apply scans) of those passes: a pass's histogram has ceil(n / 4096) * 2^w words"""
    tiles = (n + TILE - 1) // TILE
    small = sum(1 for w in expected_pass_widths(keys, n) if tiles << w <= SCAN_SMALL)
    return small, expected_passes(keys, n) - small


# ------------------------------------------------------------------------------------------------ the packed path's word

def packed_bits(n):
    """sort_packed_bits: (b1, b2), the widths of the two partition levels"""
    b = 2
    while b < 2 * MAX_RADIX_BITS and (2048 << b) < n:
        b += 1
    b1 = (b + 1) // 2
    return b1, b - b1


Packed = collections.namedtuple("Packed", "total rb up b1 b2 kb words leaf_rows bucket_rows region_rows region_cap")


def packed_words(keys, n):
    """The word sort_perm_packed builds from MEASURED ranges (k_sort_pack, sort_pack_ranges): per column an optional NULL flag bit (spent
    whenever the column can hold NULLs) above kb = bits(largest image - smallest) value bits, then rb position bits, the whole left-aligned
    in 64 bits.  -> Packed:
        total, rb, up   the word's width (rb + the columns' widths), the position bits, the left shift; words is None when total > 64
        leaf_rows       words per leaf (the word's top b1 + b2 bits), 2^(b1 + b2) entries
        bucket_rows     words per (leaf, bucket): the next 10 bits, 2^(b1 + b2) * 1024 entries
        region_rows     words per first-level sub-region [digit * 8 + sub]: a tile of 4096 consecutive rows goes to sub-region
                        tile // (grid / 8) of each digit (part_tile_of_block, `blockIdx.x % a.nsub`), grid = the tile count rounded up to 8
        region_cap      part_layout.cap0 (mdb_dev_partition.hip) for the digits that can occur"""
    assert n >= 1 and len(keys) <= SORT_PACK_MAX_KEYS
    rb = 1
    while rb < 32 and (1 << rb) < n:
        rb += 1
    b1, b2 = packed_bits(n)
    total, kbs, fields, vmax = rb, [], [], 0
    for key in keys:
        bits, isnull = load(key, n)
        img = image(bits, key[3], key[4])
        lo, hi = (int(img[~isnull].min()), int(img[~isnull].max())) if (~isnull).any() else (0, 0)
        kb = (hi - lo).bit_length()
        flagged = can_hold_nulls(key, n)
        width = kb + (1 if flagged else 0)
        total += width
        kbs.append(kb)
        fields.append((img, isnull, lo, kb, flagged, bool(key[4]), width))
        vmax = (vmax << width) | ((1 << kb) if flagged else 0) | (hi - lo)
    if total > 64:
        return Packed(total, rb, None, b1, b2, kbs, None, None, None, None, None)
    up = 64 - total
    v = np.zeros(n, dtype=np.uint64)
    for img, isnull, lo, kb, flagged, desc, width in fields:
        d = np.where(isnull, np.uint64(0), img - np.uint64(lo))
        if flagged:
            d = d | ((isnull == desc).astype(np.uint64) << np.uint64(kb))
        v = (v << np.uint64(width)) | d              # (width <= 64 - rb < 64)
    w = ((v << np.uint64(rb)) | np.arange(n, dtype=np.uint64)) << np.uint64(up)
    lb = b1 + b2
    leaf = (w >> np.uint64(64 - lb)).astype(np.int64)
    bucket = ((w >> np.uint64(64 - lb - 10)) & np.uint64(1023)).astype(np.int64)
    digit = (w >> np.uint64(64 - b1)).astype(np.int64)
    tiles = (n + TILE - 1) // TILE
    per = ((tiles + 7) // 8 * 8) // 8
    sub = (np.arange(n, dtype=np.int64) // TILE) // per
    wmax = ((((vmax << rb) | (n - 1)) << up) & ((1 << 64) - 1))
    digits0 = min((wmax >> (64 - b1)) + 1, 1 << b1)
    avg0 = (n + digits0 * PART_NSUB - 1) // (digits0 * PART_NSUB)
    cap0 = (avg0 * 5 // 4 + 1024 + 63) & ~63
    return Packed(total, rb, up, b1, b2, kbs, w, np.bincount(leaf, minlength=1 << lb), np.bincount(leaf * 1024 + bucket, minlength=1024 << lb),
                  np.bincount(digit * PART_NSUB + sub, minlength=(1 << b1) * PART_NSUB), cap0)


def sort_form(keys, n):
    """the form mdb_dev_sort_perm takes by the conditions written in sort_perm_impl / sort_perm_packed: "tiny", "packed", "redo" (the
    packed path ran and a region, a leaf or a bucket overflowed: the fixed-capacity scatter flags a reservation with
    `fast_base + total_d <= a.cap` false, k_sort_leaf a bucket with `m > SORT_BUCKET_MAX`) or "general" """
    if n <= SORT_TINY_ROWS and len(keys) <= SORT_PACK_MAX_KEYS:
        return "tiny"
    if n < SORT_PACK_MIN_ROWS or len(keys) > SORT_PACK_MAX_KEYS:
        return "general"
    p = packed_words(keys, n)
    if p.total > 64:
        return "general"
    over = p.region_rows.max() > p.region_cap or p.leaf_rows.max() > SORT_LEAF_CAP or p.bucket_rows.max() > SORT_BUCKET_MAX
    return "redo" if over else "packed"


# ------------------------------------------------------------------------------------------------ top-k: the gates of topk_rec

def _ieee_at_or_before(bits, thr_bits, desc):
    """the filter's comparison: column <= threshold (ASC) / >= threshold (DESC) as IEEE 754 doubles; false for NaN"""
    with np.errstate(invalid="ignore"):
        v, t = bits.view(np.float64), np.array([thr_bits], dtype=np.uint64).view(np.float64)[0]
        return v >= t if desc else v <= t


def topk_form(keys, n, k):
    """-> (topk_sample launches, *out_candidates) of mdb_dev_topk_perm by the gates of topk_rec: at least 8 * 2048 rows; the threshold's
    rank 2 * ceil(k / stride) + 3 below 2048 / 4; the threshold is the sample's (positions i * stride) element of that rank in the first
    key's order; no NULL threshold under DESC, no NaN threshold; the rows at or before the threshold on the first key - NULL rows under
    ASC where the column can hold NULLs, NaN rows of a DOUBLE key always - number m with k <= m <= n / 2; then the same again over them"""
    k = min(k, n)
    if n == 0 or k == 0:
        return 0, n
    cols = [load(key, n) + (key[3], key[4], can_hold_nulls(key, n)) for key in keys]
    raw0 = load(keys[0], n, raw=True)[0]            # (the NaN gate looks at the threshold's bytes, also under a NULL bit)
    launches = 0
    while True:
        stride = n // TOPK_SAMPLE
        rank = 2 * ((k + stride - 1) // stride) + 3 if stride else TOPK_SAMPLE
        if not (n >= 8 * TOPK_SAMPLE and rank < TOPK_SAMPLE // 4):
            return launches, n
        launches += 1
        bits, isnull, is_double, desc, nullable = cols[0]
        at = np.arange(TOPK_SAMPLE, dtype=np.int64) * stride
        sb, sn = bits[at], isnull[at]
        sperm = _lexsort([((sn == bool(desc)).astype(np.uint8), np.where(sn, np.uint64(0), image(sb, is_double, desc)))])
        thr_bits, thr_null = sb[sperm[rank]], bool(sn[sperm[rank]])
        if is_double and np.isnan(raw0[at][sperm[rank]:sperm[rank] + 1].view(np.float64)[0]):
            return launches, n
        if desc and thr_null:
            return launches, n
        keep = np.zeros(n, dtype=bool)
        if not thr_null:
            if is_double:
                keep = _ieee_at_or_before(bits, thr_bits, desc) & ~isnull
            else:
                sv, st = bits.view(np.int64), np.array([thr_bits], dtype=np.uint64).view(np.int64)[0]
                keep = (sv >= st if desc else sv <= st) & ~isnull
        if not desc and nullable:
            keep = keep | isnull
        if is_double:
            with np.errstate(invalid="ignore"):
                keep = keep | (np.isnan(bits.view(np.float64)) & ~isnull)
        m = int(keep.sum())
        if not (k <= m <= n // 2):
            return launches, n
        cols = [(b[keep], z[keep], d, ds, nl) for b, z, d, ds, nl in cols]
        raw0, n = raw0[keep], m


def range_sampled_rows(n):
    """the rows k_sort_ranges looks at when the ranges come from a sample of 2^17 rows (one row inside every stretch of n // 2^17 rows)"""
    step = n // (1 << 17)
    k = np.arange(1 << 17, dtype=np.uint64)
    jitter = ((k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)) % np.uint64(step) if step > 1 else np.zeros(1 << 17, dtype=np.uint64)
    return (k * np.uint64(step) + jitter).astype(np.int64)


# ================================================================================================ the shapes both test files share
#
# A Case names an operator call and the form the device has to take for it (the tables in tests/test_sort_forms_gpu.py):
#   op      "sort" | "topk" | "distinct" | "group"
#   make    () -> the keys on the host; arrays shared between keys (a row-id vector above all) are the SAME object in each
#   form    sort: tiny | packed | resampled | redo | general, "+norow" appended when a row-id vector holds MDB_NO_ROW
#           topk: no_sample | sampled_fell_back | one_level | two_levels
#           distinct / group: vkey (heads over the packed sort's composite values) | tiny_cells | general_cells | redo_cells
#   opts    k; env (knobs); premise(keys, n) (asserts what the shape claims about itself); cand ((lo, hi) bounds of *out_candidates)

Case = collections.namedtuple("Case", "op name n make form opts")

SORT_FORMS = {"tiny", "packed", "resampled", "redo", "general", "packed+norow", "general+norow", "tiny+norow"}
TOPK_FORMS = {"no_sample", "sampled_fell_back", "one_level", "two_levels"}
HEADS_FORMS = {"vkey", "tiny_cells", "general_cells", "redo_cells"}
FORM_TABLE = ({("sort", f) for f in SORT_FORMS} | {("topk", f) for f in TOPK_FORMS} | {(op, f) for op in ("distinct", "group") for f in HEADS_FORMS})

NEG_NAN = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
POS_NAN_PAYLOAD = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]
DOUBLE_SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1.1e-308, -1.1e-308, np.nan, NEG_NAN, POS_NAN_PAYLOAD, 1.0, -1.0,
                            1.7976931348623157e308, -1.7976931348623157e308])


def _rng(*seed):
    return np.random.default_rng([int(s) & 0xFFFFFFFF for s in seed])


def int_range_column(n, b, lo_kind, rng):
    """INT64 values whose images differ in exactly b bits: lo (a multiple of 2^b) and lo + 2^b - 1 both present (rows 0 and 1)"""
    if b == 64:
        v = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        lo, hi = I64_MIN, I64_MAX
    else:
        lo = {"zero": 0, "negative": -(5 << b), "min": I64_MIN}[lo_kind]
        hi = lo + (1 << b) - 1
        v = lo + rng.integers(0, 1 << b, n, dtype=np.int64)
    v[0] = lo
    if n > 1:
        v[1] = hi
    return v


def double_specials_column(n, rng):
    """both signs, both zeros, both infinities, denormals, NaNs of both signs and two payloads among ordinary values (the specials lead
    the column, so a prefix of 15 rows has them all, and recur at random)"""
    v = np.round(rng.normal(0, 1e3, n), 1)
    pick = rng.random(n) < 0.2
    v[pick] = DOUBLE_SPECIALS[rng.integers(0, len(DOUBLE_SPECIALS), int(pick.sum()))]
    m = min(n, len(DOUBLE_SPECIALS))
    v[:m] = DOUBLE_SPECIALS[:m]
    return v


def nulls_column(n, kind, rng):
    """None | "bitmap" (bound, no NULL) | "few" (rows 0 and 1 never: a range column keeps its extremes) | "all" """
    if kind is None:
        return None
    if kind == "bitmap":
        return np.zeros(n, dtype=bool)
    if kind == "all":
        return np.ones(n, dtype=bool)
    z = rng.random(n) < 0.02
    z[:2] = False
    if n > 2:
        z[2] = True
    return z


def const_keys(n):
    """four leading keys of one value each: with a fifth key they send any row count to the general path and decide nothing"""
    return [(np.full(n, 42 + i, dtype=np.int64), None, None, False, bool(i & 1)) for i in range(4)]


# ---- the general path

GENERAL_ROWS = [2049, 4095, 4096, 4097, 8193, 262_143, 262_145]
GENERAL_BITS = [0, 1, 7, 8, 9, 16, 17, 64]
FIVE_KEYS_FROM = 1 << 18        # from here on only five keys keep a call on the general path


def general_cases(n):
    """per differing-bit count and position of the range one INT64 key (behind four constant keys from 2^18 rows on); direction and
    NULLs rotate with the case and the row count so that over GENERAL_ROWS every bit count meets ASC and DESC and none / few / all NULL;
    a DOUBLE key of every special value in both directions; two- and three-key cases whose first key has long runs"""
    out, ni = [], GENERAL_ROWS.index(n)
    lead = (lambda: const_keys(n)) if n >= FIVE_KEYS_FROM else (lambda: [])

    def one(b, lo_kind, desc, nk, seed):
        def make():
            rng = _rng(n, b, seed)
            return lead() + [(int_range_column(n, b, lo_kind, rng), nulls_column(n, nk, rng), None, False, desc)]

        def premise(keys, n_):
            assert differing_bits(keys[-1], n_) == (0 if nk == "all" else b)
            assert null_passes(keys, n_) == (0 if nk in (None, "bitmap") else 1)
        return Case("sort", f"bits{b}_{lo_kind}_{'desc' if desc else 'asc'}_{nk}", n, make, "general", {"premise": premise, "bits": b, "nulls": nk, "desc": desc})
    c = 0
    for b in GENERAL_BITS:
        for lo_kind in (("min",) if b == 64 else ("zero", "negative", "min")):
            out.append(one(b, lo_kind, bool((c + ni) & 1), (None, "few", "all")[(c + ni) % 3], c))
            c += 1
    for desc in (False, True):
        def make_d(desc=desc):
            rng = _rng(n, 77, desc)
            return lead() + [(double_specials_column(n, rng), nulls_column(n, "few", rng), None, True, desc)]
        out.append(Case("sort", f"double_specials_{'desc' if desc else 'asc'}", n, make_d, "general", {}))
    if n < FIVE_KEYS_FROM:
        def make_runs(nkeys):
            def make():
                rng = _rng(n, 78, nkeys)
                runs = ((np.arange(n) // 500) % 3).astype(np.int64)                     # long runs of three values
                b = rng.integers(-4, 4, n, dtype=np.int64)
                keys = [(runs, None, None, False, True), (b, nulls_column(n, "few", rng), None, False, False)]
                if nkeys == 3:
                    keys.append((rng.integers(0, 1 << 17, n, dtype=np.int64), None, None, False, True))
                return keys
            return make
        out.append(Case("sort", "two_keys_long_runs", n, make_runs(2), "general", {}))
        out.append(Case("sort", "three_keys_long_runs", n, make_runs(3), "general", {}))
    return out


# ---- the tiny path

TINY_ROWS = [1, 2, 63, 64, 65, 2047, 2048]


def _tiny_keys(n, nkeys, variant, seed):
    """variant: direct | rid (every key through one row-id vector with repeats) | norow (the same vector with MDB_NO_ROW in it)"""
    rng = _rng(n, nkeys, seed)
    m = n if variant == "direct" else 2 * n + 3
    rid = None
    if variant != "direct":
        rid = rng.integers(0, m, n).astype(np.uint32)
        if variant == "norow":
            rid[rng.random(n) < 0.1] = NO_ROW
            rid[n // 2] = NO_ROW
    if nkeys == 1:
        return [(double_specials_column(m, rng), nulls_column(m, "few", rng), rid, True, bool(seed & 1))]
    keys = [(rng.integers(-3, 3, m, dtype=np.int64), nulls_column(m, "few", rng), rid, False, False),
            (double_specials_column(m, rng), None, rid, True, True),
            (np.full(m, 7, dtype=np.int64), nulls_column(m, "bitmap", rng), rid, False, False),
            (rng.integers(I64_MIN, I64_MAX, m, dtype=np.int64, endpoint=True), nulls_column(m, "few", rng), rid, False, True)]
    return keys[:nkeys] if nkeys <= 4 else keys + [(rng.integers(0, 5, m, dtype=np.int64), None, rid, False, False)]


def tiny_cases(n):
    out = []
    for nkeys in (1, 4):
        for variant in ("direct", "rid", "norow"):
            for seed in (0, 1):
                form = "tiny" + ("+norow" if variant == "norow" else "")
                out.append(Case("sort", f"{nkeys}keys_{variant}_{seed}", n, (lambda nk=nkeys, v=variant, s=seed: _tiny_keys(n, nk, v, s)), form, {}))
    if n == SORT_TINY_ROWS:
        out.append(Case("sort", "5keys_direct", n, lambda: _tiny_keys(n, 5, "direct", 0), "general", {}))
    return out


# ---- the packed path

PACKED_ROWS = [1 << 18, (1 << 18) + 1]


def _rb(n):
    return max(1, (n - 1).bit_length())


def _shuffled(v, rng):
    return v[rng.permutation(len(v))]


def _leaf_column(n, extra, rng):
    """values of b1 + b2 bits (a value IS a leaf): the first leaf of every first-level digit holds exactly SORT_LEAF_CAP rows (+ `extra`
    in one of them), the other leaves share the rest evenly; rows in random order, so the first level's sub-regions fill evenly"""
    b1, b2 = packed_bits(n)
    per_digit = 1 << b2
    digits = 1 << b1
    rest = n - digits * SORT_LEAF_CAP - extra
    others = digits * (per_digit - 1)
    counts = np.zeros(digits * per_digit, dtype=np.int64)
    counts[::per_digit] = SORT_LEAF_CAP
    counts[3 * per_digit] += extra
    small = np.flatnonzero(counts == 0)
    counts[small] = rest // others
    counts[small[:rest % others]] += 1
    assert counts.sum() == n
    return _shuffled(np.repeat(np.arange(digits * per_digit, dtype=np.int64), counts), rng)


def _bucket_column(n, hot_rows, rng):
    """a 30-bit key t << 13 whose top 17 bits - leaf and bucket of the packed word - are t: every t twice (one of them once where the row
    count is odd), one hot t with hot_rows rows; t = 0 and t = 2^17 - 1 present, so the key has exactly 30 value bits"""
    pairs = (n - hot_rows) // 2
    t = np.concatenate([[0, (1 << 17) - 1], rng.permutation(np.arange(1, (1 << 17) - 1))[:pairs - 1]]).astype(np.int64)
    hot = t[5]
    col = np.concatenate([np.repeat(np.delete(t, 5), 2), np.full(hot_rows, hot), t[6:6 + (n - hot_rows) % 2]])
    # (the odd row doubles as a third occurrence of one t)
    assert len(col) == n
    return _shuffled(col << 13, rng)


def packed_cases(n):
    rb = _rb(n)
    b1, b2 = packed_bits(n)
    out = []

    def add(name, make, form, premise=None, env=None):
        for desc in (False, True):
            def mk(desc=desc):
                keys = make(_rng(n, len(name), sum(map(ord, name))))
                return [(k[0], k[1], k[2], k[3], (not k[4]) if desc else k[4]) for k in keys]
            out.append(Case("sort", f"{name}_{'desc' if desc else 'asc'}", n, mk, form, {"premise": premise, "env": env or {}}))

    def width(total):
        def premise(keys, n_):
            assert packed_words(keys, n_).total == total
        return premise
    add("width_64", lambda rng: [(int_range_column(n, 64 - rb, "negative", rng), None, None, False, False)], "packed", width(64))
    add("width_65", lambda rng: [(int_range_column(n, 65 - rb, "negative", rng), None, None, False, False)], "general", width(65))
    # (a first key of flag + 1 bit with a third of its rows NULL, then a uniform one: the word's top bits - flag, value, the second key's
    # top bits - spread the rows evenly over three quarters of the first-level digits and of the leaves; a NULL flag that hardly varies
    # would halve the leaves in use)
    add("width_64_with_flag", lambda rng: [(rng.integers(0, 2, n, dtype=np.int64), rng.random(n) < 1 / 3, None, False, False),
                                           (int_range_column(n, 62 - rb, "zero", rng), None, None, False, True)], "packed", width(64))
    add("width_65_with_flag", lambda rng: [(int_range_column(n, 20, "min", rng), nulls_column(n, "bitmap", rng), None, False, False),
                                           (int_range_column(n, 44 - rb, "zero", rng), None, None, False, True)], "general", width(65))

    def leaf_premise(fullest, regions_fit):
        def premise(keys, n_):
            p = packed_words(keys, n_)
            assert p.leaf_rows.max() == fullest and p.bucket_rows.max() <= SORT_BUCKET_MAX
            assert (p.region_rows.max() <= p.region_cap) == regions_fit
            if fullest == SORT_LEAF_CAP:
                assert (p.leaf_rows == SORT_LEAF_CAP).sum() >= 1 << b1
        return premise
    # a leaf of exactly SORT_LEAF_CAP words is taken: the scatter's reservation stays good while `fast_base + total_d <= a.cap`
    # (k_part_scatter, "const bool ok = fast_base + total_d <= a.cap;") - the last one ends AT the capacity
    add("leaf_exactly_full", lambda rng: [(_leaf_column(n, 0, rng), None, None, False, False)], "packed", leaf_premise(SORT_LEAF_CAP, True))
    add("leaf_one_over", lambda rng: [(_leaf_column(n, 1, rng), None, None, False, False)], "redo", leaf_premise(SORT_LEAF_CAP + 1, True))
    if n == 1 << 18:
        # 64 values of 4096 consecutive rows each: every used leaf exactly full again - but a tile's 4096 rows are ONE value, the four tiles
        # of a first-level digit go to the same sub-region (tile // 8), and 16384 words do not fit its cap0 = 3584: the FIRST level reports
        # MDB_ST_REGION_FULL (the same `fast_base + total_d <= a.cap`), whatever the leaves could hold
        def sorted_premise(keys, n_):
            p = packed_words(keys, n_)
            assert set(np.unique(p.leaf_rows)) == {0, SORT_LEAF_CAP} and (p.leaf_rows == SORT_LEAF_CAP).sum() == 64
            assert p.region_cap == 3584 and p.region_rows.max() == 16384 and p.bucket_rows.max() <= SORT_BUCKET_MAX
        add("leaf_exactly_full_consecutive_rows", lambda rng: [((np.arange(n) >> 12).astype(np.int64), None, None, False, False)], "redo", sorted_premise)

        def one_more(rng):
            v = (np.arange(n) >> 12).astype(np.int64)
            v[0] = 5                # a 4097th row of value 5 (in the same half of the stream as the others: the same leaf), one fewer of value 0
            return [(v, None, None, False, False)]

        def one_more_premise(keys, n_):
            assert packed_words(keys, n_).leaf_rows.max() == SORT_LEAF_CAP + 1
        add("leaf_one_over_consecutive_rows", one_more, "redo", one_more_premise)

    def bucket_premise(fullest):
        def premise(keys, n_):
            p = packed_words(keys, n_)
            assert p.kb == [30] and p.bucket_rows.max() == fullest and np.sort(p.bucket_rows)[-2] <= 3
            assert p.leaf_rows.max() < SORT_LEAF_CAP and p.region_rows.max() <= p.region_cap
        return premise
    add("bucket_exactly_full", lambda rng: [(_bucket_column(n, SORT_BUCKET_MAX, rng), None, None, False, False)], "packed", bucket_premise(SORT_BUCKET_MAX))
    add("bucket_one_over", lambda rng: [(_bucket_column(n, SORT_BUCKET_MAX + 1, rng), None, None, False, False)], "redo", bucket_premise(SORT_BUCKET_MAX + 1))

    def nulls_random_bytes(rng):
        v = rng.integers(0, 2, n, dtype=np.int64)
        z = rng.random(n) < 1 / 3
        v[z] = rng.integers(I64_MIN, I64_MAX, int(z.sum()), dtype=np.int64)
        return [(v, z, None, False, False), (rng.integers(0, 16, n, dtype=np.int64), None, None, False, True)]
    add("nulls_over_random_bytes", nulls_random_bytes, "packed")
    # a NULL flag that never varies is a constant top bit of the word: half the first-level digits stay empty, the other half receive twice
    # the average, and a sub-region holds 5/4 of the average + 1024 (part_layout.cap0, mdb_dev_partition.hip): from ~175 000 rows on the first level
    # reports MDB_ST_REGION_FULL (at 2^18 rows a leaf overflows as well: 64 leaves in use for 64 x 4096 rows).  A lost fast path
    wasted_bit = "redo"

    def wasted_premise(keys, n_):
        p = packed_words(keys, n_)
        assert p.region_rows.max() > p.region_cap and (p.region_rows > 0).sum() == 8 * PART_NSUB
        assert (p.leaf_rows.max() > SORT_LEAF_CAP) == (n_ == 1 << 18)
    add("bitmap_without_a_null", lambda rng: [(rng.integers(-512, 512, n, dtype=np.int64), nulls_column(n, "bitmap", rng), None, False, False)],
        wasted_bit, wasted_premise)
    add("all_null_first_key", lambda rng: [(rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64), nulls_column(n, "all", rng), None, False, False),
                                           (rng.integers(0, 1 << 16, n, dtype=np.int64), None, None, False, True)], wasted_bit, wasted_premise)

    def one_binade(sign):
        def make(rng):
            bits = np.array([sign * 1.0]).view(np.uint64)[0] + rng.integers(0, 1 << 40, n, dtype=np.int64).astype(np.uint64)
            return [(bits.view(np.float64), None, None, True, False)]
        return make

    def binade_premise(keys, n_):
        v = keys[0][0]
        assert np.all(np.abs(v) >= 1.0) and np.all(np.abs(v) < 2.0) and packed_words(keys, n_).kb == [40]
    add("double_one_binade", one_binade(1), "packed", binade_premise)
    add("double_one_negative_binade", one_binade(-1), "packed", binade_premise)
    add("double_across_binades", lambda rng: [(double_specials_column(n, rng), None, None, True, False)], "general")

    def outlier(rng):
        v = rng.integers(0, (1 << 20) - (1 << 16), n, dtype=np.int64)
        skipped = np.setdiff1d(np.arange(4000, 4400), range_sampled_rows(n))
        v[skipped[0]] = (1 << 20) - 1           # beyond the sampled range and the 1024th it is widened by; the word keeps its 20 value bits
        return [(v, None, None, False, False)]

    def outlier_premise(keys, n_):
        v = keys[0][0]
        at = np.flatnonzero(v >= (1 << 20) - (1 << 16))
        assert len(at) == 1 and at[0] not in range_sampled_rows(n_) and n_ >= 1 << 18
        seen = v[range_sampled_rows(n_)]
        assert seen.max() + ((seen.max() - seen.min()) >> 10) < v[at[0]]
    add("outlier_on_an_unsampled_row", outlier, "resampled", outlier_premise, {"MDB_SORT_RANGE_SAMPLE": "2"})
    return out


# ---- MDB_NO_ROW at 2^18 rows

def _norow_keys(n, nkeys, rng):
    m = n + 100
    rid1 = rng.integers(0, m, n).astype(np.uint32)
    rid1[rng.random(n) < 0.01] = NO_ROW
    rid1[[0, n - 1]] = NO_ROW
    rid2 = rng.integers(0, m, n).astype(np.uint32)
    za = rng.random(m) < 0.05
    a = rng.integers(-20, 20, m, dtype=np.int64)
    a[za] = rng.integers(I64_MIN, I64_MAX, int(za.sum()), dtype=np.int64)
    # (the key without NULLs leads: 128 evenly filled values are the packed word's 128 leaves)
    keys = [(rng.integers(0, 128, m, dtype=np.int64), None, rid2, False, False), (a, za, rid1, False, False),
            (rng.integers(0, 300, m, dtype=np.int64), None, rid1, False, True)]
    if nkeys == 5:
        keys += [(np.full(n, 1, dtype=np.int64), None, None, False, False), (rng.integers(0, 3, n, dtype=np.int64), None, None, False, True)]
    return keys


def norow_cases():
    n = 1 << 18
    off = {"MDB_GROUP_MULTI_PACKED": "0"}
    return [Case("sort", "norow_three_keys", n, lambda: _norow_keys(n, 3, _rng(n, 3)), "packed+norow", {"lookups": 2, "gathers": 2}),
            Case("sort", "norow_five_keys", n, lambda: _norow_keys(n, 5, _rng(n, 5)), "general+norow", {"lookups": 2, "gathers": 2}),
            Case("distinct", "norow_three_keys", n, lambda: _norow_keys(n, 3, _rng(n, 3)), "vkey", {"lookups": 2, "gathers": 2, "env": off}),
            Case("group", "norow_three_keys", n, lambda: _norow_keys(n, 3, _rng(n, 3)), "vkey", {"lookups": 2, "gathers": 2, "env": off})]


# ---- top-k

TOPK_N = 8 * TOPK_SAMPLE        # 16384: the sample reads positions 8 i


def _through(keys, n, variant, rng):
    """the same stream read through a row-id vector: the base rows in another order (and a few rows nobody reads); norow: stream positions
    3, 8 * 700 + 5, n - 1 and ~1 % more that are no multiple of 8 have no row - the sample does not see them"""
    if variant == "direct":
        return keys
    m = n + 50
    rid = rng.permutation(m)[:n].astype(np.uint32)
    out = []
    for v, z, _none, is_double, desc in keys:
        base = np.zeros(m, dtype=v.dtype)
        base[rid] = v[:n]
        zb = None
        if z is not None:
            zb = np.zeros(m, dtype=bool)
            zb[rid] = z[:n]
        out.append((base, zb, rid, is_double, desc))
    if variant == "norow":
        gone = np.flatnonzero((rng.random(n) < 0.01) & (np.arange(n) % 8 != 0))
        rid[np.concatenate([gone, [3, 8 * 700 + 5, n - 1]])] = NO_ROW
    return out


def topk_built():
    """(name, n, k, make(rng) -> direct keys, form read directly, form through a vector holding MDB_NO_ROW or None where the model says)"""
    n, big = TOPK_N, 10 ** 9
    pos = np.arange(n, dtype=np.int64)
    sampled = pos % 8 == 0
    second = lambda rng: (rng.integers(0, 1000, n, dtype=np.int64), None, None, False, True)
    I = lambda v, z=None, desc=False: (np.asarray(v, dtype=np.int64), z, None, False, desc)
    F = lambda v, z=None, desc=False: (np.asarray(v, dtype=np.float64), z, None, True, desc)
    small_seen = np.where(sampled, pos // 8, big + pos)
    large_seen = np.where(sampled, big + pos // 8, pos)

    def two_values(zeros):
        return (pos >= zeros).astype(np.int64)

    def nan_heavy(rng):
        v = rng.normal(0, 1, n)
        v[rng.random(n) < 0.3] = NEG_NAN
        return [F(v), second(rng)]

    def few_nans(desc):
        def make(rng):
            v = rng.normal(0, 1, n)
            v[[1, 9, 100, 1001]] = NEG_NAN          # (unsampled rows among them: candidates by the filter's "col <> col" alone)
            v[[2, 17, 200, 2001]] = np.nan
            v[[3, 300]] = POS_NAN_PAYLOAD
            return [F(v, None, desc), second(rng)]
        return make

    def zero_threshold(thr, other):
        # the sample's six smallest are -5 ... -1 and `thr`: the threshold is that zero; the other zero sits on two unsampled rows, which the
        # IEEE comparison of the filter keeps whichever zero the threshold is: with k = 8 both zeros are among the first k, in bit order
        def make(rng):
            v = rng.uniform(1, 2, n)
            v[8 * np.arange(6)] = [-5.0, -4.0, -3.0, -2.0, -1.0, thr]
            v[[1, 2]] = other
            return [F(v), second(rng)]
        return make

    def int_extreme(desc):
        def make(rng):
            v = rng.integers(-10 ** 6, 10 ** 6, n, dtype=np.int64)
            v[8 * np.arange(40)] = I64_MAX if desc else I64_MIN
            v[[5, 77]] = I64_MAX if desc else I64_MIN
            return [I(v, None, desc), second(rng)]
        return make

    def null_threshold(desc, rows):
        def make(rng):
            v = rng.integers(0, 10 ** 6, n, dtype=np.int64)
            z = np.zeros(n, dtype=bool)
            z[8 * np.arange(rows)] = True           # sampled NULLs
            z[[1, 2, 3, 4, 5, 6, 7]] = True         # and unsampled ones
            return [I(v, z, desc), second(rng)]
        return make

    def ties(rng):
        return [I(rng.integers(0, 50, n, dtype=np.int64)), second(rng)]
    one, fell, none = "one_level", "sampled_fell_back", "no_sample"
    return [
        ("below_the_row_gate", n - 1, 6, lambda rng: [I(rng.integers(0, 10 ** 6, n - 1, dtype=np.int64))], none, None),
        ("rank_511", n, 2032, lambda rng: [I(rng.integers(0, 10 ** 9, n, dtype=np.int64)), second(rng)], one, None),
        ("rank_513", n, 2033, lambda rng: [I(rng.integers(0, 10 ** 9, n, dtype=np.int64)), second(rng)], none, none),
        ("sample_sees_only_small_m_equals_k", n, 6, lambda rng: [I(small_seen), second(rng)], one, None),
        ("sample_sees_only_small_m_below_k", n, 7, lambda rng: [I(small_seen), second(rng)], fell, None),
        ("sample_sees_only_large", n, 6, lambda rng: [I(large_seen), second(rng)], fell, fell),
        ("half_the_rows_at_the_threshold", n, 6, lambda rng: [I(two_values(n // 2)), second(rng)], one, None),
        ("half_the_rows_and_one", n, 6, lambda rng: [I(two_values(n // 2 + 1)), second(rng)], fell, fell),
        ("ties_decided_by_a_descending_second_key", n, 6, ties, one, None),
        ("descending_null_threshold", n, 6, null_threshold(True, TOPK_SAMPLE - 5), fell, fell),
        ("ascending_null_threshold", n, 6, null_threshold(False, 6), one, None),
        ("nan_threshold", n, 6, nan_heavy, fell, fell),
        ("few_nans_ascending", n, 6, few_nans(False), one, None),
        ("few_nans_descending", n, 6, few_nans(True), one, None),
        ("threshold_minus_zero", n, 8, zero_threshold(-0.0, 0.0), one, None),
        ("threshold_plus_zero", n, 8, zero_threshold(0.0, -0.0), one, None),
        ("threshold_int64_min", n, 6, int_extreme(False), one, None),
        ("threshold_int64_max", n, 6, int_extreme(True), one, None),
    ]


def topk_cases():
    out = []
    for name, n, k, make, form, form_norow in topk_built():
        for variant in ("direct", "rid", "norow"):
            f = form if variant != "norow" else form_norow
            out.append(Case("topk", f"{name}_{variant}", n, (lambda make=make, n=n, v=variant, name=name: _through(make(_rng(len(name), n)), n, v, _rng(7, len(name)))),
                            f, {"k": k, "literal": f is not None}))
    return out


# two threshold levels.  The first level's threshold is the sample's element of rank 5 (k <= stride: 2 * 1 + 3), so it keeps about
# n * 6 / 2049 rows; the second level samples only from 16384 candidates on.  With uniform keys and k in {1, 10} nothing but n moves that
# count: 2^24 is the smallest power of two whose expectation (49 100) leaves the margin of 2 x 16384 asked for - 2^23 expects 24 600.
# The premise asserts the margin for the seed used: the first level keeps at least 2 x 16384 rows.
TWO_LEVEL_N = 1 << 24


def two_level_keys():
    rng = _rng(24, 40)
    return [(rng.integers(0, 1 << 40, TWO_LEVEL_N, dtype=np.int64), None, None, False, False),
            (rng.integers(-1000, 1000, TWO_LEVEL_N, dtype=np.int64), None, None, False, True)]


def first_level_candidates(keys, n, k):
    """rows the first threshold of topk_rec keeps (an INT64 ascending first key without NULLs)"""
    stride = n // TOPK_SAMPLE
    rank = 2 * ((k + stride - 1) // stride) + 3
    v = keys[0][0]
    return int((v <= np.sort(v[::stride][:TOPK_SAMPLE])[rank]).sum())


def two_level_cases():
    def premise(keys, n):
        for k in (1, 10):
            assert 2 * 8 * TOPK_SAMPLE <= first_level_candidates(keys, n, k) <= n // 2
    return [Case("topk", f"two_levels_k{k}", TWO_LEVEL_N, two_level_keys, "two_levels", {"k": k, "premise": premise, "literal": True, "cand": (k, 8 * TOPK_SAMPLE - 1)})
            for k in (1, 10)]


# ---- the sorted fallbacks of DISTINCT / GROUP BY

HEADS_ROWS = [2048, 2049, 1 << 18, (1 << 18) + 1]


def _narrow_pair(n, rng):
    """INT64 columns whose ranges fit the packed word: NULLs over random bytes (one group, however the bytes differ), a NULL over 0
    beside a real 0 (two groups), behind a column of 126 evenly filled values (the packed word's leaves); stream rows 0 and n - 1 are
    groups of one row, the first and the last of the sorted order as well"""
    c = rng.integers(1, 127, n, dtype=np.int64)
    c[[0, n - 1]] = [0, 127]
    a = rng.integers(-3, 4, n, dtype=np.int64)
    za = rng.random(n) < 0.2
    a[za] = rng.integers(I64_MIN, I64_MAX, int(za.sum()), dtype=np.int64)
    b = rng.integers(0, 6, n, dtype=np.int64)
    zb = (rng.random(n) < 0.5) & (b == 0)
    return [(c, None, None, False, False), (a, za, None, False, False), (b, zb, None, False, False)]


def _wide_pair(n, rng):
    """a DOUBLE column of both zeros and two NaN payloads (each its own group) with NULLs over random bytes, and an INT64 column: more than
    63 bits together"""
    x = rng.choice(np.array([0.0, -0.0, np.nan, POS_NAN_PAYLOAD, NEG_NAN, 1.5, -np.inf]), n)
    zx = rng.random(n) < 0.2
    x[zx] = rng.normal(0, 1, int(zx.sum()))
    b = rng.integers(0, 3, n, dtype=np.int64)
    x[[0, n - 1]], zx[[0, n - 1]] = [123.25, -123.25], False
    return [(x, zx, None, True, False), (b, None, None, False, False)]


def _heads_premise(groups_of=None):
    def premise(keys, n):
        first, count = group_count_multi(keys, n)
        assert first[0] == 0 and count[0] == 1 and first[-1] == n - 1 and count[-1] == 1       # run boundaries at both ends of the stream
        if groups_of is not None:
            assert len(first) == groups_of(n), len(first)
    return premise


def heads_cases(n):
    off, on = {"MDB_GROUP_MULTI_PACKED": "0"}, {}
    big = n >= SORT_PACK_MIN_ROWS
    sort_general = "tiny_cells" if n <= SORT_TINY_ROWS else "general_cells"
    out = []

    def add(name, make, form, env, premise=None):
        for op in ("distinct", "group"):
            out.append(Case(op, name, n, (lambda make=make, name=name: make(_rng(n, len(name), 5))), form, {"env": env, "premise": premise or _heads_premise()}))
    # 126 x (7 values + NULL) x (5 values + 0 + NULL over 0) and the two rows of their own, where every combination has its ~30 rows
    add("narrow_pair_knob_off", lambda rng: _narrow_pair(n, rng), "vkey" if big else sort_general, off,
        _heads_premise((lambda n_: 126 * 8 * 7 + 2) if big else None))
    # 7 values + NULL, times 3, and the two rows of their own (which bring their own b)
    add("wide_pair", lambda rng: _wide_pair(n, rng), sort_general, on, _heads_premise(lambda n_: 8 * 3 + 2))

    def five(rng):
        keys = _narrow_pair(n, rng)
        return keys + [(rng.integers(0, 2, n, dtype=np.int64), None, None, False, bool(i & 1)) for i in range(2)]
    add("five_keys", five, "general_cells", on)
    if big:
        def skewed(rng):
            keys = _narrow_pair(n, rng)
            keys[0][0][:] = keys[0][0] ** 3    # the leading values bunch at the low end of their range: the word's first leaf overflows
            return keys

        def skewed_premise(keys, n_):
            _heads_premise()(keys, n_)
            assert sort_form(keys, n_) == "redo"
        add("skewed_knob_off", skewed, "redo_cells", off, skewed_premise)
    return out


def all_cases():
    out = []
    for n in GENERAL_ROWS:
        out += general_cases(n)
    for n in TINY_ROWS:
        out += tiny_cases(n)
    for n in PACKED_ROWS:
        out += packed_cases(n)
    out += norow_cases() + topk_cases() + two_level_cases()
    for n in HEADS_ROWS:
        out += heads_cases(n)
    return out


def topk_form_name(launches, candidates, n):
    return "two_levels" if launches >= 2 else "no_sample" if launches == 0 else "sampled_fell_back" if candidates == n else "one_level"


def model_form(case, keys):
    """the form the conditions written in the code give for the case's keys (what the device must be seen doing)"""
    n = case.n
    norow = any(has_no_row(k, n) for k in keys)
    if case.op == "sort":
        f = sort_form(keys, n)
        if f == "packed" and case.opts.get("env", {}).get("MDB_SORT_RANGE_SAMPLE") == "2":
            # (ranges from a sample, widened by a 1024th on either side: a non-NULL image outside them and the word is packed again)
            seen = range_sampled_rows(n)
            for key in keys:
                bits, isnull = load(key, n)
                img = image(bits, key[3], key[4])
                s = img[seen][~isnull[seen]]
                lo, hi = int(s.min()), int(s.max())
                pad = (hi - lo) >> 10
                if int(img[~isnull].min()) < lo - pad or int(img[~isnull].max()) > hi + pad:
                    f = "resampled"
        return f + ("+norow" if norow else "")
    if case.op == "topk":
        return topk_form_name(*topk_form(keys, n, case.opts["k"]), n)
    knob_off = case.opts.get("env", {}).get("MDB_GROUP_MULTI_PACKED") == "0"
    if not knob_off and len(keys) <= SORT_PACK_MAX_KEYS:
        total = 0
        for key in keys:
            bits, isnull = load(key, n)
            img = image(bits, key[3], key[4])[~isnull]
            total += ((int(img.max()) - int(img.min())).bit_length() if img.size else 0) + (1 if can_hold_nulls(key, n) else 0)
        if total <= 63:
            return "composite"      # group_multi_packed serves the call: not a sorted fallback
    return {"tiny": "tiny_cells", "general": "general_cells", "redo": "redo_cells", "packed": "vkey"}[sort_form(keys, n)]
