"""tests/sort_model.py - the reference of the sort family's GPU tests - checked without a GPU: against a row-at-a-time restatement in plain
Python (functools.cmp_to_key over (NULL flag, image) tuples, ties by position; Python ints and struct, no numpy comparison in it), against
oracle/np_oracle's sort_perm / distinct_sel / group_count_multi where those are defined (no MDB_NO_ROW), on hand-computed columns for the
number of radix passes, and on the case list of tests/test_sort_forms_gpu.py itself: every shape's premise (leaf, bucket and region
occupancies, word widths, the rows a threshold keeps) holds, the form each case declares is the one the conditions written in the code
give for its keys, and the declared forms cover every row of the form tables."""
import collections
import functools
import struct

import numpy as np
import pytest

from oracle import np_oracle as orc
from tests import sort_model as sm

MASK64 = (1 << 64) - 1
N = 300


# ---- the second model: one row at a time

def _cell(key, k):
    """-> (is NULL, the cell's 64 bits as an unsigned Python int)"""
    values, nulls, rid = key[0], key[1], key[2]
    row = k
    if rid is not None:
        row = int(rid[k]) & 0xFFFFFFFF
        if row == 0xFFFFFFFF:
            return True, 0
    if nulls is not None and bool(nulls[row]):
        return True, 0
    v = values[row]
    return False, struct.unpack("<Q", struct.pack("<d", float(v)) if values.dtype == np.float64 else struct.pack("<q", int(v)))[0]


def _image(bits, is_double, desc):
    u = ((~bits) & MASK64 if bits >> 63 else bits | (1 << 63)) if is_double else bits ^ (1 << 63)
    return (~u) & MASK64 if desc else u


def _row_tuple(keys, k):
    out = []
    for key in keys:
        isnull, bits = _cell(key, k)
        desc = bool(key[4])
        out.append((int(isnull == desc), 0 if isnull else _image(bits, key[3], desc)))
    return out


def scalar_sort_perm(keys, n):
    rows = [(_row_tuple(keys, k), k) for k in range(n)]

    def cmp(a, b):
        for (fa, ia), (fb, ib) in zip(a[0], b[0]):
            if fa != fb:
                return -1 if fa < fb else 1
            if ia != ib:
                return -1 if ia < ib else 1
        return -1 if a[1] < b[1] else (1 if a[1] > b[1] else 0)
    return np.array([k for _t, k in sorted(rows, key=functools.cmp_to_key(cmp))], dtype=np.uint32)


def scalar_groups(keys, n):
    first, count = collections.OrderedDict(), {}
    for k in range(n):
        t = tuple(_cell(key, k) for key in keys)
        if t not in first:
            first[t], count[t] = k, 0
        count[t] += 1
    return np.array(list(first.values()), dtype=np.int64), np.array([count[t] for t in first], dtype=np.int64)


# ---- columns of every special value

@pytest.fixture(scope="module")
def cols():
    rng = np.random.default_rng(5)
    m = 2 * N
    i = rng.integers(-3, 4, m, dtype=np.int64)
    i[:6] = [sm.I64_MIN, sm.I64_MAX, 0, -1, sm.I64_MIN + 1, sm.I64_MAX - 1]
    i[rng.random(m) < 0.1] = sm.I64_MIN
    i[rng.random(m) < 0.1] = sm.I64_MAX
    d = sm.double_specials_column(m, rng)
    zi, zd = rng.random(m) < 0.2, rng.random(m) < 0.2
    i2 = i.copy()
    i2[zi] = rng.integers(sm.I64_MIN, sm.I64_MAX, int(zi.sum()), dtype=np.int64)      # NULLs over arbitrary bytes
    d2 = d.copy()
    d2[zd] = sm.NEG_NAN
    rid = rng.integers(0, m, N).astype(np.uint32)                                     # with repeats
    rid_gone = rid.copy()
    rid_gone[rng.random(N) < 0.15] = sm.NO_ROW
    rid_gone[[0, N - 1]] = sm.NO_ROW
    assert {0.0, np.inf, -np.inf, 5e-324, -5e-324} <= set(d[:15]) and np.signbit(d[1]) and d[1] == 0 and np.isnan(d[8:11]).all()
    assert len(set(rid.tolist())) < N
    return dict(i=i2, d=d2, zi=zi, zd=zd, rid=rid, rid_gone=rid_gone)


def _key_sets(c, rid):
    return [
        [(c["i"], None, rid, False, False)], [(c["i"], c["zi"], rid, False, True)], [(c["d"], None, rid, True, False)], [(c["d"], c["zd"], rid, True, True)],
        [(c["i"], c["zi"], rid, False, False), (c["d"], c["zd"], rid, True, True)],
        [(c["d"], c["zd"], rid, True, False), (c["i"], None, rid, False, True), (c["i"], c["zi"], rid, False, False)],
        [(c["i"], np.ones(len(c["i"]), dtype=bool), rid, False, False), (c["d"], None, None, True, True)],
    ]


@pytest.mark.parametrize("through", [None, "rid", "rid_gone"])
def test_model_agrees_with_the_row_at_a_time_restatement_and_the_oracle(cols, through):
    rid = cols[through] if through else None
    for keys in _key_sets(cols, rid):
        for n in (0, 1, 2, 65, N):
            want = scalar_sort_perm(keys, n)
            assert np.array_equal(sm.sort_perm(keys, n), want)
            for k in (0, 1, 2, 7, n // 2, n, n + 3):
                assert np.array_equal(sm.topk(keys, n, k), want[:k]), (n, k)
            first, count = scalar_groups(keys, n)
            gf, gc = sm.group_count_multi(keys, n)
            assert np.array_equal(gf, first) and np.array_equal(gc, count)
            assert np.array_equal(sm.distinct_sel(keys, n), first.astype(np.uint32))
            if through != "rid_gone":           # (the oracle indexes the base column with MDB_NO_ROW)
                okeys = [(k[0], k[1], None if k[2] is None else k[2][:n], k[3], k[4]) for k in keys]      # (the oracle reads the whole vector)
                assert np.array_equal(orc.sort_perm(okeys, n), want)
                assert np.array_equal(orc.distinct_sel(okeys, n), first.astype(np.uint32))
                ef, ec = orc.group_count_multi(okeys, n)
                assert np.array_equal(ef, first) and np.array_equal(ec, count)


def test_the_special_values_sort_where_the_header_says():
    v = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, sm.NEG_NAN, 5e-324, -5e-324, 1.0, 7.0], dtype=np.float64)
    z = np.zeros(10, dtype=bool)
    z[9] = True
    asc = sm.sort_perm([(v, z, None, True, False)], 10)
    assert asc.tolist() == [9, 5, 3, 7, 1, 0, 6, 8, 2, 4]          # NULL, -NaN, -inf, -denormal, -0.0, +0.0, denormal, 1.0, +inf, +NaN
    assert sm.sort_perm([(v, z, None, True, True)], 10).tolist() == asc.tolist()[::-1]
    i = np.array([0, sm.I64_MAX, sm.I64_MIN, -1], dtype=np.int64)
    assert sm.sort_perm([(i, None, None, False, False)], 4).tolist() == [2, 3, 0, 1]
    # equality is by bits: two zeros, two NaN payloads, a NULL over 0 beside a real 0 - and NULLs over different bytes are one group
    g = np.array([0.0, -0.0, np.nan, sm.POS_NAN_PAYLOAD, 0.0, 3.0, 4.0, 0.0], dtype=np.float64)
    gz = np.array([0, 0, 0, 0, 1, 1, 1, 0], dtype=bool)
    first, count = sm.group_count_multi([(g, gz, None, True, False)], 8)
    assert first.tolist() == [0, 1, 2, 3, 4] and count.tolist() == [2, 1, 1, 1, 3]


@pytest.mark.parametrize("bits,lo,hi", [(0, 5, 5), (1, 6, 7), (1, -1, -2), (7, 0, 127), (7, 128, 255), (6, 64, 127), (8, 0, 255), (8, 127, 128), (8, 256, 511), (9, 0, 511), (9, 255, 256),
                                        (16, -65536, -1), (17, 0, 65536), (63, 0, sm.I64_MAX), (63, sm.I64_MIN, -1), (64, -1, 0), (64, sm.I64_MIN, sm.I64_MAX)])
def test_expected_passes_on_hand_computed_columns(bits, lo, hi):
    """images are value + 2^63: the differing bits are those of lo XOR hi, written out by hand in the parameters (127 / 128 differ in 8
    bits, 255 / 256 in 9, -1 / 0 in all 64)"""
    v = np.array([lo, hi, lo, hi, lo], dtype=np.int64)
    assert sm.differing_bits((v, None, None, False, False), 5) == bits == sm.differing_bits((v, None, None, False, True), 5)
    passes = (bits + 7) // 8
    assert sm.expected_passes([(v, None, None, False, False)], 5) == passes
    z = np.array([0, 0, 0, 0, 1], dtype=bool)
    assert sm.expected_passes([(v, z, None, False, True)], 5) == passes + 1
    assert sm.expected_passes([(v, np.zeros(5, dtype=bool), None, False, False)], 5) == passes                 # a bitmap without a NULL
    assert sm.expected_passes([(v, np.ones(5, dtype=bool), None, False, False)], 5) == 1                        # no non-NULL row: 0 bits
    assert sm.expected_pass_widths([(v, z, None, False, False)], 5) == [8] * (bits // 8) + ([bits % 8] if bits % 8 else []) + [1]
    # several keys: the sums, last key first, whatever the other keys hold
    w = np.array([3, 3, 3, 3, 3], dtype=np.int64)
    assert sm.expected_passes([(w, z, None, False, False), (v, None, None, False, False), (w, None, None, False, True)], 5) == 1 + passes
    gone = np.array([0, 1, 2, 3, sm.NO_ROW], dtype=np.uint32)
    assert sm.expected_passes([(v, None, gone, False, False)], 5) == passes + 1                                 # "no row" is a NULL cell


def test_scan_forms_on_either_side_of_the_switch():
    v = np.arange(262_145, dtype=np.int64) & 255
    key = [(v, None, None, False, False)]
    assert sm.expected_scans(key, 262_143) == (1, 0)        # 64 tiles x 256 = 16384 words: one workgroup
    assert sm.expected_scans(key, 262_145) == (0, 1)        # 65 tiles x 256 = 16640 words: reduce / spine / apply, a partial last chunk
    assert 65 * 256 % 4096 != 0


def test_packed_word_layout_by_hand():
    """two columns at 2^18 rows: [flag | 3 value bits][2 value bits][18 position bits], left-aligned"""
    n = 1 << 18
    a = np.full(n, 10, dtype=np.int64)
    a[:3] = [15, 12, 10]
    z = np.zeros(n, dtype=bool)
    z[3] = True
    b = np.full(n, -7, dtype=np.int64)
    b[:3] = [-7, -4, -6]
    p = sm.packed_words([(a, z, None, False, False), (b, None, None, False, True)], n)
    assert (p.total, p.rb, p.up, p.b1, p.b2, p.kb) == (1 + 3 + 2 + 18, 18, 40, 4, 3, [3, 2])
    word = lambda flag, da, db, pos: (((flag << 3 | da) << 2 | db) << 18 | pos) << 40
    # DESC images grow downwards: -4 is the smallest image of b (0), -7 the largest (3)
    assert [int(x) for x in p.words[:4]] == [word(1, 5, 3, 0), word(1, 2, 0, 1), word(1, 0, 2, 2), word(0, 0, 3, 3)]
    assert p.leaf_rows.sum() == n and p.bucket_rows.sum() == n and p.region_rows.sum() == n
    assert sm.packed_bits((1 << 18) + 1) == (4, 4) and sm.packed_words([(a, None, None, False, False)], n + 1 - 1).rb == 18
    assert sm.packed_words([(np.arange(n + 1, dtype=np.int64), None, None, False, False)], n + 1).rb == 19


# ---- the case list of the GPU file

CASES = sm.all_cases()


def test_case_names_are_unique():
    ids = [(c.op, c.n, c.name) for c in CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("part", ["general", "tiny", "packed", "norow", "topk", "two_levels", "heads"])
def test_every_gpu_shape_holds_its_premise_and_declares_the_form_the_code_gives(part):
    cases = {"general": lambda: [c for n in sm.GENERAL_ROWS for c in sm.general_cases(n)], "tiny": lambda: [c for n in sm.TINY_ROWS for c in sm.tiny_cases(n)],
             "packed": lambda: [c for n in sm.PACKED_ROWS for c in sm.packed_cases(n)], "norow": sm.norow_cases, "topk": sm.topk_cases,
             "two_levels": sm.two_level_cases, "heads": lambda: [c for n in sm.HEADS_ROWS for c in sm.heads_cases(n)]}[part]()
    assert cases
    made = {}
    for c in cases:
        keys = made[id(c.make)] if id(c.make) in made else c.make()
        if part == "two_levels":
            made[id(c.make)] = keys         # (2^24 rows: built once for both k)
        for key in keys:
            rows = len(key[0]) if key[2] is None else len(key[2])
            assert rows >= c.n and (key[1] is None or len(key[1]) == len(key[0]))
        if c.opts.get("premise"):
            c.opts["premise"](keys, c.n)
        got = sm.model_form(c, keys)
        if c.form is None:                  # (a top-k case read through MDB_NO_ROW whose form the model alone says)
            assert got in sm.TOPK_FORMS
        else:
            assert got == c.form, (c.op, c.name, c.n, got, c.form)
        if "lookups" in c.opts:
            vectors = {id(k[2]) for k in keys if k[2] is not None}
            assert len(vectors) == c.opts["lookups"] and sum(1 for k in keys if sm.has_no_row(k, c.n)) == c.opts["gathers"]
        if "cand" in c.opts:
            launches, cand = sm.topk_form(keys, c.n, c.opts["k"])
            assert launches == 2 and c.opts["cand"][0] <= cand <= c.opts["cand"][1]


def test_topk_shapes_hold_what_their_names_say():
    cases = {c.name: c for c in sm.topk_cases()}
    for name, at in (("threshold_minus_zero_direct", [{40}, {1, 2}]), ("threshold_plus_zero_direct", [{1, 2}, {40}])):
        c = cases[name]
        keys = c.make()
        first = sm.topk(keys, c.n, c.opts["k"]).tolist()
        minus = len(at[0])              # both zeros among the first k, the rows of -0.0 first (among themselves by the second key)
        assert [set(first[5:5 + minus]), set(first[5 + minus:])] == at and sm.topk_form(keys, c.n, c.opts["k"]) == (1, 8)
        assert np.signbit(keys[0][0][first[5]]) and not np.signbit(keys[0][0][first[7]])
    for name, want in (("sample_sees_only_small_m_equals_k_direct", (1, 6)), ("sample_sees_only_small_m_below_k_direct", (1, sm.TOPK_N)),
                       ("half_the_rows_at_the_threshold_direct", (1, sm.TOPK_N // 2)), ("half_the_rows_and_one_direct", (1, sm.TOPK_N)),
                       ("ascending_null_threshold_direct", (1, 13)), ("rank_513_direct", (0, sm.TOPK_N)), ("below_the_row_gate_direct", (0, sm.TOPK_N - 1))):
        c = cases[name]
        assert sm.topk_form(c.make(), c.n, c.opts["k"]) == want, name
    c = cases["few_nans_ascending_direct"]
    keys = c.make()
    lead = keys[0][0][sm.topk(keys, c.n, 6)]
    assert np.isnan(lead[:4]).all() and np.signbit(lead[:4]).all() and not np.isnan(lead[4:]).any()      # the negative NaNs lead ASC
    c = cases["few_nans_descending_direct"]
    keys = c.make()
    lead = keys[0][0][sm.topk(keys, c.n, 6)]
    assert np.isnan(lead).all() and not np.signbit(lead).any()                                          # the positive ones lead DESC
    for name, extreme in (("threshold_int64_min_direct", sm.I64_MIN), ("threshold_int64_max_direct", sm.I64_MAX)):
        c = cases[name]
        keys = c.make()
        assert (keys[0][0][sm.topk(keys, c.n, 6)] == extreme).all() and sm.topk_form(keys, c.n, 6) == (1, 42)


def test_general_cases_meet_every_bit_count_in_both_directions_and_with_every_null_kind():
    seen = collections.defaultdict(set)
    for n in sm.GENERAL_ROWS:
        for c in sm.general_cases(n):
            if "bits" in c.opts:
                seen[c.opts["bits"]].add((c.opts["desc"], c.opts["nulls"]))
    assert sorted(seen) == sm.GENERAL_BITS
    for b, combos in seen.items():
        assert {d for d, _ in combos} == {False, True} and {z for _, z in combos} == {None, "few", "all"}, b


def test_the_declared_forms_cover_every_row_of_the_form_tables():
    have = collections.Counter((c.op, c.form) for c in CASES if c.form is not None)
    assert set(have) >= sm.FORM_TABLE, sm.FORM_TABLE - set(have)
    assert set(have) <= sm.FORM_TABLE
