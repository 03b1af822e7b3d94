"""tests/filter_model.py - the reference of the filter kernels' GPU tests - checked without a GPU: against a second evaluator that walks
one row at a time with Python int / float / struct (no numpy comparison anywhere in it), against oracle/np_oracle.filter_positions on
the programs both understand, and on the program list itself: every program separates the test columns, so neither an all-true nor an
all-false kernel passes any case - except the comparisons that nothing can satisfy (filter_model.provably_empty), which are kept for
exactly that answer."""
import struct

import numpy as np
import pytest

from oracle import np_oracle as orc
from tests import filter_model as fm

N_SCALAR = 513
N_LIST = 4097

MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def cols():
    return fm.make_columns(N_LIST + 7)


# ---- the second evaluator: one row, plain Python

def _signed(u):
    return u - (1 << 64) if u >> 63 else u


def _cell(col, k):
    """-> (is NULL, the cell's 64 bits as an unsigned Python int)"""
    values, nulls, rid = col
    row = k
    if rid is not None:
        row = int(rid[k]) & 0xFFFFFFFF
        if row == 0xFFFFFFFF:
            return True, 0
    if nulls is not None and bool(nulls[row]):
        return True, 0
    return False, struct.unpack("<Q", values[row].tobytes())[0]


def _as_float(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def _compare(cmp_, typ, lu, ru):
    if typ == fm.T_DOUBLE:
        l, r = _as_float(lu), _as_float(ru)      # Python floats compare as IEEE doubles: NaN unordered, -0.0 == 0.0
    else:
        l, r = _signed(lu), _signed(ru)
    return {fm.CMP_LT: l < r, fm.CMP_GT: l > r, fm.CMP_NE: l != r, fm.CMP_EQ: l == r, fm.CMP_LE: l <= r, fm.CMP_GE: l >= r}[cmp_]


def _row(prog, cols, k):
    st = []
    for (op, cmp_, typ, a, b, imm) in prog:
        if op in (fm.P_CMP_COL_CONST, fm.P_CMP_CONST_COL):
            null, u = _cell(cols[a], k)
            c = fm.imm_bits(imm, typ) & MASK64
            st.append(not null and (_compare(cmp_, typ, u, c) if op == fm.P_CMP_COL_CONST else _compare(cmp_, typ, c, u)))
        elif op == fm.P_CMP_COL_COL:
            na, ua = _cell(cols[a], k)
            nb, ub = _cell(cols[b], k)
            st.append(not na and not nb and _compare(cmp_, typ, ua, ub))
        elif op == fm.P_ISNULL:
            st.append(_cell(cols[a], k)[0] != bool(cmp_))
        elif op == fm.P_CONST:
            st.append(int(imm) != 0)
        elif op == fm.P_IN_BITS:
            null, u = _cell(cols[a], k)
            hit = (u >> 6) < b and bool((int(imm[u >> 6]) >> (u & 63)) & 1)
            st.append(not null and (hit != bool(cmp_)))
        elif op == fm.P_IN_SET:
            null, u = _cell(cols[a], k)
            if typ == fm.T_DOUBLE:
                v = _as_float(u)
                member = any(v == float(m) for m in imm)      # IEEE ==: -0.0 is 0.0, a NaN equals nothing - as a cell and as a member
            else:
                member = any(_signed(u) == int(m) for m in imm)
            st.append(not null and (member != bool(cmp_)))
        else:
            r, l = st.pop(), st.pop()
            st.append((l and r) if op == fm.P_AND else ((l or r) if op == fm.P_OR else (l != r)))
    assert len(st) == 1
    return bool(st[0])


@pytest.mark.parametrize("rid", [False, True], ids=["direct", "rid"])
def test_model_equals_row_at_a_time_evaluator(cols, rid):
    bound = fm.bind(cols, rid)
    if rid:
        assert (cols["rid"][:N_SCALAR] == fm.NO_ROW).any()
    for name, _kind, prog in fm.all_programs():
        got = fm.evaluate(prog, bound, N_SCALAR)
        assert got.dtype == bool and got.shape == (N_SCALAR,)
        exp = np.array([_row(prog, bound, k) for k in range(N_SCALAR)])
        assert np.array_equal(got, exp), (name, np.flatnonzero(got != exp)[:5])


def test_no_row_never_indexes_the_base_column():
    """a row id of MDB_NO_ROW is a NULL cell even where the base column is shorter than any index it could stand for"""
    vals = np.array([5, 6], dtype=np.int64)
    rid = np.array([1, fm.NO_ROW, 0, -1], dtype=np.int64)      # -1 in an int32 vector is the same row id
    col = [(vals, None, rid)]
    assert fm.evaluate([fm.cc(fm.CMP_GE, fm.T_INT64, 0, 0)], col, 4).tolist() == [True, False, True, False]
    assert fm.evaluate([fm.isnull(0)], col, 4).tolist() == [False, True, False, True]
    assert fm.evaluate([fm.in_set(0, np.array([0, 5]), fm.T_INT64, True)], col, 4).tolist() == [True, False, False, False]
    assert fm.evaluate([fm.in_bits(0, np.array([1 << 5], dtype=np.uint64), True)], col, 4).tolist() == [True, False, False, False]


def test_ieee_and_full_width_corner_cases():
    nan_a, nan_b = np.array([fm.NAN_A, fm.NAN_B], dtype=np.uint64).view(np.float64)
    x = np.array([nan_a, nan_b, -0.0, 0.0, 5e-324, -np.inf])
    col = [(x, None, None), (np.array([nan_a, 1.0, 0.0, -0.0, 0.0, np.inf]), None, None)]
    D = fm.T_DOUBLE
    for cmp_ in fm.CMPS:
        r = fm.evaluate([fm.cc(cmp_, D, 0, float("nan"))], col, 6)
        assert r.tolist() == [cmp_ == fm.CMP_NE] * 6, cmp_
    assert fm.evaluate([fm.colcol(fm.CMP_EQ, D, 0, 1)], col, 6).tolist() == [False, False, True, True, False, False]
    assert fm.evaluate([fm.colcol(fm.CMP_NE, D, 0, 1)], col, 6).tolist() == [True, True, False, False, True, True]
    assert fm.evaluate([fm.cc(fm.CMP_GT, D, 0, 0.0)], col, 6).tolist() == [False, False, False, False, True, False]
    assert fm.evaluate([fm.in_set(0, np.array([0.0, float("nan")]), D)], col, 6).tolist() == [False, False, True, True, False, False]
    assert fm.evaluate([fm.in_set(0, np.array([0.0, float("nan")]), D, True)], col, 6).tolist() == [True, True, False, False, True, True]
    a = np.array([fm.I64_MIN, fm.I64_MAX, -1, 0], dtype=np.int64)
    icol = [(a, None, None)]
    assert fm.evaluate([fm.cc(fm.CMP_LT, fm.T_INT64, 0, 0)], icol, 4).tolist() == [True, False, True, False]
    assert fm.evaluate([fm.kc(fm.CMP_LT, fm.T_INT64, 0, fm.I64_MAX - 1)], icol, 4).tolist() == [False, True, False, False]
    assert fm.evaluate([fm.cc(fm.CMP_GE, fm.T_INT64, 0, fm.I64_MIN)], icol, 4).all()
    # a negative id is beyond every bit table
    assert fm.evaluate([fm.in_bits(0, np.array([~np.uint64(0)] * 2))], icol, 4).tolist() == [False, False, False, True]


def test_model_equals_np_oracle_where_both_apply(cols):
    """np_oracle.filter_positions knows neither MDB_NO_ROW nor the two lookup instructions, and takes a DOUBLE constant as a value"""
    bound = fm.bind(cols)
    rid = np.where(cols["rid"] == fm.NO_ROW, 3, cols["rid"]).astype(np.int64)
    through = [(v, nl, rid) for (v, nl, _r) in bound]
    ran = 0
    for name, _kind, prog in fm.all_programs():
        if any(i[0] in (fm.P_IN_BITS, fm.P_IN_SET) for i in prog):
            continue
        theirs = [(op, c, t, a, b, float(np.array([fm.imm_bits(imm, t)], dtype=np.int64).view(np.float64)[0]) if t == fm.T_DOUBLE and
                   op in (fm.P_CMP_COL_CONST, fm.P_CMP_CONST_COL) else imm) for (op, c, t, a, b, imm) in prog]
        with np.errstate(invalid="ignore"):
            exp = orc.filter_positions(theirs, bound, N_LIST)
            exp_rid = orc.filter_positions(theirs, through, N_LIST)
        assert np.array_equal(np.flatnonzero(fm.evaluate(prog, bound, N_LIST)), exp), name
        assert np.array_equal(np.flatnonzero(fm.evaluate(prog, through, N_LIST)), exp_rid), name
        ran += 1
    assert ran > 150


def test_every_program_separates_the_test_columns(cols):
    progs = fm.all_programs()
    assert len({name for name, _k, _p in progs}) == len(progs)
    empty = 0
    for rid in (False, True):
        bound = fm.bind(cols, rid)
        for name, _kind, prog in progs:
            r = fm.evaluate(prog, bound, N_LIST)
            if all(i[0] == fm.P_CONST for i in prog):
                continue
            if fm.provably_empty(prog):
                assert not r.any(), name
                empty += 1
                continue
            assert r.any() and not r.all(), (name, rid, int(r.sum()))
    # per binding: col-const and const-col of  < INT64_MIN, > INT64_MAX, < -inf, > +inf  (8) and five operators against a NaN (10)
    assert empty == 2 * 18


def test_program_list_is_what_the_forms_need():
    progs = fm.all_programs()
    kinds = {k: [p for _n, kk, p in progs if kk == k] for k in ("cmp1", "terms", "inset", "general")}
    assert len(kinds["cmp1"]) == 6 * len(fm.INT_CONSTS) and len(kinds["inset"]) == 4
    assert all(len(p) <= 64 for _n, _k, p in progs)
    assert len(fm.left_deep()) == 63 and len(fm.right_deep()) == 63
    n_terms = sorted({sum(i[0] in (fm.P_CMP_COL_CONST, fm.P_CMP_CONST_COL) for i in p) for p in kinds["terms"]})
    assert n_terms == [1, 2, 8]
    for cmp_ in fm.CMPS:      # every operator as the only kind of term, ANDed and ORed
        for conn in (fm.P_AND, fm.P_OR):
            assert any({i[1] for i in p if i[0] == fm.P_CMP_COL_CONST} == {cmp_} and all(i[0] in (fm.P_CMP_COL_CONST, conn) for i in p)
                       for p in kinds["terms"]), (cmp_, conn)
    consts = {i[5] for p in kinds["terms"] for i in p if i[0] in (fm.P_CMP_COL_CONST, fm.P_CMP_CONST_COL)}
    assert fm.I64_MIN in consts and fm.I64_MAX in consts
    ops = {i[0] for p in kinds["general"] for i in p}
    assert {fm.P_AND, fm.P_OR, fm.P_XOR, fm.P_IN_BITS, fm.P_IN_SET, fm.P_ISNULL, fm.P_CONST, fm.P_CMP_COL_COL, fm.P_CMP_CONST_COL} <= ops
