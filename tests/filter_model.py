"""The predicate programs of mdb_dev_filter / mdb_dev_filter_project (include/mdb_dev.h) restated in vectorised numpy: the reference
that tests/test_filter_forms_gpu.py holds every kernel form of mdb_dev_filter.hip against, and that tests/test_cpu_filter_model.py
checks on the CPU.  Besides evaluate() the module builds what both of those files share: the columns and the program list.

A program is a list of (op, cmp, type, a, b, imm), the fields of struct mdb_pred_insn.  Two instructions carry, in the MODEL's form of
a program, data instead of a device address:

    MDB_P_IN_SET    imm = the member list (a numpy array: int64 for MDB_T_INT64, float64 for MDB_T_DOUBLE), b is ignored
    MDB_P_IN_BITS   imm = the bit table (a numpy uint64 array), b = its length in words

A column is (values, nulls, rid): values an int64 or float64 array (read by its bits, as the device does: the instruction's type says
how they compare), nulls a bool array over the BASE rows or None, rid a row-id vector over the stream or None (identity).

Semantics (mdb_dev.h, mdb_dev_filter.hip's header):
    cell            NULL when its row id is MDB_NO_ROW (the base column is then not indexed at all) or its NULL bit is set
    comparison      false when an operand is NULL; MDB_T_INT64 signed and full-width; MDB_T_DOUBLE as IEEE 754: a NaN on either side
                    makes every operator false except <>, which it makes true; -0.0 equals +0.0
    MDB_P_ISNULL    (the cell is NULL) XOR cmp
    MDB_P_CONST     imm != 0
    AND / OR / XOR  plain booleans over a stack
    MDB_P_IN_BITS   false for a NULL cell; otherwise (word (value >> 6, unsigned) < b and the bit is set) XOR cmp - a negative id is
                    beyond every table
    MDB_P_IN_SET    false for a NULL cell; otherwise (member) XOR (cmp != 0); MDB_T_INT64 compares bit for bit, MDB_T_DOUBLE takes +-0
                    as one member and a NaN cell as a member of nothing (IN false, NOT IN true)
"""
import struct

import numpy as np

P_CMP_COL_CONST, P_CMP_CONST_COL, P_CMP_COL_COL, P_ISNULL, P_CONST, P_AND, P_OR, P_XOR, P_IN_BITS, P_IN_SET = range(1, 11)
CMP_LT, CMP_GT, CMP_NE, CMP_EQ, CMP_LE, CMP_GE = 1, 2, 3, 4, 5, 6
CMPS = (CMP_LT, CMP_GT, CMP_NE, CMP_EQ, CMP_LE, CMP_GE)
CMP_NAME = {CMP_LT: "lt", CMP_GT: "gt", CMP_NE: "ne", CMP_EQ: "eq", CMP_LE: "le", CMP_GE: "ge"}
T_INT64, T_DOUBLE = 0, 1
NO_ROW = 0xFFFFFFFF
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

_CMP = {CMP_LT: np.less, CMP_GT: np.greater, CMP_NE: np.not_equal, CMP_EQ: np.equal, CMP_LE: np.less_equal, CMP_GE: np.greater_equal}


def double_bits(x):
    """the bits of a double as a signed 64-bit integer (what mdb_pred_insn.imm holds)"""
    return struct.unpack("<q", struct.pack("<d", x))[0]


def imm_bits(imm, typ):
    """an instruction's constant as signed 64-bit bits: a Python float of a MDB_T_DOUBLE instruction is converted, an int is the bits"""
    if typ == T_DOUBLE and isinstance(imm, float):
        return double_bits(imm)
    imm = int(imm)
    return imm - (1 << 64) if imm > I64_MAX else imm


def _bits(values):
    a = np.ascontiguousarray(values)
    assert a.dtype.itemsize == 8, a.dtype
    return a.view(np.int64)


def load(col, n):
    """-> (bits int64[n], isnull bool[n]) of the first n stream positions; a NULL cell's bits are 0"""
    values, nulls, rid = col
    bits = _bits(values)
    if rid is None:
        v = bits[:n]
        isnull = np.zeros(n, dtype=bool) if nulls is None else np.asarray(nulls, dtype=bool)[:n].copy()
    else:
        r = np.asarray(rid)[:n].astype(np.int64) & NO_ROW
        present = r != NO_ROW
        row = np.where(present, r, 0)      # MDB_NO_ROW never indexes the base column
        v = bits[row]
        isnull = ~present
        if nulls is not None:
            isnull = isnull | (present & np.asarray(nulls, dtype=bool)[row])
    return np.where(isnull, 0, v), isnull


def _as(typ, bits):
    return bits.view(np.float64) if typ == T_DOUBLE else bits


def _const(typ, imm):
    b = np.array([imm_bits(imm, typ)], dtype=np.int64)
    return _as(typ, b)[0]


def set_members(typ, members):
    """the canonical distinct members as int64 bits: for MDB_T_DOUBLE -0.0 becomes +0.0 and NaNs are dropped"""
    if typ == T_DOUBLE:
        m = np.ascontiguousarray(members, dtype=np.float64)
        m = m[~np.isnan(m)]
        m = np.where(m == 0, 0.0, m)
        return np.unique(m.view(np.int64))
    return np.unique(np.ascontiguousarray(members, dtype=np.int64))


def evaluate(prog, cols, n):
    """the program's verdict on stream positions 0 .. n-1 -> bool[n]"""
    st = []
    with np.errstate(invalid="ignore"):
        for (op, cmp_, typ, a, b, imm) in prog:
            if op == P_CMP_COL_CONST or op == P_CMP_CONST_COL:
                v, isnull = load(cols[a], n)
                c = _const(typ, imm)
                r = _CMP[cmp_](_as(typ, v), c) if op == P_CMP_COL_CONST else _CMP[cmp_](c, _as(typ, v))
                st.append(~isnull & r)
            elif op == P_CMP_COL_COL:
                va, na = load(cols[a], n)
                vb, nb = load(cols[b], n)
                st.append(~na & ~nb & _CMP[cmp_](_as(typ, va), _as(typ, vb)))
            elif op == P_ISNULL:
                _, isnull = load(cols[a], n)
                st.append(isnull ^ bool(cmp_))
            elif op == P_CONST:
                st.append(np.full(n, imm_bits(imm, T_INT64) != 0))
            elif op == P_IN_BITS:
                v, isnull = load(cols[a], n)
                table = np.ascontiguousarray(imm, dtype=np.uint64)
                assert len(table) == b
                u = v.view(np.uint64)
                word = u >> np.uint64(6)
                inside = word < np.uint64(b)
                w = table[np.where(inside, word, np.uint64(0)).astype(np.int64)] if b else np.zeros(n, dtype=np.uint64)
                hit = inside & (((w >> (u & np.uint64(63))) & np.uint64(1)) != 0)
                st.append(~isnull & (hit ^ bool(cmp_)))
            elif op == P_IN_SET:
                v, isnull = load(cols[a], n)
                if typ == T_DOUBLE:
                    f = v.view(np.float64)
                    v = np.where(f == 0, np.int64(0), v)
                    member = np.isin(v, set_members(typ, imm)) & ~np.isnan(f)
                else:
                    member = np.isin(v, set_members(typ, imm))
                st.append(~isnull & (member ^ bool(cmp_)))
            elif op in (P_AND, P_OR, P_XOR):
                r = st.pop()
                l = st.pop()
                st.append((l & r) if op == P_AND else ((l | r) if op == P_OR else (l ^ r)))
            else:
                raise ValueError(f"unknown predicate opcode {op}")
    assert len(st) == 1, "malformed program"
    return st[0]


# ------------------------------------------------------------------------------------------------ columns

INT_SPECIALS = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], dtype=np.int64)
NAN_A, NAN_B = 0x7FF8000000000000, 0xFFF8000000000001
DBL_SPECIAL_BITS = np.array([double_bits(-np.inf), double_bits(-1.5), double_bits(-5e-324), double_bits(-0.0), double_bits(0.0),
                             double_bits(5e-324), double_bits(1.5), double_bits(np.inf), NAN_A, NAN_B - (1 << 64)], dtype=np.int64)
INT_CONSTS = (I64_MIN, -1, 0, 7, I64_MAX)
DBL_CONSTS = (-np.inf, -0.0, 0.0, 5e-324, 1.5, np.inf, float("nan"))

# column slots of the shared program list
SLOT_A, SLOT_B, SLOT_X, SLOT_Y, SLOT_C = 0, 1, 2, 3, 4


def _int_column(rng, n):
    kind = rng.integers(0, 3, n)
    small = rng.integers(-50, 51, n, dtype=np.int64)
    wide = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    return np.where(kind == 0, rng.choice(INT_SPECIALS, n), np.where(kind == 1, small, wide))


def _double_column(rng, n):
    normal = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
    bits = np.where(rng.random(n) < 0.4, rng.choice(DBL_SPECIAL_BITS, n), normal.view(np.int64))
    return bits.view(np.float64)


def make_columns(rows, seed=1234):
    """The columns of the filter tests over `rows` base rows, and a row-id vector of rows - 7 stream positions over them.

    a, b   INT64: a third of the cells from INT_SPECIALS, a third from [-50, 50], the rest full range; b == a in about 20 % of the rows
    x, y   DOUBLE: 40 % of the cells from DBL_SPECIAL_BITS (infinities, denormals, both zeros, two NaNs), the rest normals times
           10^[-8, 8]; y is bit-equal to x in 10 % of the rows and, in about 5 %, the other zero or the other NaN
    c      INT64 from [-50, 50], the column without a NULL bitmap
    *_null 10 % NULL, independently per column
    rid    5 % MDB_NO_ROW
    """
    rng = np.random.default_rng(seed)
    a = _int_column(rng, rows)
    b = np.where(rng.random(rows) < 0.2, a, _int_column(rng, rows))
    x = _double_column(rng, rows)
    y = _double_column(rng, rows)
    y = np.where(rng.random(rows) < 0.1, x.view(np.int64), y.view(np.int64)).view(np.float64)
    xb = x.view(np.int64)
    twin = rng.random(rows) < 0.3       # zeros and NaNs are 16 % of x: about 5 % of all rows
    other_zero = np.where(xb == 0, double_bits(-0.0), 0)
    other_nan = np.where(xb == NAN_A, NAN_B - (1 << 64), NAN_A)
    yb = np.where(twin & (x == 0), other_zero, np.where(twin & np.isnan(x), other_nan, y.view(np.int64)))
    y = yb.view(np.float64)
    c = rng.integers(-50, 51, rows, dtype=np.int64)
    nulls = {k: rng.random(rows) < 0.1 for k in ("a", "b", "x", "y")}
    rid = rng.integers(0, rows, rows - 7).astype(np.uint32)
    rid[rng.random(rows - 7) < 0.05] = NO_ROW
    return dict(a=a, b=b, x=x, y=y, c=c, a_null=nulls["a"], b_null=nulls["b"], x_null=nulls["x"], y_null=nulls["y"], rid=rid)


def bind(w, rid=False):
    """the model's column list in slot order, direct or all through the row-id vector"""
    r = w["rid"] if rid else None
    return [(w["a"], w["a_null"], r), (w["b"], w["b_null"], r), (w["x"], w["x_null"], r), (w["y"], w["y_null"], r), (w["c"], None, r)]


# ------------------------------------------------------------------------------------------------ programs
# (name, kind, program).  kind = the kernel form that mdb_dev_filter's dispatch gives the program over a base-table stream:
#   "cmp1"     ONE comparison of an INT64 column with a constant (col <cmp> const)
#   "terms"    comparisons of one INT64 column with constants, all ANDed or all ORed (filter_one_column_terms)
#   "inset"    ONE MDB_P_IN_SET
#   "general"  everything else: the interpreters

# members / bit table of the mixed composite
SET_I64 = np.array([I64_MIN, -1, 7, 13, -40, 25, I64_MAX - 1], dtype=np.int64)
SET_DBL = np.array([-0.0, np.inf, float("nan"), 1.5, -5e-324])
BIT_TABLE = np.array([0x0000F0F0F0F0F0F3, 0x00000000FFFF0000], dtype=np.uint64)     # ids 0 and 1 set, 2 and 3 not ...


def cc(cmp_, typ, slot, imm):
    return (P_CMP_COL_CONST, cmp_, typ, slot, 0, imm)


def kc(cmp_, typ, slot, imm):
    return (P_CMP_CONST_COL, cmp_, typ, slot, 0, imm)


def colcol(cmp_, typ, sa, sb):
    return (P_CMP_COL_COL, cmp_, typ, sa, sb, 0)


def isnull(slot, negate=False):
    return (P_ISNULL, 1 if negate else 0, 0, slot, 0, 0)


def const(v):
    return (P_CONST, 0, 0, 0, 0, v)


def in_set(slot, members, typ, negate=False):
    return (P_IN_SET, 1 if negate else 0, typ, slot, 0, members)


def in_bits(slot, table, negate=False):
    return (P_IN_BITS, 1 if negate else 0, T_INT64, slot, len(table), table)


AND, OR, XOR = (P_AND, 0, 0, 0, 0, 0), (P_OR, 0, 0, 0, 0, 0), (P_XOR, 0, 0, 0, 0, 0)


def _cname(c):
    if isinstance(c, float):
        return "nan" if c != c else repr(c)
    return {I64_MIN: "min", I64_MAX: "max"}.get(c, str(c))


def generated_programs():
    """all six operators x {col-const, const-col, col-col} x {INT64, DOUBLE} over INT_CONSTS / DBL_CONSTS; IS [NOT] NULL; CONST"""
    out = []
    for typ, tn, slot, other, consts in ((T_INT64, "i", SLOT_A, SLOT_B, INT_CONSTS), (T_DOUBLE, "d", SLOT_X, SLOT_Y, DBL_CONSTS)):
        for cmp_ in CMPS:
            for c in consts:
                out.append((f"{tn}_col_{CMP_NAME[cmp_]}_{_cname(c)}", "cmp1" if typ == T_INT64 else "general", [cc(cmp_, typ, slot, c)]))
                out.append((f"{tn}_{_cname(c)}_{CMP_NAME[cmp_]}_col", "general", [kc(cmp_, typ, slot, c)]))
            out.append((f"{tn}_col_{CMP_NAME[cmp_]}_col", "general", [colcol(cmp_, typ, slot, other)]))
    for slot, nm in ((SLOT_A, "a"), (SLOT_X, "x")):
        out.append((f"{nm}_is_null", "general", [isnull(slot)]))
        out.append((f"{nm}_is_not_null", "general", [isnull(slot, True)]))
    out.append(("const_0", "general", [const(0)]))
    out.append(("const_1", "general", [const(1)]))
    return out


_LEAVES = [cc(CMP_LT, T_INT64, SLOT_A, 0), cc(CMP_GT, T_DOUBLE, SLOT_X, 0.0), colcol(CMP_LE, T_INT64, SLOT_A, SLOT_B),
           kc(CMP_GE, T_INT64, SLOT_C, 3), isnull(SLOT_Y), colcol(CMP_NE, T_DOUBLE, SLOT_X, SLOT_Y), cc(CMP_EQ, T_INT64, SLOT_B, -1),
           kc(CMP_LT, T_DOUBLE, SLOT_Y, 1.5), cc(CMP_GE, T_INT64, SLOT_C, -10), isnull(SLOT_B, True), cc(CMP_LE, T_DOUBLE, SLOT_Y, -0.0)]
_OPS = [XOR, AND, XOR, OR, XOR]
DEEP_LEAVES = 32      # 2 * 32 - 1 = 63 instructions: the longest well-formed program within MDB_PRED_MAX_INSNS = 64


def left_deep():
    """leaf leaf op leaf op ...: 63 instructions, the stack never deeper than 2"""
    p = [_LEAVES[0]]
    for i in range(1, DEEP_LEAVES):
        p += [_LEAVES[i % len(_LEAVES)], _OPS[i % len(_OPS)]]
    return p


def right_deep():
    """32 leaves, then 31 connectives: 63 instructions, the stack 32 deep - the deepest a well-formed program of at most 64 instructions
    gets (the validator's own limit of 60 is beyond what 64 instructions can push and still end on one value)"""
    p = [_LEAVES[i % len(_LEAVES)] for i in range(DEEP_LEAVES)]
    p += [_OPS[(i + 1) % len(_OPS)] for i in range(DEEP_LEAVES - 2)] + [XOR]
    return p


def composite_programs():
    ai, ax = T_INT64, T_DOUBLE
    return [
        ("and2", "general", [cc(CMP_LT, ai, SLOT_A, 0), cc(CMP_GT, ai, SLOT_B, 0), AND]),
        ("or2", "general", [cc(CMP_EQ, ai, SLOT_A, I64_MIN), cc(CMP_EQ, ai, SLOT_B, I64_MAX), OR]),
        ("xor2", "general", [cc(CMP_LT, ai, SLOT_A, 7), cc(CMP_GE, ax, SLOT_X, -0.0), XOR]),
        ("xor_of_nulls", "general", [isnull(SLOT_A), isnull(SLOT_X), XOR]),
        ("and_or", "general", [cc(CMP_LE, ai, SLOT_A, -1), colcol(CMP_EQ, ai, SLOT_A, SLOT_B), AND, cc(CMP_GT, ax, SLOT_Y, np.inf), OR]),
        ("or_and_xor", "general", [colcol(CMP_LT, ax, SLOT_X, SLOT_Y), kc(CMP_LT, ai, SLOT_C, 0), OR, isnull(SLOT_B, True), AND,
                                   kc(CMP_NE, ax, SLOT_X, float("nan")), XOR]),
        ("const_in_tree", "general", [const(1), cc(CMP_NE, ai, SLOT_A, 0), AND, const(0), OR, const(1), XOR]),
        ("double_eq_both_zeros", "general", [cc(CMP_EQ, ax, SLOT_X, -0.0), cc(CMP_EQ, ax, SLOT_Y, 0.0), AND]),
        ("two_columns_range", "general", [cc(CMP_GE, ai, SLOT_A, I64_MIN + 1), cc(CMP_LE, ai, SLOT_B, I64_MAX - 1), AND,
                                          cc(CMP_NE, ai, SLOT_C, 0), AND]),
        ("in_bits", "general", [in_bits(SLOT_A, BIT_TABLE)]),
        ("not_in_bits_or_null", "general", [in_bits(SLOT_A, BIT_TABLE, True), isnull(SLOT_A), OR]),
        ("in_set_i64", "inset", [in_set(SLOT_A, SET_I64, ai)]),
        ("not_in_set_i64", "inset", [in_set(SLOT_A, SET_I64, ai, True)]),
        ("in_set_dbl", "inset", [in_set(SLOT_X, SET_DBL, ax)]),
        ("not_in_set_dbl", "inset", [in_set(SLOT_X, SET_DBL, ax, True)]),
        ("mixed", "general", [in_set(SLOT_A, SET_I64, ai), in_set(SLOT_X, SET_DBL, ax, True), AND, in_bits(SLOT_C, BIT_TABLE), OR,
                              in_set(SLOT_Y, SET_DBL, ax), in_set(SLOT_B, SET_I64, ai, True), XOR, AND,
                              colcol(CMP_GE, ax, SLOT_X, SLOT_Y), cc(CMP_LT, ai, SLOT_B, 7), AND, in_bits(SLOT_B, BIT_TABLE, True), XOR, OR]),
        ("left_deep_63", "general", left_deep()),
        ("right_deep_63", "general", right_deep()),
    ]


def term_programs():
    """programs that filter_one_column_terms accepts, all on slot 0 (column a): every operator as the only kind of term, INT64_MIN and
    INT64_MAX as constants, exactly 1, 2 and 8 terms, IS NOT NULL among ANDed and IS NULL among ORed terms, a const-col term"""
    t = T_INT64
    out = []
    pairs = {CMP_LT: (7, I64_MAX), CMP_GT: (-1, I64_MIN), CMP_NE: (I64_MIN, I64_MAX), CMP_EQ: (0, 0), CMP_LE: (I64_MAX - 1, -1), CMP_GE: (I64_MIN + 1, 1)}
    for cmp_ in CMPS:
        c1, c2 = pairs[cmp_]
        out.append((f"t_and_{CMP_NAME[cmp_]}", "terms", [cc(cmp_, t, SLOT_A, c1), cc(cmp_, t, SLOT_A, c2), AND]))
        o1, o2 = (I64_MIN, I64_MAX) if cmp_ == CMP_EQ else ((0, 0) if cmp_ == CMP_NE else (c1, c2))
        out.append((f"t_or_{CMP_NAME[cmp_]}", "terms", [cc(cmp_, t, SLOT_A, o1), cc(cmp_, t, SLOT_A, o2), OR]))
    out += [
        ("t_one_term_and_not_null", "terms", [cc(CMP_GT, t, SLOT_A, 0), isnull(SLOT_A, True), AND]),
        ("t_one_term_or_null", "terms", [cc(CMP_EQ, t, SLOT_A, 7), isnull(SLOT_A), OR]),
        ("t_range_not_null", "terms", [isnull(SLOT_A, True), cc(CMP_GE, t, SLOT_A, -50), AND, cc(CMP_LE, t, SLOT_A, 50), AND]),
        ("t_or_null_extremes", "terms", [cc(CMP_EQ, t, SLOT_A, I64_MIN), isnull(SLOT_A), OR, cc(CMP_EQ, t, SLOT_A, I64_MAX), OR]),
        ("t_const_col", "terms", [kc(CMP_GT, t, SLOT_A, 7), kc(CMP_LT, t, SLOT_A, I64_MIN), AND]),      # 7 > a AND min < a
        ("t_and_8", "terms", [cc(CMP_GE, t, SLOT_A, I64_MIN + 1), cc(CMP_LE, t, SLOT_A, I64_MAX - 1), AND, cc(CMP_NE, t, SLOT_A, 0), AND,
                              cc(CMP_NE, t, SLOT_A, 1), AND, cc(CMP_NE, t, SLOT_A, -1), AND, cc(CMP_GT, t, SLOT_A, -40), AND,
                              cc(CMP_LT, t, SLOT_A, I64_MAX), AND, kc(CMP_NE, t, SLOT_A, 7), AND]),
        ("t_or_8", "terms", [cc(CMP_EQ, t, SLOT_A, I64_MIN), cc(CMP_EQ, t, SLOT_A, -1), OR, cc(CMP_EQ, t, SLOT_A, 0), OR,
                             cc(CMP_EQ, t, SLOT_A, 7), OR, cc(CMP_EQ, t, SLOT_A, I64_MAX), OR, cc(CMP_EQ, t, SLOT_A, 13), OR,
                             cc(CMP_EQ, t, SLOT_A, -33), OR, cc(CMP_GT, t, SLOT_A, I64_MAX - 1), OR]),
    ]
    return out


def all_programs():
    return generated_programs() + composite_programs() + term_programs()


def provably_empty(prog):
    """a single comparison that no value satisfies, whatever the column holds: below the least value, above the greatest, or any
    operator but <> against a NaN.  (The program list keeps them: a kernel must answer "no row" there too.)"""
    if len(prog) != 1 or prog[0][0] not in (P_CMP_COL_CONST, P_CMP_CONST_COL):
        return False
    op, cmp_, typ, _a, _b, imm = prog[0]
    if op == P_CMP_CONST_COL:      # const <cmp> col  ==  col <flipped cmp> const
        cmp_ = {CMP_LT: CMP_GT, CMP_GT: CMP_LT, CMP_LE: CMP_GE, CMP_GE: CMP_LE}.get(cmp_, cmp_)
    if typ == T_INT64:
        return (cmp_ == CMP_LT and imm == I64_MIN) or (cmp_ == CMP_GT and imm == I64_MAX)
    if imm != imm:
        return cmp_ != CMP_NE
    return (cmp_ == CMP_LT and imm == -np.inf) or (cmp_ == CMP_GT and imm == np.inf)
