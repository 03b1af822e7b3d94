"""Every kernel form of mdb_dev_filter.hip against tests/filter_model.py, bit for bit, with the form asserted after every call.

filter_run() chooses among (profiler name: kernel):
    onerow      filter_pred_bits: k_pred_bits<0>           a bound column has a row-id vector or starts 8 bytes off a 16-byte boundary
    pair        filter_pred_bits: k_pred_bits_pair<0>      all bound columns direct, the program not special
    cmp1        filter_pred_bits: k_pred_bits_cmp1<CMP>    filter(), one INT64 col-const comparison, n < 2^18
    scan_cmp1   scan_project: k_scan_project_cmp1<CMP,8>   the same program in filter() from 2^18 rows on and in filter_project() at any n
    terms       filter_pred_bits: k_pred_bits_terms<OR>    filter(), a term list on one INT64 column
    scan_terms  scan_project: k_scan_project_terms<OR,8>   filter_project(), the same programs
    inset       filter_in_set: k_pred_bits_inset<LDS>      one MDB_P_IN_SET (its own matrix: tests/test_in_set_gpu.py)
behind every bitmap form filter() launches filter_bits_to_sel: k_bits_to_sel, and filter_project() lets the bitmap kernel go on into
filt_fused_tail (no launch of its own: the bitmap kernel under filter_project IS that tail's case).

Each test opens a context of its own with the profiler on: mdb_dev_prof_symbols lists the kernels launched since then, and the set of
them has to be exactly the named form's after every single call - a case that reaches another form fails there.

Row counts: around a ballot word (64), a two-row span (128), a row block of the bitmap forms (4096) and of the one-pass forms (16384),
mdb_dev_filter's switch to the one-pass form (2^18), and one count with 66 row blocks in front of the last one per look-back (more
predecessors than one wave polls at a time).  The columns hold INT64_MIN / INT64_MAX, NaNs, both zeros, infinities and denormals
(filter_model.make_columns); they are built once at the largest count, the tests take prefixes.

The validator's nesting limit of 60 cannot be reached by a well-formed program of MDB_PRED_MAX_INSNS = 64 instructions (k pushes
need k - 1 connectives); the deep programs here are the longest there are: 63 instructions, the stack 32 deep and 2 deep."""
import collections

import numpy as np
import pytest

from midoridb_amd import dev as D
from tests import filter_model as fm

pytestmark = pytest.mark.gpu

BITMAP_ROWS = [1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8193]
ONE_PASS_ROWS = BITMAP_ROWS + [16383, 16384, 16385, 32769]
SWITCH = 1 << 18                  # mdb_dev_filter: one comparison takes the one-pass form from here on
LONG_TAIL = 66 * 4096 + 3         # 67 row blocks of filt_fused_tail
LONG_SCAN = 66 * 16384 + 3        # 67 row blocks of scan_project_body
NMAX = LONG_SCAN

PROGRAMS = fm.all_programs()
BY_KIND = {k: [(n_, p) for n_, kk, p in PROGRAMS if kk == k] for k in ("cmp1", "terms", "inset", "general")}
BY_NAME = {n_: p for n_, _k, p in PROGRAMS}

BITS, SEL = ("filter_pred_bits", "k_pred_bits"), ("filter_bits_to_sel", "k_bits_to_sel")
PROJECT_FORMS = {       # form -> {(profiler name, kernel)} of one mdb_dev_filter_project
    "onerow": {BITS}, "pair": {("filter_pred_bits", "k_pred_bits_pair")}, "cmp1": {("filter_pred_bits", "k_pred_bits_cmp1")},
    "terms": {("filter_pred_bits", "k_pred_bits_terms")}, "inset": {("filter_in_set", "k_pred_bits_inset")},
    "scan_cmp1": {("scan_project", "k_scan_project_cmp1")}, "scan_terms": {("scan_project", "k_scan_project_terms")},
}
FILTER_FORMS = {f: (k if f.startswith("scan") else k | {SEL}) for f, k in PROJECT_FORMS.items() if f != "scan_terms"}
PROF_NAMES = ("filter_pred_bits", "scan_project", "filter_in_set", "filter_bits_to_sel")

RAN = collections.Counter()       # (call, form) -> (program, row count) cases that ran and asserted their form


@pytest.fixture
def ctx():
    """a device context of this test's own, profiling on: prof_symbols() then lists what this test launched and nothing else"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this environment")
    from midoridb_amd.dev import DeviceCtx
    c = DeviceCtx(0)
    c.prof_enable(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(dev):
    """the columns on the host and on the device, the misaligned copy, the row-id vector, the two sets and the bit table"""
    host = fm.make_columns(NMAX + 7)
    d = {k: dev.to_dev(host[k]) for k in ("a", "b", "x", "y", "c", "rid")}
    for k in ("a", "b", "x", "y"):
        d[k + "_null"] = dev.nullbits_dev(host[k + "_null"])
    shifted = dev.to_dev(np.concatenate([np.zeros(1, dtype=np.int64), host["a"]]))
    d["a_mis"] = shifted[1:]                       # the same cells one 8-byte step off a 16-byte boundary
    d["a_copy"] = dev.to_dev(host["a"])            # ... and at another aligned address
    d["table"] = dev.to_dev(fm.BIT_TABLE)
    assert all(d[k].data_ptr() % 16 == 0 for k in ("a", "b", "x", "y", "c", "a_copy", "table")) and shifted.data_ptr() % 16 == 0
    assert d["a_mis"].data_ptr() % 16 == 8
    assert (host["rid"][:64] == fm.NO_ROW).any() and int(host["rid"][host["rid"] != fm.NO_ROW].max()) > NMAX
    sets = {fm.T_INT64: dev.make_set(fm.SET_I64), fm.T_DOUBLE: dev.make_set(fm.SET_DBL, D.T_DOUBLE)}
    yield dict(host=host, d=d, sets=sets, keep=shifted)
    for s in sets.values():
        s.close()
    print("\nfilter forms, (program, row count) cases per call and form:")
    for (call, form), cnt in sorted(RAN.items()):
        print(f"    {call:15s} {form:11s} {cnt}")


# ------------------------------------------------------------------------------------------------ helpers

def _device_prog(world, prog):
    """the model's form of a program -> the device's: the member list / bit table replaced by the uploaded image's address"""
    out = []
    for (op, c, t, a, b, imm) in prog:
        if op == fm.P_IN_SET:
            assert imm is (fm.SET_DBL if t == fm.T_DOUBLE else fm.SET_I64)
            out.append(world["sets"][t].insn(a, bool(c)))
        elif op == fm.P_IN_BITS:
            assert imm is fm.BIT_TABLE
            out.append((op, c, t, a, b, world["d"]["table"].data_ptr()))
        else:
            out.append((op, c, t, a, b, imm))
    return out


def _bind_dev(world, variant="direct"):
    """the five slots of the program list on the device.  direct: base columns; rid: all through the row-id vector; mis: slot 0 at the
    misaligned address"""
    d = world["d"]
    r = d["rid"] if "rid" in variant else None
    a = d["a_mis"] if "mis" in variant else d["a"]
    return [(a, d["a_null"], r), (d["b"], d["b_null"], r), (d["x"], d["x_null"], r), (d["y"], d["y_null"], r), (d["c"], None, r)]


_MODEL = {}


def _model(world, name, prog, n, tag="direct", cols=None):
    """the model's verdicts for rows 0 .. n-1 (a row's verdict does not depend on n: computed once per program and binding for the
    largest count of n's size class, then sliced).  tag names the binding; cols = its host columns when it is not direct / rid"""
    cap = 8193 if n <= 8193 else (32769 if n <= 32769 else n)
    key = (name, tag, cap)
    if key not in _MODEL:
        _MODEL[key] = fm.evaluate(prog, cols if cols is not None else fm.bind(world["host"], tag == "rid"), cap)
    return _MODEL[key][:n]


def _ran(ctx):
    return {(nm, s.split("<")[0]) for nm in PROF_NAMES for s in ctx.prof_symbols(nm)}


def _filter(ctx, world, form, prog, cols, n, expect, label):
    ctx.prof_reset()
    got = ctx.filter(_device_prog(world, prog), cols, n).cpu().numpy().astype(np.int64)
    assert _ran(ctx) == FILTER_FORMS[form], (label, n, form, sorted(_ran(ctx)))
    RAN[("filter", form)] += 1
    exp = np.flatnonzero(expect)
    assert got.shape == exp.shape and np.array_equal(got, exp), (label, n, len(got), len(exp))


def _project(ctx, world, form, prog, cols, n, expect, proj_dev, proj_host, label):
    """proj_dev = [(values, nullbits or None)] on the device, proj_host = the same columns on the host as (values, nulls or None)"""
    ctx.prof_reset()
    m, outs = ctx.filter_project(_device_prog(world, prog), cols, n, proj_dev)
    assert _ran(ctx) == PROJECT_FORMS[form], (label, n, form, sorted(_ran(ctx)))
    RAN[("filter_project", form)] += 1
    keep = np.flatnonzero(expect)
    assert m == len(keep), (label, n, m, len(keep))
    for c, ((vals, nulls), (ov, on)) in enumerate(zip(proj_host, outs)):
        got = ov.cpu().numpy().view(np.int64)
        assert got.shape == (m,) and np.array_equal(got, np.ascontiguousarray(vals[:n]).view(np.int64)[keep]), (label, n, "column", c)
        if nulls is None:
            assert on is None, (label, n, "column", c)
        else:
            assert on is not None, (label, n, "column", c)
            assert np.array_equal(D.unpack_nullbits(on.cpu().numpy().view(np.uint64), m), nulls[:n][keep]), (label, n, "NULL bits", c)


def _projection(world, own="a"):
    """the predicate's own column, a second INT64 column with NULLs, a DOUBLE column without a bitmap, and both INT64 columns again"""
    d, h = world["d"], world["host"]
    dev = [(d[own], d["a_null"]), (d["b"], d["b_null"]), (d["x"], None), (d[own], d["a_null"]), (d["b"], d["b_null"])]
    host = [(h["a"], h["a_null"]), (h["b"], h["b_null"]), (h["x"], None), (h["a"], h["a_null"]), (h["b"], h["b_null"])]
    return dev, host


def _no_bitmap(world):
    """slot 0 = column a without its NULL bitmap, nothing else bound -> (device binding, host binding)"""
    return [(world["d"]["a"], None, None)], [(world["host"]["a"], None, None)]


# ------------------------------------------------------------------------------------------------ filter(): the two interpreters

@pytest.mark.parametrize("n", BITMAP_ROWS)
@pytest.mark.parametrize("variant", ["direct", "rid", "mis", "rid+mis"])
def test_filter_interpreters_run_the_whole_program_list(ctx, world, variant, n):
    """direct columns: the pair interpreter - a program that filter_run would give to a specialised kernel is made general by "AND TRUE";
    a row-id vector, the misaligned copy of slot 0, or both: the one-row interpreter, whatever the program"""
    form = "pair" if variant == "direct" else "onerow"
    cols = _bind_dev(world, variant)
    for name, kind, prog in PROGRAMS:
        run = prog + [fm.const(1), fm.AND] if variant == "direct" and kind != "general" else prog
        exp = _model(world, name, prog, n, "rid" if "rid" in variant else "direct")
        _filter(ctx, world, form, run, cols, n, exp, (name, variant))


# ------------------------------------------------------------------------------------------------ filter(): the specialised forms

@pytest.mark.parametrize("n", BITMAP_ROWS + [SWITCH - 1])
def test_filter_one_comparison_bitmap_form(ctx, world, n):
    nb_dev, nb_host = _no_bitmap(world)
    for name, prog in BY_KIND["cmp1"]:
        _filter(ctx, world, "cmp1", prog, _bind_dev(world), n, _model(world, name, prog, n), name)
        _filter(ctx, world, "cmp1", prog, nb_dev, n, _model(world, name, prog, n, "no_bitmap", nb_host), (name, "no bitmap"))


@pytest.mark.parametrize("n", [SWITCH, SWITCH + 1])
def test_filter_one_comparison_one_pass_form(ctx, world, n):
    nb_dev, nb_host = _no_bitmap(world)
    for name, prog in BY_KIND["cmp1"]:
        _filter(ctx, world, "scan_cmp1", prog, _bind_dev(world), n, _model(world, name, prog, n), name)
        _filter(ctx, world, "scan_cmp1", prog, nb_dev, n, _model(world, name, prog, n, "no_bitmap", nb_host), (name, "no bitmap"))


@pytest.mark.parametrize("n", BITMAP_ROWS + [SWITCH + 1])
def test_filter_term_list_bitmap_form(ctx, world, n):
    """term lists keep the three passes in filter() at every row count; IS NULL among ORed terms with and without a bitmap"""
    nb_dev, nb_host = _no_bitmap(world)
    for name, prog in BY_KIND["terms"]:
        _filter(ctx, world, "terms", prog, _bind_dev(world), n, _model(world, name, prog, n), name)
        _filter(ctx, world, "terms", prog, nb_dev, n, _model(world, name, prog, n, "no_bitmap", nb_host), (name, "no bitmap"))


def test_filter_one_pass_long_look_back(ctx, world):
    """67 row blocks of 16384 rows: the last ones have more predecessors than the 64 a wave polls at a time"""
    for name in ("i_col_lt_0", "i_col_ne_7", "i_col_ge_min"):
        _filter(ctx, world, "scan_cmp1", BY_NAME[name], _bind_dev(world), LONG_SCAN, _model(world, name, BY_NAME[name], LONG_SCAN), name)


# ------------------------------------------------------------------------------------------------ forced survivor patterns

PATTERNS = ["every_row", "no_row", "row_0", "last_row", "rows_63_64", "one_percent"]
EQ7 = [fm.cc(fm.CMP_EQ, fm.T_INT64, 0, 7)]
GT0 = [fm.cc(fm.CMP_GT, fm.T_INT64, 0, 0)]
RANGE_1_7 = [fm.cc(fm.CMP_GE, fm.T_INT64, 0, 1), fm.cc(fm.CMP_LE, fm.T_INT64, 0, 7), fm.AND]
IN_7_8 = [fm.cc(fm.CMP_EQ, fm.T_INT64, 0, 8), fm.cc(fm.CMP_EQ, fm.T_INT64, 0, 7), fm.OR]


def _pattern(pattern, n):
    """a column of n cells that passes all four programs above exactly in the pattern's rows (7 there, -7 elsewhere)"""
    keep = np.zeros(n, dtype=bool)
    if pattern == "every_row":
        keep[:] = True
    elif pattern == "row_0":
        keep[0] = True
    elif pattern == "last_row":
        keep[n - 1] = True
    elif pattern == "rows_63_64":
        keep[63:65] = True
    elif pattern == "one_percent":
        keep[np.random.default_rng(n).random(n) < 0.01] = True
    return np.where(keep, np.int64(7), np.int64(-7)), keep


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("form,n", [("cmp1", 129), ("cmp1", 4097), ("cmp1", 8193), ("scan_cmp1", SWITCH + 1),
                                    ("terms", 129), ("terms", 4097), ("terms", 8193)])
def test_filter_specialised_forms_survivor_patterns(ctx, world, form, n, pattern):
    vals, keep = _pattern(pattern, n)
    col = [(ctx.to_dev(vals), None, None)]
    for prog in ((RANGE_1_7, IN_7_8) if form == "terms" else (EQ7, GT0)):
        exp = fm.evaluate(prog, [(vals, None, None)], n)
        assert np.array_equal(exp, keep)
        _filter(ctx, world, form, prog, col, n, exp, (pattern, form))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("form", ["scan_cmp1", "scan_terms"])
@pytest.mark.parametrize("n", [129, 16385, 32769])
def test_filter_project_one_pass_forms_survivor_patterns(ctx, world, form, n, pattern):
    vals, keep = _pattern(pattern, n)
    d_vals, d, h = ctx.to_dev(vals), world["d"], world["host"]
    for prog in ((RANGE_1_7, IN_7_8) if form == "scan_terms" else (EQ7, GT0)):
        exp = fm.evaluate(prog, [(vals, None, None)], n)
        assert np.array_equal(exp, keep)
        _project(ctx, world, form, prog, [(d_vals, None, None)], n, exp, [(d_vals, None), (d["b"], d["b_null"])],
                 [(vals, None), (h["b"], h["b_null"])], (pattern, form))


# ------------------------------------------------------------------------------------------------ filter_project(): every form under it

@pytest.mark.parametrize("n", ONE_PASS_ROWS)
def test_filter_project_one_comparison_one_pass(ctx, world, n):
    pd, ph = _projection(world)
    for name, prog in BY_KIND["cmp1"]:
        _project(ctx, world, "scan_cmp1", prog, _bind_dev(world), n, _model(world, name, prog, n), pd, ph, name)


@pytest.mark.parametrize("n", ONE_PASS_ROWS)
def test_filter_project_term_list_one_pass(ctx, world, n):
    pd, ph = _projection(world)
    nb_dev, nb_host = _no_bitmap(world)
    for name, prog in BY_KIND["terms"]:
        _project(ctx, world, "scan_terms", prog, _bind_dev(world), n, _model(world, name, prog, n), pd, ph, name)
        _project(ctx, world, "scan_terms", prog, nb_dev, n, _model(world, name, prog, n, "no_bitmap", nb_host), pd, ph, (name, "no bitmap"))


@pytest.mark.parametrize("n", BITMAP_ROWS)
def test_filter_project_pair_interpreter_and_tail(ctx, world, n):
    pd, ph = _projection(world)
    for name, prog in BY_KIND["general"]:
        _project(ctx, world, "pair", prog, _bind_dev(world), n, _model(world, name, prog, n), pd, ph, name)


@pytest.mark.parametrize("n", BITMAP_ROWS)
@pytest.mark.parametrize("variant", ["rid", "mis"])
def test_filter_project_one_row_interpreter_and_tail(ctx, world, variant, n):
    """the predicate through the row-id vector (the projected columns are the scanned table's own rows), or on the misaligned copy -
    which the tail, copying cell by cell, also projects"""
    pd, ph = _projection(world, "a_mis" if variant == "mis" else "a")
    for name, _kind, prog in PROGRAMS:
        _project(ctx, world, "onerow", prog, _bind_dev(world, variant), n, _model(world, name, prog, n, "rid" if variant == "rid" else "direct"),
                 pd, ph, (name, variant))


@pytest.mark.parametrize("n", BITMAP_ROWS)
def test_filter_project_set_probe_and_tail(ctx, world, n):
    pd, ph = _projection(world)
    for name, prog in BY_KIND["inset"]:
        _project(ctx, world, "inset", prog, _bind_dev(world), n, _model(world, name, prog, n), pd, ph, name)


@pytest.mark.parametrize("form", ["pair", "onerow", "inset", "cmp1", "terms"])
def test_filter_project_tail_long_look_back(ctx, world, form):
    """67 row blocks of 4096 rows through filt_fused_tail behind each bitmap kernel (cmp1 / terms: a projected column at the misaligned
    address keeps the call off the one-pass kernels)"""
    n = LONG_TAIL
    names = {"pair": ("mixed", "right_deep_63"), "onerow": ("mixed", "d_col_ne_nan"), "inset": ("in_set_i64", "not_in_set_dbl"),
             "cmp1": ("i_col_le_-1", "i_col_eq_max"), "terms": ("t_and_8", "t_or_null_extremes")}[form]
    pd, ph = _projection(world, "a_mis" if form in ("cmp1", "terms") else "a")
    tag = "rid" if form == "onerow" else "direct"
    for name in names:
        _project(ctx, world, form, BY_NAME[name], _bind_dev(world, tag), n, _model(world, name, BY_NAME[name], n, tag), pd, ph, name)


@pytest.mark.parametrize("form", ["scan_cmp1", "scan_terms"])
def test_filter_project_one_pass_long_look_back(ctx, world, form):
    n = LONG_SCAN
    names = ("i_col_gt_-1", "i_col_ne_min") if form == "scan_cmp1" else ("t_or_8", "t_range_not_null")
    pd, ph = _projection(world)
    for name in names:
        _project(ctx, world, form, BY_NAME[name], _bind_dev(world), n, _model(world, name, BY_NAME[name], n), pd, ph, name)


# ------------------------------------------------------------------------------------------------ the dispatch conditions

@pytest.mark.parametrize("other", ["direct", "rid", "mis", "mis_first"])
def test_filter_one_pass_needs_every_bound_column_direct(ctx, world, other):
    """2^18 + 1 rows, one INT64 col-const comparison, and a second bound column that the program never reads: read through the row-id
    vector or at the misaligned address it keeps the call on the three passes (mdb_dev_filter and filter_run decide alike: the one-row
    interpreter must not be handed the one-pass kernel's look-back words); with two direct columns the call takes the one pass"""
    d, h, n = world["d"], world["host"], SWITCH + 1
    slot = 1 if other == "mis_first" else 0
    cols = {"direct": [(d["a"], d["a_null"], None), (d["b"], d["b_null"], None)],
            "rid": [(d["a"], d["a_null"], None), (d["b"], d["b_null"], d["rid"])],
            "mis": [(d["a"], d["a_null"], None), (d["a_mis"], None, None)],
            "mis_first": [(d["a_mis"], None, None), (d["a"], d["a_null"], None)]}[other]
    host = [(h["a"], h["a_null"], None)] * 2
    for cmp_ in fm.CMPS:
        for c in (7, fm.I64_MIN):
            prog = [fm.cc(cmp_, fm.T_INT64, slot, c)]
            exp = _model(world, f"slot{slot}_{cmp_}_{c}", prog, n, "two_columns", host)
            _filter(ctx, world, "scan_cmp1" if other == "direct" else "onerow", prog, cols, n, exp, (other, cmp_, c))


@pytest.mark.parametrize("n", [1, 129, 4097, 16385, 32769])
@pytest.mark.parametrize("kind", ["cmp1", "terms"])
@pytest.mark.parametrize("aligned", [False, True], ids=["misaligned", "aligned"])
def test_filter_project_one_pass_needs_aligned_projected_columns(ctx, world, aligned, kind, n):
    """a projected column 8 bytes off a 16-byte boundary: the bitmap kernel and the tail that copies cell by cell; the same cells at an
    aligned address: the one-pass kernel, which reads projected columns two rows per load"""
    d, h = world["d"], world["host"]
    pd = [(d["a"], d["a_null"]), (d["a_copy" if aligned else "a_mis"], d["a_null"]), (d["b"], d["b_null"]), (d["a_copy" if aligned else "a_mis"], None)]
    ph = [(h["a"], h["a_null"]), (h["a"], h["a_null"]), (h["b"], h["b_null"]), (h["a"], None)]
    form = ("scan_" + kind) if aligned else kind
    progs = [(nm, p) for nm, p in BY_KIND[kind] if kind == "terms" or nm.endswith("_7") or nm.endswith("_max")]
    assert len(progs) >= 12
    for name, prog in progs:
        _project(ctx, world, form, prog, _bind_dev(world), n, _model(world, name, prog, n), pd, ph, (name, aligned))
