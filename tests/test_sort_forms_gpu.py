"""Every kernel form of mdb_dev_sort.hip - ORDER BY, ORDER BY ... LIMIT k, and the sorted fallbacks of SELECT DISTINCT and of GROUP BY over
several columns - against tests/sort_model.py, exactly (np.array_equal on permutations, positions and counts), with the form asserted
after every call from the launch counts by profiler name (MDB_LAUNCH in mdb_dev_sort.hip, mdb_dev_partition.hip, mdb_dev_core.hip).

mdb_dev_sort_perm
    tiny        n <= 2048, <= 4 keys                               orderby_tiny = 1, no other orderby_*
    packed      n >= 2^18, <= 4 keys, word <= 64 bits, no overflow orderby_range = 1, orderby_pack = 1, orderby_leaf = 1, no other orderby_*
    resampled   MDB_SORT_RANGE_SAMPLE=2, a row outside the sample  orderby_range_sample = 1, orderby_range = 1, orderby_pack = 2, orderby_leaf = 1
    redo        the packed path ran and reported SORT_ST_REDO      packed's launches and the general path's
    general     everything else                                    orderby_load = keys, orderby_hist = orderby_scatter = expected_passes,
                                                                   orderby_nullflag = keys whose stream holds a NULL, no orderby_pack / _leaf;
                                                                   orderby_range = 1 where only the word's width kept the call off the packed
                                                                   path; per pass one scan_small, or scan_reduce + scan_spine + scan_apply
                                                                   where its histogram (ceil(n / 4096) * 2^w words) is longer than 16384
    +norow      a row-id vector holds MDB_NO_ROW                   no_row_lookup = distinct vectors, gather64 = keys read through one that does;
                                                                   then one of the forms above
mdb_dev_topk_perm: (topk_sample launches, *out_candidates)
    no_sample (0, n)   sampled_fell_back (1, n)   one_level (1, < n)   two_levels (2, < 16384)
mdb_dev_distinct_sel / mdb_dev_group_count_multi, the sorted fallbacks (no groupby_pack; distinct_heads / groupby_heads = 1)
    vkey            MDB_GROUP_MULTI_PACKED=0 and the packed sort succeeds: k_*_heads_vkey over the sort's composite values
    tiny_cells, general_cells, redo_cells   k_*_heads comparing cells behind the sort form named (more than 63 bits in all, five keys,
                                            the knob off below 2^18 rows, the knob off and the packed sort redone)

Three forms that are not what one would guess, read off the code (the code's condition is the contract):
  - the exactly-full-leaf shape of 64 values x 4096 CONSECUTIVE rows is "redo": its leaves fit (`fast_base + total_d <= a.cap` holds AT the
    capacity) but the first level puts a digit's four one-value tiles into one sub-region of 3584 words.  The same leaves filled from rows
    in random order are "packed", and a 4097th row makes either "redo".
  - a column whose NULL flag never varies (a bitmap without a NULL, an all-NULL first key) is "redo" from ~175 000 rows on: the constant
    top bit leaves half the first-level digits empty and the others overflow their 5/4-average sub-regions.
  - under DESC the sample orders NULLs LAST: a NULL threshold needs all but `rank` sampled rows NULL, not rank + 1 of them.

The shapes, their premises and the forms they declare are built and checked without a GPU by tests/test_cpu_sort_model.py."""
import collections
import time

import numpy as np
import pytest

from midoridb_amd import dev as D
from tests import sort_model as sm

pytestmark = pytest.mark.gpu

RAN = collections.Counter()       # (operator, form) -> cases that ran and asserted their form


@pytest.fixture
def ctx():
    """a device context of this test's own, profiling on: the launch counts are this test's and nothing else's"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this environment")
    c = D.DeviceCtx(0)
    c.prof_enable(True)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nsort forms, cases per operator and form:")
    for (op, form), cnt in sorted(RAN.items()):
        print(f"    {op:9s} {form:18s} {cnt}")


# ------------------------------------------------------------------------------------------------ helpers

def _upload(ctx, keys):
    """the keys on the device; an array bound to several keys (a row-id vector above all) is uploaded once: the same address in each"""
    seen = {}

    def put(a, f):
        if a is None:
            return None
        if id(a) not in seen:
            seen[id(a)] = f(a)
        return seen[id(a)]
    return [(put(v, ctx.to_dev), put(z, ctx.nullbits_dev), put(rid, ctx.to_dev), D.T_DOUBLE if is_double else D.T_INT64, desc)
            for v, z, rid, is_double, desc in keys]


def _launches(ctx):
    return {name: cnt for name, (cnt, _ms) in ctx.prof_read().items() if cnt}


def _np(t):
    return t.cpu().numpy()


def _check_no_row(c, keys, n, label):
    vectors = {id(k[2]) for k in keys if k[2] is not None}
    assert c.get("no_row_lookup", 0) == len(vectors), (label, c)
    assert c.get("gather64", 0) == sum(1 for k in keys if sm.has_no_row(k, n)), (label, c)


def _check_sort_launches(c, form, keys, n, label, own=True):
    """c = launches by name of one call whose sort has to be of `form` (own: the call is the sort alone - the orderby_range and scan
    launches are all its own)"""
    ranges = own
    ob = {k: v for k, v in c.items() if k.startswith("orderby_") and (ranges or not k.startswith("orderby_range"))}
    packed = {"orderby_range": 1, "orderby_pack": 1, "orderby_leaf": 1}
    if form == "tiny":
        want = {"orderby_tiny": 1}
    elif form == "packed":
        want = dict(packed)
    elif form == "resampled":
        want = {"orderby_range_sample": 1, "orderby_range": 1, "orderby_pack": 2, "orderby_leaf": 1}
    else:
        assert form in ("general", "redo")
        passes, nullflags = sm.expected_passes(keys, n), sm.null_passes(keys, n)
        want = {"orderby_load": len(keys)}
        if passes:
            want["orderby_hist"] = want["orderby_scatter"] = passes
        if nullflags:
            want["orderby_nullflag"] = nullflags
        if form == "redo":
            want.update(packed)
        elif n >= sm.SORT_PACK_MIN_ROWS and len(keys) <= sm.SORT_PACK_MAX_KEYS:
            want["orderby_range"] = 1       # measured, found too wide for the word
        if form == "general" and own:       # (the packed path's partition scans as well)
            small, big = sm.expected_scans(keys, n)
            got = tuple(c.get(k, 0) for k in ("scan_small", "scan_reduce", "scan_spine", "scan_apply"))
            assert got == (small, big, big, big), (label, "scans", got, (small, big))
    if not ranges:
        want = {k: v for k, v in want.items() if not k.startswith("orderby_range")}
    assert ob == want, (label, form, ob, want)


def _run_case(ctx, case, monkeypatch, keys=None, kd=None):
    """one case: the call, the result against the model, the form from the launches"""
    keys = case.make() if keys is None else keys
    n, label = case.n, (case.op, case.name, case.n)
    if case.opts.get("premise"):
        case.opts["premise"](keys, n)
    kd = _upload(ctx, keys) if kd is None else kd
    with monkeypatch.context() as m:
        for k, v in case.opts.get("env", {}).items():
            m.setenv(k, v)
        ctx.prof_reset()
        if case.op == "sort":
            got = _np(ctx.sort_perm(kd, n)).view(np.uint32)
        elif case.op == "topk":
            got, cand = ctx.topk_perm(kd, n, case.opts["k"])
            got = _np(got).view(np.uint32)
        elif case.op == "distinct":
            got = _np(ctx.distinct_sel(kd, n)).view(np.uint32)
        else:
            first, count = ctx.group_count_multi(kd, n)
            got = (_np(first).view(np.uint32).astype(np.int64), _np(count))
        c = _launches(ctx)
    _check_no_row(c, keys, n, label)
    form = case.form
    if case.op == "sort":
        want = sm.sort_perm(keys, n)
        assert got.shape == want.shape and np.array_equal(got, want), (label, "result")
        _check_sort_launches(c, form.split("+")[0], keys, n, label)
        assert form.endswith("+norow") == any(sm.has_no_row(k, n) for k in keys)
    elif case.op == "topk":
        k = case.opts["k"]
        want = sm.topk(keys, n, k)
        assert got.shape == want.shape and np.array_equal(got, want), (label, "result", cand)
        launches, model_cand = sm.topk_form(keys, n, k)
        model = sm.topk_form_name(launches, model_cand, n)
        form = form or model            # (read through MDB_NO_ROW: the model's word alone)
        assert form == model, (label, form, model)
        assert (c.get("topk_sample", 0), cand) == (launches, model_cand), (label, form, c.get("topk_sample", 0), cand, launches, model_cand)
        assert {"no_sample": launches == 0 and cand == n, "sampled_fell_back": launches == 1 and cand == n, "one_level": launches == 1 and cand < n,
                "two_levels": launches == 2 and cand < 8 * sm.TOPK_SAMPLE}[form], (label, form, launches, cand)
    else:
        first, count = sm.group_count_multi(keys, n)
        if case.op == "distinct":
            assert got.shape == first.shape and np.array_equal(got, first.astype(np.uint32)), (label, "result")
        else:
            assert got[0].shape == first.shape and np.array_equal(got[0], first) and np.array_equal(got[1], count), (label, "result")
        heads = "distinct_heads" if case.op == "distinct" else "groupby_heads"
        assert c.get(heads, 0) == 1 and "groupby_pack" not in c, (label, c)
        kernels = {s.split("<")[0] for s in ctx.prof_symbols(heads)}
        kernel = ("k_distinct_heads" if case.op == "distinct" else "k_group_heads") + ("_vkey" if form == "vkey" else "")
        assert kernels == {kernel}, (label, kernels, kernel)
        sort_form = {"vkey": "packed", "tiny_cells": "tiny", "general_cells": "general", "redo_cells": "redo"}[form]
        # (group_multi_packed, finding the columns too wide in front of the sort, measures ranges of its own; the compaction of the head
        # flags behind it scans as well)
        _check_sort_launches(c, sort_form, keys, n, label, own=False)
    RAN[(case.op, form)] += 1


# ------------------------------------------------------------------------------------------------ mdb_dev_sort_perm

@pytest.mark.parametrize("n", sm.GENERAL_ROWS)
def test_sort_general_path_digit_widths_nulls_and_scan_forms(ctx, monkeypatch, n):
    """images that differ in exactly 0, 1, 7, 8, 9, 16, 17 and 64 bits, at zero, below it and at INT64_MIN; one radix pass per 8 of them and
    one per key that holds a NULL: a pass too few is a wrong result, a pass too many a silent slowdown, and both fail here.  262 143 rows put
    an 8-bit pass's histogram at 16384 words (one workgroup scans it), 262 145 at 16640 (reduce / spine / apply, a partial last chunk)"""
    for case in sm.general_cases(n):
        _run_case(ctx, case, monkeypatch)


@pytest.mark.parametrize("n", sm.TINY_ROWS)
def test_sort_tiny_path_and_its_boundaries(ctx, monkeypatch, n):
    for case in sm.tiny_cases(n):
        _run_case(ctx, case, monkeypatch)


@pytest.mark.parametrize("n", sm.PACKED_ROWS)
def test_sort_packed_path_word_width_leaf_and_bucket_edges(ctx, monkeypatch, n):
    for case in sm.packed_cases(n):
        _run_case(ctx, case, monkeypatch)


def test_no_row_at_scale_two_keys_gathered_the_third_not(ctx, monkeypatch):
    for case in sm.norow_cases():
        if case.op == "sort":
            _run_case(ctx, case, monkeypatch)


# ------------------------------------------------------------------------------------------------ mdb_dev_topk_perm

@pytest.mark.parametrize("variant", ["direct", "rid", "norow"])
def test_topk_every_gate_of_the_threshold_on_built_inputs(ctx, monkeypatch, variant):
    cases = [c for c in sm.topk_cases() if c.name.endswith("_" + variant)]
    assert len(cases) == len(sm.topk_built())
    for case in cases:
        _run_case(ctx, case, monkeypatch)


def test_topk_two_threshold_levels(ctx, monkeypatch):
    """2^24 rows (why no fewer: tests/sort_model.py, TWO_LEVEL_N): two topk_sample launches and fewer than 16384 candidates"""
    t0 = time.time()
    cases = sm.two_level_cases()
    keys = cases[0].make()
    kd = _upload(ctx, keys)
    for case in cases:
        _run_case(ctx, case, monkeypatch, keys=keys, kd=kd)
    print(f"\ntop-k over {sm.TWO_LEVEL_N} rows, two threshold levels, k = 1 and 10: {time.time() - t0:.1f} s with the model")


# ------------------------------------------------------------------------------------------------ DISTINCT / GROUP BY: the sorted fallbacks

def _heads_cases():
    return [c for n in sm.HEADS_ROWS for c in sm.heads_cases(n)] + [c for c in sm.norow_cases() if c.op != "sort"]


@pytest.mark.parametrize("case", _heads_cases(), ids=lambda c: f"{c.op}-{c.name}-{c.n}")
def test_sorted_fallbacks_name_the_heads_kernel_that_ran(ctx, monkeypatch, case):
    """(a context per case: a context's kernel list per profiler name only grows)"""
    _run_case(ctx, case, monkeypatch)
