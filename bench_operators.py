#!/usr/bin/env python3
"""bench_operators.py - per-operator measurements of the OTHER rows of the hot path, beside the
headline pipeline that bench.py times: scan+filter (config 1 scaled up), materialising join with payload
(config 2), single-table GROUP BY, three-way join.  Not part of the driver's bench contract; writes one
JSON document (default profiles/r02/operators.json) with milliseconds and the rate on each operator's
algorithmic bytes, all measured with HIP events through the library's per-kernel profiler.

    python bench_operators.py [--out profiles/r02/operators.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from midoridb_amd import dev as D  # noqa: E402
from midoridb_amd.dev import DeviceCtx  # noqa: E402


def timed(dev, fn, reps=5, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / reps * 1e3
    dev.prof_enable(True)
    dev.prof_reset()
    fn()
    prof = dev.prof_read()
    dev.prof_enable(False)
    return ms, {k: round(v[1], 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])[:8]}, out


def outer_join_rows(dev, res):
    """outer_complete_1e8 (mdb_dev_outer_complete beside the device-to-device copy of the bytes it must move, the project's
    yardstick, alternating in one run) and left_join_pairs_1e8 (the LEFT JOIN statement against the same statement with JOIN)"""
    n = 100_000_000
    i = torch.arange(n, dtype=torch.int32, device=dev.device)
    pp = i[(i & 3) != 3].contiguous()       # 0.75 * 10^8 pairs over as many distinct positions; every fourth position has no pair
    del i
    po = torch.arange(pp.numel(), dtype=torch.int32, device=dev.device)
    J, U = pp.numel(), n // 4
    src = torch.empty((8 * J + 8 * (J + U)) // 8, dtype=torch.int64, device=dev.device)
    dst = torch.empty_like(src)
    copy_ms, oc_ms = [], []
    kern = {}
    for rep in range(4):                    # (the first turn warms both up and is dropped)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        copy_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        op, oo = dev.outer_complete(pp, po, n)
        torch.cuda.synchronize()
        oc_ms.append((time.perf_counter() - t0) * 1e3)
        assert op.numel() == J + U
        del op, oo
    dev.prof_enable(True)
    dev.prof_reset()
    dev.outer_complete(pp, po, n)
    kern = {k: round(v[1], 4) for k, v in sorted(dev.prof_read().items(), key=lambda kv: -kv[1][1])[:8]}
    dev.prof_enable(False)
    ms, cms = min(oc_ms[1:]), min(copy_ms[1:])
    res["outer_complete_1e8"] = {"n_p": n, "pairs": J, "unmatched": U, "ms": ms, "ms_all": oc_ms[1:], "copy_ms": cms, "copy_ms_all": copy_ms[1:],
                                 "times_the_copy": ms / cms, "algorithmic_bytes": 8 * J + 8 * (J + U), "kernels_ms": kern,
                                 "note": "copy_ms: torch device-to-device copy that reads 8 J + 8 (J + U) bytes and writes as many, same run"}
    del pp, po, src, dst
    torch.cuda.empty_cache()
    from midoridb_amd.query import DB
    with DB() as db:
        db.execute("CREATE TABLE A (id_a INT);")
        db.execute("CREATE TABLE B (id_b INT);")
        db.generate("A", n, 42)
        db.generate("B", n, 43, [3 * n // 4])   # B's keys lie in [0, 0.75 n): a quarter of A has no partner
        db.results_on_device(True)
        t = {"JOIN": [], "LEFT JOIN": []}
        rows = {}
        for rep in range(3):
            for kind in t:
                r = db.query_device(f"SELECT A.id_a, B.id_b FROM A {kind} B ON A.id_a = B.id_b;", copy=False)
                t[kind].append(db.last_call_ms)
                rows[kind] = r[3]
        inner, left = min(t["JOIN"][1:]), min(t["LEFT JOIN"][1:])
        res["left_join_pairs_1e8"] = {"rows_per_table": n, "inner_rows": rows["JOIN"], "left_rows": rows["LEFT JOIN"], "inner_call_ms": inner,
                                      "left_call_ms": left, "difference_ms": left - inner, "inner_call_ms_all": t["JOIN"][1:],
                                      "left_call_ms_all": t["LEFT JOIN"][1:],
                                      "note": "query_execute() with results kept on the device; the statements alternate"}


def full_join_rows(dev, res):
    """outer_complete_full_1e7: mdb_dev_outer_complete_full beside mdb_dev_outer_complete over the same 10^7 pairs, alternating in one
    run - 10^7 positions on either side, the preserved positions ascending with repeats and gaps, the partner positions in no order
    (what a hash join delivers); about 0.37 of either side occurs in no pair"""
    n = 10_000_000
    g = torch.Generator(device=dev.device)
    g.manual_seed(6)
    pp = torch.sort(torch.randint(0, n, (n,), dtype=torch.int32, device=dev.device, generator=g)).values.contiguous()
    po = torch.randint(0, n, (n,), dtype=torch.int32, device=dev.device, generator=g)
    left_ms, full_ms = [], []
    for rep in range(6):                    # (the first turn warms both up and is dropped)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        op, oo = dev.outer_complete(pp, po, n)
        torch.cuda.synchronize()
        left_ms.append((time.perf_counter() - t0) * 1e3)
        rows_left = op.numel()
        del op, oo
        t0 = time.perf_counter()
        op, oo, uo = dev.outer_complete_full(pp, po, n, n)
        torch.cuda.synchronize()
        full_ms.append((time.perf_counter() - t0) * 1e3)
        assert op.numel() == rows_left + uo
        del op, oo
    kern = {}
    for name, fn in (("left", lambda: dev.outer_complete(pp, po, n)), ("full", lambda: dev.outer_complete_full(pp, po, n, n))):
        dev.prof_enable(True)
        dev.prof_reset()
        fn()
        kern[name] = {k: round(v[1], 4) for k, v in sorted(dev.prof_read().items(), key=lambda kv: -kv[1][1])}
        dev.prof_enable(False)
    res["outer_complete_full_1e7"] = {"n_p": n, "n_o": n, "pairs": n, "unmatched_p": rows_left - n, "unmatched_o": uo, "left_ms": min(left_ms[1:]),
                                      "full_ms": min(full_ms[1:]), "full_over_left": min(full_ms[1:]) / min(left_ms[1:]), "left_ms_all": left_ms[1:],
                                      "full_ms_all": full_ms[1:], "kernels_ms": kern,
                                      "note": "wall time per call, both synchronise twice; kernels_ms: one further call each with per-launch events"}


def in_set_rows(dev, res):
    """in_set_1e8: WHERE k IN (list) over 10^8 INT64 rows through mdb_dev_filter (bitmap, scan, positions) at about 1 % and about 50 %
    selectivity - a 1000-value list (MDB_P_IN_SET, table in LDS) and a 10^6-value list (table in global memory) beside the two forms that
    ran before lists compiled to a lookup: an 8-value list (k_pred_bits_terms) and one comparison.  The column is a permutation modulo
    (list length / selectivity), the list a random choice of that domain.  pred_ms = the predicate kernel alone (HIP events)."""
    n = 100_000_000
    rng = np.random.default_rng(5)
    out = {"rows": n, "lds_values": dev.in_set_lds_values(), "cases": {}}
    for sel in (0.01, 0.5):
        for name, k in (("one_compare", 0), ("terms_8", 8), ("set_1000", 1000), ("set_1000000", 1_000_000)):
            domain = n if k == 0 else int(round(k / sel))
            v = dev.gen_keys(n, 0, n, 7, 0 if domain == n else domain)
            keep = None
            if k == 0:
                prog = [(D.P_CMP_COL_CONST, D.CMP_LT, D.T_INT64, 0, 0, int(sel * n))]
            elif k <= 8:
                prog = []
                for i in range(k):
                    prog.append((D.P_CMP_COL_CONST, D.CMP_EQ, D.T_INT64, 0, 0, i))
                    if i:
                        prog.append((D.P_OR, 0, 0, 0, 0, 0))
            else:
                keep = dev.make_set(rng.choice(domain, k, replace=False))
                prog = [keep.insn(0)]
            ms, kern, m = timed(dev, lambda: dev.filter(prog, [(v, None, None)], n).numel())
            pred = {kk: vv for kk, vv in kern.items() if kk in ("filter_in_set", "filter_pred_bits", "scan_project")}
            out["cases"][f"{name}@{sel}"] = {"list_values": k, "domain": domain, "rows_out": m, "selectivity": m / n, "ms": ms,
                                             "pred_ms": sum(pred.values()), "kernels_ms": kern,
                                             "column_GBs_pred": 8 * n / (sum(pred.values()) * 1e-3) / 1e9 if pred else None}
            if keep is not None:
                keep.close()
            del v
            torch.cuda.empty_cache()
        c = out["cases"]
        out[f"lds_over_terms8@{sel}"] = {"pred_ms": c[f"set_1000@{sel}"]["pred_ms"] / c[f"terms_8@{sel}"]["pred_ms"],
                                         "ms": c[f"set_1000@{sel}"]["ms"] / c[f"terms_8@{sel}"]["ms"], "target": 1.25}
    res["in_set_1e8"] = out


def aggregate_rows(dev, res, n=100_000_000):
    """aggregate_1e8: GROUP BY k, SUM(v) over 10^8 rows at 4, 1000 and 10^5 groups with INT64 v (groups in LDS up to
    mdb_dev_group_aggregate_lds_groups(1), sorted segments beyond) and DOUBLE v (sorted segments: a floating-point sum is never
    order-free), and SUM(v) without GROUP BY.  Per case: group_count_ms = the same shape's GROUP BY k, COUNT(*) (mdb_dev_group_count,
    which the aggregate operator needs first and which this operator does not change), aggregate_ms = mdb_dev_group_aggregate alone,
    wall time per call with its synchronisation; copy_ms = a device-to-device copy of one 8-byte column of the same rows in the same
    run - 16 bytes moved per row, what one key and one value per row are at the box's copy rate."""
    out = {"rows": n, "lds_groups_1_aggregate": dev.group_aggregate_lds_groups(1), "cases": {}}
    src = torch.empty(n, dtype=torch.int64, device=dev.device).zero_()
    dst = torch.empty_like(src)
    copy_ms = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    del src, dst
    out["copy_ms"] = min(copy_ms[1:])
    out["copy_ms_all"] = copy_ms[1:]
    out["copy_GBs"] = 16 * n / (out["copy_ms"] * 1e-3) / 1e9
    v = dev.gen_payload(n, 0, 11, 0)
    d = dev.gen_payload(n, 0, 12, 1)
    for groups in (4, 1000, 100_000):
        keys = dev.gen_keys(n, 0, n, 43, groups)
        gms, gkern, (first, cnt) = timed(dev, lambda: dev.group_count(keys, None), reps=3, warmup=1)
        dkeys = [(keys, None, None, D.T_INT64, False)]
        for name, col, ty in (("int64", v, D.T_INT64), ("double", d, D.T_DOUBLE)):
            ams, akern, got = timed(dev, lambda: dev.group_aggregate(dkeys, n, first, [(D.AGG_SUM, ty, col, None, None)]), reps=3, warmup=1)
            out["cases"][f"sum_{name}@{groups}"] = {"groups": int(first.numel()), "form": got[2], "group_count_ms": gms, "aggregate_ms": ams,
                                                    "statement_ms": gms + ams, "aggregate_over_copy": ams / out["copy_ms"],
                                                    "group_count_kernels_ms": gkern, "kernels_ms": akern}
        del keys, first, cnt
        torch.cuda.empty_cache()
    for name, col, ty in (("int64", v, D.T_INT64), ("double", d, D.T_DOUBLE)):
        ams, akern, got = timed(dev, lambda: dev.group_aggregate([], n, None, [(D.AGG_SUM, ty, col, None, None)]), reps=3, warmup=1)
        out["cases"][f"sum_{name}@ungrouped"] = {"groups": 1, "form": got[2], "aggregate_ms": ams, "aggregate_over_copy": ams / out["copy_ms"],
                                                  "kernels_ms": akern}
    res["aggregate_1e8"] = out


def count_distinct_rows(dev, res, n=100_000_000):
    """count_distinct_1e8: GROUP BY k, COUNT(DISTINCT v) over 10^8 INT64 rows at 4, 1000 and 10^5 groups, v inside spans of 10^3 and 10^6
    values (a permutation modulo the span, the range promised as the catalog would) and once full-range without a range.  Per case, wall
    time per call with its synchronisation after a warm-up call: count_distinct_ms = mdb_dev_group_count_distinct alone in the form it
    chooses (`form`), sorted_ms = the same call with MDB_COUNT_DISTINCT_BITMAP=0 where the bitmap form ran (what the switch between the
    forms is judged by), group_count_ms = the shape's GROUP BY k, COUNT(*) that delivers first[] beforehand, workaround_ms =
    mdb_dev_group_count_multi over (k, v) - the device part of SELECT DISTINCT k, v, what a user runs today before a recount on the host."""
    out = {"rows": n, "bitmap_bits": dev.count_distinct_bitmap_bits(), "lds_groups": dev.group_count_distinct_lds_groups(), "cases": {}}
    spans = {"1e3": 1000, "1e6": 1_000_000}
    vals = {name: dev.gen_keys(n, 0, n, 44, span) for name, span in spans.items()}
    vals["full"] = torch.mul(dev.gen_payload(n, 0, 11, 0), -7046029254386353131)       # (wraps: every bit of the 64 varies)
    for groups in (4, 1000, 100_000):
        keys = dev.gen_keys(n, 0, n, 43, groups)
        gms, _, (first, cnt) = timed(dev, lambda: dev.group_count(keys, None), reps=3, warmup=1)
        dkeys = [(keys, None, None, D.T_INT64, False)]
        for name, v in vals.items():
            if name == "full" and groups != 1000:
                continue
            rng_ = (0, spans[name] - 1) if name in spans else None
            call = lambda: dev.group_count_distinct(dkeys, n, first, [(D.T_INT64, v, None, None, rng_)])    # noqa: E731
            ms, kern, got = timed(dev, call, reps=3, warmup=1)
            case = {"groups": int(first.numel()), "form": got[1][0], "group_count_ms": gms, "count_distinct_ms": ms, "kernels_ms": kern,
                    "distinct_total": int(got[0][0].sum())}
            if got[1][0] == 1:
                os.environ["MDB_COUNT_DISTINCT_BITMAP"] = "0"
                try:
                    sms, skern, sgot = timed(dev, call, reps=3, warmup=1)
                finally:
                    del os.environ["MDB_COUNT_DISTINCT_BITMAP"]
                assert sgot[1][0] == 2 and torch.equal(sgot[0][0], got[0][0])
                case.update({"sorted_ms": sms, "sorted_kernels_ms": skern})
            wkeys = dkeys + [(v, None, None, D.T_INT64, False)]
            wms, wkern, wgot = timed(dev, lambda: dev.group_count_multi(wkeys, n), reps=3, warmup=1)
            case.update({"workaround_ms": wms, "workaround_rows": int(wgot[0].numel()), "workaround_kernels_ms": wkern})
            assert case["workaround_rows"] == case["distinct_total"]
            out["cases"][f"span_{name}@{groups}"] = case
            del got, wgot
            torch.cuda.empty_cache()
        del keys, first, cnt
        torch.cuda.empty_cache()
    res["count_distinct_1e8"] = out


def window_rows(dev, res, n=100_000_000):
    """window_1e8: ROW_NUMBER() and SUM(v) OVER (PARTITION BY k ORDER BY o) over 10^8 rows at 4, 1000 and 10^6 partitions - both functions
    in ONE mdb_dev_window call, wall time per call with its synchronisation -, and beside it mdb_dev_sort_perm alone on the same two keys:
    the sort is the operator's first step, the difference is what the head bitmaps and the scan passes cost."""
    out = {"rows": n, "cases": {}}
    v = dev.gen_payload(n, 0, 11, 0)
    o = dev.gen_payload(n, 0, 13, 0)
    outs = [torch.empty(n, dtype=torch.int64, device=dev.device) for _ in range(2)]      # (allocated once: the call's own time is measured)
    nulls = [torch.empty((n + 63) // 64, dtype=torch.int64, device=dev.device) for _ in range(2)]
    for parts in (4, 1000, 1_000_000):
        k = dev.gen_keys(n, 0, n, 43, parts)
        part = [(k, None, None, D.T_INT64, False)]
        order = [(o, None, None, D.T_INT64, False)]
        sms, skern, _ = timed(dev, lambda: dev.sort_perm(part + order, n), reps=3, warmup=1)
        wms, wkern, got = timed(dev, lambda: dev.window(part, order, n, [(D.WIN_ROW_NUMBER,), (D.WIN_SUM, D.T_INT64, v, None, None)], outs=outs, nulls=nulls),
                                reps=3, warmup=1)
        out["cases"][f"row_number_sum@{parts}"] = {"partitions": parts, "form": got[2], "window_ms": wms, "sort_perm_ms": sms, "window_over_sort": wms / sms,
                                                   "kernels_ms": wkern, "sort_kernels_ms": skern}
        del k, got
        torch.cuda.empty_cache()
    res["window_1e8"] = out


def setops_rows(dev, res, n_probe=100_000_000, n_build=10_000_000):
    """setops: 10^8 probe rows x 10^7 build rows over one and over two INT64 columns, wall time per call with its synchronisation after
    a warm-up call.  rows_semi_ms = mdb_dev_rows_semi alone (every probe row, no DISTINCT in front); distinct_sel_ms = mdb_dev_distinct_sel
    over the probe side alone, the statement's first step; intersect_ms = the whole
    SELECT ... INTERSECT SELECT ... through query_execute(), the result kept on the device; and, for one column, in_subquery_ms = the
    statement that could be written before there were set operations, SELECT DISTINCT k FROM A WHERE k IN (SELECT k FROM B) - the same rows
    while k holds no NULL.  Column 0: A a permutation of [0, 10^8) modulo 2 * 10^7, B a permutation of [0, 10^7) - half of A's rows are
    members; column 1: modulo 4 on both sides."""
    from midoridb_amd.query import DB
    out = {"probe_rows": n_probe, "build_rows": n_build, "cases": {}}
    with DB() as db:
        db.execute("CREATE TABLE A (k INT, k2 INT);")
        db.execute("CREATE TABLE B (j INT, j2 INT);")
        db.generate("A", n_probe, 42, [2 * n_build, 4])
        db.generate("B", n_build, 52, [0, 4])
        db.results_on_device(True)
        pk = [dev.gen_keys(n_probe, 0, n_probe, 42, 2 * n_build), dev.gen_keys(n_probe, 0, n_probe, 43, 4)]
        bk = [dev.gen_keys(n_build, 0, n_build, 52, 0), dev.gen_keys(n_build, 0, n_build, 53, 4)]
        for ncols, la, lb in ((1, "k", "j"), (2, "k, k2", "j, j2")):
            probe = [(c, None, None, D.T_INT64, False) for c in pk[:ncols]]
            build = [(c, None, None, D.T_INT64, False) for c in bk[:ncols]]
            ms, kern, (sel, info) = timed(dev, lambda: dev.rows_semi(probe, n_probe, build, n_build), reps=2, warmup=1)
            case = {"columns": ncols, "rows_semi_ms": ms, "rows_semi_hits": int(sel.numel()), "members": info["members"], "log2_slots": info["log2_slots"],
                    "form": info["form"], "kernels_ms": kern}
            del sel
            dms, dkern, first = timed(dev, lambda: dev.distinct_sel(probe, n_probe), reps=1, warmup=1)      # (the statement's first step, alone)
            case.update({"distinct_sel_ms": dms, "distinct_rows": int(first.numel()), "distinct_kernels_ms": dkern})
            del first
            sql = f"SELECT {la} FROM A INTERSECT SELECT {lb} FROM B;"
            runs = []
            for _ in range(3):
                got = db.query_device(sql, copy=False)
                runs.append(db.last_call_ms)
            case.update({"intersect_ms": min(runs[1:]), "intersect_ms_all": runs, "intersect_rows": got[3]})
            if ncols == 1:
                sub = "SELECT DISTINCT k FROM A WHERE k IN (SELECT j FROM B);"
                runs = []
                for _ in range(3):
                    got = db.query_device(sub, copy=False)
                    runs.append(db.last_call_ms)
                case.update({"in_subquery_ms": min(runs[1:]), "in_subquery_ms_all": runs, "in_subquery_rows": got[3]})
                assert case["in_subquery_rows"] == case["intersect_rows"]
            out["cases"][f"int64x{ncols}"] = case
            torch.cuda.empty_cache()
    res["setops"] = out


def subquery_rows(dev, res):
    """subquery_set: the right side of k IN (SELECT ...) as a device set - make_set_from_column (mdb_dev_set_from_column: scan, fill,
    insert, and the rebuild where the members need a smaller table) beside the route that existed before it for the same cells: the
    column copied to the host, then make_set (mdb_set_build on one host thread + the upload, mdb_dev_set_create).  Three shapes:
    10^7 distinct values in 10^7 rows; 10^8 rows over 1000 distinct values (ends in the rebuild and an LDS-size image; the host
    builder takes at most 2^26 values, so the host route has to drop the duplicates first - numpy.unique - and its plain form is
    recorded as refused); 10^7 rows through a row-id vector (the host route copies both and indexes there).  The two routes alternate
    in one run; wall time per call, each call synchronises; kernels_ms from the library's profiler (HIP events), in a call of its
    own.  bytes_read = the cells (and row ids) the scan and the insertion read once each, bytes_table = the slots filled."""
    out = {"cases": {}}
    shapes = (("distinct_1e7", 10_000_000, 0, False), ("dup1000_1e8", 100_000_000, 1000, False), ("rid_1e7", 10_000_000, 0, True))
    for name, n, modulus, with_rid in shapes:
        col = dev.gen_keys(n, 0, n, 7, modulus)
        rid = torch.randperm(n, device=dev.device).to(torch.int32) if with_rid else None

        def on_device():
            s = dev.make_set_from_column(col, None, rid)
            info = (int(s.info.members), int(s.info.log2_slots), int(s.info.rebuilt))
            s.close()
            return info

        refused = []

        def through_host():
            vals = col.cpu().numpy()
            if rid is not None:
                vals = vals[rid.cpu().numpy()]
            try:
                s = dev.make_set(vals)
            except D.DeviceError:
                if not refused:
                    refused.append(True)
                s = dev.make_set(np.unique(vals))
            b = s.insn(0)[4]
            s.close()
            return b

        dev_ms, host_ms = [], []
        for turn in range(4):                   # (the first turn warms both up and is dropped)
            for fn, into in ((on_device, dev_ms), (through_host, host_ms)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn()
                torch.cuda.synchronize()
                into.append((time.perf_counter() - t0) * 1e3)
                if fn is on_device:
                    info = got
                else:
                    assert got == info[1], (got, info)      # both routes end in a table of the same size
        dev.prof_enable(True)
        dev.prof_reset()
        on_device()
        prof = dev.prof_read()
        dev.prof_enable(False)
        first_log2 = min(27, max(4, int(np.ceil(np.log2(max(2 * n, 16))))))
        out["cases"][name] = {"rows": n, "members": info[0], "log2_slots": info[1], "rebuilt": info[2],
                              "device_ms": min(dev_ms[1:]), "device_ms_all": dev_ms[1:], "host_route_ms": min(host_ms[1:]),
                              "host_route_ms_all": host_ms[1:], "host_route_needed_unique": bool(refused),
                              "host_over_device": min(host_ms[1:]) / min(dev_ms[1:]),
                              "kernels_ms": {k: round(v[1], 4) for k, v in prof.items() if k.startswith("set_")},
                              "kernel_launches": {k: v[0] for k, v in prof.items() if k.startswith("set_")},
                              "bytes_read": 2 * n * (8 + (4 if with_rid else 0)), "bytes_table": 8 * ((1 << first_log2) + (1 << info[1]) * info[2])}
        del col, rid
        torch.cuda.empty_cache()
    res["subquery_set"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r04", "operators.json"))
    ap.add_argument("--configs1", action="store_true", help="only the two BASELINE configs[0..1] shapes (scan_filter_1e8, join_payload_1e7): "
                                                             "what profiles/collect.sh runs under rocprofv3")
    ap.add_argument("--outer", action="store_true", help="only the outer join's rows (outer_complete_1e8, left_join_pairs_1e8)")
    ap.add_argument("--in-set", action="store_true", help="only the IN-list rows (in_set_1e8: set lookups beside an 8-value term list and one comparison)")
    ap.add_argument("--aggregates", action="store_true", help="only the SUM / MIN / MAX / AVG rows (aggregate_1e8: GROUP BY k, SUM(v) at 4, 1000 and 10^5 "
                                                               "groups with INT64 and DOUBLE v, and SUM(v) without GROUP BY)")
    ap.add_argument("--full-join", action="store_true", help="only the FULL JOIN completion's row (outer_complete_full_1e7: beside the LEFT completion "
                                                              "of the same pairs)")
    ap.add_argument("--subquery", action="store_true", help="only the IN (SELECT ...) set builder's row (subquery_set: make_set_from_column at three "
                                                             "shapes beside the column copied to the host and make_set)")
    ap.add_argument("--count-distinct", action="store_true", help="only the COUNT(DISTINCT col) rows (count_distinct_1e8: GROUP BY k, COUNT(DISTINCT v) at "
                                                                   "4, 1000 and 10^5 groups and value spans of 10^3, 10^6 and 2^64, per form, beside "
                                                                   "mdb_dev_group_count_multi over (k, v))")
    ap.add_argument("--window", action="store_true", help="only the window functions' row (window_1e8: ROW_NUMBER and SUM(v) OVER (PARTITION BY k ORDER BY o) "
                                                           "at 4, 1000 and 10^6 partitions, beside mdb_dev_sort_perm alone on the same keys)")
    ap.add_argument("--setops", action="store_true", help="only the set operations' row (setops: 10^8 probe rows x 10^7 build rows over one and two "
                                                           "INT64 columns - mdb_dev_rows_semi alone, the whole INTERSECT statement, and for one column "
                                                           "SELECT DISTINCT ... WHERE k IN (SELECT ...))")
    args = ap.parse_args()
    dev = DeviceCtx(0)
    res = {}
    # one flag, one group of rows: run it, write the document, print it whole
    only = (("setops", setops_rows), ("window", window_rows), ("count_distinct", count_distinct_rows), ("subquery", subquery_rows),
            ("full_join", full_join_rows), ("aggregates", aggregate_rows), ("in_set", in_set_rows))
    for flag, rows in only:
        if getattr(args, flag):
            rows(dev, res)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
            print(json.dumps(res, indent=1))
            return
    if args.outer:
        outer_join_rows(dev, res)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: {kk: vv for kk, vv in d.items() if kk != "kernels_ms"} for k, d in res.items()}, indent=1))
        return

    # ---- scan + WHERE (config 1 shape at 10^8 rows): SELECT v FROM T WHERE v > N/2 ; v = permutation
    n = 100_000_000
    v = dev.gen_keys(n, 0, n, 7, 0)
    prog = [(D.P_CMP_COL_CONST, D.CMP_GT, D.T_INT64, 0, 0, n // 2)]

    def scan_filter():
        # scan + WHERE + projection in one operator and ONE pass (mdb_dev_filter_project): the kernel that evaluates the
        # predicate writes the survivors at their final positions (decoupled look-back); the output tensor is the
        # library's buffer itself (no copy)
        m, _ = dev.filter_project(prog, [(v, None, None)], n, [(v, None)])
        return m
    ms, kern, m = timed(dev, scan_filter)

    def scan_filter_unfused():
        sel = dev.filter(prog, [(v, None, None)], n)
        out, _ = dev.gather64(v, None, sel, sel.numel())
        return sel.numel()
    ms_unfused, kern_unfused, _ = timed(dev, scan_filter_unfused)
    algo = 8 * n + 8 * m            # read every value once, write the survivors once
    res["scan_filter_1e8"] = {"rows_in": n, "rows_out": m, "ms": ms, "algorithmic_bytes": algo,
                              "algorithmic_GBs": algo / (ms * 1e-3) / 1e9, "kernels_ms": kern,
                              "device_ms": sum(kern.values()), "device_algorithmic_GBs": algo / (sum(kern.values()) * 1e-3) / 1e9,
                              "unfused_ms": ms_unfused, "unfused_kernels_ms": kern_unfused,
                              "note": "mdb_dev_filter_project: one pass, survivors written at their final positions (decoupled look-back over "
                                      "16384-row blocks); 50% selectivity; ms = wall time per call incl. the host synchronisation that returns the "
                                      "row count, device_ms = the operator's kernels; unfused = filter (bitmap, scan, positions) + projection "
                                      "gather, the round-1 path"}

    # ---- materialising join with payload (config 2): 10^7 x 10^7, 1:1 keys, 4 output columns
    n2 = 10_000_000
    a_id, a_f = dev.gen_keys(n2, 0, n2, 42, 0), dev.gen_keys(n2, 0, n2, 43, 0)
    b_id, b_f = dev.gen_keys(n2, 0, n2, 50, 0), dev.gen_keys(n2, 0, n2, 51, 0)

    def join_payload():
        l, r = dev.join_pairs(a_id, None, b_id, None)
        j = l.numel()
        # the projection as the executor plans it (mdb_exec_result.c: locate_column, projection pass 1): B's join key holds A's value in every joined
        # tuple, so both key columns of SELECT * are ONE gather of A's column through the left row ids (ascending: near-sequential
        # reads); the payload columns are gathered through their own row ids; one launch
        # ... and when every left row found exactly one partner (last_plan()["pairs_identity"]: the primary-key join) the left row ids
        # are 0, 1, 2 ...: A's columns are read as they stand
        lid = None if dev.last_pairs_identity() else l
        dev.gather_cols([(a_id, None, lid), (a_f, None, lid), (b_f, None, r)], j)
        return j
    ms_pairs, kern_pairs, j = timed(dev, join_payload, reps=3, warmup=1)
    algo = 8 * 2 * n2 + 8 * 2 * n2 + 8 * 4 * j      # keys + payload columns read once, 4 result columns written

    def join_payload_carried():
        # the executor's plan since round 4 (mdb_exec_join.c: join_with_payload): every left row has its one partner, so B's payload cell
        # travels through B's one partition level and lands at the left row's place - no partner row ids, no compaction, no random
        # gather; A's columns are read as they stand (copied: the result owns its columns), B's key column is A's
        out = dev.join_payload(a_id, None, b_id, None, [b_f])
        if out is None:
            return join_payload()
        dev.gather_cols([(a_id, None, None), (a_f, None, None)], n2)
        return n2
    ms, kern, j = timed(dev, join_payload_carried, reps=3, warmup=1)
    res["join_payload_1e7"] = {"rows_per_table": n2, "joined_rows": j, "ms": ms, "joined_rows_per_s": j / (ms * 1e-3),
                               "algorithmic_bytes": algo, "algorithmic_GBs": algo / (ms * 1e-3) / 1e9, "frac_of_peak": algo / (ms * 1e-3) / 1e9 / 8000.0,
                               "kernels_ms": kern,
                               "note": "mdb_dev_join_payload: the right table's payload cell carried through its one partition level and written at "
                                       "the left row's place (every left row has its one partner: verified on the device) + the copies of A's "
                                       "two columns into the result; B's key column is A's",
                               "pairs_path": {"ms": ms_pairs, "kernels_ms": kern_pairs,
                                              "note": "round 3's plan: mdb_dev_join_pairs (pairs in the reference's (l, r) order) + the projection in "
                                                      "one launch (mdb_dev_gather_cols): 3 gathers for the 4 result columns"}}

    def join_payload4():
        l, r = dev.join_pairs(a_id, None, b_id, None)
        j = l.numel()
        dev.gather_cols([(a_id, None, l), (b_id, None, r), (a_f, None, l), (b_f, None, r)], j)
        return j
    ms, kern, j = timed(dev, join_payload4, reps=3, warmup=1)
    res["join_payload_1e7_four_gathers"] = {"rows_per_table": n2, "joined_rows": j, "ms": ms, "kernels_ms": kern,
                                            "note": "the same with every result column gathered on its own (the round-1 plan)"}
    if args.configs1:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: {kk: vv for kk, vv in d.items() if kk != "kernels_ms"} for k, d in res.items()}, indent=1))
        return

    # ---- the row-order payload join at 10^8 x 10^8 rows (mdb_dev_rowjoin.hip; BASELINE configs[4]'s join-only shape at operator level): one right
    #      table with one and two cells, and B and C in ONE call (mdb_dev_join_payload_multi: the left table's tiles sorted once)
    ka, kb, kc = dev.gen_keys(n, 0, n, 42, 0), dev.gen_keys(n, 0, n, 43, 0), dev.gen_keys(n, 0, n, 44, 0)
    pb, pc = kb * 3 + 1, kc * 5 - 2
    for name, fn, cols in (("join_payload_1e8_one_cell", lambda: dev.join_payload(ka, None, kb, None, [pb])[0].numel(), 1),
                           ("join_payload_1e8_two_cells", lambda: dev.join_payload(ka, None, kb, None, [pb, kb])[0].numel(), 2),
                           ("join_payload_multi_1e8_two_tables", lambda: dev.join_payload_multi(ka, [(kb, [pb]), (kc, [pc])], 0, n - 1)[0][0].numel(), 2)):
        ms, kern, j = timed(dev, fn, reps=3, warmup=1)
        tables = 2 if "multi" in name else 1
        algo = 8 * n + tables * 8 * n + cols * 8 * n + cols * 8 * j         # key columns and payload columns read once, the carried columns written
        res[name] = {"rows_per_table": n, "joined_rows": j, "carried_columns": cols, "ms": ms, "joined_rows_per_s": j / (ms * 1e-3), "algorithmic_bytes": algo,
                     "frac_of_peak": algo / (ms * 1e-3) / 1e9 / 8000.0, "kernels_ms": kern, "payload_tables": dev.last_plan()["payload_tables"],
                     "note": "every left row has its one partner in every right table (verified on the device); the carried columns in the left table's row order"}
    got = dev.join_payload_multi(ka, [(kb, [pb]), (kc, [pc])], 0, n - 1)
    res["join_payload_multi_1e8_two_tables"]["identical_to_f_of_key"] = bool(torch.equal(got[0][0], ka * 3 + 1) and torch.equal(got[1][0], ka * 5 - 2))
    del ka, kb, kc, pb, pc, got
    torch.cuda.empty_cache()

    # ---- single-table GROUP BY key COUNT(*) at 10^8 rows, 6.25M groups of 16
    keys = dev.gen_keys(n, 0, n, 43, n // 16)

    def group_by():
        f, c = dev.group_count(keys, None)
        return f.numel()
    ms, kern, g = timed(dev, group_by)
    algo = 8 * n + 12 * g
    res["group_count_1e8"] = {"rows": n, "groups": g, "ms": ms, "algorithmic_bytes": algo,
                              "algorithmic_GBs": algo / (ms * 1e-3) / 1e9, "kernels_ms": kern}
    gk_out = (torch.empty(n, dtype=torch.int64, device=dev.device), torch.empty(n, dtype=torch.int64, device=dev.device))

    def group_by_keys():
        r = dev.group_count_keys(keys, None, out=gk_out)
        return -1 if r is None else r[0].numel()
    ms, kern, gk = timed(dev, group_by_keys)
    algo = 8 * n + 16 * max(gk, 0)
    res["group_count_keys_any_order_1e8"] = {"rows": n, "groups": gk, "ms": ms, "algorithmic_bytes": algo, "algorithmic_GBs": algo / (ms * 1e-3) / 1e9,
                                            "kernels_ms": kern, "note": "mdb_dev_group_count_keys: (key, COUNT) pairs in unspecified order - no row "
                                                                          "ids, no ordering sort (mdb_database_groups_any_order)"}
    del gk_out

    # ---- three-way join on one key (config 5 shape), 10^7 rows per table, 1:1:1
    c_id = dev.gen_keys(n2, 0, n2, 60, 0)

    def three_way():
        l, r = dev.join_pairs(a_id, None, b_id, None)
        k_ab, _ = dev.gather64(a_id, None, l, l.numel())     # key column of the joined stream
        p, q = dev.join_pairs(k_ab, None, c_id, None)
        ra = dev.gather32(l, p)                               # compose row ids: A, B through the second join
        rb = dev.gather32(r, p)
        return p.numel()
    ms, kern, j3 = timed(dev, three_way, reps=3, warmup=1)
    res["three_way_join_1e7"] = {"rows_per_table": n2, "joined_rows": j3, "ms": ms, "joined_rows_per_s": j3 / (ms * 1e-3),
                                 "kernels_ms": kern}

    # ---- BASELINE config 5 shape on one GPU at full size: (A join B) join C on one key, 10^8 rows per table, then
    #      GROUP BY the key + COUNT(*); row ids composed through both joins (what a payload projection would gather with)
    del a_id, a_f, b_id, b_f, c_id
    torch.cuda.empty_cache()
    big = [dev.gen_keys(n, 0, n, s, 0) for s in (42, 43, 44)]

    def three_way_group():
        l, r = dev.join_pairs(big[0], None, big[1], None)
        k_ab, _ = dev.gather64(big[0], None, l, l.numel())
        p, q = dev.join_pairs(k_ab, None, big[2], None)
        ra, rb = dev.gather32(l, p), dev.gather32(r, p)
        key, _ = dev.gather64(k_ab, None, p, p.numel())
        first, cnt = dev.group_count(key, None)
        return first.numel()
    ms, kern, g3 = timed(dev, three_way_group, reps=2, warmup=1)
    res["three_way_join_group_1e8"] = {"rows_per_table": n, "groups": g3, "ms": ms, "joined_rows_per_s": n / (ms * 1e-3), "kernels_ms": kern,
                                       "note": "BASELINE configs[4] shape on ONE GPU: two materialising joins (unique keys) + GROUP BY + COUNT(*)"}

    def three_way_fused():
        k, c, f, j = dev.join_group_count_multi(big[0], None, [(big[1], None), (big[2], None)])
        return k.numel()
    ms, kern, g3f = timed(dev, three_way_fused, reps=3, warmup=1)
    res["three_way_join_group_fused_1e8"] = {"rows_per_table": n, "groups": g3f, "ms": ms, "joined_rows_per_s": n / (ms * 1e-3), "kernels_ms": kern,
                                             "one_pass": dev.last_join_multi(),
                                             "note": "the same query through mdb_dev_join_group_count_multi: every table partitioned once, the right "
                                                     "tables' counts multiplied in the leaf kernel, the groups ordered once; no joined row exists"}

    def three_way_unordered():
        k, c, j = dev.join_group_count_multi_unordered(big[0], None, [(big[1], None), (big[2], None)])
        return k.numel()
    ms, kern, g3u = timed(dev, three_way_unordered, reps=3, warmup=1)
    res["three_way_join_group_unordered_1e8"] = {"rows_per_table": n, "groups": g3u, "ms": ms, "joined_rows_per_s": n / (ms * 1e-3), "kernels_ms": kern,
                                                 "unordered_form": dev.last_join_unordered(),
                                                 "note": "the same call without MDB_ORDER_FIRST (mdb_database_groups_any_order): no row ids, no ordering sort"}
    del big
    torch.cuda.empty_cache()

    # ---- ORDER BY (extension): stable sort permutation of 10^8 rows on one INT64 key with 27
    #      significant bits (value range + stream position fit one word: range pass, pack pass, two scatter levels, a
    #      per-leaf LDS sort), the same with two key columns, and a top-k over the north-star groups through query_execute()
    k1 = dev.gen_keys(n, 0, n, 77, 0)
    k2 = dev.gen_keys(n, 0, n, 78, 512)

    def order_by():
        return dev.sort_perm([(k1, None, None, D.T_INT64, False)], n).numel()
    ms, kern, _ = timed(dev, order_by, reps=3, warmup=1)
    algo = n * 8 + n * (8 + 8) + 2 * n * (8 + 8) + n * (8 + 4)  # range read; pack read + write; two scatter levels; leaf read + perm out
    res["order_by_1e8"] = {"rows": n, "ms": ms, "rows_per_s": n / (ms * 1e-3), "moved_bytes": algo,
                           "moved_GBs": algo / (ms * 1e-3) / 1e9, "kernels_ms": kern,
                           "note": "mdb_dev_sort_perm, permutation keys < 2^27: packed-word path (the stable 8-bit LSD passes it "
                                   "replaces took 4.6 ms); moved_bytes is what this method moves, not a lower bound"}

    def order_by_limit():
        return dev.topk_perm([(k1, None, None, D.T_INT64, False)], n, 10)[1]
    ms, kern, cand = timed(dev, order_by_limit, reps=3, warmup=1)
    res["order_by_limit10_1e8"] = {"rows": n, "k": 10, "rows_sorted": cand, "ms": ms, "rows_per_s": n / (ms * 1e-3),
                                   "algorithmic_GBs": n * 8 / (ms * 1e-3) / 1e9, "kernels_ms": kern,
                                   "note": "mdb_dev_topk_perm: sample threshold + one filter pass + sort of the candidates, against order_by_1e8's "
                                           "full sort; algorithmic bytes = one read of the key column"}

    def order_by2():
        return dev.sort_perm([(k2, None, None, D.T_INT64, True), (k1, None, None, D.T_INT64, False)], n).numel()
    ms, kern, _ = timed(dev, order_by2, reps=3, warmup=1)
    res["order_by_two_keys_1e8"] = {"rows": n, "ms": ms, "rows_per_s": n / (ms * 1e-3), "kernels_ms": kern,
                                    "note": "ORDER BY k2 DESC, k1 ASC (9 + 27 value bits + 27 position bits = 63 bits: one word)"}
    # GROUP BY a column of 1000 distinct values (the direct LDS-table path) - the other common shape of the operator
    def group_by_small():
        return dev.group_count(k2, None)[0].numel()
    ms, kern, gsmall = timed(dev, group_by_small, reps=5, warmup=2)
    res["group_count_small_range_1e8"] = {"rows": n, "groups": gsmall, "ms": ms, "rows_per_s": n / (ms * 1e-3),
                                          "algorithmic_GBs": n * 8 / (ms * 1e-3) / 1e9, "kernels_ms": kern,
                                          "note": "GROUP BY over 512 distinct values + COUNT(*): one streaming pass, per-workgroup LDS tables "
                                                  "(3.8 ms through the partitioned path's hot-key kernels)"}

    # GROUP BY two columns + COUNT(*) (composite-key semantics; round 6: the columns' composite value as one key column through the
    # single-column operator where the ranges fit 63 bits together - sort, run heads, run lengths before and otherwise)
    k3 = dev.gen_keys(n, 0, n, 79, 300)

    def group_by2():
        return dev.group_count_multi([(k2, None, None, D.T_INT64, False), (k3, None, None, D.T_INT64, False)], n)[0].numel()
    ms, kern, groups2 = timed(dev, group_by2, reps=3, warmup=1)
    res["group_by_two_columns_1e8"] = {"rows": n, "groups": groups2, "ms": ms, "rows_per_s": n / (ms * 1e-3), "kernels_ms": kern,
                                       "note": "GROUP BY k2, k3 (512 x 300 value combinations) + COUNT(*), first-occurrence order"}

    def distinct2():
        return dev.distinct_sel([(k2, None, None, D.T_INT64, False), (k3, None, None, D.T_INT64, False)], n).numel()
    ms, kern, groups2 = timed(dev, distinct2, reps=3, warmup=1)
    res["distinct_two_columns_1e8"] = {"rows": n, "distinct": groups2, "ms": ms, "rows_per_s": n / (ms * 1e-3), "kernels_ms": kern,
                                       "note": "SELECT DISTINCT k2, k3: first rows of the combinations, ascending"}
    del k3
    del k2
    del k1

    # ---- the north-star query end to end through the drop-in C API (query_execute), tables generated on the
    #      device: includes planning, the device pipeline and the D2H copy of the result columns
    from midoridb_amd.query import DB
    del v, keys
    torch.cuda.empty_cache()
    with DB() as db:
        # BASELINE configs[1] through the drop-in API: 10^7 x 10^7 rows, 4 result columns (320 MB of result over PCIe)
        db.execute("CREATE TABLE A2 (id_a2 INT, f1 INT);")
        db.execute("CREATE TABLE B2 (id_b2 INT, f2 INT);")
        db.generate("A2", n2, 42)
        db.generate("B2", n2, 50)
        q2 = "SELECT * FROM A2 INNER JOIN B2 ON A2.id_a2 = B2.id_b2;"
        db.query(q2)
        r2 = db.query(q2)
        res["join_payload_via_query_execute_1e7"] = {"rows_per_table": n2, "joined_rows": r2.nrows, "executor_ms": r2.exec_ms, "call_ms": db.last_call_ms,
                                                     "note": "query_execute(): plan + join + projection + D2H of 4 x 10^7 x 8 B into pinned host columns"}
    with DB() as db:
        db.execute("CREATE TABLE A (id_a INT);")
        db.execute("CREATE TABLE B (id_b INT);")
        db.generate("A", n, 42)
        db.generate("B", n, 43, [n // 16])
        q = "SELECT id_a, COUNT(*) FROM A INNER JOIN B ON A.id_a = B.id_b GROUP BY id_a;"
        db.query(q)
        t0 = time.perf_counter()
        r = db.query(q)
        wall = (time.perf_counter() - t0) * 1e3
        call = db.last_call_ms
        qk = ("SELECT id_a, COUNT(*) FROM A INNER JOIN B ON A.id_a = B.id_b GROUP BY id_a HAVING COUNT(*) > 1 "
              "ORDER BY id_a DESC LIMIT 10;")
        db.query(qk)
        t1 = time.perf_counter()
        rk = db.query(qk)
        res["north_star_top10_via_query_execute_1e8"] = {"rows_per_table": n, "result_rows": rk.nrows, "executor_ms": rk.exec_ms,
                                                         "call_ms": db.last_call_ms, "python_wall_ms": (time.perf_counter() - t1) * 1e3,
                                                         "note": "fused join+group count, HAVING filter, ORDER BY (radix sort of 6.25M groups), LIMIT"}
        # BASELINE configs[4] shape with aggregation: A JOIN B JOIN C on one key + GROUP BY + COUNT(*): the fused operator is
        # chained, none of the 1.6*10^9 joined rows is materialised
        db.execute("CREATE TABLE C (id_c INT);")
        db.generate("C", n, 44, [n // 16])
        q3 = "SELECT id_a, COUNT(*) FROM A INNER JOIN B ON A.id_a = B.id_b INNER JOIN C ON A.id_a = C.id_c GROUP BY id_a;"
        db.query(q3)
        t2 = time.perf_counter()
        r3 = db.query(q3)
        res["three_way_fused_via_query_execute_1e8"] = {
            "rows_per_table": n, "groups": r3.nrows, "joined_rows": r3.joined_rows, "executor_ms": r3.exec_ms,
            "call_ms": db.last_call_ms, "python_wall_ms": (time.perf_counter() - t2) * 1e3,
            "joined_rows_per_s": r3.joined_rows / (r3.exec_ms * 1e-3),
            "note": "chained fused join + group count (B and C hold every key < n/16 sixteen times: COUNT(*) = 256 per group); "
                    "executor_ms includes the D2H of the 6.25 M result rows"}
        res["north_star_via_query_execute_1e8"] = {
            "rows_per_table": n, "groups": r.nrows, "joined_rows": r.joined_rows, "executor_ms": r.exec_ms, "call_ms": call,
            "python_wall_ms": wall, "joined_rows_per_s_call": r.joined_rows / (call * 1e-3),
            "note": "query_execute() on device-resident tables; executor_ms = plan + device pipeline + D2H of the result "
                    "(2 columns x G x 8 B over PCIe); call_ms = wall time of the C call (query_execute) alone; python_wall_ms adds "
                    "the binding's copy of the result columns into numpy arrays (not part of the C API)"}

    torch.cuda.empty_cache()
    outer_join_rows(dev, res)
    torch.cuda.empty_cache()
    aggregate_rows(dev, res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in d.items() if kk != "kernels_ms"} for k, d in res.items()}, indent=1))


if __name__ == "__main__":
    main()
