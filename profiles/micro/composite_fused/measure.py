#!/usr/bin/env python3
"""The fused join + GROUP BY plan on a composite key: the measurements behind the table there.  One mode per call, one JSON
document per mode.

    python profiles/micro/composite_fused/measure.py unpack [--rows 10000000] --out unpack.json
        mdb_dev_join_key_unpack of `rows` packed group keys into 2 and 4 columns, alternating with a torch device-to-device copy whose
        read + written bytes equal the kernel's (the project's yardstick), six turns each, the first dropped
    python profiles/micro/composite_fused/measure.py statement [--rows 10000000] --out statement.json
        SELECT xa, ya, COUNT(*) FROM A JOIN B ON xa = xb AND ya = yb GROUP BY xa, ya over rows x rows rows, x with 1000 values, y with
        10 000, with MDB_COMPOSITE_FUSED unset / =0, six alternations after a warm-up turn, results kept on the device: medians, and the
        knob-off spread
    python profiles/micro/composite_fused/measure.py bench --parent-tree DIR [--turns 3] [--first parent|this] --out bench.json
        bench.py --gpus 1 as a child process, in DIR (a built checkout of the parent commit) against this tree, alternating: no code on
        that path changes, so the two must agree within the parent's own spread (--first: which of the two runs first in every turn -
        the second run of a pair starts on a device the first has just used)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)


def unpack_rows(n):
    import torch
    from midoridb_amd.dev import DeviceCtx, join_key_layout
    dev = DeviceCtx(0)
    res = {"groups": n}
    ranges = [(0, 999), (-5000, 4999), (10**12, 10**12 + 7), (0, 65535)]
    for nc in (2, 4):
        lay = join_key_layout(ranges[:nc], ranges[:nc])
        assert lay["ntaken"] == nc
        cols = [dev.gen_keys(n, 0, n, 11 + c, hi - lo + 1) + lo for c, (lo, hi) in enumerate(ranges[:nc])]
        keys, _, nulls = dev.join_key_pack(lay, [(c, None, None) for c in cols], n)
        assert nulls == 0
        outs = [torch.empty(n, dtype=torch.int64, device=dev.device) for _ in range(nc)]
        moved = 8 * n + 8 * nc * n						# read + written
        src = torch.empty(moved // 16, dtype=torch.int64, device=dev.device)	# a copy reads and writes its size: half of `moved` each way
        dst = torch.empty_like(src)
        call_ms, copy_ms = [], []
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src)
            torch.cuda.synchronize()
            copy_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            dev.join_key_unpack(lay, keys, n, out_cols=outs)
            call_ms.append((time.perf_counter() - t0) * 1e3)
        for c in range(nc):
            assert torch.equal(outs[c], cols[c])
        dev.prof_enable(True)
        kern = []
        for _ in range(3):
            dev.prof_reset()
            dev.join_key_unpack(lay, keys, n, out_cols=outs)
            kern.append(dev.prof_read()["join_key_unpack"][1])
        dev.prof_enable(False)
        res[f"{nc}_columns"] = {"bytes_read_plus_written": moved, "call_ms_all": call_ms[1:], "copy_ms_all": copy_ms[1:], "kernel_ms_all": kern,
                                "call_ms": statistics.median(call_ms[1:]), "copy_ms": statistics.median(copy_ms[1:]), "kernel_ms": min(kern),
                                "call_times_the_copy": statistics.median(call_ms[1:]) / statistics.median(copy_ms[1:]),
                                "kernel_times_the_copy": min(kern) / min(copy_ms[1:]), "kernel_tb_per_s": moved / min(kern) / 1e9,
                                "note": "call_ms: the whole synchronising call, wall clock; kernel_ms: HIP events around the launch; "
                                        "copy_ms: torch copy of bytes_read_plus_written / 2 bytes (reads them, writes them), wall clock"}
        del src, dst, outs, cols, keys
    dev.close()
    return res


def statement_rows(n):
    import numpy as np
    from midoridb_amd.query import DB
    rng = np.random.default_rng(17)
    res = {"rows_per_table": n, "x_values": 1000, "y_values": 10_000, "on": [], "off": []}
    with DB() as db:
        db.execute("CREATE TABLE A (xa INT, ya INT, ta INT);")
        db.execute("CREATE TABLE B (xb INT, yb INT, tb INT);")
        for t in "AB":
            db.append_columns(t, [rng.integers(0, 1000, n, dtype=np.int64), rng.integers(0, 10_000, n, dtype=np.int64), np.arange(n, dtype=np.int64)])
        db.results_on_device(True)
        sql = "SELECT xa, ya, COUNT(*) FROM A JOIN B ON xa = xb AND ya = yb GROUP BY xa, ya;"
        for turn in range(7):				# (the first turn warms both ways up and is dropped)
            for knob in ("on", "off"):
                if knob == "off":
                    os.environ["MDB_COMPOSITE_FUSED"] = "0"
                else:
                    os.environ.pop("MDB_COMPOSITE_FUSED", None)
                f0, j0 = db.composite_fused(), db.composite_joins()
                r = db.query_device(sql, copy=False)
                out = {"call_ms": db.last_call_ms, "groups": r[3], "joined_rows": r[4], "composite_fused": db.composite_fused() - f0,
                       "composite_joins": db.composite_joins() - j0}
                assert out["composite_fused"] == (1 if knob == "on" else 0), out
                if turn:
                    res[knob].append(out)
                print(turn, knob, out, flush=True)
        os.environ.pop("MDB_COMPOSITE_FUSED", None)
    on, off = [o["call_ms"] for o in res["on"]], [o["call_ms"] for o in res["off"]]
    assert {o["groups"] for o in res["on"]} == {o["groups"] for o in res["off"]} and {o["joined_rows"] for o in res["on"]} == {o["joined_rows"] for o in res["off"]}
    res["summary"] = {"on_median_ms": statistics.median(on), "off_median_ms": statistics.median(off), "off_min_ms": min(off), "off_max_ms": max(off),
                      "on_min_ms": min(on), "on_max_ms": max(on), "off_over_on": statistics.median(off) / statistics.median(on)}
    return res


def bench_alternating(parent_tree, turns, first):
    parent_tree = os.path.abspath(parent_tree)
    if not os.path.exists(os.path.join(parent_tree, "midoridb_amd", "libmidoridb_amd.so")):
        raise SystemExit(f"{parent_tree}: no built checkout")
    res = {"cmd": "bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline", "first_of_every_turn": first, "parent": [], "this": []}
    for turn in range(turns):
        for which in (("parent", "this") if first == "parent" else ("this", "parent")):
            tree = parent_tree if which == "parent" else ROOT
            env = {k: v for k, v in os.environ.items() if k not in ("MDB_LIBRARY", "PYTHONPATH")}
            p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"],
                               cwd=tree, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
            if p.returncode != 0:		# (a run that failed: nothing more is started)
                raise SystemExit(f"bench.py ({which}) ended with {p.returncode}:\n{p.stderr[-2000:]}")
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            out = {"value": line["value"], "ms_per_step": line.get("ms_per_step")}
            res[which].append(out)
            print(turn, which, out, flush=True)
    pv, tv = [o["value"] for o in res["parent"]], [o["value"] for o in res["this"]]
    res["summary"] = {"parent_median": statistics.median(pv), "parent_min": min(pv), "parent_max": max(pv), "this_median": statistics.median(tv),
                      "this_min": min(tv), "this_max": max(tv), "this_over_parent": statistics.median(tv) / statistics.median(pv)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["unpack", "statement", "bench"])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--first", choices=["parent", "this"], default="parent")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.mode == "unpack":
        res = unpack_rows(args.rows)
    elif args.mode == "statement":
        res = statement_rows(args.rows)
    else:
        res = bench_alternating(args.parent_tree, args.turns, args.first)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
