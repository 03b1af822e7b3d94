#!/usr/bin/env python3
"""Composite join keys: the measurements behind the table there.  One mode per call, one JSON document per mode.

    python profiles/micro/composite_join/measure.py pack [--rows 100000000] --out pack.json
        mdb_dev_join_key_pack over 2 and 4 columns without a row-id vector, alternating with a torch device-to-device copy whose
        read + written bytes equal the kernel's (the project's yardstick), four turns each, the first dropped
    python profiles/micro/composite_join/measure.py statement --shape a|b [--rows 10000000] --out a.json
        SELECT ta, tb FROM A JOIN B ON xa = xb AND ya = yb with MDB_COMPOSITE_JOIN unset / =0, three alternations, results kept on the
        device; a statement that the library refuses (the first key's pairs do not fit) is recorded with its error text
          a: x has 1000 values, (x, y) is unique       b: x is nearly unique (1 % of the rows repeat a neighbour's value), y = x mod 5
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def pack_rows(n):
    from midoridb_amd.dev import DeviceCtx, join_key_layout
    dev = DeviceCtx(0)
    res = {"rows": n}
    ranges = [(0, 999), (-5000, 4999), (10**12, 10**12 + 7), (0, 65535)]
    cols = [dev.gen_keys(n, 0, n, 11 + c, hi - lo + 1) + lo for c, (lo, hi) in enumerate(ranges)]
    key = torch.empty(n, dtype=torch.int64, device=dev.device)
    bits = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev.device)
    for nc in (2, 4):
        lay = join_key_layout(ranges[:nc], ranges[:nc])
        assert lay["ntaken"] == nc
        moved = 8 * nc * n + 8 * n + 8 * ((n + 63) // 64)			# read + written
        src = torch.empty(moved // 16, dtype=torch.int64, device=dev.device)	# a copy reads and writes its size: half of `moved` each way
        dst = torch.empty_like(src)
        args = [(c, None, None) for c in cols[:nc]]
        pack_ms, copy_ms = [], []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src)
            torch.cuda.synchronize()
            copy_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            _, _, nulls = dev.join_key_pack(lay, args, n, out_key=key, out_nullbits=bits)
            pack_ms.append((time.perf_counter() - t0) * 1e3)
            assert nulls == 0
        dev.prof_enable(True)
        kern = []
        for _ in range(3):
            dev.prof_reset()
            dev.join_key_pack(lay, args, n, out_key=key, out_nullbits=bits)
            kern.append(dev.prof_read()["join_key_pack"][1])
        dev.prof_enable(False)
        res[f"{nc}_columns"] = {"bytes_read_plus_written": moved, "call_ms_all": pack_ms[1:], "copy_ms_all": copy_ms[1:], "kernel_ms_all": kern,
                                "kernel_ms": min(kern), "copy_ms": min(copy_ms[1:]), "kernel_times_the_copy": min(kern) / min(copy_ms[1:]),
                                "kernel_tb_per_s": moved / min(kern) / 1e9,
                                "note": "call_ms: the whole call with its read-back of the count; kernel_ms: HIP events around the launch; "
                                        "copy_ms: torch copy of bytes_read_plus_written / 2 bytes (reads them, writes them), wall clock"}
        del src, dst
    dev.close()
    return res


def statement_rows(shape, n):
    from midoridb_amd.query import DB, QueryError
    rng = np.random.default_rng(17)
    if shape == "a":
        i = np.arange(n, dtype=np.int64)
        xa, ya = i % 1000, i // 1000
        p = rng.permutation(n)
        xb, yb = xa[p], ya[p]
    else:
        xa = rng.permutation(n).astype(np.int64)
        rep = rng.random(n) < 0.01
        rep[0] = False
        xa[rep] = xa[np.flatnonzero(rep) - 1]		# 1 % of the rows repeat the value of the row in front of them
        xb = xa[rng.permutation(n)]
        ya, yb = xa % 5, xb % 5
    res = {"shape": shape, "rows_per_table": n, "on": [], "off": []}
    with DB() as db:
        db.execute("CREATE TABLE A (xa INT, ya INT, ta INT);")
        db.execute("CREATE TABLE B (xb INT, yb INT, tb INT);")
        db.append_columns("A", [xa, ya, np.arange(n, dtype=np.int64)])
        db.append_columns("B", [xb, yb, np.arange(n, dtype=np.int64)])
        db.results_on_device(True)
        sql = "SELECT ta, tb FROM A JOIN B ON xa = xb AND ya = yb;"
        for turn in range(4):				# (the first turn warms both ways up and is dropped)
            for knob in ("on", "off"):
                if knob == "off":
                    os.environ["MDB_COMPOSITE_JOIN"] = "0"
                else:
                    os.environ.pop("MDB_COMPOSITE_JOIN", None)
                c0 = db.composite_joins()
                try:
                    r = db.query_device(sql, copy=False)
                    out = {"call_ms": db.last_call_ms, "rows": r[3], "composite_joins": db.composite_joins() - c0}
                except QueryError as e:
                    out = {"error": str(e)[:300]}
                if turn:
                    res[knob].append(out)
                print(turn, knob, out, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["pack", "statement"])
    ap.add_argument("--shape", choices=["a", "b"], default="a")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res = pack_rows(args.rows or 100_000_000) if args.mode == "pack" else statement_rows(args.shape, args.rows or 10_000_000)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
