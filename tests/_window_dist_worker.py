"""Worker for tests/test_window_gpu.py::test_sharded_mode_refuses_window_functions: two ranks on one GPU (the host-memory test
transport of tests/_dist_gpu_worker.py).  Every rank must get the refusal of fn(...) OVER (...) from the statement alone - before
anything is exchanged, so no rank is left waiting in a collective - and COUNT(*) goes on working afterwards."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests._dist_gpu_worker import gloo_transport  # noqa: E402


def main():
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from midoridb_amd.query import DB, QueryError
    from midoridb_amd.dist import DatabaseDevice
    with DB() as db:
        dx = gloo_transport(DatabaseDevice(db, 0), world, rank)
        dx.attach_to_database(db)
        db.execute("CREATE TABLE A (k INT, v INT);")
        db.append_columns("A", [np.arange(100, dtype=np.int64) % 7, np.arange(100, dtype=np.int64) + 100 * rank])
        for fn, name in (("ROW_NUMBER()", "ROW_NUMBER"), ("RANK()", "RANK"), ("DENSE_RANK()", "DENSE_RANK"), ("COUNT(*)", "COUNT"), ("SUM(v)", "SUM"),
                         ("MIN(v)", "MIN"), ("MAX(v)", "MAX"), ("AVG(v)", "AVG")):
            for sql in (f"SELECT {fn} OVER () FROM A;", f"SELECT k, {fn} OVER (PARTITION BY k ORDER BY v) AS x FROM A HAVING x > 1 ORDER BY k;"):
                try:
                    db.query(sql)
                    raise AssertionError(f"{sql} was executed in sharded mode")
                except QueryError as ex:
                    assert "sharded mode" in str(ex) and f"{name} ... OVER is not executed" in str(ex), str(ex)
        res = db.query("SELECT COUNT(*) FROM A;")
        assert int(res.columns[0][0]) == 100 * world
    dist.barrier()
    if rank == 0:
        print("sharded window functions refused ok", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
