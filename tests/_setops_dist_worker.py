"""Worker for tests/test_setops_gpu.py::test_sharded_mode_refuses_set_operations: two ranks on one GPU (the host-memory test
transport of tests/_dist_gpu_worker.py).  Every rank must get the refusal of UNION [ALL] / INTERSECT / EXCEPT from the statement alone -
before anything is exchanged, so no rank is left waiting in a collective - and COUNT(*) goes on working afterwards."""
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
        db.execute("CREATE TABLE B (j INT, w INT);")
        db.append_columns("A", [np.arange(100, dtype=np.int64) % 7, np.arange(100, dtype=np.int64) + 100 * rank])
        db.append_columns("B", [np.arange(50, dtype=np.int64) % 5, np.arange(50, dtype=np.int64)])
        for op in ("UNION", "UNION ALL", "INTERSECT", "EXCEPT"):
            for sql in (f"SELECT k FROM A {op} SELECT j FROM B;", f"SELECT k, v FROM A {op} SELECT j, w FROM B ORDER BY k LIMIT 3;"):
                try:
                    db.query(sql)
                    raise AssertionError(f"{sql} was executed in sharded mode")
                except QueryError as ex:
                    assert "sharded mode" in str(ex) and "set operations run on one GPU" in str(ex), str(ex)
        res = db.query("SELECT COUNT(*) FROM A;")
        assert int(res.columns[0][0]) == 100 * world
    dist.barrier()
    if rank == 0:
        print("sharded set operations refused ok", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
