"""Worker for tests/test_subquery_gpu.py::test_sharded_mode_refuses_subqueries: two ranks on one GPU (the host-memory test transport of
tests/_dist_gpu_worker.py).  Every rank must get the refusal of IN / NOT IN (SELECT ...) from the statement alone - before anything is
exchanged, so no rank is left waiting in a collective - for SELECT, DELETE and UPDATE, and COUNT(*) goes on working afterwards."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests._dist_gpu_worker import gloo_transport  # noqa: E402

MESSAGE = "sharded mode: IN (SELECT ...) is not executed (subqueries run on one GPU)"


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
        db.execute("CREATE TABLE B (bk INT, bv INT);")
        db.append_columns("A", [np.arange(100, dtype=np.int64) % 7, np.arange(100, dtype=np.int64) + 100 * rank])
        db.append_columns("B", [np.arange(50, dtype=np.int64) % 5, np.arange(50, dtype=np.int64)])
        sets = db.subquery_sets()
        for sql in ("SELECT k FROM A WHERE k IN (SELECT bk FROM B);",
                    "SELECT k FROM A WHERE v > 3 AND k NOT IN (SELECT bk FROM B WHERE bv > 10);",
                    "SELECT k, COUNT(*) FROM A GROUP BY k HAVING k IN (SELECT bk FROM B);",
                    "DELETE FROM A WHERE k IN (SELECT bk FROM B);",
                    "UPDATE A SET v = 1 WHERE k NOT IN (SELECT bk FROM B);"):
            try:
                (db.query if sql.startswith("SELECT") else db.execute)(sql)
                raise AssertionError(f"{sql} was executed in sharded mode")
            except QueryError as ex:
                assert MESSAGE in str(ex), str(ex)
        assert db.subquery_sets() == sets
        res = db.query("SELECT COUNT(*) FROM A;")
        assert int(res.columns[0][0]) == 100 * world
    dist.barrier()
    if rank == 0:
        print("sharded subqueries refused ok", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
