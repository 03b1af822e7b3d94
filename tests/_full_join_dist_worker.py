"""Worker for tests/test_full_join_gpu.py::test_sharded_mode_refuses_full_joins: two ranks on one GPU (the host-memory test
transport of tests/_dist_gpu_worker.py).  Every rank must get the refusal of a FULL join from the statement alone, in the words
LEFT and RIGHT joins are refused with - before anything is exchanged, so no rank is left waiting in a collective - and inner joins
go on working afterwards."""
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
        db.execute("CREATE TABLE A (id_a INT);")
        db.execute("CREATE TABLE B (id_b INT);")
        db.append_columns("A", [np.arange(100, dtype=np.int64) + 100 * rank])
        db.append_columns("B", [np.arange(0, 200, 2, dtype=np.int64)[50 * rank:50 * rank + 50]])
        for kind in ("FULL JOIN", "FULL OUTER JOIN"):
            try:
                db.query(f"SELECT * FROM A {kind} B ON A.id_a = B.id_b;")
                raise AssertionError(f"{kind} was executed in sharded mode")
            except QueryError as ex:
                assert "sharded mode" in str(ex) and "OUTER JOIN is not executed (outer joins run on one GPU)" in str(ex), str(ex)
        res = db.query("SELECT COUNT(*) FROM A INNER JOIN B ON A.id_a = B.id_b;")
        assert int(res.columns[0][0]) == 100
    dist.barrier()
    if rank == 0:
        print("sharded full join refused ok", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
