"""the fused join + GROUP BY plan on a composite key: its two entry points are exported by the built library, declared in the public
headers and bound in Python (no GPU needed)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "midoridb_amd", "libmidoridb_amd.so")


def test_library_exports_both():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "mdb_dev_join_key_unpack" in syms
    assert "mdb_database_composite_fused" in syms


def test_headers_declare_both():
    dev = open(os.path.join(ROOT, "include", "mdb_dev.h")).read()
    qry = open(os.path.join(ROOT, "include", "mdb_query.h")).read()
    assert re.search(r"\bint\s+mdb_dev_join_key_unpack\s*\(\s*mdb_dev_ctx\s*\*", dev)
    assert re.search(r"\bunsigned long long\s+mdb_database_composite_fused\s*\(\s*struct database\s*\*", qry)


def test_python_bindings():
    from midoridb_amd.dev import DeviceCtx
    from midoridb_amd.query import DB
    assert callable(getattr(DB, "composite_fused"))
    assert callable(getattr(DeviceCtx, "join_key_unpack"))
