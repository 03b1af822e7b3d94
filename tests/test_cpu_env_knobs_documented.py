"""Every environment knob the library reads is named in INTEGRATION.md or in a public header: a knob that exists only in the
source is a behaviour a maintainer cannot find."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_knob_read_by_value_is_documented():
    """the knobs read through mdb_knob_set / _off / _int / _str (mdb_knob.c) and the settings read through getenv"""
    knobs = set()
    for f in glob.glob(os.path.join(ROOT, "midoridb_amd", "csrc", "*")):
        if f.endswith((".hip", ".c", ".h")):
            knobs |= set(re.findall(r'(?:getenv|mdb_knob\w*)\(\s*"(M[A-Z0-9_]+)"', open(f).read()))
    assert len(knobs) > 20
    docs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        docs += open(h).read()
    missing = sorted(k for k in knobs if k not in docs)
    assert not missing, missing


def test_the_environment_is_read_in_one_place():
    """mdb_knob.c is the library's one reader of its MDB_* knobs - kept per process, dropped by mdb_dev_reload_knobs(); the
    device layer calls getenv nowhere, the host C only for the MIDORIDB_* database settings"""
    n = 0
    for f in glob.glob(os.path.join(ROOT, "midoridb_amd", "csrc", "*.hip")):
        n += len(re.findall(r'\bgetenv\(', open(f).read()))
    assert n == 0, n
    reader = os.path.join(ROOT, "midoridb_amd", "csrc", "mdb_knob.c")
    assert re.search(r'\bgetenv\(\s*name\s*\)', open(reader).read())
    for f in glob.glob(os.path.join(ROOT, "midoridb_amd", "csrc", "*.[ch]")):
        if f != reader:
            args = re.findall(r'\bgetenv\(\s*([^)]*)\)', open(f).read())
            assert all(a.startswith('"MIDORIDB_') for a in args), (os.path.basename(f), args)

