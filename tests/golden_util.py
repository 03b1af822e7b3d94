"""Helpers shared by the golden-fixture tests."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def all_cases(*files):
    out = []
    for fn in files:
        out.extend(load(fn))
    return out


def table_arrays(case, tname):
    """-> (list of 8-byte numpy columns, list of NULL arrays or None) for one fixture table."""
    t = case["tables"][tname]
    types = ddl_types(case)[tname]
    cols = []
    for c, ty in zip(t["cols"], types):
        cols.append(np.array(c, dtype=np.float64 if ty == "DOUBLE" else np.int64))
    nulls = None
    if t["nulls"] is not None:
        nulls = [None if x is None else np.array(x, dtype=np.uint8) for x in t["nulls"]]
    return cols, nulls


def ddl_types(case):
    """{table: [INT|DOUBLE per column]} parsed from the fixture's CREATE statements."""
    out = {}
    for s in case["ddl"]:
        name = s.split()[2]
        body = s[s.index("(") + 1:s.rindex(")")]
        out[name] = [p.split()[1].upper().replace("INTEGER", "INT") for p in body.split(",")]
    return out


def ddl_columns(case):
    out = {}
    for s in case["ddl"]:
        name = s.split()[2]
        body = s[s.index("(") + 1:s.rindex(")")]
        out[name] = [p.split()[0] for p in body.split(",")]
    return out


# ---- DML scripts (tests/golden/dml.json) ---------------------------------------------------------------

def script_schema(sql):
    """CREATE TABLE T (a INT, x DOUBLE) -> ("T", ["a", "x"], ["INT", "DOUBLE"])."""
    name = sql.split()[2]
    body = sql[sql.index("(") + 1:sql.rindex(")")]
    cols = [p.split()[0] for p in body.split(",")]
    types = [p.split()[1].upper().replace("INTEGER", "INT") for p in body.split(",")]
    return name, cols, types


def insert_values(sql, types):
    """INSERT INTO T VALUES (1, NULL, 0.5); -> [1, None, 0.5] (python ints / floats / None)."""
    body = sql[sql.index("(", sql.upper().index("VALUES")) + 1:sql.rindex(")")]
    out = []
    for tok, ty in zip(body.split(","), types):
        tok = tok.strip()
        out.append(None if tok.upper() == "NULL" else (float(tok) if ty == "DOUBLE" else int(tok)))
    return out


def raw_cell(v):
    """python value -> the 8 raw bytes as int64 (what the fixtures store), None stays None."""
    if v is None:
        return None
    if isinstance(v, float):
        return int(np.array([v], dtype=np.float64).view(np.int64)[0])
    return int(v)


# ---- the reference's answers to inputs the tests generate themselves (tests/golden/live_reference.json) ----------------------
# A test that used to need the reference library at run time (oracle/_ref, built only where the reference sources lie) compares
# with the answer recorded here; where oracle/_ref is built it also recomputes that answer live, which must agree.  Record new
# entries with oracle/_ref built (and MDB_REFERENCE_TREE naming the reference's source tree for its header layouts):
#   MDB_RECORD_GOLDEN=1 python -m pytest tests/<file>::<test>

LIVE = "live_reference.json"


def _plain(x):
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return [_plain(v) for v in x.tolist()]
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    return x


def digest(obj):
    """sha256 of a result (names, rows, anything JSON can hold; numpy scalars as Python numbers) in one canonical text form"""
    import hashlib
    return hashlib.sha256(json.dumps(_plain(obj), sort_keys=True).encode()).hexdigest()


def reference_answer(key, live=None):
    """The stored answer under `key` (plain JSON data, often a digest()).  `live`: None where oracle/_ref is not built, else a function
    that computes the same answer through the reference now."""
    path = os.path.join(GOLDEN, LIVE)
    stored = load(LIVE) if os.path.exists(path) else {}
    if live is not None:
        got = live()
        if os.environ.get("MDB_RECORD_GOLDEN") == "1":
            stored[key] = got
            with open(path, "w") as f:
                json.dump(stored, f, indent=1, sort_keys=True)
                f.write("\n")
        assert stored.get(key) == got, f"the live reference disagrees with the stored answer {key!r}"
    assert key in stored, f"no stored reference answer {key!r} in tests/golden/{LIVE}"
    return stored[key]
