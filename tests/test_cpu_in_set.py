"""Host half of IN / NOT IN lists of any length (no GPU needed): the set builder mdb_set.c against Python sets - the table the
MDB_P_IN_SET kernels probe, with the same hash and probe sequence (mdb_set_image_contains) -, the front end on a 10^5-value
list, and the builder as a stand-alone program under AddressSanitizer + UBSan (nothing sanitized is loaded into Python)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
T_INT64, T_DOUBLE = 0, 1


def _lib():
    from midoridb_amd import dev as D
    from midoridb_amd.lib import load_library
    lib = load_library()
    D._bind(lib)
    return lib, D


class _Set:
    def __init__(self, values, typ=T_INT64):
        self.lib, D = _lib()
        a = np.ascontiguousarray(values, dtype=np.float64 if typ == T_DOUBLE else np.int64).view(np.int64)
        self.img = D.SetImage()
        rc = self.lib.mdb_set_build(ctypes.c_void_p(a.ctypes.data) if a.size else None, a.size, typ, ctypes.byref(self.img))
        assert rc == 0, rc
        self.n = a.size

    def has(self, v):
        if isinstance(v, float):
            v = int(np.float64(v).view(np.int64))
        return bool(self.lib.mdb_set_image_contains(ctypes.byref(self.img), int(v)))

    def words(self):
        return np.ctypeslib.as_array(self.img.words, shape=(2 + self.img.slots,)).copy()

    def check_shape(self, distinct):
        img = self.img
        assert img.members == distinct
        assert img.slots == 1 << img.log2_slots and img.slots >= 16
        assert 2 * img.members <= img.slots, "load above 1/2"
        assert img.longest_run < img.slots, "no empty slot ends a probe"
        w = self.words()
        assert int(w[0]) == img.empty and int(w[1]) == img.slots
        assert int((w[2:] != np.uint64(img.empty)).sum()) == distinct      # the marker is no member, every member sits in one slot

    def close(self):
        self.lib.mdb_set_image_free(ctypes.byref(self.img))


@pytest.mark.parametrize("n", [9, 1000, 1 << 20])
def test_random_lists_against_python_sets(n):
    rng = np.random.default_rng(n)
    vals = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
    vals[: n // 3] = vals[n // 3: 2 * (n // 3)]          # duplicates
    s = _Set(vals)
    members = set(vals.tolist())
    s.check_shape(len(members))
    probes = rng.choice(vals, 2000).tolist() + rng.integers(I64_MIN, I64_MAX, 2000, dtype=np.int64).tolist()
    probes += (vals[:500] + 1).tolist() + (vals[:500] ^ (1 << 62)).tolist()
    for v in probes:
        assert s.has(v) == (v in members), v
    if n >= 1000:       # the longest probe is far from the table: random keys at load <= 1/2 cluster logarithmically
        assert s.img.longest_run < 64 * max(1, int(np.log2(n)))
    s.close()


def test_extreme_values_as_members_and_as_non_members():
    ext = [I64_MIN, I64_MAX, 0, -1]
    s = _Set(ext + list(range(100, 109)))
    s.check_shape(13)
    for v in ext:
        assert s.has(v)
    assert not s.has(1) and not s.has(I64_MIN + 1) and not s.has(I64_MAX - 1) and not s.has(-2)
    s.close()
    s = _Set(list(range(100, 120)))
    s.check_shape(20)
    for v in ext:
        assert not s.has(v)
    s.close()
    # the marker the builder would try first is itself a member: another one is chosen, the member stays a member
    s = _Set([I64_MIN] + list(range(1, 30)))
    assert s.img.empty != (1 << 63) and s.has(I64_MIN)
    s.check_shape(30)
    # a probe for the marker's own bit pattern is a miss
    e = s.img.empty
    assert not s.has(e - (1 << 64) if e >= (1 << 63) else e)
    s.close()


@pytest.mark.parametrize("kind", ["high_bits", "consecutive"])
def test_adversarial_keys_spread(kind):
    """4096 multiples of 2^40 (the low 40 bits all zero) and 4096 consecutive values: a hash that looks at one end of the word
    piles either of them up"""
    vals = np.arange(4096, dtype=np.int64) * ((1 << 40) if kind == "high_bits" else 1) + (0 if kind == "high_bits" else 10**9)
    s = _Set(vals)
    s.check_shape(4096)
    assert s.img.slots == 8192
    assert s.img.longest_run <= 64, s.img.longest_run
    members = set(vals.tolist())
    for v in vals[::7].tolist() + (vals[::7] + (1 << 39)).tolist() + (vals[::5] + 4096).tolist():
        assert s.has(v) == (v in members)
    s.close()


def test_double_sets_compare_like_ieee_equality():
    s = _Set([-0.0, 1.5, float("inf"), float("nan"), 2.5, 3.5, 4.5, 5.5, 6.5, 7.5], T_DOUBLE)
    s.check_shape(9)             # the NaN is dropped, -0.0 is stored as +0.0
    assert s.has(0.0) and s.has(-0.0) and s.has(float("inf")) and s.has(1.5)
    assert not s.has(float("-inf")) and not s.has(float("nan")) and not s.has(1.25)
    s.close()
    s = _Set([0.0, -0.0, float("-inf")] + [float(i) for i in range(1, 9)], T_DOUBLE)
    s.check_shape(10)
    assert s.has(-0.0) and s.has(float("-inf")) and not s.has(float("inf"))
    s.close()


def test_empty_list_and_refusals():
    s = _Set([])
    s.check_shape(0)
    assert s.img.longest_run == 0
    for v in (0, -1, I64_MIN, I64_MAX, 12345):
        assert not s.has(v)
    s.close()
    lib, D = _lib()
    img = D.SetImage()
    one = np.zeros(1, dtype=np.int64)
    assert lib.mdb_set_build(ctypes.c_void_p(one.ctypes.data), 1, 7, ctypes.byref(img)) != 0                  # unknown type
    assert lib.mdb_set_build(ctypes.c_void_p(one.ctypes.data), (1 << 26) + 1, 0, ctypes.byref(img)) != 0      # beyond MDB_SET_MAX_VALUES
    assert not img.words
    assert lib.mdb_dev_in_set_lds_values() == 2048


def test_the_table_is_sized_by_the_distinct_values():
    """a list that repeats its values (or holds NaNs) gets the table of its distinct values: what mdb_dev_in_set_lds_values() promises
    does not depend on how the list was pasted together"""
    base = np.arange(2048, dtype=np.int64) * 5 - 17
    for vals, members, slots in ((np.concatenate([base, base[:512]]), 2048, 4096), (np.tile(base, 3), 2048, 4096),
                                 (np.concatenate([base, [99991], base]), 2049, 8192), (np.tile(base[:9], 100), 9, 64),
                                 (np.zeros(5000, dtype=np.int64), 1, 16)):
        s = _Set(vals)
        s.check_shape(members)
        assert s.img.slots == slots, (len(vals), s.img.slots)
        for x in vals[::13].tolist():
            assert s.has(x)
        assert not s.has(4) and not s.has(-18)        # (members are 3 modulo 5, or 0)
        s.close()
    s = _Set([float("nan")] * 3000 + [1.5, -0.0, 0.0], T_DOUBLE)
    s.check_shape(2)
    assert s.img.slots == 16 and s.has(0.0) and s.has(1.5) and not s.has(float("nan"))
    s.close()


def test_small_tables_are_built_at_a_quarter_load():
    for n, slots in ((9, 64), (1000, 4096), (1024, 4096), (1025, 4096), (2048, 4096), (2049, 8192)):
        s = _Set(np.arange(n, dtype=np.int64) * 3)
        assert s.img.slots == slots, (n, s.img.slots)
        s.close()


def test_front_end_takes_a_list_of_100000_values():
    lib, _ = _lib()
    lib.mdb_sql_to_rpn.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.mdb_sql_to_rpn.restype = ctypes.c_int
    sql = "SELECT k FROM T WHERE k NOT IN (" + ",".join(str(i * 7 - 350000) for i in range(100000)) + ");"
    buf, err = ctypes.create_string_buffer(4 << 20), ctypes.create_string_buffer(1024)
    assert lib.mdb_sql_to_rpn(sql.encode(), buf, len(buf), err, len(err)) == 0, err.value
    toks = buf.value.decode().strip().split("\n")
    assert toks[:3] == ["NAME k", "TABLE T", "NAME k"] and toks[3] == "NUMBER -350000" and toks[100002] == "NUMBER 349993"
    assert toks[-4:] == ["ISNOTIN 100000", "WHERE", "SELECT 0 3", "STMT"]
    assert lib.mdb_sql_to_rpn(sql.replace("NOT IN", "IN").encode(), buf, len(buf), err, len(err)) == 0, err.value
    toks = buf.value.decode().strip().split("\n")
    assert len(toks) == 100007 and toks[-4:] == ["ISIN 100000", "WHERE", "SELECT 0 3", "STMT"]
    # ... and the executor's half of the front end (RPN reader, plan builder, name resolution, type checks) walks the whole list on any
    # machine, before a device is asked for: a type error in the LAST of the 10^5 values is found and named.  (The statement itself
    # runs in tests/test_in_set_gpu.py.)
    from midoridb_amd.query import DB, QueryError
    with DB() as db:
        db.execute("CREATE TABLE T (k INT, s VARCHAR(8));")
        for stmt in (sql, sql.replace("SELECT k FROM T", "DELETE FROM T")):
            with pytest.raises(QueryError) as ei:
                db.execute(stmt.replace("349993)", "'x')"))
            assert "requires an VARCHAR() column" in str(ei.value), str(ei.value)


_SAN_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mdb_dev.h"

static uint64_t rng_state = 0x1234567ull;
static uint64_t rnd(void)
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

static int cmp64(const void *a, const void *b)
{
	const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
	return x < y ? -1 : x > y;
}

int main(void)
{
	static const uint64_t sizes[] = { 0, 1, 9, 15, 16, 17, 1000, 2048, 2049, 65536, 300001 };
	for (size_t si = 0; si < sizeof(sizes) / sizeof(sizes[0]); si++) {
		for (int type = 0; type < 2; type++) {
			const uint64_t n = sizes[si];
			int64_t *v = malloc((n ? n : 1) * 8), *sorted = malloc((n ? n : 1) * 8);
			struct mdb_set_image img;
			for (uint64_t i = 0; i < n; i++) {
				/* narrow and wide values, duplicates; as doubles: small integers, so that no NaN arises */
				uint64_t r = rnd();
				if (type == 1) {
					double d = (double)(int64_t)(r % (4 * n + 1)) - (double)n;
					memcpy(&v[i], &d, 8);
				} else {
					v[i] = (i & 3) == 0 ? (int64_t)(r % (2 * n + 1)) : (int64_t)r;
				}
			}
			if (mdb_set_build(v, n, type, &img))
				return 2;
			if (2 * img.members > img.slots || img.longest_run >= img.slots || img.words[0] != img.empty || img.words[1] != img.slots)
				return 3;
			memcpy(sorted, v, n * 8);
			qsort(sorted, n, 8, cmp64);
			for (uint64_t i = 0; i < n; i += (n > 5000 ? 7 : 1))
				if (!mdb_set_image_contains(&img, v[i]))
					return 4;
			for (int t = 0; t < 20000; t++) {
				int64_t q = (t & 1) ? (int64_t)rnd() : (int64_t)(rnd() % (4 * n + 1));
				if (type == 1) {
					double d = (double)(int64_t)(rnd() % (6 * n + 1)) - 2.0 * (double)n + ((t & 2) ? 0.5 : 0.0);
					memcpy(&q, &d, 8);
				}
				int want = n && bsearch(&q, sorted, n, 8, cmp64) != NULL;
				if (type == 1 && q == (int64_t)0x8000000000000000ull) {	/* -0.0 is +0.0 */
					int64_t z = 0;
					want = n && bsearch(&z, sorted, n, 8, cmp64) != NULL;
				}
				if (mdb_set_image_contains(&img, q) != want)
					return 5;
			}
			mdb_set_image_free(&img);
			mdb_set_image_free(&img);	/* (idempotent) */
			free(v);
			free(sorted);
		}
	}
	puts("set builder ok");
	return 0;
}
"""


def test_builder_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """mdb_set.c + a main of this test's own, compiled with -fsanitize=address,undefined and run as a program: random lists of
    both types, members and non-members probed against a sorted copy"""
    if not shutil.which("gcc"):
        pytest.skip("needs gcc")
    src = tmp_path / "set_main.c"
    src.write_text(_SAN_MAIN)
    exe = tmp_path / "set_main"
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan",      # the runtimes inside the program: it needs nothing preloaded
                        "-I" + os.path.join(ROOT, "include"), str(src), os.path.join(ROOT, "midoridb_amd", "csrc", "mdb_set.c"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "set builder ok" in r.stdout, (r.returncode, r.stdout[-3000:])
