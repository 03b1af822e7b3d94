"""The column memo (midoridb_amd/csrc/mdb_dev_memo.h) - what the join / GROUP BY operators remember about key columns - driven without
a device: the header is plain C++17, so a main of this test's own, compiled with the host sanitizers and run as a program, checks the
serve counts of every verdict, the shared counter of the unique-key join's two sides, the range drop and the LRU of column pairs with
made-up addresses.  (The operators' use of it is pinned on the GPU: tests/test_dev_ops_gpu.py::test_remembered_verdicts_expire_on_schedule.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MAIN = r"""
#include <stdio.h>
#include "mdb_dev_memo.h"

#define CHECK(c)                                                      \
	do {                                                          \
		if (!(c)) {                                           \
			printf("line %d: %s\n", __LINE__, #c);        \
			return 1;                                     \
		}                                                     \
	} while (0)

static const void *P(uintptr_t a) { return (const void *)a; }

/* the verdicts as the operators key them: (which, left column?, right column?, right length without a right column?, serves; 0 = no expiry) */
struct row {
	mdb_verdict_id id;
	bool has_l, has_r, bare_nr;
	int serves;
};
static const row ROWS[] = {
	{ VD_NARROW, true, true, false, MDB_HINT_SERVES },	{ VD_SAMPLE, true, true, false, MDB_HINT_SERVES },
	{ VD_DISTINCT, true, false, false, MDB_HINT_SERVES },	{ VD_EXACT, true, false, true, MDB_HINT_SERVES },
	{ VD_JK_DUP, true, true, false, MDB_HINT_SERVES },	{ VD_JP_BAD, true, true, false, MDB_HINT_SERVES },
	{ VD_LW_BAD, true, false, true, MDB_BAD_SERVES },	{ VD_L4_BAD, true, false, true, MDB_BAD_SERVES },
	{ VD_PW_BAD, false, true, false, 0 },			{ VD_REC32, true, true, false, 0 },
	{ VD_LAST_GROUPS, true, true, false, 0 },
};

static int serve_counts(void)
{
	CHECK(MDB_HINT_SERVES == 31 && MDB_BAD_SERVES == 32 && MDB_MEMO_SLOTS == 8);
	for (const row &r : ROWS) {
		mdb_col_memo m;
		mdb_verdict &v = m.vd[r.id];
		const void *kl = r.has_l ? P(0x10000) : NULL, *kr = r.has_r ? P(0x20000) : NULL;
		const uint64_t nl = r.has_l ? 600 : 0, nr = (r.has_r || r.bare_nr) ? 700 : 0;
		CHECK(!v.holds(kl, nl, kr, nr) && !v.serve(kl, nl, kr, nr, 31) && !v.served());
		CHECK(!v.holds(NULL, 0, NULL, 0));	/* (nothing noted is no verdict about no column) */
		v.note(kl, nl, kr, nr);
		CHECK(v.holds(kl, nl, kr, nr) && !v.served());
		if (!r.serves) {	/* no expiry: the operators only peek */
			for (int i = 0; i < 40; i++)
				CHECK(v.holds(kl, nl, kr, nr));
			CHECK(!v.served());
			CHECK(!v.holds(P(0x10008), nl, kr, nr) && !v.holds(kl, nl + 1, kr, nr) && !v.holds(kl, nl, P(0x20008), nr) && !v.holds(kl, nl, kr, nr + 1));
			continue;
		}
		/* a call with any one key part different is not served and counts nothing */
		CHECK(!v.serve(P(0x10008), nl, kr, nr, r.serves) && !v.serve(kl, nl + 1, kr, nr, r.serves));
		CHECK(!v.serve(kl, nl, P(0x20008), nr, r.serves) && !v.serve(kl, nl, kr, nr + 1, r.serves));
		CHECK(!v.served());
		for (int i = 1; i <= 40; i++) {
			CHECK(v.serve(kl, nl, kr, nr, r.serves) == (i <= r.serves));
			if (i <= r.serves)
				CHECK(v.served() && v.holds(kl, nl, kr, nr));
			else
				CHECK(!v.holds(kl, nl, kr, nr));	/* (an expired verdict does not hold for a site that peeks either) */
		}
		v.note(kl, nl, kr, nr);
		CHECK(!v.served() && v.serve(kl, nl, kr, nr, r.serves) && v.served());
		/* a note in the middle starts the count again */
		for (int i = 0; i < 9; i++)
			CHECK(v.serve(kl, nl, kr, nr, r.serves));
		v.note(kl, nl, kr, nr);
		for (int i = 1; i <= r.serves + 1; i++)
			CHECK(v.serve(kl, nl, kr, nr, r.serves) == (i <= r.serves));
		v.note(kl, nl, kr, nr);
		v.clear();
		CHECK(!v.holds(kl, nl, kr, nr) && !v.serve(kl, nl, kr, nr, r.serves));
	}
	return 0;
}

/* the unique-key join's "this side has duplicates": two keys, ONE counter */
static int dup_pair(void)
{
	mdb_col_memo m;
	const void *kl = P(0x10000), *kr = P(0x20000);
	bool l = true, r = true;
	m.dup_sides(kl, 600, kr, 700, &l, &r);
	CHECK(!l && !r && m.pu_dup_skips == 0);		/* (nothing noted: nothing counted) */
	m.dup_side_note(true, kr, 700);
	for (int i = 0; i < 10; i++) {
		m.dup_sides(kl, 600, kr, 700, &l, &r);
		CHECK(!l && r);
	}
	m.dup_sides(P(0x10008), 600, kr, 701, &l, &r);	/* (other columns: neither side, not counted) */
	CHECK(!l && !r && m.pu_dup_skips == 10);
	m.dup_side_note(false, kl, 600);		/* either note zeroes the counter */
	for (int i = 1; i <= 32; i++) {
		m.dup_sides(kl, 600, kr, 700, &l, &r);
		CHECK(l && r);
	}
	m.dup_sides(kl, 600, kr, 700, &l, &r);		/* the 33rd counted call after the later note: both sides go */
	CHECK(!l && !r);
	CHECK(!m.vd[VD_PU_DUP_R].holds(NULL, 0, kr, 700) && !m.vd[VD_PU_DUP_L].holds(kl, 600, NULL, 0));
	m.dup_sides(kl, 600, kr, 700, &l, &r);
	CHECK(!l && !r);
	/* one side alone counts as well, and a call over another right column still counts for the left one */
	m.dup_side_note(false, kl, 600);
	for (int i = 1; i <= 32; i++) {
		m.dup_sides(kl, 600, P(0x30000 + 8 * i), 5, &l, &r);
		CHECK(l && !r);
	}
	m.dup_sides(kl, 600, kr, 700, &l, &r);
	CHECK(!l && !r);
	return 0;
}

/* every verdict noted over columns of its own: verdict i's left column at LEFT(i), its right one at RIGHT(i) */
static uintptr_t LEFT(int i) { return 0x100000 + 0x1000 * (uintptr_t)i; }
static uintptr_t RIGHT(int i) { return 0x900000 + 0x1000 * (uintptr_t)i; }
static void note_all(mdb_col_memo &m)
{
	for (int i = 0; i < VD_COUNT; i++)
		m.vd[i].note(P(LEFT(i)), 100 + i, P(RIGHT(i)), 200 + i);
}
static int only_gone(const mdb_col_memo &m, int gone)	/* 1: exactly verdict `gone` (-1: none) is cleared */
{
	for (int i = 0; i < VD_COUNT; i++)
		if (m.vd[i].holds(P(LEFT(i)), 100 + i, P(RIGHT(i)), 200 + i) == (i == gone))
			return 0;
	return 1;
}

static int range_drop(void)
{
	for (int i = 0; i < VD_COUNT; i++) {
		for (int side = 0; side < 2; side++) {
			const uintptr_t at = side ? RIGHT(i) : LEFT(i);
			/* (start, bytes, hit): the address at a, at b - 1, at b, below a; bytes == 0 covers one byte */
			const struct {
				uintptr_t lo;
				size_t bytes;
				bool hit;
			} drops[] = { { at, 8, true },	    { at - 15, 16, true }, { at - 16, 16, false }, { at + 1, 64, false }, { at - 100, 4000, true },
				      { at, 0, true },	    { at - 1, 0, false },  { at + 1, 0, false },   { at, 1, true } };
			for (const auto &d : drops) {
				mdb_memo_store s;
				note_all(s);
				mdb_memo_drop(&s, P(d.lo), d.bytes);
				CHECK(only_gone(s, d.hit ? i : -1));
			}
		}
		/* a one-column verdict: the absent side is no address (a drop that starts at 0 does not take it) */
		mdb_memo_store s;
		s.vd[i].note(P(LEFT(i)), 5, NULL, 0);
		mdb_memo_drop(&s, P(0), 64);
		CHECK(s.vd[i].holds(P(LEFT(i)), 5, NULL, 0));
		mdb_memo_drop(&s, P(LEFT(i)), 8);
		CHECK(!s.vd[i].holds(P(LEFT(i)), 5, NULL, 0));
	}
	/* what is not a verdict stays: payload and back-off counters */
	mdb_memo_store s;
	note_all(s);
	s.nh_result = 1;
	s.nh_distrust = 3;
	s.keyed_distrust = 4;
	s.dn_distrust = 5;
	mdb_memo_drop(&s, P(0), (size_t)1 << 30);
	for (int i = 0; i < VD_COUNT; i++)
		CHECK(!s.vd[i].holds(P(LEFT(i)), 100 + i, P(RIGHT(i)), 200 + i));
	CHECK(s.nh_distrust == 3 && s.keyed_distrust == 4 && s.dn_distrust == 5);
	return 0;
}

/* pair p: columns at PL(p), PR(p); its set is marked through the sample verdict and its payload */
static const void *PL(int p) { return P(0x1000000 + 0x10000 * (uintptr_t)p); }
static const void *PR(int p) { return P(0x5000000 + 0x10000 * (uintptr_t)p); }
static void mark(mdb_memo_store &s, int p)
{
	s.vd[VD_SAMPLE].note(PL(p), 1000 + p, PR(p), 2000 + p);
	s.sr_lo = p;
	s.nh_result = 1;
	s.gh_distinct = 7u * p;
}
static bool marked(const mdb_memo_store &s, int p)
{
	return s.vd[VD_SAMPLE].holds(PL(p), 1000 + p, PR(p), 2000 + p) && s.sr_lo == p && s.nh_result == 1 && s.gh_distinct == 7u * p;
}
static bool empty(const mdb_memo_store &s)
{
	for (int i = 0; i < VD_COUNT; i++)
		if (s.vd[i].uses >= 0 || s.vd[i].kl || s.vd[i].kr)
			return false;
	return s.nh_result == -1 && s.sr_lo == 0 && s.gh_distinct == 0 && s.nh_distrust == 0 && s.keyed_distrust == 0 && s.dn_distrust == 0 && !s.r32_ok;
}
static void to(mdb_memo_store &s, int p) { mdb_memo_switch(&s, PL(p), 1000 + p, PR(p), 2000 + p); }

static int switching(void)
{
	mdb_memo_store s;
	CHECK(empty(s));
	for (int p = 1; p <= 9; p++) {
		to(s, p);
		CHECK(empty(s));
		mark(s, p);
	}
	/* switching to the live pair changes nothing */
	const size_t aside = s.memo_lru.size();
	to(s, 9);
	CHECK(marked(s, 9) && s.memo_lru.size() == aside);
	/* nine pairs, the live one and MDB_MEMO_SLOTS others: pairs 2 to 9 come back intact, the first pair's set is gone */
	for (int p = 2; p <= 9; p++) {
		to(s, p);
		CHECK(marked(s, p));
	}
	CHECK(s.memo_lru.size() == MDB_MEMO_SLOTS - 1);
	to(s, 1);
	CHECK(empty(s));
	CHECK(s.memo_lru.size() == MDB_MEMO_SLOTS);
	for (int p = 3; p <= 9; p++) {		/* (pair 2 was the least recently used: it went for pair 1) */
		to(s, p);
		CHECK(marked(s, p));
	}
	to(s, 2);
	CHECK(empty(s));
	/* a one-column operator's pair: no right column, its length does not count */
	mdb_memo_switch(&s, PL(20), 77, NULL, 5);
	CHECK(empty(s));
	s.gh_distinct = 99;
	mdb_memo_switch(&s, PL(20), 77, NULL, 6);
	CHECK(s.gh_distinct == 99);
	to(s, 9);
	CHECK(marked(s, 9));
	mdb_memo_switch(&s, PL(20), 77, NULL, 0);
	CHECK(s.gh_distinct == 99);
	return 0;
}

/* a verdict of a put-aside set about a FOREIGN column goes alone; the set's own column takes the whole set along */
static int drops_and_sets(void)
{
	mdb_memo_store s;
	const void *foreign = P(0x7000000);
	for (int p = 4; p <= 7; p++) {
		to(s, p);
		mark(s, p);
	}
	to(s, 4);
	s.vd[VD_PW_BAD].note(NULL, 0, foreign, 55);
	to(s, 5);
	s.vd[VD_PW_BAD].note(NULL, 0, foreign, 55);
	to(s, 6);
	const size_t before = s.memo_lru.size();
	mdb_memo_drop(&s, foreign, 8 * 55);
	CHECK(s.memo_lru.size() == before);
	to(s, 4);
	CHECK(marked(s, 4) && !s.vd[VD_PW_BAD].holds(NULL, 0, foreign, 55));
	to(s, 5);
	CHECK(marked(s, 5) && !s.vd[VD_PW_BAD].holds(NULL, 0, foreign, 55));
	to(s, 6);
	CHECK(marked(s, 6));
	mdb_memo_drop(&s, PR(4), 8);		/* pair 4's right column is released ... */
	CHECK(s.memo_lru.size() == before - 1);
	mdb_memo_drop(&s, PL(5), 0);		/* ... pair 5's left column is written to */
	CHECK(s.memo_lru.size() == before - 2);
	CHECK(marked(s, 6));
	to(s, 4);
	CHECK(empty(s));
	to(s, 5);
	CHECK(empty(s) && s.nh_result == -1);
	to(s, 7);
	CHECK(marked(s, 7));
	/* the live set's own column: its verdicts about that column go, the set stays the live one */
	mdb_memo_drop(&s, PL(7), 8);
	CHECK(!s.vd[VD_SAMPLE].holds(PL(7), 1007, PR(7), 2007) && s.gh_distinct == 49u);
	/* forgetting a guess: the narrow verdict, the sample behind it, and one fresh look */
	s.vd[VD_NARROW].note(PL(7), 1007, PR(7), 2007);
	s.vd[VD_SAMPLE].note(PL(7), 1007, PR(7), 2007);
	s.forget_guess();
	CHECK(s.nh_result == -1 && s.nh_distrust == 1 && !s.vd[VD_NARROW].holds(PL(7), 1007, PR(7), 2007) && !s.vd[VD_SAMPLE].holds(PL(7), 1007, PR(7), 2007));
	return 0;
}

int main(void)
{
	if (serve_counts() || dup_pair() || range_drop() || switching() || drops_and_sets())
		return 1;
	puts("column memo ok");
	return 0;
}
"""


def test_memo_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """mdb_dev_memo.h + a main of this test's own, compiled with -fsanitize=address,undefined and run as a program (nothing preloaded,
    nothing loaded into python): serve counts, the shared counter of the unique-key join's sides, range drops, the LRU of column pairs"""
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    src = tmp_path / "memo_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "memo_main"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan",      # the runtimes inside the program: it needs nothing preloaded
                        "-I" + os.path.join(ROOT, "midoridb_amd", "csrc"), str(src), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "column memo ok" in r.stdout, (r.returncode, r.stdout[-3000:])
