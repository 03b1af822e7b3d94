/*
 * mdb_dev_memo.h - what the join / GROUP BY operators remember about key columns.  Host-only, plain C++17, no HIP: a program
 * without a device can drive all of it (tests/test_cpu_memo.py does, under the host sanitizers).
 *
 * Every remembered fact is an mdb_verdict: keyed by the columns' device addresses and lengths, counted as it is used, verified
 * on the device whenever it is applied - a stale one costs a failed attempt, never a result.  mdb_col_memo holds one verdict
 * per fact (with the fact's payload beside it); mdb_memo_store holds the live set of ONE pair of key columns and the sets of
 * the last MDB_MEMO_SLOTS pairs, so queries that alternate over several table pairs do not evict each other's verdicts and pay
 * the key sample + its host sync on every call.
 */
#ifndef MDB_DEV_MEMO_H
#define MDB_DEV_MEMO_H

#include <stdint.h>
#include <string.h>
#include <utility>
#include <vector>

#define MDB_MEMO_SLOTS 8
/* A remembered sample / verdict is served to this many calls after it was noted, then the data is looked at again (one tiny
 * kernel + sync - ~50 us, a tenth of a 10^7-row query - every 32nd call; a buffer refilled with another distribution runs that
 * long on a plan that is exact but may not be the best; a hint the data contradicts is noticed by the kernels at once) */
#define MDB_HINT_SERVES 31
/* ... and a "this fast form overflowed / found duplicates" to this many, then the fast form is tried again: the columns go by
 * address and length, and a caller's allocator hands the same addresses out for other data */
#define MDB_BAD_SERVES 32

/* One remembered fact about up to two columns.  A one-column verdict passes NULL, 0 for the absent side. */
struct mdb_verdict {
	const void *kl = NULL, *kr = NULL;
	uint64_t nl = 0, nr = 0;
	int uses = -1;			/* -1: nothing noted; else the calls answered from memory since the note */

	void note(const void *l, uint64_t n_l, const void *r, uint64_t n_r)
	{
		kl = l;
		nl = n_l;
		kr = r;
		nr = n_r;
		uses = 0;
	}
	/* a look that counts nothing */
	bool holds(const void *l, uint64_t n_l, const void *r, uint64_t n_r) const
	{
		return uses >= 0 && kl == l && nl == n_l && kr == r && nr == n_r;
	}
	/* a look that counts: true for the first max_serves calls after a note, then the verdict is gone until it is noted again */
	bool serve(const void *l, uint64_t n_l, const void *r, uint64_t n_r, int max_serves)
	{
		if (!holds(l, n_l, r, n_r))
			return false;
		if (++uses > max_serves) {
			clear();
			return false;
		}
		return true;
	}
	/* answered from memory at least once since it was noted (false right after a note: the data itself was looked at) */
	bool served() const { return uses > 0; }
	void clear() { *this = mdb_verdict(); }
	/* one of its columns starts inside [a, b) */
	bool touches(uintptr_t a, uintptr_t b) const
	{
		return uses >= 0 && ((kl && (uintptr_t)kl >= a && (uintptr_t)kl < b) || (kr && (uintptr_t)kr >= a && (uintptr_t)kr < b));
	}
};

/* the facts, by (key; serves after a note) */
enum mdb_verdict_id {
	/* outcome of the last narrow-form decision, by the key columns it was made for (kl, nl, kr, nr - nr = 0 without kr;
	 * MDB_HINT_SERVES): a repeated query over the same columns skips the sampling kernel and its sync (every key is still verified
	 * while it is partitioned).  Payload: nh_* */
	VD_NARROW,
	/* range of the last key sample (smallest / largest of 2 x 4096 evenly spaced keys), by the columns it was taken from (kl, nl,
	 * kr, nr; MDB_HINT_SERVES).  Payload: sr_* */
	VD_SAMPLE,
	/* distinct values among the sampled keys of a column (group_hashed_try; kl, nl; MDB_HINT_SERVES).  Payload: gh_distinct */
	VD_DISTINCT,
	/* left key column (and the two row counts: kl, nl, nr - 0 without a right table) whose histogram-free partition layout
	 * overflowed last time: the exact layout at once (MDB_HINT_SERVES; a failed attempt costs a whole partition pass) */
	VD_EXACT,
	/* right key column (and row count: kr, nr) the one-level unique-key join (join_pairs_unique_wide) gave up on (no expiry) */
	VD_PW_BAD,
	/* key columns whose join had COUNTs above 1 (mdb_dev_join_keys asks for the COUNT column at once; the pair; MDB_HINT_SERVES) */
	VD_JK_DUP,
	/* key columns mdb_dev_join_payload found not to be an every-left-row-has-its-partner join (the pair; MDB_HINT_SERVES) */
	VD_JP_BAD,
	/* right key column (kr, nr) that the unique-key join found duplicates in, and the left key column (kl, nl) that did (both: a
	 * true N:M join, the general path): not tried again for MDB_BAD_SERVES calls, counted for both sides at once (dup_sides) */
	VD_PU_DUP_R,
	VD_PU_DUP_L,
	/* the last join over the pair fitted every COUNT(*) into a 4-byte group record, or not: r32_ok (no expiry) */
	VD_REC32,
	/* the left key column (and the two row counts: kl, nl, nr) for which a 16-bit row count of the one-level direct leaves
	 * (k_leaf_wide) overflowed last: two levels for these columns (MDB_BAD_SERVES) */
	VD_LW_BAD,
	/* ... and the one for which k_leaf_wide4's 5-bit / 4-bit counts did (more than 31 right or 15 left rows of a key):
	 * k_leaf_wide's 16-bit counts at once (MDB_BAD_SERVES) */
	VD_L4_BAD,
	/* what the last join over the pair delivered (no expiry).  Payload: lg_* */
	VD_LAST_GROUPS,
	VD_COUNT
};

struct mdb_col_memo {
	mdb_verdict vd[VD_COUNT];	/* EVERY verdict lives here: memo_drop() walks the array, none can be left out of invalidation */
	/* VD_NARROW */
	int nh_result = -1;		/* -1 nothing remembered, 0 wide, 1 narrow */
	int64_t nh_base = 0;		/* the window centre that went with "narrow" */
	uint32_t nh_kbits = 0;		/* ... and the compact window the sample offered (0 = none): [nh_lo, nh_lo + 2^nh_kbits) */
	int64_t nh_lo = 0;
	bool nh_r_based = false;	/* ... and the compact window was taken from the right table's keys alone */
	bool nh_prunable = false;	/* ... or at least not all of it (min-max pruning worth recording the right table's range) */
	bool nh_by_span = false;	/* ... because its sampled SPAN is small (min-max pruning does the work, no bitmap) */
	bool nh_selective = false;	/* ... and whether the right table looked like it covers a small part of the left table's keys */
	int nh_distrust = 0;		/* > 0: a remembered "narrow" just proved wrong (buffer reused for other data): sample again for a while */
	/* VD_SAMPLE */
	int64_t sr_lo = 0, sr_hi = 0;
	int64_t sr_rlo = 0, sr_rhi = 0;	/* the right table's sampled extremes (last sample) */
	uint64_t sr_span_l = 0, sr_span_r = 0;	/* spans of the two tables' sampled keys (last sample) */
	/* VD_DISTINCT */
	uint32_t gh_distinct = 0;
	/* VD_PU_DUP_R / VD_PU_DUP_L */
	int pu_dup_skips = 0;
	/* VD_REC32 */
	bool r32_ok = false;
	int keyed_distrust = 0;		/* > 0: a COUNT(*) did not fit a keyed group record lately - plain records for the next operators */
	/* VD_LAST_GROUPS: the last join over the pair delivered lg_groups groups: when that is under a quarter of the left rows, most left
	 * rows find no partner whatever the tables' sizes and ranges say (a right table of few distinct keys spread over the left
	 * table's range): the next join filters them early */
	uint64_t lg_groups = 0;
	uint32_t lg_nextra = 0;		/* (further right tables of that join: the three-table operator remembers too) */
	uint64_t lg_joined = 0;		/* ... and lg_joined joined rows: nearly every left row a group of COUNT 1 -> the groups as one bit per row (k_leaf_wide12) */
	int dn_distrust = 0;		/* calls for which that form is not tried (its exception list overflowed) */

	/* a REMEMBERED narrow-form guess proved wrong: the buffers hold other data than when it was made (a caller's allocator handed
	 * the same addresses out again) - forget it and the sample behind it, look at the data itself next time */
	void forget_guess()
	{
		vd[VD_NARROW].clear();
		nh_result = -1;
		vd[VD_SAMPLE].clear();
		nh_distrust = 1;
	}
	/* the unique-key join's two "this side has duplicates": a call that finds either counts once for both, and after
	 * MDB_BAD_SERVES counted calls both go (the buffers may hold other data by now: look again once in a while) */
	void dup_sides(const void *l, uint64_t n_l, const void *r, uint64_t n_r, bool *left_dups, bool *right_dups)
	{
		*right_dups = vd[VD_PU_DUP_R].holds(NULL, 0, r, n_r);
		*left_dups = vd[VD_PU_DUP_L].holds(l, n_l, NULL, 0);
		if ((*right_dups || *left_dups) && ++pu_dup_skips > MDB_BAD_SERVES) {
			*right_dups = *left_dups = false;
			vd[VD_PU_DUP_R].clear();
			vd[VD_PU_DUP_L].clear();
		}
	}
	void dup_side_note(bool right, const void *keys, uint64_t n)
	{
		if (right)
			vd[VD_PU_DUP_R].note(NULL, 0, keys, n);
		else
			vd[VD_PU_DUP_L].note(keys, n, NULL, 0);
		pu_dup_skips = 0;
	}
};

static inline void memo_reset(mdb_col_memo &m)
{
	m = mdb_col_memo();
}

/* A verdict is keyed by a column's ADDRESS and length.  A buffer that is released (its address will be handed out again), or
 * written to through the library (UPDATE: mdb_dev_scatter_set64; an upload into an existing buffer), takes what was learned
 * about it along: the next operator over that address samples afresh instead of trusting a verdict about other data (results
 * never depended on it - every verdict is verified on the device - but a wrong one costs a failed attempt). */
static inline void memo_drop(mdb_col_memo &m, uintptr_t a, uintptr_t b)
{
	for (mdb_verdict &v : m.vd)
		if (v.touches(a, b))
			v.clear();
}

struct mdb_memo_key {
	const void *kl, *kr;
	uint64_t nl, nr;
	bool operator==(const mdb_memo_key &o) const { return kl == o.kl && kr == o.kr && nl == o.nl && nr == o.nr; }
};

/* the live set (the base), the key-column pair it belongs to, and the other pairs' sets */
struct mdb_memo_store : mdb_col_memo {
	mdb_memo_key memo_key = { NULL, NULL, 0, 0 };
	std::vector<std::pair<mdb_memo_key, mdb_col_memo>> memo_lru;	/* most recently used last */
};

/* the bytes [lo, lo + bytes) are released or overwritten (bytes = 0: one byte - verdicts go by a column's first byte) */
static inline void mdb_memo_drop(mdb_memo_store *s, const void *lo, size_t bytes)
{
	const uintptr_t a = (uintptr_t)lo, b = a + (bytes ? bytes : 1);
	memo_drop(*s, a, b);
	/* the sets put aside for other column pairs: a set whose own columns are touched goes altogether */
	for (size_t i = 0; i < s->memo_lru.size();) {
		const mdb_memo_key &k = s->memo_lru[i].first;
		const bool own = (k.kl && (uintptr_t)k.kl >= a && (uintptr_t)k.kl < b) || (k.kr && (uintptr_t)k.kr >= a && (uintptr_t)k.kr < b);
		if (own) {
			s->memo_lru.erase(s->memo_lru.begin() + (long)i);
			continue;
		}
		memo_drop(s->memo_lru[i].second, a, b);
		i++;
	}
}

/* make the live memo the one of the key-column pair (kl, nl, kr, nr) - kr = NULL for a one-column operator (GROUP BY): the set
 * of the pair used before is put aside, the pair's own set (or an empty one) comes back */
static inline void mdb_memo_switch(mdb_memo_store *s, const void *kl, uint64_t nl, const void *kr, uint64_t nr)
{
	const mdb_memo_key key{ kl, kr, nl, kr ? nr : 0 };
	if (s->memo_key == key)
		return;
	mdb_col_memo &live = *s;
	/* put the live set aside under the pair it belongs to */
	if (s->memo_key.kl) {
		size_t i = 0;
		while (i < s->memo_lru.size() && !(s->memo_lru[i].first == s->memo_key))
			i++;
		if (i < s->memo_lru.size())
			s->memo_lru.erase(s->memo_lru.begin() + (long)i);
		s->memo_lru.push_back(std::make_pair(s->memo_key, live));
		if (s->memo_lru.size() > MDB_MEMO_SLOTS)
			s->memo_lru.erase(s->memo_lru.begin());
	}
	size_t i = 0;
	while (i < s->memo_lru.size() && !(s->memo_lru[i].first == key))
		i++;
	if (i < s->memo_lru.size()) {
		live = s->memo_lru[i].second;
		s->memo_lru.erase(s->memo_lru.begin() + (long)i);
	} else {
		memo_reset(live);
	}
	s->memo_key = key;
}

#endif /* MDB_DEV_MEMO_H */
