/*
 * mdb_dev_join_internal.h - what the translation units of the join / GROUP BY operators share: the leaf-table helpers, the
 * argument block of the fused operator's leaf kernels, the retry codes of its driver, and the host functions that cross the files
 *
 *   mdb_dev_join.hip       fused join + GROUP BY key + COUNT(*): the staged driver (plan, retries, split and N-way forms), the entry points, plain GROUP BY driver, mdb_dev_explain_*
 *   mdb_dev_join_leaf.hip  its per-leaf LDS kernels (hashed tables, direct-address tables, hot keys, the NULL group) and their launchers
 *   mdb_dev_leaf_wide.hip  ... and the kernels that join a whole first-level digit per workgroup
 *   mdb_dev_keyform.hip    the key sample and what it decides: narrow form, compact window, pruning hints (for every file below as well)
 *   mdb_dev_join_small.hip the forms that answer before the staged driver: single workgroup, any order, mdb_dev_group_count_keys
 *   mdb_dev_order.hip      ordering of the group records by first row id
 *   mdb_dev_groupby.hip    plain GROUP BY fast paths (small value range, few distinct values)
 *   mdb_dev_pairs.hip      materialising INNER JOIN
 */
#ifndef MDB_DEV_JOIN_INTERNAL_H
#define MDB_DEV_JOIN_INTERNAL_H

#include <stdlib.h>
#include <stddef.h>
#include "mdb_dev_internal.h"

/* ------------------------------------------------------------------ shared leaf helpers */

#define LEAF_THREADS 512		/* pairs-join leaf kernels */
#define GC_THREADS 1024		/* group-count leaf kernel: 16 waves x 2 workgroups = 32 waves/CU hide the LDS probe latency */
#define GC_EMIT_ITERS ((GC_SLOTS + 1 + GC_THREADS - 1) / GC_THREADS)	/* table slots visited per thread */
#define GC_REC_CHUNK 16384u	/* record-list slots a workgroup reserves at a time (one global atomic per chunk) */
#define LEAF_BATCH 2		/* keys loaded per thread before the first is consumed */
#define GC_SLOTS 3833u		/* group-count table (prime, for double hashing): 20 B/slot -> 75 KiB, two workgroups per CU */
#define GC_TARGET 1536u		/* average build keys per leaf (load factor ~0.4) */
#define PJ_SLOTS 2039u		/* pairs table (prime) */
#define PJ_TARGET 640u
#define PJ_CHUNK 2048u		/* right-side rows staged per sweep in the emit kernel */

__device__ static inline uint32_t leaf_slot(uint64_t hv, uint32_t slots)
{
	const uint32_t x = (uint32_t)hv * 0x9E3779B1u;
	return (uint32_t)(((uint64_t)x * slots) >> 32);
}

/* Double hashing: the probe step comes from the other half of the hashed key, in [1, slots - 1]; the table
 * sizes are prime, so every step visits all slots.  Linear probing clusters: at load 0.4 the longest of the
 * 64 probe chains a wave waits for was ~2x longer, and the wave pays the longest. */
__device__ static inline uint32_t leaf_step(uint64_t hv, uint32_t slots)
{
	const uint32_t y = (uint32_t)(hv >> 32) * 0x85EBCA6Bu;
	return 1u + (uint32_t)(((uint64_t)y * (slots - 1)) >> 32);
}

/* insert-or-find hv (hv != 0); returns the slot or 0xFFFFFFFF when the table is full; *created = this call
 * claimed the slot (exactly one caller per distinct key sees true) */
__device__ static inline uint32_t leaf_insert(unsigned long long *keys, uint32_t slots, uint64_t hv, bool *created = nullptr)
{
	uint32_t s = leaf_slot(hv, slots);
	const uint32_t step = leaf_step(hv, slots);
	for (uint32_t probe = 0; probe < slots; probe++) {
		const unsigned long long old = atomicCAS(&keys[s], 0ull, (unsigned long long)hv);
		if (old == 0ull || old == hv) {
			if (created)
				*created = old == 0ull;
			return s;
		}
		s += step;
		if (s >= slots)
			s -= slots;
	}
	return 0xFFFFFFFFu;
}

/* find hv (hv != 0) after the build phase; 0xFFFFFFFF = absent */
__device__ static inline uint32_t leaf_find(const unsigned long long *keys, uint32_t slots, uint64_t hv)
{
	uint32_t s = leaf_slot(hv, slots);
	const uint32_t step = leaf_step(hv, slots);
	for (uint32_t probe = 0; probe < slots; probe++) {
		const unsigned long long cur = keys[s];
		if (cur == hv)
			return s;
		if (cur == 0ull)
			return 0xFFFFFFFFu;
		s += step;
		if (s >= slots)
			s -= slots;
	}
	return 0xFFFFFFFFu;
}

#define GC_MAX_EXTRA 2		/* right tables beyond the first one (mdb_dev_join_group_count_multi: up to 3 right tables) */

struct gc_args {
	const uint64_t *hv_l;
	const uint32_t *rid_l;
	const uint32_t *off_l;		/* exact leaf offsets, or ... */
	const uint32_t *cnt_l;		/* ... rows per leaf of the fixed-capacity (fast) layout */
	uint32_t cap_l;			/* 0 = exact offsets */
	const uint64_t *hv_r;		/* NULL: plain GROUP BY over the left stream */
	const uint32_t *off_r;
	const uint32_t *cnt_r;
	uint32_t cap_r;
	int64_t *dense_cnt;		/* dense mode: [n_l], zeroed: COUNT(*) written at the group's first L position */
	uint32_t dense_n;		/* ... = n_l: a first row id is checked against it before it indexes dense_cnt[] - a fixed-capacity region that
					 * overflowed (status bit 1: the operator is redone) holds slots nobody wrote, with whatever an earlier call left */
	unsigned long long *rec;	/* record mode: one 64-bit record per group, (first << (64 - kbits)) | COUNT(*) */
	uint32_t *rec_count;		/* record mode: list slots handed out so far (the list has zero-filled gaps) */
	uint32_t *rec_valid;		/* record mode: number of real records (= groups) */
	uint32_t rec_cap;		/* record mode: capacity of the list */
	uint32_t kbits;			/* record mode: bits of a left row id (0 = dense mode) */
	unsigned long long *joined;	/* sum of all counts */
	uint32_t *status;		/* bit 0: a leaf table overflowed */
	uint32_t nleaves;
	uint32_t heavy_l, heavy_r;	/* rows of a side from which a leaf counts as hot (>= GC_HEAVY and >= 8x the side's average leaf) */
	uint32_t narrow;		/* narrow form: hv_l[i] = hash32 << 32 | row id (rid_l unused), hv_r = array of 4-byte hash32 */
	uint32_t rec32;			/* direct-address leaves: the records are written as 4-byte words (first row id << (32 - kbits)) | COUNT(*) - the
					 * caller has seen, for these very columns, that every COUNT fits; one that does not raises status bit 9 and
					 * the operator is redone with 8-byte records */
	uint32_t keyed_cbits;		/* direct-address leaves, != 0: KEYED group records - (first row id, hashed key, COUNT(*)) with COUNT in
					 * the low keyed_cbits bits and the key_bits-wide hashed key above it: the ordering kernel decodes the
					 * group key from the record instead of gathering it from the key column (selective joins: the groups'
					 * first rows are scattered over the left table, every gathered key costs a 128-byte line) */
	uint32_t merge_all;		/* plain GROUP BY: the key sample held duplicates (some 10^4 - 10^5 distinct values): merge equal
					 * values per wave in every leaf, not only in the oversize ones */
	/* further right tables joined on the SAME key (A JOIN B ON a = b JOIN C ON a = c ... GROUP BY a: BASELINE configs[4]) -
	 * direct-address leaves only: partitioned exactly like the right table (4-byte words, fixed-capacity leaves), counted into
	 * LDS arrays of their own; a key's right count becomes the PRODUCT of its counts in all right tables */
	/* k_leaf_wide4, rg_rec != NULL: the group records are written straight into the ordering kernel's ranges of 2^rg_shift first row ids -
	 * region r of rg_cap records at rg_rec + r * rg_cap, its fill in rg_cnt[r] (zeroed by the caller) - instead of one list that two scatter
	 * levels then partition by row id; a range that outgrows its region raises flag 8192 */
	unsigned long long *rg_rec;
	uint32_t *rg_cnt;
	uint32_t rg_cap, rg_shift, rg_n;
	/* k_leaf_wide12, dn_bits != NULL (nearly every left row a group of COUNT 1 - remembered from the last call over these columns): no
	 * record per group.  One bit per LEFT row, set by the caller, cleared here for every row that is no group's first row (no partner, or
	 * not the first of its key); groups whose COUNT is not 1 are appended to dn_exc as first row << 32 | COUNT (mdb_dev_dense.hip expands) */
	unsigned int *dn_bits;
	unsigned long long *dn_exc;
	uint32_t dn_exc_cap;
	uint32_t *dn_cnt;		/* [0] bits cleared, [1] exceptions */
	uint32_t dn_pilot;		/* != 0 (dn_bits = dn_exc = NULL): the pilot - the first dn_pilot digits only, nothing but the counters is written */
	uint32_t nextra;
	const uint32_t *hv_x[GC_MAX_EXTRA];
	const uint32_t *cnt_x[GC_MAX_EXTRA];
	uint32_t cap_x[GC_MAX_EXTRA];
};

/* narrow word -> the 64-bit value the leaf tables work with (both halves = the 32-bit hash, so that the slot and the
 * probe step still come from different multipliers; 0 only for the key whose hash is 0) */
__device__ static inline uint64_t gc_narrow_hv(uint64_t w)
{
	const uint32_t h = (uint32_t)(w >> 32);
	return ((uint64_t)h << 32) | h;
}

__device__ static inline void gc_leaf_range(const uint32_t *off, const uint32_t *cnt, uint32_t cap, uint32_t leaf, uint32_t *b,
					    uint32_t *e)
{
	if (cap) {
		const uint32_t c = cnt[leaf];
		*b = leaf * cap;
		*e = *b + (c < cap ? c : cap);
	} else {
		*b = off[leaf];
		*e = off[leaf + 1];
	}
}

#define LW_THREADS 1024
#define LW_MIN_REM 6u		/* tables of 64 entries at least (key windows from 2^15 values: that few values per first-level region - their
				 * number varies by 13 % - need the looser regions of mdb_part_request.loose) */
#define LW_EMIT_REM 11u		/* from here on every thread owns at least one 32-bit word of halves in the emit pass */
#define LW_MAX_REM 14u
#define LW_UNROLL 4

__device__ static inline unsigned long long lw_block_sum(unsigned long long v, unsigned long long *s_red)
{
#pragma unroll
	for (int o = 32; o; o >>= 1)
		v += __shfl_down(v, o, MDB_WAVE);
	__syncthreads();	/* protect s_red against a previous use */
	if (mdb_lane() == 0)
		s_red[threadIdx.x >> 6] = v;
	__syncthreads();
	unsigned long long t = 0;
#pragma unroll
	for (int w = 0; w < LW_THREADS / 64; w++)
		t += s_red[w];
	return t;
}

/* internal return codes of the operator's attempts (never leave the library): ONE enum, so that no two can share a value
 * (round 5 gave GC_RETRY_NODENSE the value of GC_NOT_SERVED and an unserved three-table operator was retried six times) */
enum gc_internal_rc {
	GC_RETRY_EXACT = 1000,	/* internal: a fast-layout leaf overflowed, redo with exact histograms */
	GC_RETRY_DENSE,	/* internal: a COUNT(*) does not fit a group record, redo with the dense ordering */
	GC_RETRY_BUILD_L,	/* internal: the right side's distinct keys overflowed a leaf table, redo building on the left side */
	GC_RETRY_WIDE,	/* internal: a key outside the int32 range met the narrow form, redo with 64-bit hashes */
	GC_RETRY_PLAIN,	/* internal: a key outside the compact window (the sample missed the column's extremes): redo in the plain narrow form */
	GC_RETRY_UNKEYED,	/* internal: a COUNT(*) does not fit a keyed group record (ctx->keyed_distrust is set): redo with plain records */
	GC_RETRY_REC64,	/* internal: 4-byte group records were written on a remembered verdict that no longer holds: redo with 8-byte ones */
	GC_RETRY_TWO_LEVEL,	/* internal: a 16-bit row count of k_leaf_wide overflowed (VD_LW_BAD remembers the columns): redo with two levels */
	GC_RETRY_NODENSE,	/* internal: the bit-per-row form of the groups met more groups of COUNT != 1 than its list holds (ctx->dn_distrust is set) */
	GC_EXPLAINED,	/* internal: mdb_dev_explain_*() - the plan is written, nothing was launched */
	GC_NOT_SERVED,	/* internal: further right tables, but the operator did not take the two-level direct-address form (or a product of counts overflowed, or a hot leaf): the caller chains two-table operators instead */
};
/* ---- the fused operator's flags in word 0 of ctx->d_status (beside the common MDB_ST_* ones), raised by its leaf kernels and the kernels that feed
 * them, read by gc_finish, tiny_group_count and the three-table caller */
#define GC_ST_TABLE_FULL 1u		/* a leaf's hash table is full */
#define GC_ST_COUNT_NOT_REC64 4u	/* a COUNT(*) does not fit a 64-bit record beside the row id */
#define GC_ST_COUNT_NOT_REC32 16u	/* ... nor a 4-byte record */
#define GC_ST_HOT_LEAVES 64u		/* leaves left to the hot-key path */
#define GC_ST_COUNT_NOT_KEYED 256u	/* a COUNT(*) does not fit a keyed record */
#define GC_ST_REC32_STALE 512u		/* 4-byte records were written on a remembered verdict that no longer holds */
#define GC_ST_ROWS_NOT_16BIT 1024u	/* a 16-bit row count of the one-level leaves (k_leaf_wide) overflowed */
#define GC_ST_PRODUCT_WIDE 2048u	/* a product of the right tables' counts beyond 32 bits */
#define GC_ST_COUNTS_NOT_4BYTE 4096u	/* k_leaf_wide4's count fields overflowed */
#define GC_ST_RANGE_FULL 8192u		/* an ordering range outgrew its region */
#define GC_ST_LEFT_DUPS 32768u		/* a key that has partners has several rows in the LEFT table (raised by the direct-address leaf kernels) */
#define GC_ST_EXC_FULL 131072u		/* the bit-per-row form's exception list overflowed */
static_assert(mdb_flags_distinct({ MDB_ST_REGION_FULL, MDB_ST_LIST_FULL, MDB_ST_KEY_OUTSIDE, GC_ST_TABLE_FULL, GC_ST_COUNT_NOT_REC64, GC_ST_COUNT_NOT_REC32,
				   GC_ST_HOT_LEAVES, GC_ST_COUNT_NOT_KEYED, GC_ST_REC32_STALE, GC_ST_ROWS_NOT_16BIT, GC_ST_PRODUCT_WIDE, GC_ST_COUNTS_NOT_4BYTE,
				   GC_ST_RANGE_FULL, GC_ST_LEFT_DUPS, GC_ST_EXC_FULL }),
	      "fused operator: two status flags share a bit");

/* the single-workgroup operators (k_tiny_group_count, k_tiny_join_pairs) WRITE word 0 - nothing else has run - and word GC_STW_LIST_LEN: the
 * number of results, and this flag when they are more than the caller's buffers hold */
#define TINY_ST_OVER_CAP 4096u

/* ---- the words of ctx->d_status the fused operator uses (4-byte word indices).  Shared in time: [10..21] hold the key sample's extremes
 * BEFORE the operator starts (gc_sample_range reads them back at once); while it runs [12..13] are the bit-per-row counters, [16..17] the
 * right table's key range and [20..21] the window - all inside the sample's words, which are dead by then. */
#define GC_STW_LIST_LEN 1	/* slots of the record list handed out so far (the tiny and any-order operators: the number of groups) */
#define GC_STW_JOINED 2		/* [2..3] joined rows (u64) */
#define GC_STW_NULL_STATS 4	/* [4..7] NULL group: rows, first row (two u64) */
#define GC_STW_RECORDS 8	/* real records = groups */
#define GC_STW_LAST_FIRST 9	/* one-level leaves: the largest first row id; plain GROUP BY's sample: distinct values */
#define GC_STW_SAMPLE 10	/* [10..21] the key sample's six 8-byte extremes */
#define GC_STW_DN_CLEARED 12	/* bit-per-row form: bits cleared ... */
#define GC_STW_DN_EXC 13	/* ... and exceptions listed */
#define GC_STW_MINMAX 16	/* [16..17] the right table's smallest / largest key - window base (min-max pruning) */
#define GC_STW_WINDOW 20	/* [20..21] 0 and 2^key_bits - 1: the whole window as a pruning range (further right tables drop what lies outside) */
#define GC_STW_MINMAX64 40	/* [40..43] the right table's smallest / largest key as two signed 64-bit words (min-max pruning, 64-bit form) */

/* what the host copies back from word 0 on (to ctx->h_pinned + MDB_HP_STATUS): 40 bytes where the bit-per-row counters are not needed, 56 with them */
struct gc_readback {
	uint32_t flags;
	uint32_t list_len;
	uint64_t joined;
	uint64_t null_stats[2];
	uint32_t groups;
	uint32_t last_first;
	uint32_t sample_head[2];	/* (not the operator's) */
	uint32_t dn_cleared;
	uint32_t dn_exceptions;
};
#define GC_RB_BYTES 40
#define GC_RB_BYTES_DN 56
static_assert(sizeof(gc_readback) == GC_RB_BYTES_DN && offsetof(gc_readback, flags) == 4 * MDB_STW_FLAGS && offsetof(gc_readback, list_len) == 4 * GC_STW_LIST_LEN &&
		      offsetof(gc_readback, joined) == 4 * GC_STW_JOINED && offsetof(gc_readback, null_stats) == 4 * GC_STW_NULL_STATS &&
		      offsetof(gc_readback, groups) == 4 * GC_STW_RECORDS && offsetof(gc_readback, last_first) == 4 * GC_STW_LAST_FIRST &&
		      offsetof(gc_readback, sample_head) == 4 * GC_STW_SAMPLE && offsetof(gc_readback, dn_cleared) == 4 * GC_STW_DN_CLEARED &&
		      offsetof(gc_readback, dn_exceptions) == 4 * GC_STW_DN_EXC && GC_RB_BYTES == 4 * GC_STW_SAMPLE,
	      "gc_readback does not lie over the status words");

/* one table of a join call: its key column, the column's NULL bits (or NULL) and its rows */
struct gc_table {
	const int64_t *keys;
	const uint64_t *nulls;
	uint64_t n;
};

/* the two tables of a call; the call with the sides swapped is gc_sides{ s.r, s.l }.  One column: r = { NULL, NULL, 0 } */
struct gc_sides {
	gc_table l, r;
};

/* where a call's groups go: key / first may be NULL (not wanted), joined as well */
struct gc_out {
	int64_t *key, *count;
	uint32_t *first;
	uint64_t cap;
	uint64_t *groups, *joined;
	void clear() const
	{
		*groups = 0;
		if (joined)
			*joined = 0;
	}
};

struct gc_window {
	uint32_t kbits;		/* 0 = no compact window */
	int64_t lo;
	bool selective;		/* the right table's sampled keys cover less than a quarter of the left table's sampled key range, or the right
				 * table has less than a quarter of the left table's rows: most left rows will find no partner (semi-join filter) */
	bool by_span;		/* ... the former: min-max pruning at the first level will drop them, no bitmap needed */
	bool prunable;		/* the right table's sampled keys cover less than 7/8 of the left table's sampled range: worth recording the
				 * right table's exact range for min-max pruning */
	bool r_based;		/* the compact window covers the RIGHT table's sampled keys only (by_span, unsplit call): the left rows outside
				 * it are exactly the ones min-max pruning drops - fewer key bits, hence fewer and larger leaves */
	bool fast1;		/* plain GROUP BY, duplicates in the key sample: the fixed-capacity layout only if the ONE-level form applies */
};

/* what gc_narrow_guess decides for a call's key columns.  narrow: try the narrow form; base: centre of the 2^32-wide window of key values it
 * will be tried with (0 = the plain int32 range, whenever the sampled keys lie inside it); win: the compact window the sample offers */
struct gc_key_form {
	bool narrow;
	int64_t base;
	gc_window win;
};

#define TINY_ROWS (GC_THREADS * LEAF_BATCH)	/* rows per table up to which ONE workgroup does the whole operator in LDS */
#define GC_NARROW_MIN_ROWS (1u << 20)
#define GC_NARROW_SAMPLE 4096u

/* position of sample t: pseudo-random, not evenly spaced - generated or periodic data (an affine sequence, a table sorted by
 * a low-cardinality column) looks very different at a fixed stride than it is */
__device__ static inline uint64_t gc_sample_pos(uint32_t t, uint64_t n)
{
	return mdb_fmix64(0x9E3779B97F4A7C15ull * (uint64_t)(t + 1)) % n;
}

/* ---- host functions that cross the files (definitions: see the list at the top) */
uint64_t gc_rec_capacity(mdb_dev_ctx *ctx, uint64_t n_l);
bool order_bits(uint64_t n_l, uint32_t *kbits, int *sb1, int *sb2);
/* ranges of 2^ORDER_RANGE_BITS first row ids, ORDER_RANGE_CAP records each, as k_order_leaf_sparse ranks them: whether records of a table of
 * n_l rows expected to number `groups` may be written into them by the leaf kernel itself, and the ordering of such ranges */
#define ORDER_RANGE_BITS 16u
#define ORDER_RANGE_CAP 8192u
bool order_ranges_apply(uint64_t n_l, uint32_t kbits, uint64_t groups, uint32_t *nranges);
int order_presorted(mdb_dev_ctx *ctx, const unsigned long long *regions, const uint32_t *counts, uint32_t nranges, uint32_t kbits, uint32_t *out_first,
		    int64_t *out_count, const int64_t *keys, int64_t *out_key, bool keys32, uint32_t keyed_cbits, uint32_t key_bits, int64_t key_lo,
		    uint64_t early_cap = 0);
uint32_t order_digits0(uint64_t n_l, uint32_t kbits, int sb1);
int order_records(mdb_dev_ctx *ctx, const unsigned long long *rec, uint64_t list_len, uint64_t n_l, uint32_t kbits, int sb1,
			 int sb2, uint32_t *out_first, int64_t *out_count, uint32_t *out_val32, const int64_t *keys, int64_t *out_key,
			 bool keys32 = false, bool rec32 = false, uint32_t keyed_cbits = 0, uint32_t key_bits = 0, int64_t key_lo = 0,
			 bool in32 = false /* the list already holds 4-byte records */, uint64_t n_rec = 0 /* records in the list (0: unknown) */);
size_t order_records_arena_bytes(uint64_t cap, uint64_t n_l, uint32_t kbits, int sb1, int sb2);
bool ld_disabled(void);
/* the first four status words - flags, GC_STW_LIST_LEN, GC_STW_JOINED as two halves - copied to the pinned block, waited for: *h points at them */
int gc_status_head(mdb_dev_ctx *ctx, const uint32_t **h);
static inline uint64_t gc_status_joined(const uint32_t *h)
{
	return (uint64_t)h[GC_STW_JOINED] | ((uint64_t)h[GC_STW_JOINED + 1] << 32);
}

/* ---- mdb_dev_keyform.hip: the key sample and the key form it decides */
int gc_sample_range(mdb_dev_ctx *ctx, const gc_sides &s, bool fresh, int64_t *lo, int64_t *hi, bool keys32 = false);
void gc_compact_window(int64_t lo, int64_t hi, uint32_t *kbits, int64_t *wlo, bool exact = false);
void gc_narrow_note(mdb_dev_ctx *ctx, const gc_sides &s, bool narrow, int64_t base = 0, uint32_t key_bits = 0, int64_t key_lo = 0);
bool gc_learned_selective(const mdb_dev_ctx *ctx, const gc_sides &s);
int gc_narrow_guess(mdb_dev_ctx *ctx, const gc_sides &s, gc_key_form *kf, bool keys32 = false, bool prune_ok = false /* unsplit call: min-max pruning can run */);

/* The forms that take a compact window from the key sample ALONE (any-order join, mdb_dev_group_count_keys, the band / tile sort of
 * mdb_dev_group_count) and check every key against it on the device: sample, window, form - and on a key outside the window of a REMEMBERED
 * sample (the column's contents have changed since) the sample is taken again, once; outside a sample just taken: not served, and the next few
 * calls look at the data itself (nh_distrust).  fresh: as gc_sample_range takes it; of: whose sampled range the window pads; exact_stats: a range
 * from the caller's statistics is the column's own - no margin.  form(lo, kbits) reports a gc_form_rc or an error (< 0), and so does this. */
enum gc_form_rc { GC_FORM_DONE = 0, GC_FORM_NOT_SERVED = 1, GC_FORM_KEY_OUTSIDE = 2 };
enum gc_window_of { GC_WINDOW_BOTH, GC_WINDOW_RIGHT };
template <typename Form>
static int gc_windowed_try(mdb_dev_ctx *ctx, const gc_sides &s, bool fresh, gc_window_of of, bool exact_stats, Form form)
{
	for (int attempt = 0; attempt < 2; attempt++) {
		int64_t lo = 0, hi = 0;
		int rc = gc_sample_range(ctx, s, attempt > 0 || fresh, &lo, &hi);
		if (rc)
			return rc;
		const bool remembered = ctx->vd[VD_SAMPLE].served();
		const bool right = of == GC_WINDOW_RIGHT;
		uint32_t kb = 0;
		int64_t wlo = 0;
		gc_compact_window(right ? ctx->sr_rlo : lo, right ? ctx->sr_rhi : hi, &kb, &wlo, !right && exact_stats && ctx->plan.from_stats != 0);
		if (!kb)
			return GC_FORM_NOT_SERVED;
		rc = form(wlo, kb);
		if (rc != GC_FORM_KEY_OUTSIDE)
			return rc;
		if (!(remembered && attempt == 0)) {
			ctx->nh_distrust = 8;	/* a key outside the sampled window: look at the data itself the next few times */
			return GC_FORM_NOT_SERVED;
		}
	}
	return GC_FORM_NOT_SERVED;
}

/* ---- mdb_dev_join_small.hip, mdb_dev_groupby.hip: the forms that answer before the staged driver.  0 = done, 1 = not served, < 0 = error */
int tiny_group_count(mdb_dev_ctx *ctx, const gc_sides &s, bool has_r, bool null_group, const gc_out &out);
int gc_unordered_try(mdb_dev_ctx *ctx, const gc_sides &s, const gc_out &out, const gc_table *x = NULL, int nextra = 0);
int group_hashed_try(mdb_dev_ctx *ctx, const gc_table &t, bool null_group, const gc_out &out);
int group_direct_try(mdb_dev_ctx *ctx, const gc_sides &s, bool null_group, const gc_out &out);

/* ---- mdb_dev_join_leaf.hip: one workgroup per leaf */
#define LD_MAX_REM 12u		/* direct-address leaves: tables of at most 2^LD_MAX_REM entries */
#define GC_HEAVY (8u * GC_THREADS * LEAF_BATCH)	/* floor of the hot threshold (gc_args.heavy_l / heavy_r) */
int leaf_hashed_launch(mdb_dev_ctx *ctx, const gc_args &a, bool has_r, bool build_r, bool narrow);
int leaf_direct_launch(mdb_dev_ctx *ctx, const gc_args &a, uint32_t rem, uint32_t shift, bool has_r, int nextra);
int leaf_bitmap_launch(mdb_dev_ctx *ctx, const uint32_t *hv_r, const uint32_t *cnt_r, uint32_t cap_r, uint32_t nleaves, uint32_t rem, uint32_t coarse, uint32_t shift,
		       uint32_t *bits);
int leaf_null_group_launch(mdb_dev_ctx *ctx, const gc_args &a, const uint64_t *null_l, uint64_t n_l);
size_t leaf_hot_arena_bytes(void);
int leaf_hot_launch(mdb_dev_ctx *ctx, const gc_args &a, bool has_r, bool build_r);
int leaf_gather_i32_launch(mdb_dev_ctx *ctx, const int32_t *keys, const uint32_t *sel, uint64_t n, int64_t *out);
/* mdb_dev_leaf_wide.hip: one workgroup per first-level digit */
int leaf_wide_launch(mdb_dev_ctx *ctx, const gc_args &a, uint32_t nleaves, uint32_t rem, uint32_t shift, uint32_t nsub, bool has_r, bool r16);
int leaf_wide4_launch(mdb_dev_ctx *ctx, const gc_args &a, uint32_t nleaves, uint32_t rem, uint32_t shift, uint32_t nsub);
bool leaf_wide12_fits(const mdb_dev_ctx *ctx, uint64_t n_l, uint64_t n_r, uint64_t n_x);
int leaf_wide12_launch(mdb_dev_ctx *ctx, const gc_args &a, uint32_t nleaves, uint32_t rem, uint32_t nsub, int nextra);

#endif /* MDB_DEV_JOIN_INTERNAL_H */
