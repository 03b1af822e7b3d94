/*
 * mdb_dev_join_small.hip - the forms of the fused join + GROUP BY key + COUNT(*) operator that answer before its staged driver (split off
 * mdb_dev_join.hip; what the files share: mdb_dev_join_internal.h): the single-workgroup operator for tiny inputs (k_tiny_group_count),
 * the any-order operator (gc_unordered_try: no row ids, no ordering sort - the sharded operator's pipeline on one GPU) and
 * mdb_dev_group_count_keys, the same pipeline over one column.  The entry points in mdb_dev_join.hip try them first.
 */
#include "mdb_dev_join_internal.h"

/* the shape of these forms' plans in the plan record (the staged driver's: gc_plan_note): every shape field, so that none is left over from an operator these follow */
static void gc_plan_shape(mdb_dev_ctx *ctx, uint32_t key_form, uint32_t levels, uint32_t minmax_pruned, uint32_t any_order)
{
	struct mdb_dev_plan_info *o = &ctx->plan;
	o->key_form = key_form;
	o->key_bits = 0;
	o->levels = levels;
	o->digits = 512;
	o->minmax_pruned = minmax_pruned;
	o->semijoin = 0;
	o->any_order = any_order;
	o->ranged_order = 0;
	o->multi_one_pass = 0;
}

/* ------------------------------------------------------------------ tiny inputs: one kernel, one workgroup
 *
 * The reference's own tests and README work on a handful of rows; through the partitioned pipeline such a query is ~20
 * launches and two synchronisations (~170 us).  Up to GC_THREADS * LEAF_BATCH rows per table one workgroup does the whole
 * operator in LDS: table from the left rows (COUNT, first row), right rows counted into it, and - because a left row that
 * is the first of its group knows so - the groups leave in first-occurrence order by a prefix sum over the rows, no sort. */

struct tiny_args {
	const int64_t *keys_l;
	const uint64_t *null_l;
	uint32_t n_l;
	const int64_t *keys_r;
	const uint64_t *null_r;
	uint32_t n_r;
	uint32_t null_group;
	int64_t *out_key;
	int64_t *out_count;
	uint32_t *out_first;
	uint32_t cap;
	uint32_t *status;	/* [1] groups, [2..3] joined rows, [0] bit 12: more groups than cap */
};

template <bool HAS_R>
__global__ __launch_bounds__(GC_THREADS) void k_tiny_group_count(tiny_args a)
{
	__shared__ unsigned long long s_key[GC_SLOTS];
	__shared__ unsigned long long s_cnt[GC_SLOTS + 2];	/* [GC_SLOTS] the value whose hash is 0, [GC_SLOTS + 1] the NULL group */
	__shared__ uint32_t s_first[GC_SLOTS + 2];
	__shared__ uint32_t s_tmp[32];
	__shared__ unsigned long long s_sum;
	for (uint32_t s = threadIdx.x; s < GC_SLOTS + 2; s += GC_THREADS) {
		if (s < GC_SLOTS)
			s_key[s] = 0ull;
		s_cnt[s] = 0ull;
		s_first[s] = 0xFFFFFFFFu;
	}
	if (threadIdx.x == 0)
		s_sum = 0ull;
	__syncthreads();
	uint32_t slot[LEAF_BATCH];
#pragma unroll
	for (int u = 0; u < LEAF_BATCH; u++) {
		const uint32_t i = threadIdx.x + (uint32_t)u * GC_THREADS;
		slot[u] = 0xFFFFFFFFu;
		if (i >= a.n_l)
			continue;
		if (a.null_l && mdb_bit_is_set(a.null_l, i)) {
			if (!HAS_R && a.null_group)
				slot[u] = GC_SLOTS + 1;
		} else {
			const uint64_t hv = mdb_fmix64((uint64_t)a.keys_l[i]);
			slot[u] = hv ? leaf_insert(s_key, GC_SLOTS, hv) : GC_SLOTS;	/* 2048 values at most: the table cannot fill */
		}
		if (slot[u] != 0xFFFFFFFFu) {
			atomicAdd(&s_cnt[slot[u]], 1ull);
			atomicMin(&s_first[slot[u]], i);
		}
	}
	__syncthreads();
	if (HAS_R) {
#pragma unroll
		for (int u = 0; u < LEAF_BATCH; u++) {
			const uint32_t j = threadIdx.x + (uint32_t)u * GC_THREADS;
			if (j >= a.n_r || (a.null_r && mdb_bit_is_set(a.null_r, j)))
				continue;
			const uint64_t hv = mdb_fmix64((uint64_t)a.keys_r[j]);
			const uint32_t s = hv ? leaf_find(s_key, GC_SLOTS, hv) : GC_SLOTS;
			if (s != 0xFFFFFFFFu && (uint32_t)s_cnt[s])
				atomicAdd(&s_cnt[s], 1ull << 32);
		}
		__syncthreads();
	}
	/* a left row that is the first of its group (and whose group survives the join) is a result row */
	bool head[LEAF_BATCH];
	unsigned long long cnt[LEAF_BATCH];
	unsigned long long joined = 0;
#pragma unroll
	for (int u = 0; u < LEAF_BATCH; u++) {
		const uint32_t i = threadIdx.x + (uint32_t)u * GC_THREADS;
		head[u] = false;
		cnt[u] = 0;
		if (slot[u] != 0xFFFFFFFFu && s_first[slot[u]] == i) {
			const unsigned long long c2 = s_cnt[slot[u]];
			const unsigned long long cl = (uint32_t)c2, cr = c2 >> 32;
			cnt[u] = HAS_R ? cl * cr : cl;
			head[u] = cnt[u] != 0;
			joined += cnt[u];
		}
	}
	/* positions: rows are visited in index order across (u, thread): row = u * GC_THREADS + thread, so the prefix runs
	 * over u = 0 first, then u = 1 */
	uint32_t base = 0;
#pragma unroll
	for (int u = 0; u < LEAF_BATCH; u++) {
		uint32_t total;
		const uint32_t ex = mdb_block_excl_scan(head[u] ? 1u : 0u, s_tmp, &total);
		if (head[u]) {
			const uint32_t pos = base + ex;
			if (pos < a.cap) {
				const uint32_t i = threadIdx.x + (uint32_t)u * GC_THREADS;
				if (a.out_first)
					a.out_first[pos] = i;
				a.out_count[pos] = (int64_t)cnt[u];
				if (a.out_key)
					a.out_key[pos] = a.keys_l[i];
			}
		}
		base += total;
	}
	if (joined)
		atomicAdd(&s_sum, joined);
	__syncthreads();
	if (threadIdx.x == 0) {
		a.status[MDB_STW_FLAGS] = base > a.cap ? TINY_ST_OVER_CAP : 0u;
		a.status[GC_STW_LIST_LEN] = base;
		*(unsigned long long *)(a.status + GC_STW_JOINED) = s_sum;
	}
}

/* 0 = done, 1 = not applicable, < 0 = error */
int tiny_group_count(mdb_dev_ctx *ctx, const gc_sides &s, bool has_r, bool null_group, const gc_out &out)
{
	if (s.l.n == 0 || s.l.n > TINY_ROWS || (has_r && (s.r.n == 0 || s.r.n > TINY_ROWS)) || (!out.count && !ctx->explaining))
		return 1;
	ctx->plan.small_form = 1;
	if (ctx->explaining)
		return MIDORIDB_OK;
	tiny_args a;
	memset(&a, 0, sizeof(a));
	a.keys_l = s.l.keys;
	a.null_l = s.l.nulls;
	a.n_l = (uint32_t)s.l.n;
	a.keys_r = s.r.keys;
	a.null_r = s.r.nulls;
	a.n_r = has_r ? (uint32_t)s.r.n : 0u;
	a.null_group = null_group ? 1u : 0u;
	a.out_key = out.key;
	a.out_count = out.count;
	a.out_first = out.first;
	a.cap = out.cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)out.cap;
	a.status = ctx->d_status;
	if (has_r) {
		MDB_LAUNCH(ctx, "tiny_join_group_count", k_tiny_group_count<true>, 1, GC_THREADS, a);
	} else {
		MDB_LAUNCH(ctx, "tiny_group_count", k_tiny_group_count<false>, 1, GC_THREADS, a);
	}
	const uint32_t *h = NULL;
	const int rc = gc_status_head(ctx, &h);
	if (rc)
		return rc;
	if (h[MDB_STW_FLAGS] & TINY_ST_OVER_CAP)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group output capacity %llu too small for %llu groups", (unsigned long long)out.cap,
				   (unsigned long long)h[GC_STW_LIST_LEN]);
	*out.groups = h[GC_STW_LIST_LEN];
	if (out.joined)
		*out.joined = gc_status_joined(h);
	gc_plan_shape(ctx, 0, 2, 0, 0);
	return 0;
}

/* The any-order pipeline on the window [wlo, wlo + 2^kb): the sharded operator's receiver (mdb_dev_shard.hip) on this GPU's own first-level regions.
 * tab[0] is the left table (none: right_only - every leaf slot with rows is a group), tab[1..ntab-1] the right ones, partitioned last to first
 * as in the ordered operator.  Reports a gc_form_rc for gc_windowed_try, or an error; on GC_FORM_DONE *h points at the status words */
static int any_order_form(mdb_dev_ctx *ctx, const gc_table *tab, uint32_t ntab, bool right_only, int64_t span_l, int64_t wlo, uint32_t kb, int64_t *out_key,
			  int64_t *out_count, uint64_t cap, mdb_shard_plan *plan, const uint32_t **h)
{
	if (kb > 30u)
		return GC_FORM_NOT_SERVED;
	const uint64_t n_max[MDB_SHARD_MAX_TABS] = { tab[0].n, tab[1].n, ntab > 2 ? tab[2].n : 0, ntab > 3 ? tab[3].n : 0 };
	if (mdb_shard_plan_make(1, 0, ntab, n_max, 0, span_l, wlo, wlo + (int64_t)((1ull << kb) - 1), plan))
		return GC_FORM_NOT_SERVED;
	plan->right_only = right_only;
	int rc = mdb_arena_begin(ctx, mdb_shard_arena_bytes(plan));
	if (rc)
		return rc;
	MDB_HIP(ctx, hipMemsetAsync(ctx->d_status, 0, 16 * sizeof(uint32_t), ctx->stream));
	const void *regions[MDB_SHARD_MAX_TABS] = { NULL, NULL, NULL, NULL };
	const uint32_t *cursors[MDB_SHARD_MAX_TABS] = { NULL, NULL, NULL, NULL };
	for (int t = (int)ntab - 1; t >= 0; t--)	/* (a left table of no rows: all-zero counters) */
		if ((rc = mdb_shard_partition(ctx, plan, t, tab[t].keys, tab[t].nulls, tab[t].n, &regions[t], &cursors[t])))
			return rc;
	rc = mdb_shard_join(ctx, plan, regions, cursors, out_key, out_count, cap);	/* (world 1: what was sent is what arrived) */
	if (rc || (rc = gc_status_head(ctx, h)))
		return rc;
	if (!(*h)[MDB_STW_FLAGS])
		return GC_FORM_DONE;
	if (mdb_knob_set("MDB_DEBUG_UNORDERED"))
		fprintf(stderr, "any-order form not served: flags %u (k %u, b2 %u, rem %u)\n", (*h)[MDB_STW_FLAGS], plan->kbits, plan->b2, plan->rem);
	return ((*h)[MDB_STW_FLAGS] & MDB_ST_KEY_OUTSIDE) ? GC_FORM_KEY_OUTSIDE : GC_FORM_NOT_SERVED;
}

/* Groups in UNSPECIFIED order (the caller did not pass MDB_ORDER_FIRST and wants no first rows): nothing has to remember which
 * left row a group began with, so no row id travels through the partition levels and no ordering sort runs - the pipeline of the
 * sharded operator's receiver (mdb_dev_shard.hip) on this GPU's own first-level regions: 4-byte (or 2-byte) words of the k-bit
 * window hash for BOTH tables, counts per leaf, (key decoded from the table slot, COUNT) written where the leaf kernel finds it.
 * Window = the right table's sampled key range, padded like the compact form's; every right key is checked against it on the
 * device, left rows outside it join nothing.  10^8 x 10^8 unique keys: 1.5 ms of kernels where the ordered operator takes 2.56.
 * 0 = done, 1 = not served (window too wide, a key outside it, skew, a region overflow ...): the ordered operator answers. */
int gc_unordered_try(mdb_dev_ctx *ctx, const gc_sides &s, const gc_out &out, const gc_table *x, int nextra)
{
	if (s.l.n + s.r.n < (1ull << 21) || ctx->narrow_mode == 0 || ld_disabled() || nextra < 0 || 2 + nextra > MDB_SHARD_MAX_TABS)
		return 1;
	const gc_table tab[MDB_SHARD_MAX_TABS] = { s.l, s.r, nextra > 0 ? x[0] : gc_table{ NULL, NULL, 0 }, nextra > 1 ? x[1] : gc_table{ NULL, NULL, 0 } };
	mdb_shard_plan plan;
	const uint32_t *h = NULL;
	const int rc = gc_windowed_try(ctx, s, ctx->nh_distrust > 0, GC_WINDOW_RIGHT, false, [&](int64_t wlo, uint32_t kb) -> int {
		if (!ctx->sr_span_r || !ctx->sr_span_l)
			return GC_FORM_NOT_SERVED;
		return any_order_form(ctx, tab, 2u + (uint32_t)nextra, false, (int64_t)(ctx->sr_span_l + ctx->sr_span_l / 8), wlo, kb, out.key,
				      ctx->unordered_no_counts ? NULL : out.count, out.cap, &plan, &h);
	});
	if (rc)
		return rc;
	*out.groups = h[MDB_SHARD_STW_GROUPS];
	if (out.joined)
		*out.joined = (uint64_t)h[MDB_SHARD_STW_JOINED] | ((uint64_t)h[MDB_SHARD_STW_JOINED + 1] << 32);
	gc_plan_shape(ctx, 2, plan.b2 ? 2 : 1, 1, 1);
	return 0;
}

/* GROUP BY key + COUNT(*) of ONE column as (key, COUNT) pairs in unspecified order (include/mdb_dev.h): the any-order operator's
 * pipeline with the table in the right table's place and no left table - one first level of 2-byte words (two levels beyond
 * 2^27 values), every leaf slot with rows is a group.  1 = not served (NULL keys, keys beyond a 2^30-value window, skew that
 * overflows a region, small tables): the caller's ordered operator answers. */
extern "C" int mdb_dev_group_count_keys(mdb_dev_ctx *ctx, const int64_t *keys, const uint64_t *nullbits, uint64_t n, int64_t *out_key,
					int64_t *out_count, uint64_t cap, uint64_t *out_groups)
{
	mdb_plan_scope plan_scope(ctx);
	if (!ctx || !out_groups || !out_key || !out_count)
		return -MIDORIDB_ERROR;
	*out_groups = 0;
	if (nullbits || n < (1ull << 21) || ctx->narrow_mode == 0 || ld_disabled())
		return 1;
	mdb_memo_switch(ctx, keys, n, NULL, 0);
	const gc_table tab[2] = { { NULL, NULL, 0 }, { keys, NULL, n } };	/* (the column in the right table's place) */
	mdb_shard_plan plan;
	const uint32_t *h = NULL;
	const int rc = gc_windowed_try(ctx, { tab[1], tab[0] }, ctx->nh_distrust > 0, GC_WINDOW_BOTH, false, [&](int64_t wlo, uint32_t kb) -> int {
		return any_order_form(ctx, tab, 2, true, 0, wlo, kb, out_key, out_count, cap, &plan, &h);
	});
	if (!rc)
		*out_groups = h[MDB_SHARD_STW_GROUPS];
	return rc;
}
