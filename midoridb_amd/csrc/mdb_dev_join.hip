/*
 * mdb_dev_join.hip - the fused INNER JOIN + GROUP BY join key + COUNT(*) operator (north-star query): the staged driver - the plan of
 * an attempt (which key form, which leaf form, pruning: gc_choose_form), its arena (gc_arena_need), the stages of gc_begin / gc_finish,
 * the retries between attempts (group_count_common) - the split form for the multi-GPU exchange, the N-way form, and the entry points
 *
 *   mdb_dev_join_group_count[_multi | _begin / _finish | _i32]
 *   mdb_dev_group_count       GROUP BY key + COUNT(*) over one key column (fast paths: mdb_dev_groupby.hip)
 *   mdb_dev_explain_*         the plans as data, made by the same decision code
 *
 * The per-leaf kernels and their launchers live in mdb_dev_join_leaf.hip and mdb_dev_leaf_wide.hip, the key sample and the key-form
 * decision in mdb_dev_keyform.hip, the forms that answer before this driver (single workgroup, any order, mdb_dev_group_count_keys) in
 * mdb_dev_join_small.hip, the ordering of the group records in mdb_dev_order.hip, the materialising join (mdb_dev_join_pairs) in
 * mdb_dev_pairs.hip, the 4096-digit pass in mdb_dev_shard.hip; what the files share is mdb_dev_join_internal.h.
 *
 * Reference semantics reproduced (file:line = reference src/engine/executor_select.c):
 *   - a NULL join key matches nothing (:557-579)            -> NULL keys were dropped at level 0
 *   - N:M duplicates: every pair is a joined row (:1096-1141) -> COUNT = cntL * cntR per key
 *   - GROUP BY keeps the first row of each group, in order (:1542-1583)
 *                                                            -> groups ordered by first L position
 *   - join output is left-major / right-minor (:1096-1141)   -> pairs ordered by (pos_l, pos_r)
 */
#include "mdb_dev_join_internal.h"
#include "mdb_dev_rowjoin.h"

/* ------------------------------------------------------------------ compaction of the dense count array
 * (implemented in mdb_dev_filter.hip: predicate "count <> 0" -> ascending positions) */
size_t mdb_filter_arena_bytes(uint64_t n);
int mdb_filter_nonzero64(mdb_dev_ctx *ctx, const int64_t *vals, uint64_t n, uint32_t *out_sel, uint32_t **d_total);

/* ------------------------------------------------------------------ group-count drivers */

/* MDB_DIRECT_LEAF=0 keeps the compact narrow form off (A/B measurements, soaks of the hashed leaf kernel) */
bool ld_disabled(void)
{
	return mdb_knob_off("MDB_DIRECT_LEAF");
}

/* slots of the group-record list: every group once, plus the zero-filled gaps of the chunked reservation
 * (at most one leaf's worth per chunk, one unfinished chunk per workgroup) */
uint64_t gc_rec_capacity(mdb_dev_ctx *ctx, uint64_t n_l)
{
	return n_l + n_l / 4 + (uint64_t)(4 * ctx->num_cus + 4) * GC_REC_CHUNK + 4096;	/* two kernel instances, one open chunk per workgroup */
}

int gc_status_head(mdb_dev_ctx *ctx, const uint32_t **h)
{
	*h = reinterpret_cast<const uint32_t *>(ctx->h_pinned);
	MDB_HIP(ctx, hipMemcpyAsync(ctx->h_pinned, ctx->d_status, 16, hipMemcpyDeviceToHost, ctx->stream));
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return MIDORIDB_OK;
}

/* one call of the operator as its entry points prepare it: the tables, where the result goes, and the plan so far - the part that
 * group_count_common's retry loop edits between attempts */
struct gc_request {
	gc_table l, r;			/* (r.n: the rows announced, in the split form) */
	gc_out out;
	bool has_r, null_group;
	bool keys32;			/* both key columns are int32 arrays (received over xGMI in the 4-byte wire format) */
	int nextra;			/* further right tables on the same key (mdb_dev_join_group_count_multi) */
	gc_table x[GC_MAX_EXTRA];
	bool fast, records, no_build_r;
	gc_key_form kf;			/* narrow: 32-bit hashes, the left words carry the row ids; base: centre of the key window (mdb_partition_table);
					 * win: the compact window and the key sample's hints (gc_window) */
};

/* The operator runs in two halves so that a multi-GPU pipeline can partition the left table while the right table is still arriving over xGMI
 * (mdb_dev_join_group_count_begin / _finish).  The state of one attempt: its request - a copy: the split form finds it in ctx->pending_op after
 * begin() has returned, and gc_choose_form may take back what the request offers (rq.fast, rq.kf.narrow) - and what gc_begin makes of it */
struct gc_state {
	gc_request rq;
	bool active;
	bool defer_ok;		/* the caller runs gc_begin and gc_finish back to back: the left table may be partitioned in gc_finish */
	bool own_call;		/* begin and finish are the two halves of ONE operator call (not the split API): the first-level cursors and the ordering
				 * ranges' fills may live in the status block's counter area, cleared with it (MDB_ZERO_BLK_*) */
	uint32_t key_bits;	/* compact narrow form offered by the key sample: every key in [rq.kf.win.lo, rq.kf.win.lo + 2^key_bits) (0 = none) */
	bool direct;		/* ... taken: the leaves are joined by k_leaf_direct (decided in gc_choose_form, where the leaf count is known) */
	bool one_level;		/* ... by k_leaf_wide: ONE partition level of 9 bits, tables of 2^(key_bits - 9) entries */
	bool wide12;		/* ... by k_leaf_wide over the digits of ONE 4096-digit pass per table (mdb_scatter4096): key windows of 2^24 ... 2^27 values */
	bool defer_l;		/* the LEFT table is partitioned after the right one, in gc_finish (compact narrow form, unsplit call): the
				 * right table's first level records its exact key range, the left table's drops the rows outside */
	bool defer_l64;		/* the same in the 64-bit form (keys that fit no 2^32 window): min-max pruning on the raw keys */
	uint32_t semijoin;	/* != 0: the LEFT table is partitioned after the right one (gc_finish), its second level dropping the rows
				 * whose bit is clear in a bitmap of the right table's hashed keys; the value is log2 of the adjacent
				 * hashed values that share a bit, plus 1 */
	int b1, b2;
	mdb_part_result pl;
};

/* the state of one attempt from its request; own_call: begin and finish run back to back (gc_state.defer_ok, .own_call) */
static void gc_state_fill(gc_state *st, const gc_request &rq, bool own_call)
{
	memset(st, 0, sizeof(*st));
	st->rq = rq;
	st->key_bits = rq.kf.narrow ? rq.kf.win.kbits : 0u;
	st->defer_ok = own_call;
	st->own_call = own_call;
}

/* a remembered "these columns overflow the digit-per-workgroup leaves' counts" (VD_LW_BAD) serves MDB_BAD_SERVES calls */
static bool gc_lw_bad(mdb_dev_ctx *ctx, const gc_state *st)
{
	return ctx->vd[VD_LW_BAD].serve(st->rq.l.keys, st->rq.l.n, NULL, st->rq.r.n, MDB_BAD_SERVES);
}

/* the partition request of one of the operator's tables: the plan of this attempt, the key form (mdb_part_request.narrow) and its window */
static mdb_part_request gc_table_request(const gc_state *st, const int64_t *keys, const uint64_t *nulls, uint64_t n, int narrow)
{
	mdb_part_request rq;
	memset(&rq, 0, sizeof(rq));
	rq.keys = keys;
	rq.nullbits = nulls;
	rq.n = n;
	rq.keys32 = st->rq.keys32;
	rq.bits1 = st->b1;
	rq.bits2 = st->b2;
	rq.fast = st->rq.fast;
	rq.narrow = narrow;
	rq.narrow_base = st->direct ? st->rq.kf.win.lo : st->rq.kf.base;
	rq.narrow_kbits = st->direct ? st->key_bits : 0u;
	return rq;
}

/* the left table's first-level cursors in the status block's counter area, which an unsplit call has cleared (the right table's lie in front of them) */
static void gc_left_cursors(mdb_dev_ctx *ctx, const gc_state *st, mdb_part_request *rq)
{
	if (st->own_call) {
		rq->cursor0_ext = ctx->d_status + MDB_ZERO_BLK_OFF + MDB_ZERO_BLK_SLOT;
		rq->cursor0_ext_words = MDB_ZERO_BLK_SLOT;
	}
}

/* the form of this attempt: partition bits, which leaves (one_level, wide12, direct), what waits for the right table (defer_l, defer_l64,
 * semijoin).  Launches nothing, allocates nothing.  MIDORIDB_OK, GC_NOT_SERVED (further right tables that the form does not count) or an error */
static int gc_choose_form(mdb_dev_ctx *ctx, gc_state *st)
{
	mdb_choose_bits(st->rq.l.n, GC_TARGET, &st->b1, &st->b2);
	const bool lw_bad = gc_lw_bad(ctx, st);
	if (st->rq.kf.win.r_based && !(st->rq.has_r && st->defer_ok && !st->active && st->rq.fast))
		st->key_bits = 0;	/* (a window of the right table's keys only needs the left table pruned: not in this call - plain narrow form) */
	/* key windows of 2^15 ... 2^23 values: one 9-bit level and k_leaf_wide (MDB_ONE_LEVEL=0 switches it off; tables of fewer
	 * than 2^21 rows in all keep the two-level form, whose fixed costs are smaller) */
	st->one_level = st->rq.kf.narrow && st->key_bits >= 9u + LW_MIN_REM && st->key_bits <= 9u + LW_MAX_REM && st->rq.fast && st->rq.records &&
			!ld_disabled() && !lw_bad &&
			st->rq.l.n + (st->rq.has_r ? st->rq.r.n : 0) >= (1ull << 21) &&
			st->rq.l.n < 3000000000ull && st->rq.r.n < 3000000000ull &&
			!mdb_knob_off("MDB_ONE_LEVEL");
	if (st->rq.nextra)
		st->one_level = false;	/* (further right tables: the two-level direct-address kernel counts them) */
	/* key windows of 2^24 ... 2^27 values (10^8 unique keys: variants U and S): what two 9-bit levels and k_leaf_direct did - the left
	 * table's 8-byte words written and read twice - is ONE 4096-digit pass per table (2-byte words for the right table, 4-byte row words
	 * for the left one) and k_leaf_wide12 over digits of up to 2^15 values.  Unsplit calls of a two-table join over int64 columns, at
	 * most 2^27 left rows (the leaf keeps a first row in 27 bits) and region capacities the leaf's registers hold; from 2^24 rows in all
	 * (measured equal to the two-level form at 8 * 10^6 rows per table, 15 % faster at 10^8: profiles/micro/one_pass_4096_sweep.py;
	 * MDB_WIDE12_MIN=<rows> moves the threshold, MDB_WIDE12=0 switches the form off) */
	{
		const long long min_knob = mdb_knob_int("MDB_WIDE12_MIN", 0);
		const uint64_t min_rows = min_knob > 0 ? (uint64_t)min_knob : (1ull << 24);
		st->wide12 = !st->one_level && st->rq.kf.narrow && st->rq.has_r && st->key_bits > 9u + LW_MAX_REM && st->key_bits <= 12u + LW_MAX_REM + 1u && st->rq.fast &&
			     st->rq.records && !ld_disabled() && st->defer_ok && !st->active && st->rq.nextra <= 1 && !st->rq.keys32 &&
			     !st->rq.kf.win.prunable /* (a right table that covers part of the left table's key range: min-max pruning drops most left rows first) */ &&
			     !lw_bad &&
			     st->rq.l.n + st->rq.r.n >= min_rows && st->rq.l.n <= (1ull << 27) /* (k_leaf_wide12 keeps a first row in 27 bits) */ &&
			     st->rq.r.n < 0xF0000000ull && !mdb_knob_off("MDB_WIDE12");
		/* ... and a digit's words must fit the leaf kernel's registers: 8 sub-regions of at most LW12_LB (LW12_RB) chunks per thread */
		if (st->wide12 && !leaf_wide12_fits(ctx, st->rq.l.n, st->rq.r.n, st->rq.nextra ? st->rq.x[0].n : 0))
			st->wide12 = false;
	}
	if (st->wide12) {
		st->b1 = 12;
		st->b2 = 0;
	}
	if (st->one_level) {
		st->b1 = st->key_bits <= 15u ? 8 : 9;	/* (a 2^15-value window: 256 regions of 128 values - see gc_window.fast1) */
		st->b2 = 0;
	} else if (st->rq.kf.win.fast1) {
		st->rq.fast = false;	/* (two fast levels: leaves of one or two values with thousands of rows each - regions would overflow) */
	}
	/* the narrow form of a join needs the right side's 4-byte layout (two fast levels); plain GROUP BY has no such limit */
	if (!st->one_level && !st->wide12 && st->rq.kf.narrow && st->rq.has_r && !mdb_partition_w32_applies(st->rq.r.n, st->b1, st->b2, st->rq.fast))
		st->rq.kf.narrow = false;
	/* compact narrow form + direct-address leaves: what the partition leaves of the key_bits-wide hash must index a table
	 * of at most 2^LD_MAX_REM entries; fewer than 2^4 would mean leaves of a handful of keys with thousands of rows each
	 * (same-address LDS atomics: the hashed kernel's wave-level merging handles those better) */
	st->direct = st->rq.kf.narrow && st->key_bits && st->rq.fast && st->b2 > 0 && st->rq.records && !ld_disabled() &&
		     st->key_bits >= (uint32_t)(st->b1 + st->b2) + 4u && st->key_bits <= (uint32_t)(st->b1 + st->b2) + LD_MAX_REM;
	if (st->one_level || st->wide12)
		st->direct = true;
	if (st->rq.nextra && !(st->direct && st->rq.has_r && st->rq.fast))
		return GC_NOT_SERVED;
	if (st->direct && !st->one_level && !st->wide12) {
		/* the direct-address kernel has no table to overflow and pays a fixed price per leaf (three barriers, the emit scan):
		 * it prefers FEWER, larger leaves than the hashed kernel's 3833-slot table allows - tables of 2^LD_MAX_REM entries when
		 * the second level has the bits to give (10^8 x 10^8 rows: 2^15 leaves of 2 x 3052 rows instead of 2^16; second-level
		 * fan-out 128: -4 % on its scatter kernels as well). */
		/* (further right tables take 4 more bytes of LDS per entry each: tables of 2^11 entries keep three workgroups on a CU -
		 * three tables of 10^8 rows: leaf kernel 0.72 -> 0.52 ms) */
		const uint32_t want = st->rq.nextra ? LD_MAX_REM - 1u : LD_MAX_REM;
		while (st->b2 > 1 && st->key_bits - (uint32_t)(st->b1 + st->b2) < want &&
		       (1u << (st->b1 + st->b2 - 1)) >= 16u * (uint32_t)ctx->num_cus)	/* ... while every workgroup still has leaves to walk */
			st->b2--;
	}
	/* two 9-bit levels give at most 2^18 leaves; a leaf's LDS hash table holds GC_SLOTS distinct keys.  The direct-address
	 * kernel has no such table (its leaves hold whatever rows share 2^rem key values): 10^9 x 10^9 rows of surrogate keys run
	 * on one GPU */
	if (!st->direct && (st->rq.l.n >> (st->b1 + st->b2)) > (uint64_t)GC_SLOTS * 7 / 10)
		return mdb_set_err(ctx, -MIDORIDB_ERROR,
				   "%llu build rows exceed what one GPU shard groups in LDS (about %llu): partition the tables across GPUs "
				   "(mdb_dev_partition_by_dest)",
				   (unsigned long long)st->rq.l.n, (unsigned long long)(((uint64_t)GC_SLOTS * 7 / 10) << (2 * MDB_MAX_RADIX_BITS)));
	/* Semi-join filter: when the key sample says that most left rows have no partner (a fact table joined with a
	 * dimension that covers part of its key range - the benchmark's variant D: 1 row in 16), the right table is
	 * partitioned FIRST, its hashed keys become a bitmap (k_leaf_bitmap: one contiguous slice per leaf), and the second
	 * partition level of the left table drops every row whose bit is clear before it is ranked and written: that level's
	 * writes and the leaf kernel's reads shrink to the rows that may have a partner.  The slice of a first-level digit
	 * (<= 32 KiB: one bit per 2^c adjacent hashed values when the window is wide) is staged in LDS per tile; the first level
	 * cannot filter - its rows are in table order, a lookup there costs a 128-byte line from L2 per row (measured: slower).
	 * A wrong hint costs time, never results.  MDB_SEMIJOIN=0 switches it off, MDB_SEMIJOIN_SLICE=<log2 bits> sizes the slice. */
	/* Min-max pruning, when the call is not split and the key sample says the right table's keys do not cover the left
	 * table's whole range (or a bitmap is wanted, which also needs the right table first): the right table goes first and its first partition level
	 * records the exact range of its keys (a pair of stores per tile, reduced by one small kernel); the left table's first level reads the two words
	 * from device memory and drops every row outside - the classic dimension-range pruning of a fact table, exact, at the
	 * price of one compare per row.  Where it removes most left rows (the right table's SPAN is small: by_span) the bitmap
	 * below would filter nothing more and is not built. */
	char prune_env[2];		/* MDB_MINMAX_PRUNE - 0: never, 2: whatever the key sample says (tests) */
	mdb_knob_str("MDB_MINMAX_PRUNE", prune_env, sizeof(prune_env));
	st->defer_l = st->rq.kf.narrow && st->rq.fast && (st->b2 > 0 || st->one_level) && st->rq.has_r && st->defer_ok && !st->active &&
		      (st->rq.kf.win.prunable || (st->direct && st->rq.kf.win.selective) || prune_env[0] == '2') && prune_env[0] != '0';
	/* ... and in the 64-bit form (hashes, snowflake ids: keys beyond every 2^32 window) just the same - the range test does not
	 * care how wide the keys are: the right table's first level records the smallest and the largest KEY, the left table's drops
	 * the rows outside before they are hashed, ranked or written (12 bytes per row and level in this form) */
	st->defer_l64 = !st->rq.kf.narrow && st->rq.fast && st->b2 > 0 && st->rq.has_r && st->defer_ok && !st->active && !st->rq.nextra && !st->rq.keys32 &&
			(st->rq.kf.win.prunable || prune_env[0] == '2') && prune_env[0] != '0';
	st->semijoin = 0;
	if (st->defer_l && st->direct && !st->one_level && st->rq.kf.win.selective && !st->rq.kf.win.by_span) {
		const long long slice = mdb_knob_int("MDB_SEMIJOIN_SLICE", 0);
		const uint32_t slice_max = slice >= 7 && slice <= 18 ? (uint32_t)slice : 17u;	/* log2 bits: 2^17 = 16 KiB */
		const uint32_t below0 = st->key_bits - (uint32_t)st->b1;		/* hash bits below the first-level digit */
		const uint32_t coarse = below0 > slice_max ? below0 - slice_max : 0u;
		const uint32_t rem = st->key_bits - (uint32_t)(st->b1 + st->b2);
		if (!mdb_knob_off("MDB_SEMIJOIN") && coarse <= 3u && rem >= coarse + 5u && below0 - coarse >= 7u)
			st->semijoin = coarse + 1u;
	}
	return MIDORIDB_OK;
}

/* the bytes of scratch arena the attempt takes, stage by stage */
static size_t gc_arena_need(mdb_dev_ctx *ctx, const gc_state *st)
{
	size_t need = st->wide12 ? mdb_scatter4096_arena_bytes(ctx, st->rq.l.n, true)
		      : st->one_level ? mdb_partition_level0_arena_bytes(st->rq.l.n, st->b1, st->rq.kf.win.fast1) : mdb_partition_arena_bytes(st->rq.l.n, st->b1, st->b2, true, st->rq.fast);
	if (st->semijoin)
		need += mdb_align_up(((size_t)1 << (st->key_bits - (st->semijoin - 1u))) / 8) + 4096;
	if (st->one_level && st->rq.has_r) {	/* (k_leaf_wide4's ranged emit: the ordering kernel's ranges, filled by the leaf kernel - tables of up to 1536 ranges) */
		const size_t ranges = (st->rq.l.n >> ORDER_RANGE_BITS) + 2 < 1538 ? (size_t)(st->rq.l.n >> ORDER_RANGE_BITS) + 2 : 1538;
		need += mdb_align_up(ranges * ORDER_RANGE_CAP * 8) + mdb_align_up(ranges * 4) + 512;
	}
	if (st->defer_l)
		need += mdb_align_up(mdb_part_minmax_words(st->rq.r.n) * 4) + 256;
	if (st->defer_l64)
		need += mdb_align_up(mdb_part_minmax_words(st->rq.r.n) * 8) + 256;
	if (st->rq.has_r)
		need += st->wide12 ? mdb_scatter4096_arena_bytes(ctx, st->rq.r.n, false)
		      : st->one_level ? mdb_partition_level0_arena_bytes(st->rq.r.n, st->b1)
				      : mdb_partition_arena_bytes(st->rq.r.n, st->b1, st->b2, false, st->rq.fast);
	for (int x = 0; x < st->rq.nextra; x++)
		need += st->wide12 ? mdb_scatter4096_arena_bytes(ctx, st->rq.x[x].n, false) : mdb_partition_arena_bytes(st->rq.x[x].n, st->b1, st->b2, false, st->rq.fast) + 512;
	{
		uint32_t kb = 0;
		int s1 = 0, s2 = 0;
		need += mdb_align_up(gc_rec_capacity(ctx, st->rq.l.n) * 8) + mdb_align_up(st->rq.l.n * 4) + 4096;
		need += leaf_hot_arena_bytes();	/* hot-key path (only touched when needed) */
		if (st->rq.records && order_bits(st->rq.l.n, &kb, &s1, &s2))
			need += mdb_partition_raw_arena_bytes(gc_rec_capacity(ctx, st->rq.l.n), s1, s2, 1u << (kb - (uint32_t)(s1 + s2)), true,
							      order_digits0(st->rq.l.n, kb, s1), (uint64_t)1 << (kb - (uint32_t)s1)) +
				mdb_partition_raw_arena_bytes(gc_rec_capacity(ctx, st->rq.l.n), s1, s2, 1u << (kb - (uint32_t)(s1 + s2)), false, 0) +
				2 * (((size_t)1 << (s1 + s2)) + 4096) * 8;
		else
			need += mdb_filter_arena_bytes(st->rq.l.n);
	}
	if (st->wide12 && st->rq.nextra <= 1)	/* (the groups as one bit per left row + exceptions, mdb_dev_dense.hip) */
		need += mdb_dense_arena_bytes(st->rq.l.n) + mdb_align_up((st->rq.l.n / 8 + 4096) * 8);
	return need;
}

/* first half: choose the form, size and claim the scratch arena, clear the status words, partition the left table */
static int gc_begin(mdb_dev_ctx *ctx, gc_state *st)
{
	int rc = gc_choose_form(ctx, st);
	if (rc)
		return rc;
	const size_t need = gc_arena_need(ctx, st);
	if (ctx->explaining) {	/* (mdb_dev_explain_*: the plan is made - no arena, no launch) */
		ctx->plan.arena_mib = (uint32_t)((need + (1u << 20) - 1) >> 20);
		return GC_EXPLAINED;
	}
	rc = mdb_arena_begin(ctx, need);
	if (rc)
		return rc;
	/* d_status u32 words: [0] flags (bit 0 leaf table overflow, bit 1 fast-layout region overflow, bit 2
	 * COUNT too large for a record), [1] record count, [2..3] joined rows (u64), [4..7] NULL-group stats */
	if (st->own_call && !st->wide12) {
		/* the status words and, behind them, the counters this call's kernels start from zero: one fill for all of them */
		MDB_HIP(ctx, hipMemsetAsync(ctx->d_status, 0, ((size_t)MDB_ZERO_BLK_OFF + MDB_ZERO_BLK_WORDS) * 4, ctx->stream));
	} else {
		MDB_HIP(ctx, hipMemsetAsync(ctx->d_status, 0, 16 * sizeof(uint32_t), ctx->stream));
	}
	if (!st->defer_l && !st->defer_l64 && !st->wide12) {
		mdb_part_request rq = gc_table_request(st, st->rq.l.keys, st->rq.l.nulls, st->rq.l.n, st->rq.kf.narrow ? 1 : 0);
		rq.want_rid = !st->rq.kf.narrow;
		rq.level0_only = st->one_level;
		rq.loose = st->one_level && st->rq.kf.win.fast1;
		if (st->one_level)
			gc_left_cursors(ctx, st, &rq);
		rc = mdb_partition_table(ctx, rq, &st->pl);
		if (rc)
			return rc;
	}
	st->active = true;
	return MIDORIDB_OK;
}

/* ---- decisions that only a caller's statistics open (mdb_dev_call_stats), shared by the operator and by mdb_dev_explain_join_group_count */
/* one-level joins: the groups are few enough (a group needs a right key: at most as many as values in the right column's range) for the
 * ordering kernel's ranges - k_leaf_wide4 writes its records straight into them on the FIRST call */
static bool gc_ranged_by_stats(const mdb_dev_ctx *ctx, const int64_t *keys_l, const int64_t *keys_r, uint64_t n_l, uint64_t n_r, uint32_t kbits, uint32_t *rg_n)
{
	if (!(ctx->cs_on && !ctx->explain_as_sample && ctx->cs_kl == keys_l && ctx->cs_has_r && ctx->cs_kr == keys_r && ctx->cs_r.min <= ctx->cs_r.max))
		return false;
	const uint64_t span_r = (uint64_t)ctx->cs_r.max - (uint64_t)ctx->cs_r.min + 1;
	uint64_t bound = span_r && span_r < n_r ? span_r : n_r;
	bound = bound < n_l ? bound : n_l;
	return order_ranges_apply(n_l, kbits, bound, rg_n);
}

/* the one-pass 4096-digit join of two tables: no key twice in the left column, none twice in the right one (MDB_COL_DISTINCT, measured at
 * ingest), and the right column holds EVERY value of its range, which covers the left column's - every left row is a group of COUNT 1,
 * whatever the statement before this one was: the groups leave as one bit per left row without a pilot launch and its host round trip */
static bool gc_bits_by_stats(const mdb_dev_ctx *ctx, int nextra, const int64_t *keys_l, const int64_t *keys_r, uint64_t n_r)
{
	return !nextra && ctx->dn_distrust == 0 && ctx->cs_on && !ctx->explain_as_sample && ctx->cs_kl == keys_l && ctx->cs_has_r && ctx->cs_kr == keys_r &&
	       (ctx->cs_l.flags & MDB_COL_DISTINCT) && (ctx->cs_r.flags & MDB_COL_DISTINCT) && !ctx->cs_r.nulls && ctx->cs_r.min <= ctx->cs_r.max &&
	       (uint64_t)ctx->cs_r.max - (uint64_t)ctx->cs_r.min + 1 == n_r && ctx->cs_l.min >= ctx->cs_r.min && ctx->cs_l.max <= ctx->cs_r.max;
}

/* whether the bit-per-row form of the groups may be asked at all (every left row must reach the leaf kernel for its bit to be looked at) */
static bool gc_bits_possible(const gc_state *st, bool records, bool has_r, uint64_t cap, uint64_t n_l)
{
	return st->wide12 && st->rq.nextra <= 1 && records && has_r && cap && n_l >= ((uint64_t)1 << 22) && !st->rq.l.nulls && !st->rq.kf.win.r_based &&
	       !mdb_knob_off("MDB_JOIN_BITS");
}

/* the shape of the plan gc_begin made, in the plan record: written at the end of gc_finish and by gc_explain_fill */
static void gc_plan_note(mdb_dev_ctx *ctx, const gc_state *st)
{
	struct mdb_dev_plan_info *o = &ctx->plan;
	o->key_form = st->direct ? 2u : (st->rq.kf.narrow ? 1u : 0u);
	o->key_bits = st->direct ? st->key_bits : 0u;
	o->levels = (st->one_level || st->wide12) ? 1u : 2u;
	o->digits = st->wide12 ? 4096u : 512u;
	o->minmax_pruned = (st->defer_l || st->defer_l64) ? 1u : 0u;
	o->semijoin = st->semijoin;
	o->multi_one_pass = st->rq.nextra ? 1u : 0u;
}

/* mdb_dev_explain_join_group_count: the plan gc_begin has just made, as mdb_dev_last_plan would report it after the run */
static void gc_explain_fill(mdb_dev_ctx *ctx, const gc_state *st)
{
	struct mdb_dev_plan_info *o = &ctx->plan;
	uint32_t kbits = 0, rg_n = 0;
	int sb1 = 0, sb2 = 0;
	const bool records = st->rq.records && order_bits(st->rq.l.n, &kbits, &sb1, &sb2);
	gc_plan_note(ctx, st);
	mdb_explain_sampled(ctx);
	const bool w16 = st->one_level && st->rq.has_r && !mdb_knob_off("MDB_WORDS16");
	const bool leaf4 = st->one_level && st->rq.has_r && w16 && records && !st->rq.null_group && st->rq.l.n <= (1ull << 27) && st->key_bits >= (uint32_t)st->b1 + 10u;
	o->ranged_order = leaf4 && gc_ranged_by_stats(ctx, st->rq.l.keys, st->rq.r.keys, st->rq.l.n, st->rq.r.n, kbits, &rg_n) ? 1u : 0u;
	if (gc_bits_possible(st, records, st->rq.has_r, st->rq.out.cap, st->rq.l.n))
		o->groups_as_bits = gc_bits_by_stats(ctx, st->rq.nextra, st->rq.l.keys, st->rq.r.keys, st->rq.r.n) ? 3u : 1u /* (a pilot launch decides) */;
}

/* ---- gc_finish, the operator's second half, in stages.  They share this record of what one attempt has decided and made so far. */
struct gc_run {
	gc_state *st;
	gc_table r;			/* the right table */
	gc_out out;
	bool build_r;			/* hash table on the side with fewer rows per leaf (the leaves are sized by the left table) */
	mdb_part_result pl, pr, px[GC_MAX_EXTRA];
	bool records;			/* record mode (the groups sorted by first row id); false: dense mode, the fallback */
	uint32_t kbits;
	int sb1, sb2;
	unsigned long long *rec;
	int64_t *dense;
	uint32_t *sel;
	gc_args a;
	uint32_t keyed_cbits;
	bool leaf4;			/* one-level join through k_leaf_wide4 */
	bool ranged;			/* ... that writes its records into the ordering kernel's ranges */
	uint32_t rg_n;
	bool ordered_early;		/* order_presorted was launched behind the leaf kernel, before the status came back */
	bool tail_queued;		/* ... and the host has waited for the status alone: that kernel may still be running (gc_read_status) */
	unsigned long long *dn_bits;	/* != NULL: the groups leave as one bit per left row */
	gc_readback *rb;		/* the status words as last read back (ctx->h_pinned + MDB_HP_STATUS) */
	uint32_t dn_cleared, dn_exceptions;
	uint64_t G, list_len;
};

/* stage 1a: both tables (and a further right one) through one 4096-digit pass each; a key outside the window is reported (the left table's, when the
 * window was taken from the right table's keys alone, is dropped: it has no partner) */
static int gc_partition_wide12(mdb_dev_ctx *ctx, gc_run *g)
{
	gc_state *st = g->st;
	int rc;
	if (g->r.n > st->rq.r.n)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "right table larger than announced at begin()");
	void *rb = NULL, *lb = NULL;
	uint32_t *rcur = NULL, *lcur = NULL;
	const uint32_t cap_r = mdb_scatter4096_cap(ctx, g->r.n, false), cap_l = mdb_scatter4096_cap(ctx, st->rq.l.n, true);
	const uint32_t rel_hi = (uint32_t)((1ull << st->key_bits) - 1ull);
	rc = mdb_scatter4096(ctx, g->r.keys, g->r.nulls, g->r.n, st->rq.kf.win.lo, st->key_bits, true, 0u, cap_r, false, "part_scatter_wide12_r", &rb, &rcur);
	if (rc)
		return rc;
	rc = mdb_scatter4096(ctx, st->rq.l.keys, st->rq.l.nulls, st->rq.l.n, st->rq.kf.win.lo, st->key_bits, !st->rq.kf.win.r_based, rel_hi, cap_l, true, "part_scatter_wide12_l", &lb, &lcur);
	if (rc)
		return rc;
	memset(&g->pl, 0, sizeof(g->pl));
	g->pl.hv = (uint64_t *)lb;
	g->pl.leaf_cnt = lcur;
	g->pl.leaf_cap = cap_l;
	g->pr.hv = (uint64_t *)rb;
	g->pr.leaf_cnt = rcur;
	g->pr.leaf_cap = cap_r;
	g->pl.nleaves = g->pr.nleaves = 4096u;
	g->pl.bits_total = g->pr.bits_total = 12u;
	g->pl.nsub = g->pr.nsub = 8u;
	g->pl.w32 = g->pr.w32 = true;
	g->pr.w16 = true;
	if (st->rq.nextra) {
		/* the further right table like the first one; its keys outside the window are dropped, not reported: the window holds every key of
		 * the left table, so such a key joins nothing */
		void *xb = NULL;
		uint32_t *xcur = NULL;
		const uint32_t cap_x = mdb_scatter4096_cap(ctx, st->rq.x[0].n, false);
		rc = mdb_scatter4096(ctx, st->rq.x[0].keys, st->rq.x[0].nulls, st->rq.x[0].n, st->rq.kf.win.lo, st->key_bits, false, rel_hi, cap_x, false, "part_scatter_wide12_r", &xb, &xcur);
		if (rc)
			return rc;
		g->px[0].hv = (uint64_t *)xb;
		g->px[0].leaf_cnt = xcur;
		g->px[0].leaf_cap = cap_x;
	}
	return MIDORIDB_OK;
}

/* stage 1b: the right table through the radix levels; where the left table waits for it, it leaves its key range behind (min-max pruning) */
static int gc_partition_right(mdb_dev_ctx *ctx, gc_run *g)
{
	gc_state *st = g->st;
	if (g->r.n > st->rq.r.n)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "right table larger than announced at begin()");
	if (st->rq.kf.narrow && !st->one_level && !mdb_partition_w32_applies(g->r.n, st->b1, st->b2, st->rq.fast))
		return GC_RETRY_WIDE;	/* split form: the left side was prepared narrow for a right table of another size */
	mdb_part_request rq = gc_table_request(st, g->r.keys, g->r.nulls, g->r.n, st->rq.kf.narrow ? 2 : 0);
	rq.level0_only = st->one_level;
	rq.out16 = st->one_level && !mdb_knob_off("MDB_WORDS16");
	if (st->own_call && (st->defer_l || st->one_level || st->defer_l64)) {
		rq.cursor0_ext = ctx->d_status + MDB_ZERO_BLK_OFF;
		rq.cursor0_ext_words = MDB_ZERO_BLK_SLOT;
	}
	if (st->defer_l) {
		rq.minmax_out = ctx->d_status + GC_STW_MINMAX;
		rq.minmax_tiles = (uint32_t *)mdb_arena_take(ctx, mdb_part_minmax_words(g->r.n) * 4);
		if (!rq.minmax_tiles)
			return -MIDORIDB_INTERNAL;
	}
	if (st->defer_l64) {
		rq.minmax64_out = reinterpret_cast<long long *>(ctx->d_status + GC_STW_MINMAX64);
		rq.minmax64_tiles = (unsigned long long *)mdb_arena_take(ctx, mdb_part_minmax_words(g->r.n) * 8);
		if (!rq.minmax64_tiles)
			return -MIDORIDB_INTERNAL;
	}
	return mdb_partition_table(ctx, rq, &g->pr);
}

/* stage 1c: the further right tables, partitioned exactly like the first: same window, same bits, 4-byte words.  Their keys outside the window are
 * dropped, not reported: the window holds every key of the left table (or of the first right table, with the left one pruned to it), so such a
 * key joins nothing */
static int gc_partition_extras(mdb_dev_ctx *ctx, gc_run *g)
{
	gc_state *st = g->st;
	uint32_t *h = reinterpret_cast<uint32_t *>(ctx->h_pinned + MDB_HP_SEND_RANGE);
	h[0] = 0u;
	h[1] = st->key_bits >= 32u ? 0xFFFFFFFFu : ((1u << st->key_bits) - 1u);
	MDB_HIP(ctx, hipMemcpyAsync(ctx->d_status + GC_STW_WINDOW, h, 8, hipMemcpyHostToDevice, ctx->stream));
	for (int x = 0; x < st->rq.nextra; x++) {
		if (!mdb_partition_w32_applies(st->rq.x[x].n, st->b1, st->b2, st->rq.fast))
			return GC_NOT_SERVED;
		mdb_part_request rq = gc_table_request(st, st->rq.x[x].keys, st->rq.x[x].nulls, st->rq.x[x].n, 2);
		rq.narrow_base = st->rq.kf.win.lo;
		rq.narrow_kbits = st->key_bits;
		rq.range_in = ctx->d_status + GC_STW_WINDOW;
		int rc = mdb_partition_table(ctx, rq, &g->px[x]);
		if (rc)
			return rc;
		if (!g->px[x].w32 || !g->px[x].leaf_cap || !g->px[x].leaf_cnt || g->px[x].nleaves != (1u << (st->b1 + st->b2)))
			return GC_NOT_SERVED;
	}
	return MIDORIDB_OK;
}

/* stage 1d: the left table where it waited for the right one - pruned to the right table's key range (64-bit form, or narrow form), or filtered
 * through a bitmap of the right table's hashed keys (semi-join) */
static int gc_partition_left(mdb_dev_ctx *ctx, gc_run *g, bool form64)
{
	gc_state *st = g->st;
	mdb_part_request rq = gc_table_request(st, st->rq.l.keys, st->rq.l.nulls, st->rq.l.n, form64 ? 0 : 1);
	int rc;
	if (form64) {
		rq.want_rid = true;
		rq.range64_in = reinterpret_cast<const long long *>(ctx->d_status + GC_STW_MINMAX64);
		rq.expect_pruned = st->rq.kf.win.by_span;
		rc = mdb_partition_table(ctx, rq, &st->pl);
	} else if (!st->semijoin) {
		rq.range_in = ctx->d_status + GC_STW_MINMAX;
		rq.expect_pruned = st->rq.kf.win.by_span && !st->one_level;
		/* (a key sample's guess keeps the general first level: what the last join over these columns delivered, or the caller's statistics) */
		rq.selective = st->rq.kf.win.selective && (gc_learned_selective(ctx, { st->rq.l, g->r }) ||
						 (ctx->cs_on && !ctx->explain_as_sample && ctx->cs_kl == st->rq.l.keys && ctx->cs_has_r && ctx->cs_kr == g->r.keys));
		rq.level0_only = st->one_level;
		gc_left_cursors(ctx, st, &rq);
		rc = mdb_partition_table(ctx, rq, &st->pl);
	} else {
		/* the right table's hashed keys as a bitmap, then the left table through it */
		const mdb_part_result &pr = g->pr;
		const uint32_t coarse = st->semijoin - 1u, rem = st->key_bits - (uint32_t)(st->b1 + st->b2);
		const size_t bytes = ((size_t)1 << (st->key_bits - coarse)) / 8;
		uint32_t *bits = (uint32_t *)mdb_arena_take(ctx, bytes);
		if (!bits)
			return -MIDORIDB_INTERNAL;
		if (!pr.leaf_cap || !pr.w32)
			return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "semi-join filter: the right table is not in the 4-byte fixed-capacity layout");
		if ((rc = leaf_bitmap_launch(ctx, reinterpret_cast<const uint32_t *>(pr.hv), pr.leaf_cnt, pr.leaf_cap, pr.nleaves, rem, coarse, 32u - st->key_bits, bits)))
			return rc;
		rq.narrow_base = st->rq.kf.win.lo;
		rq.narrow_kbits = st->key_bits;
		rq.range_in = ctx->d_status + GC_STW_MINMAX;
		rq.expect_pruned = st->rq.kf.win.by_span;
		rq.bits = bits;
		rq.words = 1u << (st->key_bits - (uint32_t)st->b1 - coarse - 5u);
		rq.shift = 32u - st->key_bits + coarse;
		rc = mdb_partition_table(ctx, rq, &st->pl);
	}
	if (!rc)
		g->pl = st->pl;
	return rc;
}

/* stage 1: every table that gc_begin has not partitioned, in the order the stream needs them */
static int gc_partition(mdb_dev_ctx *ctx, gc_run *g)
{
	gc_state *st = g->st;
	int rc;
	if (st->wide12 && (rc = gc_partition_wide12(ctx, g)))
		return rc;
	if (st->rq.has_r && !st->wide12 && (rc = gc_partition_right(ctx, g)))
		return rc;
	if (st->defer_l64 && (rc = gc_partition_left(ctx, g, true)))
		return rc;
	if (st->rq.nextra && !st->wide12 && (rc = gc_partition_extras(ctx, g)))
		return rc;
	if (((st->defer_l && !st->semijoin) || st->semijoin) && (rc = gc_partition_left(ctx, g, false)))
		return rc;
	return MIDORIDB_OK;
}

/* stage 2a: the result's buffers - record mode (sort the groups by first row id) or dense mode (fallback) - and the leaf kernels' arguments as far
 * as the partitioned tables fix them */
static int gc_args_begin(mdb_dev_ctx *ctx, gc_run *g)
{
	gc_state *st = g->st;
	const uint64_t n_l = st->rq.l.n;
	g->records = st->rq.records && order_bits(n_l, &g->kbits, &g->sb1, &g->sb2);
	g->sel = (uint32_t *)mdb_arena_take(ctx, n_l * 4);
	if (g->records)
		g->rec = (unsigned long long *)mdb_arena_take(ctx, gc_rec_capacity(ctx, n_l) * 8);
	else
		g->dense = (int64_t *)mdb_arena_take(ctx, n_l * 8);
	if (!g->sel || (!g->rec && !g->dense))
		return -MIDORIDB_INTERNAL;
	if (g->dense)
		MDB_HIP(ctx, hipMemsetAsync(g->dense, 0, n_l * 8, ctx->stream));
	gc_args &a = g->a;
	a.hv_l = g->pl.hv;
	a.rid_l = g->pl.rid;
	a.off_l = g->pl.leaf_off;
	a.cnt_l = g->pl.leaf_cnt;
	a.cap_l = g->pl.leaf_cap;
	a.hv_r = g->pr.hv;
	a.off_r = g->pr.leaf_off;
	a.cnt_r = g->pr.leaf_cnt;
	a.cap_r = g->pr.leaf_cap;
	a.dense_cnt = g->dense;
	a.dense_n = (uint32_t)n_l;
	a.rec = g->rec;
	a.rec_count = ctx->d_status + GC_STW_LIST_LEN;
	a.rec_valid = ctx->d_status + GC_STW_RECORDS;
	a.rec_cap = g->records ? (uint32_t)gc_rec_capacity(ctx, n_l) : 0;
	a.kbits = g->records ? g->kbits : 0;
	a.joined = (unsigned long long *)(ctx->d_status + GC_STW_JOINED);
	a.status = ctx->d_status;
	a.nleaves = g->pl.nleaves;
	a.nextra = (uint32_t)st->rq.nextra;
	for (int x = 0; x < GC_MAX_EXTRA; x++) {
		a.hv_x[x] = x < st->rq.nextra ? reinterpret_cast<const uint32_t *>(g->px[x].hv) : NULL;
		a.cnt_x[x] = x < st->rq.nextra ? g->px[x].leaf_cnt : NULL;
		a.cap_x[x] = x < st->rq.nextra ? g->px[x].leaf_cap : 0u;
	}
	a.narrow = st->rq.kf.narrow ? 1u : 0u;
	/* 4096 sampled keys with fewer than 4050 distinct values among them: at most a few 10^5 distinct values in the column */
	a.merge_all = (!st->rq.has_r && ctx->vd[VD_DISTINCT].holds(st->rq.l.keys, n_l, NULL, 0) && ctx->gh_distinct < 4050u) ? 1u : 0u;
	/* hot = far above the side's average leaf: a much larger probe table spread evenly over the leaves is not skew */
	const uint64_t nleaves = g->pl.nleaves ? g->pl.nleaves : 1;
	const uint64_t avg_l = n_l / nleaves, avg_r = st->rq.has_r ? g->r.n / nleaves : 0;
	const uint64_t hl = 8 * avg_l > GC_HEAVY ? 8 * avg_l : GC_HEAVY, hr = 8 * avg_r > GC_HEAVY ? 8 * avg_r : GC_HEAVY;
	a.heavy_l = hl > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)hl;
	a.heavy_r = hr > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)hr;
	return MIDORIDB_OK;
}

/* stage 2b: the form of the group records - keyed, 4-byte, written into the ordering ranges - from what the context remembers of these columns */
static int gc_choose_records(mdb_dev_ctx *ctx, gc_run *g)
{
	gc_state *st = g->st;
	gc_args &a = g->a;
	const mdb_part_result &pl = g->pl, &pr = g->pr;
	const int64_t *keys_l = st->rq.l.keys, *keys_r = g->r.keys;
	const uint64_t n_l = st->rq.l.n, n_r = g->r.n;
	const bool has_r = st->rq.has_r, records = g->records;
	const uint32_t kbits = g->kbits;
	/* keyed records (see gc_args.keyed_cbits) when the join is selective - few groups, their first rows scattered over the left
	 * table - and a COUNT(*) of at least 4 bits fits beside the row id and the hashed key (10 bits at 10^8 rows, 27 key bits);
	 * a COUNT that does not fit is reported by the kernel and the operator redone with plain records (and remembered).
	 * MDB_KEYED_RECORDS=0 switches them off */
	g->keyed_cbits = 0;
	if (st->direct && has_r && !st->rq.nextra && st->rq.kf.win.selective && records && !ctx->keyed_distrust && pl.leaf_cap && pr.leaf_cap && kbits >= 13 &&
	    kbits + st->key_bits + 4u <= 64u && !mdb_knob_off("MDB_KEYED_RECORDS"))
		g->keyed_cbits = 64u - kbits - st->key_bits;
	if (ctx->keyed_distrust > 0)
		ctx->keyed_distrust--;
	a.keyed_cbits = g->keyed_cbits;
	/* 4-byte records straight from the leaf kernel when the last run over these very columns saw every COUNT(*) fit beside the
	 * row id (variant U: 10^8 records - 0.4 GB less to write and 0.4 GB less for the ordering sort to read) */
	const bool r32_same = ctx->r32_ok && ctx->vd[VD_REC32].holds(keys_l, n_l, keys_r, n_r);
	a.rec32 = (r32_same && st->direct && !st->one_level && has_r && records && !g->keyed_cbits && kbits < 32 && g->sb2 > 0 && pl.leaf_cap && pr.leaf_cap) ? 1u : 0u;
	/* one-level joins with 2-byte right words: k_leaf_wide4's 4 bytes per key value (two workgroups per CU) unless these columns are known to
	 * hold more than 31 right or 15 left rows of a key */
	g->leaf4 = st->one_level && has_r && pr.w16 && records && !st->rq.null_group && n_l <= (1ull << 27) && st->key_bits >= (uint32_t)pl.bits_total + 10u &&
		   !ctx->vd[VD_L4_BAD].serve(keys_l, n_l, NULL, n_r, MDB_BAD_SERVES);
	/* ... and when the last join over these very columns told how many groups to expect, and they are few enough for the ordering kernel's
	 * ranges of 2^16 row ids, k_leaf_wide4 writes its records straight into those ranges: no record list, none of the two scatter levels that
	 * would partition it by row id */
	g->rg_n = 0;
	g->ranged = g->leaf4 && !ctx->lg_nextra && ctx->vd[VD_LAST_GROUPS].holds(keys_l, n_l, keys_r, n_r) &&
		    order_ranges_apply(n_l, kbits, ctx->lg_groups + ctx->lg_groups / 8, &g->rg_n);
	/* ... or the caller's statistics say so before any join has run (mdb_dev_call_stats): a group needs a right key, and there are at
	 * most as many of those as values in the right column's range */
	if (!g->ranged && g->leaf4)
		g->ranged = gc_ranged_by_stats(ctx, keys_l, keys_r, n_l, n_r, kbits, &g->rg_n);
	a.rg_rec = NULL;
	a.rg_cnt = NULL;
	a.rg_cap = a.rg_shift = a.rg_n = 0;
	if (g->ranged) {
		a.rg_rec = (unsigned long long *)mdb_arena_take(ctx, (size_t)g->rg_n * ORDER_RANGE_CAP * 8);
		const bool rg_in_block = st->own_call && g->rg_n <= MDB_ZERO_BLK_WORDS - 2u * MDB_ZERO_BLK_SLOT;
		a.rg_cnt = rg_in_block ? ctx->d_status + MDB_ZERO_BLK_OFF + 2u * MDB_ZERO_BLK_SLOT : (uint32_t *)mdb_arena_take(ctx, (size_t)g->rg_n * 4);
		if (!a.rg_rec || !a.rg_cnt)
			return -MIDORIDB_INTERNAL;
		/* (the arena hands out whole 256-byte units: cleared as such - a length that is no multiple of 16 bytes costs the runtime a second fill
		 * kernel, 5 us of the step) */
		if (!rg_in_block)
			MDB_HIP(ctx, hipMemsetAsync(a.rg_cnt, 0, mdb_align_up((size_t)g->rg_n * 4), ctx->stream));
		a.rg_cap = ORDER_RANGE_CAP;
		a.rg_shift = ORDER_RANGE_BITS;
		a.rg_n = g->rg_n;
	}
	return MIDORIDB_OK;
}

/* stage 2c: The last join over these columns made nearly every left row a group of COUNT 1 (a primary key joined with another, or with its
 * foreign keys - BASELINE configs[2]'s variant U): k_leaf_wide12 then clears one bit per left row that is NO group's first row and
 * lists the groups whose COUNT is not 1, instead of a record per group and the ordering sort of 10^8 records (MDB_JOIN_BITS=0: never) */
static int gc_choose_bits(mdb_dev_ctx *ctx, gc_run *g)
{
	gc_state *st = g->st;
	gc_args &a = g->a;
	const int64_t *keys_l = st->rq.l.keys, *keys_r = g->r.keys;
	const uint64_t n_l = st->rq.l.n, n_r = g->r.n;
	int rc;
	g->dn_bits = NULL;
	a.dn_bits = NULL;
	a.dn_exc = NULL;
	a.dn_exc_cap = 0;
	a.dn_pilot = 0;
	a.dn_cnt = ctx->d_status + GC_STW_DN_CLEARED;
	/* (every left row must reach the leaf kernel for its bit to be looked at: no NULL keys, no window that covers the right table's keys
	 * only - left rows outside it are dropped by the first level; rows dropped for another reason show as G + cleared != n_l below and
	 * send the call to the record form) */
	if (!gc_bits_possible(st, g->records, st->rq.has_r, g->out.cap, n_l))
		return MIDORIDB_OK;
	bool want_bits = false, by_pilot = false, by_stats = false;
	/* The catalog says (MDB_COL_DISTINCT, measured at ingest): no key twice in the left column, none twice in the right one, and the
	 * right column holds EVERY value of its range, which covers the left column's - every left row is a group of COUNT 1, whatever
	 * the statement before this one was: no pilot launch and its host round trip, nothing remembered by the columns' addresses.
	 * (Two tables only; a promise that does not hold shows below as it does for the other two ways to get here: G + cleared != n_l,
	 * or more exceptions than the list holds - the call is redone with records.) */
	if (gc_bits_by_stats(ctx, st->rq.nextra, keys_l, keys_r, n_r)) {
		want_bits = true;
		by_stats = true;
	} else if (ctx->lg_nextra == (uint32_t)st->rq.nextra && ctx->vd[VD_LAST_GROUPS].holds(keys_l, n_l, keys_r, n_r)) {
		/* (what the last join over these very columns delivered) */
		if (ctx->lg_groups >= n_l - n_l / 16 && ctx->lg_joined <= ctx->lg_groups + ctx->lg_groups / 16) {
			if (ctx->dn_distrust > 0)
				ctx->dn_distrust--;
			else
				want_bits = true;
		}
	} else {
		/* nothing remembered (a first statement): the pilot - the same kernel over the first 64 of the 4096 digits (all rows of a key are
		 * in one digit: a fair sample of the keys), nothing written but the counters: left rows that are no group's first row, groups
		 * whose COUNT is not 1.  One in 16 of the rows at most each: the bit-per-row form */
		a.dn_pilot = 64;
		if ((rc = leaf_wide12_launch(ctx, a, g->pl.nleaves, st->key_bits - 12u, g->pl.nsub, st->rq.nextra)))
			return rc;
		a.dn_pilot = 0;
		MDB_HIP(ctx, hipMemcpyAsync(g->rb, ctx->d_status, GC_RB_BYTES_DN, hipMemcpyDeviceToHost, ctx->stream));
		MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		const uint64_t p_groups = g->rb->groups, p_cleared = g->rb->dn_cleared, p_exc = g->rb->dn_exceptions, p_rows = p_groups + p_cleared;
		want_bits = p_rows && p_cleared * 16 <= p_rows && p_exc * 16 <= p_rows;
		by_pilot = true;
		if (mdb_knob_set("MDB_DEBUG_GROUP"))
			fprintf(stderr, "join + GROUP BY (pilot over 64 digits): %llu left rows, %llu no group's first row, %llu groups of COUNT != 1 -> %s\n",
				(unsigned long long)p_rows, (unsigned long long)p_cleared, (unsigned long long)p_exc, want_bits ? "a bit per left row" : "records");
		/* (the flags of word 0 stay: they are facts about the data) */
		MDB_HIP(ctx, hipMemsetAsync(ctx->d_status + GC_STW_LIST_LEN, 0, GC_RB_BYTES_DN - 4 * GC_STW_LIST_LEN, ctx->stream));
	}
	if (want_bits) {
		if ((rc = mdb_dense_bits_begin(ctx, n_l, &g->dn_bits)))
			return rc;
		a.dn_bits = reinterpret_cast<unsigned int *>(g->dn_bits);
		a.dn_exc_cap = (uint32_t)(n_l / 8 + 4096);
		a.dn_exc = (unsigned long long *)mdb_arena_take(ctx, (size_t)a.dn_exc_cap * 8);
		if (!a.dn_exc)
			return -MIDORIDB_INTERNAL;
		ctx->plan.groups_as_bits = by_stats ? 3u : by_pilot ? 1u : 2u;
	}
	return MIDORIDB_OK;
}

/* stage 3: the leaf kernel the plan and the tables' layouts ask for, and the NULL group's kernels behind it */
static int gc_launch_leaf(mdb_dev_ctx *ctx, gc_run *g)
{
	gc_state *st = g->st;
	const gc_args &a = g->a;
	const mdb_part_result &pl = g->pl, &pr = g->pr;
	const bool has_r = st->rq.has_r;
	int rc;
	/* (the direct kernel addresses leaf i at i * cap: should a table have fallen back to exact offsets - more than 2^32
	 * region words - the hashed kernel below joins the compact words just as well, they are injective too) */
	if (st->wide12) {
		if ((rc = leaf_wide12_launch(ctx, a, pl.nleaves, st->key_bits - 12u, pl.nsub, st->rq.nextra)))
			return rc;
	} else if (st->one_level) {
		/* ... by ALL the hash bits below the first level's 9 (k_leaf_wide) */
		if (!pl.nsub || !pl.leaf_cap || (has_r && (!pr.nsub || !pr.w32 || pr.nsub != pl.nsub || pr.nleaves != pl.nleaves)))
			return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "one-level direct leaves: the tables are not in the first-level layout");
		const uint32_t rem = st->key_bits - pl.bits_total, shift = 32u - st->key_bits;
		if (has_r && pr.w16 && g->leaf4)
			rc = leaf_wide4_launch(ctx, a, pl.nleaves, rem, shift, pl.nsub);
		else
			rc = leaf_wide_launch(ctx, a, pl.nleaves, rem, shift, pl.nsub, has_r, has_r && pr.w16);
		if (rc)
			return rc;
	} else if (st->direct && pl.leaf_cap && (!has_r || pr.leaf_cap)) {
		/* compact narrow form: the leaf's table is indexed by the hash bits the partition left over */
		const uint32_t rem = st->key_bits - pl.bits_total, shift = 32u - st->key_bits;
		if (st->rq.nextra && !(pl.leaf_cap && pr.leaf_cap))
			return GC_NOT_SERVED;
		if ((rc = leaf_direct_launch(ctx, a, rem, shift, has_r, st->rq.nextra)))
			return rc;
	} else if (st->rq.nextra) {
		return GC_NOT_SERVED;
	} else if ((rc = leaf_hashed_launch(ctx, a, has_r, g->build_r, st->rq.kf.narrow))) {
		return rc;
	}
	if (st->rq.null_group && st->rq.l.nulls && (rc = leaf_null_group_launch(ctx, a, st->rq.l.nulls, st->rq.l.n)))
		return rc;
	return MIDORIDB_OK;
}

/* the ordering of ranges that the leaf kernel filled itself */
static int gc_order_presorted(mdb_dev_ctx *ctx, gc_run *g, uint64_t early_cap)
{
	const gc_state *st = g->st;
	return order_presorted(ctx, g->a.rg_rec, g->a.rg_cnt, g->rg_n, g->kbits, g->out.first, g->out.count, st->rq.l.keys, g->out.key, st->rq.keys32, g->keyed_cbits,
			       st->key_bits, st->rq.kf.win.lo, early_cap);
}

/* the status words to the host: `bytes` of them from word 0 on, and wait */
static int gc_read_back(mdb_dev_ctx *ctx, gc_run *g, size_t bytes)
{
	MDB_HIP(ctx, hipMemcpyAsync(g->rb, ctx->d_status, bytes, hipMemcpyDeviceToHost, ctx->stream));
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	g->tail_queued = false;		/* (whatever was queued behind an earlier status is complete too) */
	return MIDORIDB_OK;
}

/* stage 4: G, J and the status flags come back with one sync; the sort is sized by G ... except where the leaf kernel has filled the ordering kernel's
 * ranges itself: that kernel needs no size, and is launched right behind it (its writes bounded by the caller's capacity; should the status words
 * ask for another path, that path writes the columns again) - the step's only sync then comes after its last kernel.
 * A caller that reads its result columns in stream order (mdb_dev_results_in_stream_order) does not wait for that kernel at all: the leaf kernel
 * has written every status word, so the copy goes in front of the ordering kernel and the host waits for an event recorded behind the copy -
 * the ordering kernel runs while the call returns and the next one is prepared.  Nothing the host reads afterwards is touched by it (no status
 * of its own, its stores go to the caller's columns alone); whatever a retry path launches queues behind it on the same stream. */
static int gc_read_status(mdb_dev_ctx *ctx, gc_run *g)
{
	int rc;
	g->ordered_early = false;
	g->tail_queued = false;
	if (g->ranged && g->out.cap && ctx->stream_ordered) {
		MDB_HIP(ctx, hipMemcpyAsync(g->rb, ctx->d_status, GC_RB_BYTES_DN, hipMemcpyDeviceToHost, ctx->stream));
		MDB_HIP(ctx, hipEventRecord(ctx->ev_status, ctx->stream));
		rc = gc_order_presorted(ctx, g, g->out.cap);
		MDB_HIP(ctx, hipEventSynchronize(ctx->ev_status));
		if (rc)
			return rc;
		g->ordered_early = true;
		g->tail_queued = true;
		g->dn_cleared = g->rb->dn_cleared;
		g->dn_exceptions = g->rb->dn_exceptions;
		return MIDORIDB_OK;
	}
	if (g->ranged && g->out.cap) {
		if ((rc = gc_order_presorted(ctx, g, g->out.cap)))
			return rc;
		g->ordered_early = true;
	}
	if ((rc = gc_read_back(ctx, g, GC_RB_BYTES_DN)))	/* (with the bit-per-row form's counters) */
		return rc;
	g->dn_cleared = g->rb->dn_cleared;
	g->dn_exceptions = g->rb->dn_exceptions;
	return MIDORIDB_OK;
}

/* k_leaf_wide4's count fields overflow on these columns: k_leaf_wide at once, for MDB_BAD_SERVES calls */
static void gc_l4_bad_note(mdb_dev_ctx *ctx, const gc_run *g)
{
	ctx->vd[VD_L4_BAD].note(g->st->rq.l.keys, g->st->rq.l.n, NULL, g->r.n);
}

/* the same partitioned tables through another one-level leaf kernel: the flags this retry answers (and those the new run raises again if they still
 * apply) are taken out of word 0, the counters cleared, the status read back */
static int gc_leaf4_relaunch(mdb_dev_ctx *ctx, gc_run *g, bool wide16)
{
	const gc_state *st = g->st;
	const mdb_part_result &pl = g->pl;
	int rc;
	uint32_t *hw = reinterpret_cast<uint32_t *>(ctx->h_pinned + MDB_HP_SEND_FLAGS);
	hw[0] = g->rb->flags & ~(GC_ST_COUNTS_NOT_4BYTE | GC_ST_RANGE_FULL | GC_ST_COUNT_NOT_KEYED | GC_ST_COUNT_NOT_REC32 | MDB_ST_LIST_FULL);
	MDB_HIP(ctx, hipMemcpyAsync(ctx->d_status, hw, 4, hipMemcpyHostToDevice, ctx->stream));
	MDB_HIP(ctx, hipMemsetAsync(ctx->d_status + GC_STW_LIST_LEN, 0, 4 * (GC_STW_NULL_STATS - GC_STW_LIST_LEN), ctx->stream));	/* record-list length, joined rows */
	MDB_HIP(ctx, hipMemsetAsync(ctx->d_status + GC_STW_RECORDS, 0, 4 * (GC_STW_SAMPLE - GC_STW_RECORDS), ctx->stream));	/* records, largest first row */
	if ((rc = wide16 ? leaf_wide_launch(ctx, g->a, pl.nleaves, st->key_bits - pl.bits_total, 32u - st->key_bits, pl.nsub, true, true)
			 : leaf_wide4_launch(ctx, g->a, pl.nleaves, st->key_bits - pl.bits_total, 32u - st->key_bits, pl.nsub)))
		return rc;
	return gc_read_back(ctx, g, GC_RB_BYTES);
}

/* stage 5: a key with more rows than k_leaf_wide4's count fields hold: the same partitioned tables through k_leaf_wide (16-bit counts), now
 * and for these columns; a range of row ids with more groups than its region holds (more groups than last time, or bunched):
 * k_leaf_wide4 again, into the record list */
static int gc_leaf4_redo(mdb_dev_ctx *ctx, gc_run *g)
{
	const uint32_t partition_said = MDB_ST_REGION_FULL | MDB_ST_KEY_OUTSIDE;	/* (the whole operator is redone: nothing to save here) */
	int rc;
	if (!(g->leaf4 && (g->rb->flags & (GC_ST_COUNTS_NOT_4BYTE | GC_ST_RANGE_FULL)) && !(g->rb->flags & partition_said)))
		return MIDORIDB_OK;
	const bool counts_bad = (g->rb->flags & GC_ST_COUNTS_NOT_4BYTE) != 0;
	if (counts_bad)
		gc_l4_bad_note(ctx, g);
	g->ranged = false;
	g->a.rg_rec = NULL;
	ctx->vd[VD_LAST_GROUPS].clear();
	if ((rc = gc_leaf4_relaunch(ctx, g, counts_bad)))
		return rc;
	if (!counts_bad && (g->rb->flags & GC_ST_COUNTS_NOT_4BYTE) && !(g->rb->flags & partition_said)) {	/* (the counts overflow as well: seen only now) */
		gc_l4_bad_note(ctx, g);
		rc = gc_leaf4_relaunch(ctx, g, true);
	}
	return rc;
}

/* What the flags ask for: MIDORIDB_OK (go on), a GC_RETRY_* / GC_NOT_SERVED for the caller's retry loop (with what the context must remember for the
 * retry), or an error.  Looked at twice per attempt, and each flag belongs to one of the two looks - in this order of precedence:
 *
 *   GC_AT_LEAF, when the leaf kernel's status has arrived (what asks for another plan altogether, before the hot-key path spends time on this one):
 *     1 MDB_ST_KEY_OUTSIDE                                            GC_RETRY_PLAIN (compact window) / GC_RETRY_WIDE
 *     2 further right tables, and REGION_FULL | HOT_LEAVES | PRODUCT_WIDE  GC_NOT_SERVED
 *     3 MDB_ST_REGION_FULL                                            GC_RETRY_EXACT
 *     4 GC_ST_ROWS_NOT_16BIT                                          GC_RETRY_TWO_LEVEL
 *     5 GC_ST_HOT_LEAVES with keyed records                           GC_RETRY_UNKEYED
 *     6 4-byte records, and HOT_LEAVES | REC32_STALE                  GC_RETRY_REC64
 *   GC_AT_END, after the hot-key path (which may raise TABLE_FULL, LIST_FULL and the COUNT flags anew) and the count of the groups:
 *     7 MDB_ST_REGION_FULL                                            GC_RETRY_EXACT (row 3 has answered it unless the flag appeared since)
 *     8 GC_ST_COUNT_NOT_KEYED                                         GC_RETRY_UNKEYED
 *     9 GC_ST_COUNT_NOT_REC64                                         GC_RETRY_DENSE
 *    10 GC_ST_TABLE_FULL, table built on the right side               GC_RETRY_BUILD_L
 *    11 GC_ST_TABLE_FULL                                              error
 *    12 MDB_ST_LIST_FULL                                              error
 * GC_ST_COUNT_NOT_REC32, GC_ST_LEFT_DUPS, GC_ST_EXC_FULL and HOT_LEAVES at the end are facts for the delivery, not verdicts. */
enum gc_verdict_at { GC_AT_LEAF, GC_AT_END };
static int gc_verdict(mdb_dev_ctx *ctx, const gc_run *g, gc_verdict_at at)
{
	const gc_state *st = g->st;
	const uint32_t f = g->rb->flags;
	if (at == GC_AT_LEAF) {
		if (f & MDB_ST_KEY_OUTSIDE)
			return st->direct ? GC_RETRY_PLAIN : GC_RETRY_WIDE;	/* a key outside the window: the 32-bit hashes mean nothing */
		if (st->rq.nextra && (f & (MDB_ST_REGION_FULL | GC_ST_HOT_LEAVES | GC_ST_PRODUCT_WIDE)))
			return GC_NOT_SERVED;	/* skewed keys, hot leaves, a product of counts beyond 32 bits: the chain of two-table operators */
		if (f & MDB_ST_REGION_FULL)
			return GC_RETRY_EXACT;	/* a leaf outgrew its fixed-capacity region (skewed keys) */
		if (f & GC_ST_ROWS_NOT_16BIT) {
			/* a key with 2^16 or more rows on one side: two levels and their hot-key path, now and for these columns */
			ctx->vd[VD_LW_BAD].note(st->rq.l.keys, st->rq.l.n, NULL, st->rq.r.n);
			return GC_RETRY_TWO_LEVEL;
		}
		if ((f & GC_ST_HOT_LEAVES) && g->keyed_cbits) {
			ctx->keyed_distrust = 64;	/* hot leaves go through kernels that write plain records: redo with those everywhere */
			return GC_RETRY_UNKEYED;
		}
		if (g->a.rec32 && (f & (GC_ST_HOT_LEAVES | GC_ST_REC32_STALE))) {
			ctx->r32_ok = false;		/* a COUNT(*) that no longer fits, or hot leaves (their kernels write 8-byte records) */
			return GC_RETRY_REC64;
		}
		return MIDORIDB_OK;
	}
	if (f & MDB_ST_REGION_FULL)
		return GC_RETRY_EXACT;	/* a leaf outgrew its fixed-capacity region (skewed keys) */
	if (f & GC_ST_COUNT_NOT_KEYED) {
		ctx->keyed_distrust = 64;	/* a COUNT(*) too large for a keyed record: plain records, now and for a while */
		return GC_RETRY_UNKEYED;
	}
	if (f & GC_ST_COUNT_NOT_REC64)
		return GC_RETRY_DENSE;	/* a COUNT(*) too large to share a 64-bit record with its row id */
	if ((f & GC_ST_TABLE_FULL) && g->build_r)
		return GC_RETRY_BUILD_L;
	if (f & GC_ST_TABLE_FULL)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL,
				   "leaf hash table overflow (more than %u distinct keys in one leaf): unsupported key skew", GC_SLOTS);
	if (f & MDB_ST_LIST_FULL)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "group record list exhausted (sizing bug)");
	return MIDORIDB_OK;
}

/* the number of groups: with the status words in record mode; dense mode selects the first rows whose COUNT is not 0 and reads their number */
static int gc_count_groups(mdb_dev_ctx *ctx, gc_run *g)
{
	if (g->records) {
		g->list_len = g->rb->list_len;
		g->G = g->rb->groups;
		return MIDORIDB_OK;
	}
	uint32_t *d_total = NULL;
	int rc = mdb_filter_nonzero64(ctx, g->dense, g->st->rq.l.n, g->sel, &d_total);
	if (rc)
		return rc;
	uint64_t *h = ctx->h_pinned;
	MDB_HIP(ctx, hipMemcpyAsync(&h[MDB_HP_COUNT], d_total, 4, hipMemcpyDeviceToHost, ctx->stream));
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	g->G = (uint32_t)h[MDB_HP_COUNT];
	return MIDORIDB_OK;
}

/* stage 7a: the groups of record mode, ordered by first row id - from the bits, the ranges or the record list */
static int gc_deliver_records(mdb_dev_ctx *ctx, gc_run *g)
{
	gc_state *st = g->st;
	const gc_out &o = g->out;
	const uint64_t n_l = st->rq.l.n, G = g->G;
	const uint32_t status = g->rb->flags;
	int rc;
	/* (one-level leaves report the largest first row id: the sort's first-level regions are sized for the digits below it) */
	const uint64_t last_first = g->rb->last_first;
	const uint64_t n_ord = (st->one_level && last_first && last_first < n_l) ? last_first + 1 : n_l;
	if (g->dn_bits) {
		if (mdb_knob_set("MDB_DEBUG_GROUP"))
			fprintf(stderr, "join + GROUP BY (bit per left row): %llu groups, %u rows cleared of %llu, %u exceptions, status %u\n",
				(unsigned long long)G, g->dn_cleared, (unsigned long long)n_l, g->dn_exceptions, status);
		if ((status & GC_ST_EXC_FULL) || (uint64_t)G + g->dn_cleared != n_l) {	/* (more groups of COUNT != 1 than last time: the record form) */
			ctx->dn_distrust = 32;
			ctx->plan.groups_as_bits = 0;
			return GC_RETRY_NODENSE;
		}
		/* every left row a group: the group keys ARE the left key column, in its order - a caller that said so (MDB_KEYS_MAY_ALIAS) reads
		 * them there and nothing is copied (0.8 GB read + 0.8 GB written at 10^8 rows); every COUNT 1 and MDB_COUNTS_OPTIONAL: no COUNT
		 * column either (mdb_dev_last_plan says which) */
		const bool alias = ctx->key_alias_ok && !st->rq.keys32 && o.key && G == n_l;
		const bool ones = ctx->counts_optional && g->dn_exceptions == 0;
		ctx->plan.keys_are_left_column = alias ? 1u : 0u;
		ctx->plan.counts_all_one = ones ? 1u : 0u;
		rc = mdb_dense_emit(ctx, g->dn_bits, n_l, g->a.dn_exc, g->dn_exceptions, o.first, ones ? NULL : o.count, st->rq.l.keys, st->rq.keys32, alias ? NULL : o.key);
		if (!rc)
			MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	} else if (g->ranged && g->ordered_early)
		rc = MIDORIDB_OK;	/* (launched behind the leaf kernel: waited for with the status words, or queued behind them for a stream-ordered caller) */
	else if (g->ranged)
		rc = gc_order_presorted(ctx, g, 0);
	else
		rc = order_records(ctx, g->rec, g->list_len, n_ord, g->kbits, g->sb1, g->sb2, o.first, o.count, NULL, st->rq.l.keys, o.key, st->rq.keys32,
				   !(status & GC_ST_COUNT_NOT_REC32), g->keyed_cbits, st->key_bits, st->rq.kf.win.lo, g->a.rec32 != 0, G);
	if (rc == GC_RETRY_REC64)
		ctx->r32_ok = false;
	if (rc)
		return rc;
	/* remember whether 4-byte records would do for these columns */
	ctx->r32_ok = st->direct && !st->one_level && st->rq.has_r && !g->keyed_cbits && !(status & GC_ST_COUNT_NOT_REC32);
	ctx->vd[VD_REC32].note(st->rq.l.keys, n_l, g->r.keys, g->r.n);
	return MIDORIDB_OK;
}

/* stage 7b: the groups of dense mode - the selected first rows' counts and keys gathered */
static int gc_deliver_dense(mdb_dev_ctx *ctx, gc_run *g)
{
	const gc_state *st = g->st;
	const gc_out &o = g->out;
	const uint64_t G = g->G;
	int rc = mdb_dev_gather64(ctx, g->dense, NULL, g->sel, G, o.count, NULL);
	if (rc)
		return rc;
	if (o.key && st->rq.keys32) {
		rc = leaf_gather_i32_launch(ctx, reinterpret_cast<const int32_t *>(st->rq.l.keys), g->sel, G, o.key);
		if (rc)
			return rc;
	} else if (o.key) {
		rc = mdb_dev_gather64(ctx, st->rq.l.keys, NULL, g->sel, G, o.key, NULL);
		if (rc)
			return rc;
	}
	if (o.first)
		MDB_HIP(ctx, hipMemcpyAsync(o.first, g->sel, G * 4, hipMemcpyDeviceToDevice, ctx->stream));
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return MIDORIDB_OK;
}

/* stage 8: the result's sizes to the caller; what the next call over these columns may use (lg_*, last_left_dups*); the plan record */
static void gc_remember(mdb_dev_ctx *ctx, const gc_run *g)
{
	const gc_state *st = g->st;
	const uint32_t status = g->rb->flags;
	const uint64_t joined = g->rb->joined;
	*g->out.groups = g->G;
	if (g->out.joined)
		*g->out.joined = joined;
	if (st->rq.has_r) {
		ctx->vd[VD_LAST_GROUPS].note(st->rq.l.keys, st->rq.l.n, g->r.keys, g->r.n);
		ctx->lg_nextra = (uint32_t)st->rq.nextra;
		ctx->lg_groups = g->G;
		ctx->lg_joined = joined;
	}
	ctx->last_left_dups_known = st->direct && st->rq.has_r && !(status & GC_ST_HOT_LEAVES);	/* (the hot-key kernels and the hashed leaves do not say) */
	ctx->last_left_dups = (status & GC_ST_LEFT_DUPS) != 0;
	gc_plan_note(ctx, st);
	ctx->plan.any_order = 0;
	ctx->plan.ranged_order = g->ranged ? 1u : 0u;
}

/* second half: partition what waited for the right table, join and count in the leaves, order and deliver the groups.  MIDORIDB_OK, an error, or
 * a GC_RETRY_* / GC_NOT_SERVED that tells the caller which plan to try instead (gc_verdict) */
static int gc_finish(mdb_dev_ctx *ctx, gc_state *st, const gc_table &right, const gc_out &out)
{
	gc_run g;
	int rc;
	memset(&g, 0, sizeof(g));
	g.st = st;
	g.r = right;
	g.out = out;
	g.build_r = st->rq.has_r && !st->rq.no_build_r && right.n <= st->rq.l.n;
	g.pl = st->pl;
	g.rb = reinterpret_cast<gc_readback *>(ctx->h_pinned + MDB_HP_STATUS);
	st->active = false;
	if ((rc = gc_partition(ctx, &g)) || (rc = gc_args_begin(ctx, &g)) || (rc = gc_choose_records(ctx, &g)) || (rc = gc_choose_bits(ctx, &g)))
		return rc;
	if ((rc = gc_launch_leaf(ctx, &g)) || (rc = gc_read_status(ctx, &g)) || (rc = gc_leaf4_redo(ctx, &g)))
		return rc;
	if ((rc = gc_verdict(ctx, &g, GC_AT_LEAF)))
		return rc;
	/* stage 6: hot keys - the plain kernel left the leaves with GC_HEAVY or more rows on a side to this path */
	if ((g.rb->flags & GC_ST_HOT_LEAVES) && ((rc = leaf_hot_launch(ctx, g.a, st->rq.has_r, g.build_r)) || (rc = gc_read_back(ctx, &g, GC_RB_BYTES))))
		return rc;
	if ((rc = gc_count_groups(ctx, &g)) || (rc = gc_verdict(ctx, &g, GC_AT_END)))
		return rc;
	if (g.G > out.cap)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group output capacity %llu too small for %llu groups", (unsigned long long)out.cap, (unsigned long long)g.G);
	if (g.G && (rc = g.records ? gc_deliver_records(ctx, &g) : gc_deliver_dense(ctx, &g)))
		return rc;
	gc_remember(ctx, &g);
	ctx->last_return_early = g.tail_queued;
	return MIDORIDB_OK;
}

/* one attempt of the operator with the plan the request holds */
static int group_count_run(mdb_dev_ctx *ctx, const gc_request &rq)
{
	rq.out.clear();
	if (rq.l.n == 0 || (rq.has_r && rq.r.n == 0))
		return MIDORIDB_OK;
	gc_state st;
	gc_state_fill(&st, rq, true);
	int rc = gc_begin(ctx, &st);
	if (rc == GC_EXPLAINED)		/* (mdb_dev_explain_*: gc_begin stopped in front of its arena) */
		gc_explain_fill(ctx, &st);
	if (rc)
		return rc;
	return gc_finish(ctx, &st, rq.r, rq.out);
}

/* the request of a join (has_r) or of a plain GROUP BY with its NULL group (r = nothing), before any plan is made */
static gc_request gc_request_of(const gc_table &l, const gc_table &r, const gc_out &out, bool has_r, bool keys32 = false)
{
	return gc_request{ l, r, out, has_r, !has_r, keys32 };	/* (no further tables, no plan: zero) */
}

/* the operator over a request's tables: the first plan from what the key sample and the memo say, then up to six attempts, each GC_RETRY_*
 * editing the plan for the next */
static int group_count_common(mdb_dev_ctx *ctx, gc_request *rq)
{
	const gc_sides sides = { rq->l, rq->r };	/* (a plain GROUP BY's r is empty) */
	const int64_t *keys_l = rq->l.keys;
	const uint64_t n_l = rq->l.n, n_r = rq->r.n;
	const bool has_r = rq->has_r, keys32 = rq->keys32;
	/* first the histogram-free layout for the second partition level; the exact layout is the fallback
	 * when skewed keys overflow a leaf region (detected on the device, reported with the results) */
	rq->fast = true;
	rq->records = true;
	rq->no_build_r = false;
	int rc = MIDORIDB_OK;
	/* plain GROUP BY whose key sample held duplicates (at most a few 10^5 distinct values): the leaves hold a few values with
	 * hundreds or thousands of rows each, their sizes vary by whole multiples, and the fixed-capacity layout would overflow
	 * and be redone anyway - start with the exact layout */
	/* ... unless there are still some 10^4 - 10^5 of them (3500 distinct among 4096 sampled: about 1.3 * 10^4 in the column) and
	 * the one-level form applies: its 256 or 512 first-level regions hold 50 values or more each; sized at 1.5 x the average
	 * (mdb_part_request.loose) they take the variation of that number */
	bool fast1 = false;
	if (!has_r && ctx->vd[VD_DISTINCT].holds(keys_l, n_l, NULL, 0) && ctx->gh_distinct < 4050u) {
		if (ctx->gh_distinct >= 3500u)
			fast1 = true;
		else
			rq->fast = false;
	}
	rc = gc_narrow_guess(ctx, sides, &rq->kf, keys32, has_r);
	if (rc)
		return rc;
	rq->kf.win.fast1 = fast1;
	/* the histogram-free layout overflowed on these very columns last time (skewed or heavily duplicated keys): exact at once */
	if (rq->fast && ctx->vd[VD_EXACT].serve(keys_l, n_l, NULL, has_r ? n_r : 0, MDB_HINT_SERVES)) {
		rq->fast = false;
		rq->kf.win.fast1 = false;
	}
	for (int attempt = 0; attempt < 6; attempt++) {
		ctx->plan.retries = (uint32_t)attempt;
		rc = group_count_run(ctx, *rq);
		if ((rc == GC_RETRY_PLAIN || rc == GC_RETRY_WIDE) && ctx->guess_remembered && ctx->narrow_mode == 1 && !keys32) {
			/* a REMEMBERED verdict proved wrong: the buffers hold other data than when it was made (a caller's allocator handed
			 * the same addresses out again).  Not a reason to give the narrow forms up: forget, look at the data itself, go on */
			ctx->forget_guess();
			rc = gc_narrow_guess(ctx, sides, &rq->kf, keys32, has_r);
			if (rc)
				return rc;
			rq->kf.win.fast1 = fast1 && rq->fast;
		} else if (rc == GC_RETRY_PLAIN) {
			/* the sample missed the column's extremes: the plain narrow form (any 2^32-wide window) is tried next,
			 * and remembered for these columns */
			rq->kf.win.kbits = 0;
			if (ctx->narrow_mode == 1)
				gc_narrow_note(ctx, sides, true, rq->kf.base);
		} else if (rc == GC_RETRY_WIDE) {
			rq->kf.narrow = false;
			if (ctx->narrow_mode == 1 && !keys32) {
				ctx->nh_distrust = 8;	/* whatever said "narrow" was wrong: look at the data itself the next few times */
				gc_narrow_note(ctx, sides, false);	/* the sample missed a wide key */
			}
		} else if (rc == GC_RETRY_EXACT) {
			rq->fast = false;
			rq->kf.win.fast1 = false;
			ctx->vd[VD_EXACT].note(keys_l, n_l, NULL, has_r ? n_r : 0);
		}	/* (gc_begin then also leaves the narrow form of a join: it is only built on the fast layout) */
		else if (rc == GC_RETRY_DENSE)
			rq->records = false;
		else if (rc == GC_RETRY_UNKEYED || rc == GC_RETRY_REC64 || rc == GC_RETRY_TWO_LEVEL || rc == GC_RETRY_NODENSE)
			;		/* (gc_finish has set ctx->keyed_distrust / cleared ctx->r32_ok / noted the columns in VD_LW_BAD) */
		else if (rc == GC_RETRY_BUILD_L)
			rq->no_build_r = true;
		else
			break;
	}
	return rc == GC_EXPLAINED ? MIDORIDB_OK : rc;
}

/* MDB_KEYS_MAY_ALIAS / MDB_COUNTS_OPTIONAL of the OUTERMOST join + GROUP BY call hold for it and the operators it calls */
struct gc_alias_scope {
	mdb_dev_ctx *c;
	bool a, o;
	gc_alias_scope(mdb_dev_ctx *ctx, uint32_t f) : c(ctx), a(ctx->key_alias_ok), o(ctx->counts_optional)
	{
		if (ctx->pl_depth == 1) {
			ctx->key_alias_ok = (f & MDB_KEYS_MAY_ALIAS) != 0;
			ctx->counts_optional = (f & MDB_COUNTS_OPTIONAL) != 0;
		}
	}
	~gc_alias_scope()
	{
		c->key_alias_ok = a;
		c->counts_optional = o;
	}
};

extern "C" int mdb_dev_join_group_count(mdb_dev_ctx *ctx, const int64_t *keys_l, const uint64_t *null_l, uint64_t n_l,
					const int64_t *keys_r, const uint64_t *null_r, uint64_t n_r, uint32_t flags,
					int64_t *out_key, int64_t *out_count, uint32_t *out_first, uint64_t cap,
					uint64_t *out_groups, uint64_t *out_joined)
{
	mdb_plan_scope plan_scope(ctx);
	const gc_sides sides = { { keys_l, null_l, n_l }, { keys_r, null_r, n_r } };
	const gc_out out = { out_key, out_count, out_first, cap, out_groups, out_joined };
	out.clear();
	gc_alias_scope alias_scope_(ctx, flags);
	mdb_memo_switch(ctx, keys_l, n_l, keys_r, n_r);	/* what was learned about THIS pair of columns */
	if (!(flags & MDB_ORDER_FIRST) && !out_first && out_key && n_l && n_r) {
		/* no order asked for: no row ids, no ordering sort (otherwise - and whenever this form is not served - the groups come
		 * out in first-occurrence order, which satisfies both modes) */
		const int urc = gc_unordered_try(ctx, sides, out);
		if (urc <= 0)
			return urc;
		out.clear();
	}
	const int trc = tiny_group_count(ctx, sides, true, false, out);
	if (trc <= 0)
		return trc;
	if (n_l && n_r) {
		/* both key columns inside one window of at most 4096 values (joins on a handful of hot values): counted directly */
		gc_out direct = out;
		uint32_t *tmp_first = NULL;
		if (!out_first && mdb_cached_alloc(ctx, (cap ? cap : 1) * 4, (void **)&tmp_first))
			tmp_first = NULL;
		if (!out_first)
			direct.first = tmp_first;
		const int drc = direct.first ? group_direct_try(ctx, sides, false, direct) : 1;
		if (tmp_first)
			(void)mdb_cached_free(ctx, tmp_first);
		if (drc <= 0)
			return drc;
		out.clear();
	}
	gc_request rq = gc_request_of(sides.l, sides.r, out, true);
	return group_count_common(ctx, &rq);
}

/* ---- split form for pipelines whose right table arrives later (multi-GPU exchange) ---- */

static gc_state *gc_pending(mdb_dev_ctx *ctx)
{
	if (!ctx->pending_op)
		ctx->pending_op = calloc(1, sizeof(gc_state));
	return (gc_state *)ctx->pending_op;
}

static int gc_split_begin(mdb_dev_ctx *ctx, const gc_table &left, uint64_t n_r_max, bool keys32)
{
	gc_state *st = gc_pending(ctx);
	if (!st)
		return -MIDORIDB_NOMEM;
	gc_request rq = gc_request_of(left, { NULL, NULL, n_r_max }, { NULL, NULL, NULL, 0, NULL, NULL }, true, keys32);
	rq.fast = true;
	rq.records = true;
	if (left.n) {
		/* the window comes from the left table's sample alone: the right table is checked as it is partitioned (a key outside
		 * sends finish() to the unsplit operator, which samples both tables) */
		gc_key_form kf;
		int rc = gc_narrow_guess(ctx, { left, { NULL, NULL, 0 } }, &kf, keys32);
		rq.kf = { kf.narrow, kf.base, { kf.win.kbits, kf.win.lo } };	/* (the window alone: what the sample says of the right table's share means nothing here) */
		if (rc) {
			gc_state_fill(st, rq, false);
			return rc;
		}
	}
	gc_state_fill(st, rq, false);
	if (left.n == 0)
		return MIDORIDB_OK;	/* nothing to prepare; finish() returns the empty result */
	return gc_begin(ctx, st);
}

static int gc_split_finish(mdb_dev_ctx *ctx, const gc_table &right, const gc_out &out, bool keys32)
{
	gc_state *st = gc_pending(ctx);
	if (!st || !st->rq.l.keys)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_group_count_finish without begin");
	if (st->rq.keys32 != keys32)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_group_count_finish: key width differs from begin()");
	gc_request whole = st->rq;	/* the unsplit operator over the same tables (group_count_common makes its plan anew) */
	whole.r = right;
	whole.out = out;
	out.clear();
	int rc = MIDORIDB_OK;
	if (whole.l.n == 0 || right.n == 0) {
		if (st->active)
			rc = mdb_dev_sync(ctx);		/* drain the prepared left partition */
		st->active = false;
		st->rq.l.keys = NULL;
		return rc;
	}
	if (right.n > st->rq.r.n) {
		/* more right rows than announced (a skewed exchange sent this GPU more than its share): the scratch arena was
		 * sized for the announced table - drop the prepared left partition and run the whole operator on the real sizes */
		rc = mdb_dev_sync(ctx);
		st->active = false;
		st->rq.l.keys = NULL;
		if (rc)
			return rc;
		return group_count_common(ctx, &whole);
	}
	rc = gc_finish(ctx, st, right, out);
	st->rq.l.keys = NULL;
	if (rc == GC_RETRY_EXACT || rc == GC_RETRY_DENSE || rc == GC_RETRY_BUILD_L || rc == GC_RETRY_WIDE || rc == GC_RETRY_PLAIN || rc == GC_RETRY_UNKEYED || rc == GC_RETRY_REC64 ||
	    rc == GC_RETRY_TWO_LEVEL || rc == GC_RETRY_NODENSE)	/* skew / huge counts / wide keys: redo the whole operator */
		rc = group_count_common(ctx, &whole);
	return rc;
}

/* ---- one left table, up to three right tables, ONE key: A JOIN B ON a = b JOIN C ON a = c ... GROUP BY a, COUNT(*)
 *
 * The reference runs this shape as a recursive join (executor_select.c:1151-1280) followed by the GROUP BY loop (:1526-1588).
 * Here every table is partitioned once with the same hash; the direct-address leaf kernel counts the rows of every right
 * table into an LDS array of its own, multiplies the counts per key, and the left rows then meet ONE right count as in the
 * two-table operator (COUNT(*) = left rows x the product).  No joined row of any join exists, and the groups are ordered
 * once - where chaining two-table operators (what query_execute() did before, and what this function still does when the
 * keys do not take the compact narrow form, are skewed, or a product of counts outgrows 32 bits) partitions the group keys
 * again and orders twice. */
extern "C" int mdb_dev_join_group_count_multi(mdb_dev_ctx *ctx, const int64_t *keys_l, const uint64_t *null_l, uint64_t n_l, int n_right,
					      const int64_t *const *keys_r, const uint64_t *const *null_r, const uint64_t *n_r, uint32_t flags,
					      int64_t *out_key, int64_t *out_count, uint32_t *out_first, uint64_t cap, uint64_t *out_groups,
					      uint64_t *out_joined)
{
	mdb_plan_scope plan_scope(ctx);
	gc_alias_scope alias_scope_(ctx, flags);
	if (!out_groups || n_right < 1 || n_right > 1 + GC_MAX_EXTRA || !keys_r || !n_r)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_group_count_multi: one to %d right tables", 1 + GC_MAX_EXTRA);
	const gc_out out = { out_key, out_count, out_first, cap, out_groups, out_joined };
	out.clear();
	if (n_right == 1)
		return mdb_dev_join_group_count(ctx, keys_l, null_l, n_l, keys_r[0], null_r ? null_r[0] : NULL, n_r[0], flags, out_key, out_count, out_first,
						cap, out_groups, out_joined);
	mdb_complete_on_return complete_(ctx);	/* (several right tables: complete on return, as the chain below has always been) */
	if (!n_l)
		return MIDORIDB_OK;
	uint64_t smallest = n_l;
	for (int t = 0; t < n_right; t++) {
		if (!n_r[t])
			return MIDORIDB_OK;
		smallest = n_r[t] < smallest ? n_r[t] : smallest;
	}
	int rc = GC_NOT_SERVED;
	gc_request rq = gc_request_of({ keys_l, null_l, n_l }, { keys_r[0], null_r ? null_r[0] : NULL, n_r[0] }, out, true);
	rq.nextra = n_right - 1;
	for (int t = 1; t < n_right; t++)
		rq.x[t - 1] = { keys_r[t], null_r ? null_r[t] : NULL, n_r[t] };
	if (!(flags & MDB_ORDER_FIRST) && !out_first && out_key && smallest >= (1u << 16)) {
		/* no order asked for: every table partitioned once or twice without row ids, the right tables' counts multiplied in
		 * the leaf tables, no ordering sort */
		mdb_memo_switch(ctx, keys_l, n_l, keys_r[0], n_r[0]);
		const int urc = gc_unordered_try(ctx, { rq.l, rq.r }, out, rq.x, rq.nextra);
		if (urc <= 0) {
			if (urc == 0)
				ctx->plan.multi_one_pass = 1;
			return urc;
		}
		out.clear();
	}
	if (smallest >= (1u << 16) && n_l >= (1u << 20)) {	/* (small tables: the chain's single-workgroup and one-level forms are quicker) */
		mdb_memo_switch(ctx, keys_l, n_l, keys_r[0], n_r[0]);
		rc = group_count_common(ctx, &rq);
	}
	if (rc != GC_NOT_SERVED)
		return rc;
	if (ctx->explaining) {	/* (mdb_dev_explain_*: the chain of two-table operators - its first step's plan, multi_one_pass 0) */
		uint64_t g0 = 0, j0 = 0;
		return mdb_dev_join_group_count(ctx, keys_l, null_l, n_l, keys_r[0], null_r ? null_r[0] : NULL, n_r[0], flags, NULL, NULL, NULL, n_l ? n_l : 1, &g0, &j0);
	}
	/* ---- the chain: groups of (L, R0), then (those group keys, R1) ..., counts multiplied */
	*out_groups = 0;
	int64_t *key[2] = { NULL, NULL }, *cnt[3] = { NULL, NULL, NULL };
	uint32_t *first[2] = { NULL, NULL }, *idx = NULL;
	uint64_t G = 0, J = 0;
	const uint64_t room = n_l ? n_l : 1;
	rc = MIDORIDB_OK;
	for (int i = 0; i < 2 && !rc; i++) {
		rc = mdb_dev_alloc(ctx, room * 8, (void **)&key[i]);
		if (!rc)
			rc = mdb_dev_alloc(ctx, room * 4, (void **)&first[i]);
	}
	for (int i = 0; i < 3 && !rc; i++)
		rc = mdb_dev_alloc(ctx, room * 8, (void **)&cnt[i]);
	if (!rc)
		rc = mdb_dev_alloc(ctx, room * 4, (void **)&idx);
	int cur = 0;		/* key[cur], cnt[cur], first[cur]: the groups so far */
	if (!rc)
		rc = mdb_dev_join_group_count(ctx, keys_l, null_l, n_l, keys_r[0], null_r ? null_r[0] : NULL, n_r[0], flags, key[0], cnt[0], first[0], room, &G,
					      &J);
	for (int t = 1; t < n_right && !rc && G; t++) {
		uint64_t G2 = 0, J2 = 0;
		const int nxt = cur ^ 1;
		rc = mdb_dev_join_group_count(ctx, key[cur], NULL, G, keys_r[t], null_r ? null_r[t] : NULL, n_r[t], flags, key[nxt], cnt[2], idx, room, &G2,
					      &J2);
		if (!rc)
			rc = mdb_dev_combine_counts(ctx, cnt[cur], first[cur], idx, cnt[2], G2, cnt[nxt], first[nxt], &J);
		cur = nxt;
		G = G2;
	}
	if (!rc && G > cap)
		rc = mdb_set_err(ctx, -MIDORIDB_ERROR, "group output capacity %llu too small for %llu groups", (unsigned long long)cap, (unsigned long long)G);
	if (!rc && G) {
		hipError_t e = hipMemcpyAsync(out_count, cnt[cur], G * 8, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess && out_key)
			e = hipMemcpyAsync(out_key, key[cur], G * 8, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess && out_first)
			e = hipMemcpyAsync(out_first, first[cur], G * 4, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess)
			e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess)
			rc = mdb_set_err(ctx, -MIDORIDB_INTERNAL, "join_group_count_multi: %s", hipGetErrorString(e));
	}
	for (int i = 0; i < 2; i++) {
		(void)mdb_dev_free(ctx, key[i]);
		(void)mdb_dev_free(ctx, first[i]);
	}
	for (int i = 0; i < 3; i++)
		(void)mdb_dev_free(ctx, cnt[i]);
	(void)mdb_dev_free(ctx, idx);
	if (!rc) {
		*out_groups = G;
		if (out_joined)
			*out_joined = G ? J : 0;
	}
	return rc;
}

extern "C" int mdb_dev_join_group_count_begin(mdb_dev_ctx *ctx, const int64_t *keys_l, const uint64_t *null_l, uint64_t n_l,
					      uint64_t n_r_max)
{
	mdb_plan_scope plan_scope(ctx);
	return gc_split_begin(ctx, { keys_l, null_l, n_l }, n_r_max, false);
}

extern "C" int mdb_dev_join_group_count_finish(mdb_dev_ctx *ctx, const int64_t *keys_r, const uint64_t *null_r, uint64_t n_r,
					       uint32_t flags, int64_t *out_key, int64_t *out_count, uint32_t *out_first,
					       uint64_t cap, uint64_t *out_groups, uint64_t *out_joined)
{
	mdb_plan_scope plan_scope(ctx);
	(void)flags;
	return gc_split_finish(ctx, { keys_r, null_r, n_r }, { out_key, out_count, out_first, cap, out_groups, out_joined }, false);
}

/* ---- int32 key columns (what arrives over xGMI in the 4-byte wire format): same operator, no widening pass ---- */

extern "C" int mdb_dev_join_group_count_i32(mdb_dev_ctx *ctx, const int32_t *keys_l, uint64_t n_l, const int32_t *keys_r, uint64_t n_r,
					    uint32_t flags, int64_t *out_key, int64_t *out_count, uint32_t *out_first, uint64_t cap,
					    uint64_t *out_groups, uint64_t *out_joined)
{
	mdb_plan_scope plan_scope(ctx);
	(void)flags;
	mdb_memo_switch(ctx, keys_l, n_l, keys_r, n_r);
	gc_request rq = gc_request_of({ reinterpret_cast<const int64_t *>(keys_l), NULL, n_l }, { reinterpret_cast<const int64_t *>(keys_r), NULL, n_r },
				      { out_key, out_count, out_first, cap, out_groups, out_joined }, true, true);
	return group_count_common(ctx, &rq);
}

extern "C" int mdb_dev_join_group_count_begin_i32(mdb_dev_ctx *ctx, const int32_t *keys_l, uint64_t n_l, uint64_t n_r_max)
{
	mdb_plan_scope plan_scope(ctx);
	return gc_split_begin(ctx, { reinterpret_cast<const int64_t *>(keys_l), NULL, n_l }, n_r_max, true);
}

extern "C" int mdb_dev_join_group_count_finish_i32(mdb_dev_ctx *ctx, const int32_t *keys_r, uint64_t n_r, uint32_t flags,
						   int64_t *out_key, int64_t *out_count, uint32_t *out_first, uint64_t cap,
						   uint64_t *out_groups, uint64_t *out_joined)
{
	mdb_plan_scope plan_scope(ctx);
	(void)flags;
	return gc_split_finish(ctx, { reinterpret_cast<const int64_t *>(keys_r), NULL, n_r }, { out_key, out_count, out_first, cap, out_groups, out_joined }, true);
}

extern "C" int mdb_dev_group_count(mdb_dev_ctx *ctx, const int64_t *keys, const uint64_t *nullbits, uint64_t n, uint32_t flags,
				   uint32_t *out_first, int64_t *out_count, uint64_t cap, uint64_t *out_groups)
{
	mdb_plan_scope plan_scope(ctx);
	(void)flags;
	*out_groups = 0;
	/* The catalog says no value occurs twice in this NULL-free column (MDB_COL_DISTINCT: measured at ingest over all rows, followed through
	 * every append, dropped with an UPDATE): every row is the first and only row of its group - the reference's loop
	 * (/root/reference/src/engine/executor_select.c:1526-1588) would find no second row for any key.  Written without looking at a key:
	 * 12 bytes per row.  (The one form that TRUSTS a statistic: verifying it is the scan that measured it.) */
	if (ctx->cs_on && !ctx->explain_as_sample && ctx->cs_kl == keys && !ctx->cs_has_r && (ctx->cs_l.flags & MDB_COL_DISTINCT) && !nullbits && n && n <= cap &&
	    n < 0xFFFFFFFFull && !mdb_knob_off("MDB_GROUP_IDENTITY")) {
		if (!ctx->explaining) {
			int rc = mdb_group_identity(ctx, n, out_first, out_count);
			if (rc)
				return rc;
			*out_groups = n;
		}
		ctx->plan.from_stats = 1;
		ctx->plan.group_form = 3;
		return MIDORIDB_OK;
	}
	mdb_memo_switch(ctx, keys, n, NULL, 0);
	const gc_sides sides = { { keys, nullbits, n }, { NULL, NULL, 0 } };
	const gc_out out = { NULL, out_count, out_first, cap, out_groups, NULL };
	const int trc = tiny_group_count(ctx, sides, false, true, out);
	if (trc <= 0)
		return trc;
	const int drc = group_direct_try(ctx, sides, true, out);
	if (drc <= 0)
		return drc;
	*out_groups = 0;
	const int hrc = group_hashed_try(ctx, sides.l, true, out);
	if (hrc <= 0)
		return hrc;
	*out_groups = 0;
	/* round 5: a NULL-free key column inside a compact window of 2^18 ... 2^25 values goes through the band sort (mdb_dev_bandgroup.hip):
	 * one pass of 4-byte row words instead of 8-byte ones (and, MDB_GROUP_TILED=1, the tile sort of mdb_dev_rowjoin.hip: windows of 2^13 ... 2^27) */
	if (!nullbits && n >= ((uint64_t)1 << 21) && ctx->narrow_mode != 0 && !ld_disabled()) {
		const int brc = gc_windowed_try(ctx, sides, ctx->nh_distrust > 0, GC_WINDOW_BOTH, true, [&](int64_t wlo, uint32_t kb) -> int {
			bool outside = false;
			int rc = mdb_group_count_banded(ctx, keys, n, wlo, kb, out_first, out_count, cap, out_groups, &outside);
			if (rc <= 0)
				return rc;
			*out_groups = 0;
			if (!outside) {
				rc = mdb_group_count_tiled(ctx, keys, n, wlo, kb, out_first, out_count, cap, out_groups, &outside);
				if (rc <= 0)
					return rc;
				*out_groups = 0;
			}
			return outside ? GC_FORM_KEY_OUTSIDE : GC_FORM_NOT_SERVED;
		});
		if (brc <= 0)
			return brc;
	}
	gc_request rq = gc_request_of(sides.l, sides.r, out, false);
	return group_count_common(ctx, &rq);
}

/* ------------------------------------------------------------------ plans as data (include/mdb_dev.h: mdb_dev_explain_*)
 *
 * A context without a device - only what the decision code reads (CU count, key-form mode, an empty memo) - gets the caller's statistics
 * under two made-up column addresses, ctx->explaining is set, and the operator's ENTRY POINT is called: every path it takes stops where
 * it would launch (tiny_group_count, group_direct_try, group_count_run behind gc_begin).  The plan record it leaves is the answer. */
#define EXPLAIN_KL ((const int64_t *)0x1000)
#define EXPLAIN_KR ((const int64_t *)0x2000)
#define EXPLAIN_KX ((const int64_t *)0x3000)

static mdb_dev_ctx *explain_ctx(const struct mdb_dev_explain_request *rq, bool has_r)
{
	mdb_dev_ctx *ctx = new (std::nothrow) mdb_dev_ctx();
	if (!ctx)
		return NULL;
	memo_reset(*ctx);
	ctx->device = -1;
	ctx->num_cus = rq->num_cus ? (int)rq->num_cus : 256;
	ctx->narrow_mode = 1;
	ctx->err[0] = 0;
	ctx->explaining = true;
	ctx->explain_as_sample = rq->as_sample != 0;
	ctx->cs_on = true;
	ctx->cs_kl = EXPLAIN_KL;
	ctx->cs_l = rq->left;
	ctx->cs_has_r = has_r;
	if (has_r) {
		ctx->cs_kr = EXPLAIN_KR;
		ctx->cs_r = rq->right;
	}
	return ctx;
}

extern "C" int mdb_dev_explain_join_group_count(const struct mdb_dev_explain_request *rq, struct mdb_dev_plan_info *out)
{
	if (!rq || !out || rq->further_tables > 2)
		return -MIDORIDB_ERROR;
	mdb_dev_ctx *ctx = explain_ctx(rq, true);
	if (!ctx)
		return -MIDORIDB_NOMEM;
	const uint64_t n_l = rq->left.rows, n_r = rq->right.rows;
	const uint64_t *null_l = rq->left_nulls_bitmap ? (const uint64_t *)0x4000 : NULL;
	uint64_t groups = 0, joined = 0;
	int rc;
	if (rq->further_tables) {
		const int64_t *rk[3] = { EXPLAIN_KR, EXPLAIN_KX, EXPLAIN_KX + 0x1000 };
		const uint64_t *rn[3] = { NULL, NULL, NULL };
		const uint64_t rows[3] = { n_r, rq->further_rows[0], rq->further_rows[1] };
		rc = mdb_dev_join_group_count_multi(ctx, EXPLAIN_KL, null_l, n_l, 1 + (int)rq->further_tables, rk, rn, rows, MDB_ORDER_FIRST, NULL, NULL, NULL,
						    n_l, &groups, &joined);
	} else {
		rc = mdb_dev_join_group_count(ctx, EXPLAIN_KL, null_l, n_l, EXPLAIN_KR, NULL, n_r, MDB_ORDER_FIRST, NULL, NULL, NULL, n_l, &groups, &joined);
	}
	if (rc && mdb_knob_set("MDB_DEBUG_EXPLAIN"))
		fprintf(stderr, "mdb_dev_explain_join_group_count: %d (%s)\n", rc, ctx->err);
	*out = ctx->plan;
	delete ctx;
	return rc;
}

extern "C" int mdb_dev_explain_join_payload(const struct mdb_dev_explain_request *rq, int cells, struct mdb_dev_plan_info *out)
{
	if (!rq || !out || cells < 1 || cells > 2)
		return -MIDORIDB_ERROR;
	mdb_dev_ctx *ctx = explain_ctx(rq, true);
	if (!ctx)
		return -MIDORIDB_NOMEM;
	const void *pay[2] = { (const void *)0x5000, (const void *)0x6000 };
	void *dst[2] = { (void *)0x7000, (void *)0x8000 };
	if (rq->further_tables) {	/* several right tables on the one key: mdb_dev_join_payload_multi, the window = the statistics' ranges */
		struct mdb_dev_payload_right rt[3];
		memset(rt, 0, sizeof(rt));
		int64_t lo = rq->left.min < rq->right.min ? rq->left.min : rq->right.min, hi = rq->left.max > rq->right.max ? rq->left.max : rq->right.max;
		const uint32_t nrt = 1u + (rq->further_tables > 2u ? 2u : rq->further_tables);
		for (uint32_t t = 0; t < nrt; t++) {
			rt[t].keys = EXPLAIN_KR;
			rt[t].rows = t ? rq->further_rows[t - 1] : rq->right.rows;
			rt[t].npay = cells;
			for (int c = 0; c < cells; c++) {
				rt[t].pay_in[c] = pay[c];
				rt[t].out[c] = dst[c];
			}
		}
		int mrc = rq->left_nulls_bitmap ? 1 : mdb_dev_join_payload_multi(ctx, EXPLAIN_KL, NULL, rq->left.rows, rt, (int)nrt, lo, hi);
		if (mrc == 1)
			mrc = MIDORIDB_OK;	/* (not served: payload_form 0 - the caller joins table by table) */
		*out = ctx->plan;
		delete ctx;
		return mrc;
	}
	int rc = mdb_dev_join_payload(ctx, EXPLAIN_KL, rq->left_nulls_bitmap ? (const uint64_t *)0x4000 : NULL, rq->left.rows, EXPLAIN_KR, NULL, rq->right.rows, pay,
				      cells, dst);
	if (rc == 1)
		rc = MIDORIDB_OK;	/* (not served: payload_form 0 - mdb_dev_join_pairs and a gather answer) */
	*out = ctx->plan;
	delete ctx;
	return rc;
}

extern "C" int mdb_dev_explain_group_count(const struct mdb_dev_explain_request *rq, struct mdb_dev_plan_info *out)
{
	if (!rq || !out)
		return -MIDORIDB_ERROR;
	mdb_dev_ctx *ctx = explain_ctx(rq, false);
	if (!ctx)
		return -MIDORIDB_NOMEM;
	uint64_t groups = 0;
	const int rc = mdb_dev_group_count(ctx, EXPLAIN_KL, rq->left_nulls_bitmap ? (const uint64_t *)0x4000 : NULL, rq->left.rows, MDB_ORDER_FIRST, NULL, NULL,
					   rq->left.rows, &groups);
	*out = ctx->plan;
	delete ctx;
	return rc;
}
