/*
 * mdb_dev_keyform.hip - the key sample and the key form it decides (split off mdb_dev_join.hip; what the files share:
 * mdb_dev_join_internal.h): k_key_sample and gc_sample_range (the sampled key range of one or two columns, remembered by the columns),
 * gc_compact_window, gc_narrow_guess / gc_narrow_note (narrow form, compact window, pruning hints), gc_learned_selective.  The fused
 * join + GROUP BY (mdb_dev_join.hip, mdb_dev_join_small.hip), the plain GROUP BY fast paths (mdb_dev_groupby.hip) and the materialising
 * joins (mdb_dev_pairs.hip) all decide their key form here; the sample-window-form retry they share, gc_windowed_try, is a template and
 * stands in the header.
 */
#include "mdb_dev_join_internal.h"

/* ---- narrow form: 32-bit hashes when every key of both tables lies inside the int32 range -------------------------
 *
 * The reference's integers are 32-bit in practice (literals go through atoi, compares through int: SURVEY D5), and a
 * key column of such values does not need 8-byte hashes plus 4-byte row ids on its way through the two partition
 * levels: the left side travels as ONE word (hash32 << 32 | row id), 8 instead of 12 bytes per row and pass.  Nothing
 * is assumed: the first partition level checks every key it reads and raises status bit 7 on the first one outside the
 * range, and the operator is then redone with 64-bit hashes (GC_RETRY_WIDE).  To keep that retry for adversarial
 * inputs only, 2 x 4096 evenly spaced keys are looked at first (one tiny kernel + one sync, paid only by tables large
 * enough for the bytes to matter).  mdb_dev_set_narrow_keys(): 0 never, 1 as described (default), 2 always try. */

__device__ static inline long long gc_wave_min_i64(long long v)
{
#pragma unroll
	for (int d = 1; d < MDB_WAVE; d <<= 1) {
		const long long o = __shfl_xor(v, d, MDB_WAVE);
		v = o < v ? o : v;
	}
	return v;
}

__device__ static inline long long gc_wave_max_i64(long long v)
{
#pragma unroll
	for (int d = 1; d < MDB_WAVE; d <<= 1) {
		const long long o = __shfl_xor(v, d, MDB_WAVE);
		v = o > v ? o : v;
	}
	return v;
}

/* mm[0] = smallest, mm[1] = largest of 2 x GC_NARROW_SAMPLE evenly spaced non-NULL keys */
template <typename K>	/* int64_t, or int32_t for key columns that crossed xGMI in the 4-byte wire format */
__global__ void k_key_sample(const K *__restrict__ kl, const uint64_t *__restrict__ nl_bits, uint64_t nl,
			     const K *__restrict__ kr, const uint64_t *__restrict__ nr_bits, uint64_t nr, long long *mm)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	long long lo = 0x7FFFFFFFFFFFFFFFll, hi = -0x7FFFFFFFFFFFFFFFll - 1;
	if (t < GC_NARROW_SAMPLE) {
		if (nl) {
			const uint64_t i = gc_sample_pos(t, nl);
			if (!(nl_bits && mdb_bit_is_set(nl_bits, i))) {
				lo = kl[i];
				hi = kl[i];
			}
		}
		if (kr && nr) {
			const uint64_t j = gc_sample_pos(t, nr);
			if (!(nr_bits && mdb_bit_is_set(nr_bits, j))) {
				const long long v = kr[j];
				lo = v < lo ? v : lo;
				hi = v > hi ? v : hi;
			}
		}
	}
	lo = gc_wave_min_i64(lo);
	hi = gc_wave_max_i64(hi);
	if (mdb_lane() == 0 && lo <= hi) {
		atomicMin(&mm[0], lo);
		atomicMax(&mm[1], hi);
	}
	/* the two tables' own ranges (mm[2..3] left, mm[4..5] right): how much of the left table's key range the right one covers */
	long long llo = 0x7FFFFFFFFFFFFFFFll, lhi = -0x7FFFFFFFFFFFFFFFll - 1, rlo = llo, rhi = lhi;
	if (t < GC_NARROW_SAMPLE) {
		if (nl) {
			const uint64_t i = gc_sample_pos(t, nl);
			if (!(nl_bits && mdb_bit_is_set(nl_bits, i)))
				llo = lhi = kl[i];
		}
		if (kr && nr) {
			const uint64_t j = gc_sample_pos(t, nr);
			if (!(nr_bits && mdb_bit_is_set(nr_bits, j)))
				rlo = rhi = kr[j];
		}
	}
	llo = gc_wave_min_i64(llo);
	lhi = gc_wave_max_i64(lhi);
	rlo = gc_wave_min_i64(rlo);
	rhi = gc_wave_max_i64(rhi);
	if (mdb_lane() == 0) {
		if (llo <= lhi) {
			atomicMin(&mm[2], llo);
			atomicMax(&mm[3], lhi);
		}
		if (rlo <= rhi) {
			atomicMin(&mm[4], rlo);
			atomicMax(&mm[5], rhi);
		}
	}
}

/* smallest / largest of 2 x GC_NARROW_SAMPLE evenly spaced non-NULL keys (lo > hi: nothing but NULLs); remembered by the
 * columns, so that the decisions that need it (narrow form, direct tables) share one kernel + sync, and a repeated query
 * pays none.  fresh: take the sample again (a remembered verdict just proved wrong). */
int gc_sample_range(mdb_dev_ctx *ctx, const gc_sides &s, bool fresh, int64_t *lo, int64_t *hi, bool keys32)
{
	const int64_t *keys_l = s.l.keys, *keys_r = s.r.keys;
	const uint64_t n_l = s.l.n, n_r = keys_r ? s.r.n : 0;
	if (ctx->cs_on && ctx->cs_kl == keys_l && (!keys_r || (ctx->cs_has_r && ctx->cs_kr == keys_r)) && !keys32) {
		/* the caller's statistics of exactly these columns (mdb_dev_call_stats): what a sample would estimate, known - no kernel, no
		 * synchronisation, nothing remembered by address */
		const struct mdb_dev_col_stats &l = ctx->cs_l, &r = ctx->cs_r;
		const bool has_l = n_l && l.min <= l.max, has_r = keys_r && n_r && r.min <= r.max;
		*lo = INT64_MAX;
		*hi = INT64_MIN;
		if (has_l) {
			*lo = l.min;
			*hi = l.max;
		}
		if (has_r) {
			*lo = r.min < *lo ? r.min : *lo;
			*hi = r.max > *hi ? r.max : *hi;
		}
		ctx->sr_span_l = has_l ? (uint64_t)l.max - (uint64_t)l.min + 1 : 0;
		ctx->sr_span_r = has_r ? (uint64_t)r.max - (uint64_t)r.min + 1 : 0;
		if (has_l && !ctx->sr_span_l)
			ctx->sr_span_l = ~0ull;		/* (the whole int64 range) */
		if (has_r && !ctx->sr_span_r)
			ctx->sr_span_r = ~0ull;
		ctx->sr_rlo = has_r ? r.min : INT64_MAX;
		ctx->sr_rhi = has_r ? r.max : INT64_MIN;
		ctx->vd[VD_SAMPLE].note(keys_l, n_l, keys_r, n_r);
		ctx->sr_lo = *lo;
		ctx->sr_hi = *hi;
		ctx->plan.from_stats = 1;
		return MIDORIDB_OK;
	}
	if (!fresh && ctx->vd[VD_SAMPLE].serve(keys_l, n_l, keys_r, n_r, MDB_HINT_SERVES)) {
		*lo = ctx->sr_lo;
		*hi = ctx->sr_hi;
		return MIDORIDB_OK;
	}
	long long *mm = (long long *)(ctx->d_status + GC_STW_SAMPLE);
	int64_t *h = (int64_t *)ctx->h_pinned;
	for (int i = 0; i < 6; i += 2) {
		h[i] = INT64_MAX;
		h[i + 1] = INT64_MIN;
	}
	MDB_HIP(ctx, hipMemcpyAsync(mm, h, 48, hipMemcpyHostToDevice, ctx->stream));
	ctx->plan.samples++;
	if (keys32) {
		MDB_LAUNCH(ctx, "key_sample", k_key_sample<int32_t>, GC_NARROW_SAMPLE / 256, 256, reinterpret_cast<const int32_t *>(keys_l), s.l.nulls, n_l,
			   reinterpret_cast<const int32_t *>(keys_r), s.r.nulls, n_r, mm);
	} else {
		MDB_LAUNCH(ctx, "key_sample", k_key_sample<int64_t>, GC_NARROW_SAMPLE / 256, 256, keys_l, s.l.nulls, n_l, keys_r, s.r.nulls, n_r, mm);
	}
	MDB_HIP(ctx, hipMemcpyAsync(h, mm, 48, hipMemcpyDeviceToHost, ctx->stream));
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	*lo = h[0];
	*hi = h[1];
	/* spans of the two tables' sampled keys (0 = nothing sampled) */
	ctx->sr_span_l = h[2] <= h[3] ? (uint64_t)h[3] - (uint64_t)h[2] + 1 : 0;
	ctx->sr_span_r = h[4] <= h[5] ? (uint64_t)h[5] - (uint64_t)h[4] + 1 : 0;
	ctx->sr_rlo = h[4];
	ctx->sr_rhi = h[5];
	ctx->vd[VD_SAMPLE].note(keys_l, n_l, keys_r, n_r);
	ctx->sr_lo = *lo;
	ctx->sr_hi = *hi;
	return MIDORIDB_OK;
}

/* what was decided for these columns, for the next call over them (gc_narrow_guess serves it) */
void gc_narrow_note(mdb_dev_ctx *ctx, const gc_sides &s, bool narrow, int64_t base, uint32_t key_bits, int64_t key_lo)
{
	ctx->nh_kbits = narrow ? key_bits : 0u;
	ctx->nh_lo = key_lo;
	ctx->vd[VD_NARROW].note(s.l.keys, s.l.n, s.r.keys, s.r.keys ? s.r.n : 0);
	ctx->nh_result = narrow ? 1 : 0;
	ctx->nh_base = base;
}

/* what the previous join over the same columns learned: few groups for many left rows (every use is exact whatever it says:
 * the bitmap filter only drops rows that can have no partner) */
bool gc_learned_selective(const mdb_dev_ctx *ctx, const gc_sides &s)
{
	return !ctx->lg_nextra && ctx->vd[VD_LAST_GROUPS].holds(s.l.keys, s.l.n, s.r.keys, s.r.n) && s.r.keys && ctx->lg_groups < s.l.n / 4;
}

/* The compact window offered by a key sample [lo, hi]: the sampled span, padded by a sixteenth of itself + 4096 on either
 * side for the extremes the sample missed, rounded up to a power of two (the slack is split between the two ends).
 * *kbits = 0: none (span of 2^31 or more, or nothing but NULLs sampled).
 * exact: [lo, hi] is the catalog's range of the column (every key lies inside), not a sample's: no margin around it */
void gc_compact_window(int64_t lo, int64_t hi, uint32_t *kbits, int64_t *wlo, bool exact)
{
	*kbits = 0;
	*wlo = 0;
	if (lo > hi)
		return;
	const uint64_t span = (uint64_t)hi - (uint64_t)lo;
	if (span >= (1ull << 31))
		return;
	const uint64_t pad = exact ? 0 : span / 16 + 4096, need = span + 2 * pad + 1;
	uint32_t k = 8;
	while ((1ull << k) < need)
		k++;
	if (k > 31)
		return;
	*kbits = k;
	*wlo = (int64_t)((uint64_t)lo - pad - (((1ull << k) - need) >> 1));
}

/* the decision from the sample, the memo or the caller's statistics (gc_narrow_guess: and what int32 columns make of it) */
static int narrow_guess_int64(mdb_dev_ctx *ctx, const gc_sides &s, gc_key_form *kf, bool keys32, bool prune_ok)
{
	const int64_t *keys_r = s.r.keys;
	const uint64_t n_l = s.l.n, n_r = s.r.n;
	gc_window *win = &kf->win;
	memset(kf, 0, sizeof(*kf));	/* the wide form, no window, no hints */
	prune_ok = prune_ok && !mdb_knob_off("MDB_MINMAX_PRUNE");
	if (ctx->narrow_mode == 0 && n_l && keys_r && n_r && prune_ok && n_l + n_r >= GC_NARROW_MIN_ROWS) {
		/* the narrow forms are switched off, min-max pruning is not: what the key sample says about the two tables' ranges */
		int64_t lo = 0, hi = 0;
		const int src = gc_sample_range(ctx, s, false, &lo, &hi, keys32);
		if (src)
			return src;
		win->by_span = ctx->sr_span_l && ctx->sr_span_r && ctx->sr_span_r < ctx->sr_span_l / 4;
		win->prunable = ctx->sr_span_l && ctx->sr_span_r && ctx->sr_span_r / 7 < ctx->sr_span_l / 8;
	}
	if (ctx->narrow_mode == 0 || n_l == 0)
		return MIDORIDB_OK;
	if (ctx->narrow_mode == 2) {
		kf->narrow = true;
		return MIDORIDB_OK;
	}
	if (n_l + (keys_r ? n_r : 0) < GC_NARROW_MIN_ROWS)
		return MIDORIDB_OK;
	bool fresh = false;
	ctx->guess_remembered = false;
	const bool by_stats = ctx->cs_on && ctx->cs_kl == s.l.keys && (!keys_r || (ctx->cs_has_r && ctx->cs_kr == keys_r)) && !keys32;
	if (by_stats) {
		/* (decided afresh from the caller's statistics every time: it costs nothing and depends on nothing remembered) */
	} else if (ctx->nh_distrust > 0) {
		ctx->nh_distrust--;
		fresh = true;
	} else if (!(ctx->nh_r_based && !prune_ok) &&	/* (a window of the right table's keys alone is no use to a call that cannot prune) */
		   ctx->vd[VD_NARROW].serve(s.l.keys, n_l, keys_r, keys_r ? n_r : 0, MDB_HINT_SERVES)) {
		kf->narrow = ctx->nh_result == 1;	/* same columns as last time: what held then (gc_narrow_note) */
		ctx->guess_remembered = true;
		kf->base = ctx->nh_base;
		if (kf->narrow) {
			win->kbits = ctx->nh_kbits;
			win->lo = ctx->nh_lo;
			win->selective = ctx->nh_selective || gc_learned_selective(ctx, s);
			win->r_based = ctx->nh_r_based;
		}
		win->by_span = ctx->nh_by_span;		/* (the 64-bit form prunes by the key range as well) */
		win->prunable = ctx->nh_prunable;
		return MIDORIDB_OK;
	}
	int64_t lo = 0, hi = 0;
	const int src = gc_sample_range(ctx, s, fresh, &lo, &hi, keys32);
	if (src)
		return src;
	if (lo > hi) {
		kf->narrow = true;		/* nothing but NULLs in the sample */
	} else if (lo >= -(1ll << 31) && hi < (1ll << 31)) {
		kf->narrow = true;
	} else if ((uint64_t)hi - (uint64_t)lo < (1ull << 31)) {
		/* a window anywhere in the int64 range (surrogate keys that start at 10^12, timestamps ...): centred on the
		 * sample, so that keys up to 2^30 beyond either end of what was sampled still fit */
		kf->narrow = true;
		kf->base = (int64_t)((uint64_t)lo + (((uint64_t)hi - (uint64_t)lo) >> 1));
	}
	uint32_t kb = 0;
	int64_t wlo = 0;
	if (kf->narrow)
		gc_compact_window(lo, hi, &kb, &wlo);
	const bool by_span = keys_r && n_r && ctx->sr_span_l && ctx->sr_span_r && ctx->sr_span_r < ctx->sr_span_l / 4;
	/* ... or the last join over these very columns found a partner for under a quarter of the left rows: a right table of few
	 * distinct keys spread over the left table's whole range (no sample of 4096 keys shows that) */
	const bool selective = keys_r && n_r && (by_span || n_r < n_l / 4 || gc_learned_selective(ctx, s));
	const bool prunable = keys_r && n_r && ctx->sr_span_l && ctx->sr_span_r && ctx->sr_span_r / 7 < ctx->sr_span_l / 8;
	/* the right table covers a small part of the left table's range and min-max pruning will drop the left rows outside it:
	 * the compact window need only cover the RIGHT table's keys (variant D: 23 key bits instead of 27 - 4096 leaves of
	 * 24 000 right rows instead of 32 768 leaves of 3 000: the leaf kernel's fixed price per leaf, 0.29 -> 0.13 ms) */
	bool r_based = false;
	if (kf->narrow && by_span && prune_ok) {
		uint32_t kb2 = 0;
		int64_t wlo2 = 0;
		gc_compact_window(ctx->sr_rlo, ctx->sr_rhi, &kb2, &wlo2);
		if (kb2 && (!kb || kb2 < kb)) {
			kb = kb2;
			wlo = wlo2;
			r_based = true;
		}
	}
	ctx->nh_r_based = r_based;
	*win = { kb, wlo, selective, by_span, prunable, r_based, false };
	ctx->nh_by_span = by_span;
	ctx->nh_prunable = prunable;
	gc_narrow_note(ctx, s, kf->narrow, kf->base, kb, wlo);
	ctx->nh_selective = selective;
	return MIDORIDB_OK;
}

/* The key form of a call over these columns (gc_key_form); win.fast1 is the caller's.  int32 columns (keys32) are inside the plain narrow
 * form's window whatever the sample says; the sample offers the compact one. */
int gc_narrow_guess(mdb_dev_ctx *ctx, const gc_sides &s, gc_key_form *kf, bool keys32, bool prune_ok)
{
	const int rc = narrow_guess_int64(ctx, s, kf, keys32, prune_ok);
	if (!rc && keys32) {
		if (!kf->narrow)
			kf->win.kbits = 0;
		kf->narrow = ctx->narrow_mode != 0;
		kf->base = 0;
	}
	return rc;
}
