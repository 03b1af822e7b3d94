/*
 * mdb_dev_joinkey.hip - composite equi-join keys: ON a.x = b.x AND a.y = b.y [AND ...] as ONE 8-byte key per row, so that the
 * single-key join operators (mdb_dev_join_pairs) answer the whole conjunction at once instead of joining on the first equality
 * and filtering the pairs by the others (the reference evaluates the whole ON expression per pair:
 * src/engine/executor_select.c:1128).  Round 6 did the same for GROUP BY / DISTINCT over several columns (mdb_dev_sort.hip,
 * k_sort_pack); here every side is packed on its own, against a layout both sides share.
 *
 *   mdb_dev_join_key_layout  pure host: the bit field of every column pair from the two sides' value ranges
 *   mdb_dev_join_key_pack    one streaming kernel per side: key = sum (v_c - lo_c) << shift_c, a row with a NULL cell, without a
 *                            row (MDB_NO_ROW) or with a value outside its field gets no key (NULL bit set): it can match nothing
 *   mdb_dev_join_key_unpack  the way back, one streaming kernel: packed group keys -> the key columns (the fused join + GROUP BY
 *                            operator on a packed key, mdb_exec.c: composite_fused_plan)
 */
#include "mdb_dev_common.h"

/* ------------------------------------------------------------------ the layout (host only, no device, no context) */

static inline uint32_t jk_bit_length(uint64_t v)
{
	return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u;
}

extern "C" int mdb_dev_join_key_layout(const struct mdb_dev_col_stats *l, const struct mdb_dev_col_stats *r, int k, struct mdb_join_key_layout *out)
{
	if (!l || !r || !out || k < 0)
		return -MIDORIDB_ERROR;
	memset(out, 0, sizeof(*out));
	for (int c = 0; c < k && out->ntaken < MDB_JOIN_KEY_MAX_COLS; c++) {
		const uint32_t i = out->ntaken;
		if (l[c].min > l[c].max || r[c].min > r[c].max) {	/* a side without a non-NULL value: a field of one value, and nothing matches */
			out->empty = 1;
			out->taken[i] = c;
			out->lo[i] = 0;
			out->span[i] = 0;
			out->bits[i] = 0;
			out->ntaken++;
			continue;
		}
		const int64_t lo = l[c].min > r[c].min ? l[c].min : r[c].min;
		const int64_t hi = l[c].max < r[c].max ? l[c].max : r[c].max;
		if (lo > hi) {						/* the ranges do not intersect: the same */
			out->empty = 1;
			out->taken[i] = c;
			out->lo[i] = lo;
			out->span[i] = 0;
			out->bits[i] = 0;
			out->ntaken++;
			continue;
		}
		const uint64_t span = (uint64_t)hi - (uint64_t)lo;	/* (unsigned: [INT64_MIN, INT64_MAX] is 2^64 - 1, no signed overflow) */
		const uint32_t bits = jk_bit_length(span);
		if (out->total_bits + bits > 63)
			continue;					/* does not fit: stays a residual; later columns may still fit */
		out->taken[i] = c;
		out->lo[i] = lo;
		out->span[i] = span;
		out->bits[i] = bits;
		out->total_bits += bits;
		out->ntaken++;
	}
	uint32_t below = 0;
	for (int i = (int)out->ntaken - 1; i >= 0; i--) {		/* the first taken column is the most significant */
		out->shift[i] = below;
		below += out->bits[i];
	}
	return MIDORIDB_OK;
}

/* ------------------------------------------------------------------ the pack kernel
 *
 * Every lane packs TWO consecutive rows per round (one 16-byte load per column that is read without a row-id vector, one 16-byte
 * store of the keys), a wave 128 consecutive rows = two whole words of the NULL bitmap: the two ballots (even rows, odd rows) are
 * interleaved in scalar registers and lane 0 stores the words - no atomics on the bitmap, no memset, and the unused bits of the
 * last word are 0 because a row behind n never votes.  Rows without a key are counted per wave from the same ballots, summed per
 * workgroup in ONE 4-byte LDS word and added to the total with one atomic per workgroup.
 * Columns read without a row-id vector are read exactly once: non-temporal loads; columns read through one are gathers (rows may
 * repeat): plain loads. */
#define JK_THREADS 256u
#define JK_ROUNDS 4u
#define JK_ROWS_PER_ROUND (JK_THREADS * 2u)
#define JK_ROWS_PER_WG (JK_ROWS_PER_ROUND * JK_ROUNDS)
#define JK_NO_SLOT 0xFFu

struct jk_args {
	const int64_t *vals[MDB_JOIN_KEY_MAX_COLS];
	const uint64_t *nulls[MDB_JOIN_KEY_MAX_COLS];
	const uint32_t *rid[MDB_JOIN_KEY_MAX_COLS];	/* the DISTINCT row-id vectors of the call, nrid of them */
	int64_t lo[MDB_JOIN_KEY_MAX_COLS];
	uint64_t span[MDB_JOIN_KEY_MAX_COLS];
	uint32_t shift[MDB_JOIN_KEY_MAX_COLS];
	uint8_t slot[MDB_JOIN_KEY_MAX_COLS];		/* which of rid[] column c is read through, JK_NO_SLOT: row i is stream position i */
	uint32_t nrid;
	uint32_t vec_in;				/* bit c: vals[c] is 16-byte aligned (one 16-byte load per lane) */
	uint32_t vec_out;				/* out_key is 16-byte aligned */
	uint64_t n;
	int64_t *out_key;
	uint64_t *out_null;
	unsigned long long *out_nulls;
};

typedef unsigned long long jk_ull2 __attribute__((ext_vector_type(2)));

/* bit i of the result's even positions = bit i of x */
__device__ static inline uint64_t jk_spread(uint32_t x32)
{
	uint64_t x = x32;
	x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
	x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
	x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
	x = (x | (x << 2)) & 0x3333333333333333ull;
	x = (x | (x << 1)) & 0x5555555555555555ull;
	return x;
}

template <int NC, bool RID>
__global__ __launch_bounds__(JK_THREADS) void k_join_key_pack(const jk_args a)
{
	__shared__ uint32_t s_nulls;
	if (threadIdx.x == 0)
		s_nulls = 0;
	__syncthreads();
	const uint32_t lane = mdb_lane(), wave = threadIdx.x >> 6;
	uint32_t dropped = 0;	/* (the same in every lane of the wave) */
#pragma unroll
	for (uint32_t r = 0; r < JK_ROUNDS; r++) {
		const uint64_t wbase = (uint64_t)blockIdx.x * JK_ROWS_PER_WG + (uint64_t)r * JK_ROWS_PER_ROUND + (uint64_t)wave * 128u;
		if (wbase >= a.n)	/* (per wave; no barrier inside the loop) */
			continue;
		const uint64_t i0 = wbase + 2u * lane;
		const bool in0 = i0 < a.n, in1 = i0 + 1 < a.n;
		uint32_t rr0[NC], rr1[NC];
		if (RID) {
#pragma unroll
			for (int q = 0; q < NC; q++) {
				rr0[q] = rr1[q] = MDB_NO_ROW;
				if ((uint32_t)q < a.nrid) {
					if (in0)
						rr0[q] = a.rid[q][i0];
					if (in1)
						rr1[q] = a.rid[q][i0 + 1];
				}
			}
		}
		uint64_t key0 = 0, key1 = 0;
		bool bad0 = false, bad1 = false;
#pragma unroll
		for (int c = 0; c < NC; c++) {
			uint64_t v0 = 0, v1 = 0;
			if (!RID || a.slot[c] == JK_NO_SLOT) {
				const unsigned long long *src = reinterpret_cast<const unsigned long long *>(a.vals[c]);
				if (in1 && ((a.vec_in >> c) & 1u)) {
					const jk_ull2 v = __builtin_nontemporal_load(reinterpret_cast<const jk_ull2 *>(src + i0));
					v0 = v.x;
					v1 = v.y;
				} else {
					if (in0)
						v0 = __builtin_nontemporal_load(src + i0);
					if (in1)
						v1 = __builtin_nontemporal_load(src + i0 + 1);
				}
				if (a.nulls[c] && in0) {
					const uint64_t w = a.nulls[c][i0 >> 6];	/* (i0 is even: both rows' bits are in this word) */
					bad0 |= (w >> (i0 & 63u)) & 1ull;
					bad1 |= (w >> ((i0 & 63u) + 1u)) & 1ull;
				}
			} else {
				uint32_t row0 = MDB_NO_ROW, row1 = MDB_NO_ROW;
#pragma unroll
				for (int q = 0; q < NC; q++)
					if (a.slot[c] == q) {
						row0 = rr0[q];
						row1 = rr1[q];
					}
				if (row0 != MDB_NO_ROW) {
					v0 = (uint64_t)a.vals[c][row0];
					if (a.nulls[c])
						bad0 |= mdb_bit_is_set(a.nulls[c], row0);
				} else {
					bad0 = true;
				}
				if (row1 != MDB_NO_ROW) {
					v1 = (uint64_t)a.vals[c][row1];
					if (a.nulls[c])
						bad1 |= mdb_bit_is_set(a.nulls[c], row1);
				} else {
					bad1 = true;
				}
			}
			/* v - lo modulo 2^64 lies in [0, span] exactly when lo <= v <= lo + span: lo + span is an int64, so span <= INT64_MAX - lo,
			 * and a v below lo wraps to at least 2^64 - (lo - INT64_MIN) = 2^63 - lo, which is more */
			const uint64_t d0 = v0 - (uint64_t)a.lo[c], d1 = v1 - (uint64_t)a.lo[c];
			bad0 |= d0 > a.span[c];
			bad1 |= d1 > a.span[c];
			key0 |= d0 << a.shift[c];
			key1 |= d1 << a.shift[c];
		}
		bad0 &= in0;
		bad1 &= in1;
		key0 = bad0 ? 0ull : key0;
		key1 = bad1 ? 0ull : key1;
		unsigned long long *dst = reinterpret_cast<unsigned long long *>(a.out_key);
		if (in1 && a.vec_out) {
			jk_ull2 kv;
			kv.x = key0;
			kv.y = key1;
			*reinterpret_cast<jk_ull2 *>(dst + i0) = kv;
		} else {
			if (in0)
				dst[i0] = key0;
			if (in1)
				dst[i0 + 1] = key1;
		}
		const uint64_t b0 = __ballot(bad0), b1 = __ballot(bad1);	/* bit l: row wbase + 2 l (+ 1) */
		dropped += (uint32_t)__popcll(b0) + (uint32_t)__popcll(b1);
		if (lane == 0) {
			a.out_null[wbase >> 6] = jk_spread((uint32_t)b0) | (jk_spread((uint32_t)b1) << 1);
			if (wbase + 64u < a.n)
				a.out_null[(wbase >> 6) + 1] = jk_spread((uint32_t)(b0 >> 32)) | (jk_spread((uint32_t)(b1 >> 32)) << 1);
		}
	}
	if (lane == 0 && dropped)
		atomicAdd(&s_nulls, dropped);
	__syncthreads();
	if (threadIdx.x == 0 && s_nulls)
		atomicAdd(a.out_nulls, (unsigned long long)s_nulls);
}

template <int NC> static int jk_launch(mdb_dev_ctx *ctx, const jk_args &a, uint32_t grid)
{
	if (a.nrid)
		MDB_LAUNCH(ctx, "join_key_pack", (k_join_key_pack<NC, true>), grid, JK_THREADS, a);
	else
		MDB_LAUNCH(ctx, "join_key_pack", (k_join_key_pack<NC, false>), grid, JK_THREADS, a);
	return MIDORIDB_OK;
}

extern "C" int mdb_dev_join_key_pack(mdb_dev_ctx *ctx, const struct mdb_join_key_layout *lay, const struct mdb_join_key_col *cols, uint64_t n,
				     int64_t *out_key, uint64_t *out_nullbits, uint64_t *out_nulls)
{
	if (!ctx || !lay || !out_nulls)
		return -MIDORIDB_ERROR;
	*out_nulls = 0;
	if (lay->ntaken < 2 || lay->ntaken > MDB_JOIN_KEY_MAX_COLS || lay->empty)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_key_pack: the layout takes %u columns%s (2 ... %d pack)", lay->ntaken,
				   lay->empty ? " and is empty" : "", MDB_JOIN_KEY_MAX_COLS);
	uint32_t below = 0;
	for (int c = (int)lay->ntaken - 1; c >= 0; c--) {	/* fields that overlap or leave bit 63 would make keys that lie */
		if (lay->bits[c] != jk_bit_length(lay->span[c]) || lay->shift[c] != below || below + lay->bits[c] > 63)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_key_pack: field %d of the layout is not what mdb_dev_join_key_layout makes", c);
		below += lay->bits[c];
	}
	if (n == 0)
		return MIDORIDB_OK;
	if (!cols || !out_key || !out_nullbits)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_key_pack: columns, destination keys and NULL bits are all required");
	const uint64_t blocks = (n + JK_ROWS_PER_WG - 1) / JK_ROWS_PER_WG;
	if (blocks > 0x7FFFFFFFull)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_key_pack: %llu rows are more than one launch addresses", (unsigned long long)n);
	jk_args a;
	memset(&a, 0, sizeof(a));
	for (uint32_t c = 0; c < lay->ntaken; c++) {
		if (!cols[c].values)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_key_pack: column %u has no values", c);
		a.vals[c] = cols[c].values;
		a.nulls[c] = cols[c].nullbits;
		a.lo[c] = lay->lo[c];
		a.span[c] = lay->span[c];
		a.shift[c] = lay->shift[c];
		a.slot[c] = JK_NO_SLOT;
		if (cols[c].rid) {
			uint32_t q = 0;
			while (q < a.nrid && a.rid[q] != cols[c].rid)
				q++;
			if (q == a.nrid)
				a.rid[a.nrid++] = cols[c].rid;
			a.slot[c] = (uint8_t)q;
		} else if (((uintptr_t)cols[c].values & 15u) == 0) {
			a.vec_in |= 1u << c;
		}
	}
	a.vec_out = ((uintptr_t)out_key & 15u) == 0;
	a.n = n;
	a.out_key = out_key;
	a.out_null = out_nullbits;
	a.out_nulls = (unsigned long long *)(ctx->d_status + MDB_STW_UTIL);
	MDB_HIP(ctx, hipMemsetAsync(a.out_nulls, 0, 8, ctx->stream));
	int rc;
	if (lay->ntaken == 2)
		rc = jk_launch<2>(ctx, a, (uint32_t)blocks);
	else if (lay->ntaken == 3)
		rc = jk_launch<3>(ctx, a, (uint32_t)blocks);
	else
		rc = jk_launch<4>(ctx, a, (uint32_t)blocks);
	if (rc)
		return rc;
	uint64_t *h = ctx->h_pinned;
	MDB_HIP(ctx, hipMemcpyAsync(h + MDB_HP_COUNT, a.out_nulls, 8, hipMemcpyDeviceToHost, ctx->stream));
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	*out_nulls = h[MDB_HP_COUNT];
	return MIDORIDB_OK;
}

/* ------------------------------------------------------------------ the unpack kernel
 *
 * The way back for GROUP keys (the fused join + GROUP BY operator on a packed key returns packed group keys): out_c[i] = lo_c +
 * ((key_i >> shift_c) & (2^bits_c - 1)) in unsigned 64-bit arithmetic.  The same shape as the pack - 256 threads over 2048 consecutive
 * keys, two consecutive keys per lane and round, one 16-byte non-temporal load of the keys (read once), one 16-byte store per output
 * column, the 8-byte forms for a buffer that is not 16-byte aligned - without its LDS word, atomics and bitmap: a group key is never
 * NULL.  A lane whose keys lie behind n loads and stores nothing. */
struct jku_args {
	const int64_t *keys;
	int64_t *out[MDB_JOIN_KEY_MAX_COLS];
	int64_t lo[MDB_JOIN_KEY_MAX_COLS];
	uint64_t mask[MDB_JOIN_KEY_MAX_COLS];		/* 2^bits - 1; a field of 0 bits: 0 */
	uint32_t shift[MDB_JOIN_KEY_MAX_COLS];
	uint32_t vec_in;				/* keys is 16-byte aligned */
	uint32_t vec_out;				/* bit c: out[c] is 16-byte aligned */
	uint64_t n;
};

template <int NC>
__global__ __launch_bounds__(JK_THREADS) void k_join_key_unpack(const jku_args a)
{
	const unsigned long long *src = reinterpret_cast<const unsigned long long *>(a.keys);
#pragma unroll
	for (uint32_t r = 0; r < JK_ROUNDS; r++) {
		const uint64_t i0 = (uint64_t)blockIdx.x * JK_ROWS_PER_WG + (uint64_t)r * JK_ROWS_PER_ROUND + 2u * threadIdx.x;
		if (i0 >= a.n)
			continue;
		const bool in1 = i0 + 1 < a.n;
		uint64_t k0, k1 = 0;
		if (in1 && a.vec_in) {
			const jk_ull2 k = __builtin_nontemporal_load(reinterpret_cast<const jk_ull2 *>(src + i0));
			k0 = k.x;
			k1 = k.y;
		} else {
			k0 = __builtin_nontemporal_load(src + i0);
			if (in1)
				k1 = __builtin_nontemporal_load(src + i0 + 1);
		}
#pragma unroll
		for (int c = 0; c < NC; c++) {
			const uint64_t v0 = (uint64_t)a.lo[c] + ((k0 >> a.shift[c]) & a.mask[c]);
			const uint64_t v1 = (uint64_t)a.lo[c] + ((k1 >> a.shift[c]) & a.mask[c]);
			unsigned long long *dst = reinterpret_cast<unsigned long long *>(a.out[c]);
			if (in1 && ((a.vec_out >> c) & 1u)) {
				jk_ull2 v;
				v.x = v0;
				v.y = v1;
				*reinterpret_cast<jk_ull2 *>(dst + i0) = v;
			} else {
				dst[i0] = v0;
				if (in1)
					dst[i0 + 1] = v1;
			}
		}
	}
}

extern "C" int mdb_dev_join_key_unpack(mdb_dev_ctx *ctx, const struct mdb_join_key_layout *lay, const int64_t *keys, uint64_t n,
				       int64_t *const *out_cols)
{
	if (!ctx || !lay)
		return -MIDORIDB_ERROR;
	if (lay->ntaken < 2 || lay->ntaken > MDB_JOIN_KEY_MAX_COLS || lay->empty)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_key_unpack: the layout takes %u columns%s (2 ... %d unpack)", lay->ntaken,
				   lay->empty ? " and is empty" : "", MDB_JOIN_KEY_MAX_COLS);
	uint32_t below = 0;
	for (int c = (int)lay->ntaken - 1; c >= 0; c--) {
		if (lay->bits[c] != jk_bit_length(lay->span[c]) || lay->shift[c] != below || below + lay->bits[c] > 63)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_key_unpack: field %d of the layout is not what mdb_dev_join_key_layout makes", c);
		below += lay->bits[c];
	}
	if (n == 0)
		return MIDORIDB_OK;
	if (!keys || !out_cols)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_key_unpack: keys and destination columns are required");
	const uint64_t blocks = (n + JK_ROWS_PER_WG - 1) / JK_ROWS_PER_WG;
	if (blocks > 0x7FFFFFFFull)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_key_unpack: %llu keys are more than one launch addresses", (unsigned long long)n);
	jku_args a;
	memset(&a, 0, sizeof(a));
	for (uint32_t c = 0; c < lay->ntaken; c++) {
		if (!out_cols[c])
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "join_key_unpack: column %u has no destination", c);
		a.out[c] = out_cols[c];
		a.lo[c] = lay->lo[c];
		a.mask[c] = lay->bits[c] ? (1ull << lay->bits[c]) - 1ull : 0ull;	/* (bits <= 63) */
		a.shift[c] = lay->shift[c];
		if (((uintptr_t)out_cols[c] & 15u) == 0)
			a.vec_out |= 1u << c;
	}
	a.keys = keys;
	a.vec_in = ((uintptr_t)keys & 15u) == 0;
	a.n = n;
	if (lay->ntaken == 2)
		MDB_LAUNCH(ctx, "join_key_unpack", (k_join_key_unpack<2>), (uint32_t)blocks, JK_THREADS, a);
	else if (lay->ntaken == 3)
		MDB_LAUNCH(ctx, "join_key_unpack", (k_join_key_unpack<3>), (uint32_t)blocks, JK_THREADS, a);
	else
		MDB_LAUNCH(ctx, "join_key_unpack", (k_join_key_unpack<4>), (uint32_t)blocks, JK_THREADS, a);
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return MIDORIDB_OK;
}
