/*
 * mdb_dev_countdistinct.hip - COUNT(DISTINCT col) per group (mdb_dev_group_count_distinct): an extension, as SUM / MIN / MAX / AVG are
 * (mdb_dev_aggregate.hip) - the reference counts rows and nothing else.
 *
 * The GROUP BY operators have delivered first[G] before this operator runs.  Step A finds the group of every row once per call
 * (gid[n], shared by all columns; nothing for one group):
 *   A1  one 8-byte key and G <= mdb_dev_group_count_distinct_lds_groups(): every workgroup builds the key -> group table in LDS from the
 *       keys at first[g] (mdb_group_lds_build, mdb_dev_stream.h) and streams its rows through it.
 *   A2  otherwise: mdb_runs_find (mdb_dev_runs.hip) sorts the stream by the keys and delivers the runs' heads and their groups; one pass
 *       writes every sorted position's group to its stream position.
 * Step B answers every column by one of three forms:
 *   1  bitmap (integer cells inside a promised range): every group owns whole 64-bit words, a cell marks its bit - the word is read first
 *      and the atomic issued only while the bit is clear, so a hot value costs a cached load -, a popcount per group.  A cell outside the
 *      promised range raises CD_ST_OUT_OF_RANGE and the column is redone by form 2.
 *   2  sorted: a stable sort by (group, value); a position counts when its cell is valid and the one before belongs to another group, is
 *      NULL or holds another canonical value (NULLs sort first, -0.0 lies next to +0.0).  Counted with wave ballots, one 64-bit integer
 *      atomicAdd per wave and group.
 *   3  identity: group i is row i.
 * No floating-point atomic and no order-dependent arithmetic anywhere: the same input gives the same bytes.
 */
#include "mdb_dev_internal.h"
#include "mdb_dev_stream.h"

#define CD_LDS_THREADS 1024
#define CD_THREADS 256
#define CD_WAVE_WORDS 1024u			/* a group of up to this many bitmap words is counted by a wave, a longer one by a workgroup */
/* the operator's own flag in the groups' status word (mdb_dev_stream.h) */
#define CD_ST_OUT_OF_RANGE 4u	/* form 1: a cell outside the promised [min, max] */
static_assert(mdb_flags_distinct({ MDB_GROUPS_ST_KEY_MISSING, MDB_GROUPS_ST_RUNS_DIFFER, MDB_GROUPS_ST_PERM_RANGE, CD_ST_OUT_OF_RANGE }),
	      "count distinct: two status flags share a bit");

/* ------------------------------------------------------------------ step A1: the key -> group table in LDS */
struct cd_lds_args {
	mdb_stream_col key;
	uint64_t n;
	const uint32_t *first;
	uint32_t G, log2_slots;
	uint32_t *gid;		/* n group numbers (8-byte aligned) */
	uint32_t *status;
};

/* dynamic LDS: slots keys, then slots group numbers */
__global__ __launch_bounds__(CD_LDS_THREADS) void k_cd_gid_lds(cd_lds_args A)
{
	extern __shared__ unsigned long long s_mem[];
	const mdb_group_lds T = mdb_group_lds_build(s_mem, 1u << A.log2_slots, A.log2_slots, A.key, A.first, A.G, CD_LDS_THREADS);

	bool missing = false;
	for (uint64_t i = ((uint64_t)blockIdx.x * CD_LDS_THREADS + threadIdx.x) * 2u; i < A.n; i += (uint64_t)gridDim.x * CD_LDS_THREADS * 2u) {
		const bool two = i + 1u < A.n;
		uint64_t kb[2] = { 0, 0 };
		bool kv[2] = { true, two };
		uint32_t grp[2] = { MDB_GROUP_NONE, MDB_GROUP_NONE };
		mdb_stream_cell2(A.key, i, two, kb, kv);
#pragma unroll
		for (int r = 0; r < 2; r++) {
			if (r && !two)
				continue;
			grp[r] = mdb_group_lds_find(T, kb[r], kv[r]);
			missing = missing || grp[r] == MDB_GROUP_NONE;
		}
		if (two)
			*reinterpret_cast<uint2 *>(A.gid + i) = make_uint2(grp[0], grp[1]);	/* (i is even, gid is 8-byte aligned) */
		else
			A.gid[i] = grp[0];
	}
	if (missing)
		mdb_raise(A.status, MDB_GROUPS_ST_KEY_MISSING);
}

extern "C" uint64_t mdb_dev_group_count_distinct_lds_groups(void)
{
	uint32_t lg = MDB_SET_MIN_LOG2;
	while (mdb_group_lds_bytes(2ull << lg) <= MDB_GROUP_LDS_BUDGET)
		lg++;
	return (1ull << lg) / 2u;	/* (load <= 1/2) */
}

extern "C" uint64_t mdb_dev_count_distinct_bitmap_bits(void)
{
	return MDB_COUNT_DISTINCT_BITMAP_BITS;
}

/* ------------------------------------------------------------------ step A2: the runs of the sorted stream (mdb_runs_find) */

/* gid[stream position] = the group of the run that sorted position p lies in (the host has seen as many runs as groups and no flag: every
 * run has its group, and perm names positions below n) */
__global__ __launch_bounds__(CD_THREADS) void k_cd_run_scatter(const unsigned long long *__restrict__ hb, const uint32_t *__restrict__ base,
								const uint32_t *__restrict__ perm, uint64_t n, const uint32_t *__restrict__ rungroup,
								uint32_t *__restrict__ gid)
{
	const uint64_t p = (uint64_t)blockIdx.x * CD_THREADS + threadIdx.x;
	const uint32_t upto = mdb_runs_heads_before_wave(hb, base, p) + (uint32_t)((hb[p >> 6] >> (p & 63)) & 1ull);	/* (position 0 is a head: >= 1) */
	if (p < n)
		gid[perm[p]] = rungroup[upto - 1u];
}

/* ------------------------------------------------------------------ form 1: a bitmap per group */

/* every valid cell marks bit (value - min) of its group's words; gid == NULL: one group */
__global__ __launch_bounds__(CD_THREADS) void k_cd_mark(mdb_stream_col c, const uint32_t *__restrict__ gid, uint64_t n, uint64_t G, int64_t min, uint64_t span,
							 uint64_t wpg, unsigned long long *__restrict__ bitmap, uint32_t *status)
{
	bool outside = false;
	for (uint64_t i = ((uint64_t)blockIdx.x * CD_THREADS + threadIdx.x) * 2u; i < n; i += (uint64_t)gridDim.x * CD_THREADS * 2u) {
		const bool two = i + 1u < n;
		uint64_t vb[2] = { 0, 0 };
		bool vv[2] = { false, false };
		uint32_t g[2] = { 0u, 0u };
		mdb_stream_cell2(c, i, two, vb, vv);
		if (gid) {
			if (two) {
				const uint2 w = *reinterpret_cast<const uint2 *>(gid + i);	/* (i is even, gid is 8-byte aligned) */
				g[0] = w.x;
				g[1] = w.y;
			} else {
				g[0] = gid[i];
			}
		}
#pragma unroll
		for (int r = 0; r < 2; r++) {
			if (!vv[r] || g[r] >= G)
				continue;
			const uint64_t off = vb[r] - (uint64_t)min;	/* (a value below min wraps to a huge offset) */
			if (off >= span) {
				outside = true;
				continue;
			}
			unsigned long long *w = bitmap + (uint64_t)g[r] * wpg + (off >> 6);
			const unsigned long long bit = 1ull << (off & 63u);
			if (!(*w & bit))
				atomicOr(w, bit);
		}
	}
	if (outside)
		mdb_raise(status, CD_ST_OUT_OF_RANGE);
}

/* a wave per group: short spans */
__global__ __launch_bounds__(CD_THREADS) void k_cd_popcount_wave(const unsigned long long *__restrict__ bitmap, uint64_t G, uint64_t wpg, int64_t *__restrict__ out)
{
	const uint64_t g = (uint64_t)blockIdx.x * (CD_THREADS / MDB_WAVE) + (threadIdx.x >> 6);
	if (g >= G)
		return;
	const uint32_t lane = mdb_lane();
	uint32_t cnt = 0;
	for (uint64_t w = lane; w < wpg; w += MDB_WAVE)
		cnt += (uint32_t)__popcll(bitmap[g * wpg + w]);
	for (uint32_t d = MDB_WAVE / 2; d; d >>= 1)
		cnt += (uint32_t)__shfl_down((int)cnt, d, MDB_WAVE);
	if (lane == 0)
		out[g] = (int64_t)cnt;
}

/* a workgroup per group: long spans (at most MDB_COUNT_DISTINCT_BITMAP_BITS bits: the count fits 32 bits) */
__global__ __launch_bounds__(CD_THREADS) void k_cd_popcount_wg(const unsigned long long *__restrict__ bitmap, uint64_t wpg, int64_t *__restrict__ out)
{
	__shared__ uint32_t s_cnt[CD_THREADS / MDB_WAVE];
	const uint64_t g = blockIdx.x;
	const uint32_t lane = mdb_lane();
	uint32_t cnt = 0;
	for (uint64_t w = threadIdx.x; w < wpg; w += CD_THREADS)
		cnt += (uint32_t)__popcll(bitmap[g * wpg + w]);
	for (uint32_t d = MDB_WAVE / 2; d; d >>= 1)
		cnt += (uint32_t)__shfl_down((int)cnt, d, MDB_WAVE);
	if (lane == 0)
		s_cnt[threadIdx.x >> 6] = cnt;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t t = 0;
		for (uint32_t k = 0; k < CD_THREADS / MDB_WAVE; k++)
			t += s_cnt[k];
		out[g] = (int64_t)t;
	}
}

/* ------------------------------------------------------------------ form 2: sorted by (group, value) */

__global__ __launch_bounds__(CD_THREADS) void k_cd_widen(const uint32_t *__restrict__ gid, uint64_t n, unsigned long long *__restrict__ gid64)
{
	const uint64_t i = (uint64_t)blockIdx.x * CD_THREADS + threadIdx.x;
	if (i < n)
		gid64[i] = gid[i];
}

/* Sorted position i is a head when its cell is valid and i is the first position, or position i - 1 belongs to another group, is NULL or
 * holds another canonical value.  The position before is the lane before (a shuffle); a wave's first lane reads it from global memory.  The
 * lanes of one group are neighbours: the first lane of every group segment adds the segment's heads to out[group] (zeroed by the host). */
__global__ __launch_bounds__(CD_THREADS) void k_cd_sorted_heads(mdb_stream_col c, const uint32_t *__restrict__ gid, const uint32_t *__restrict__ perm, uint64_t n,
								 uint64_t G, unsigned long long *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * CD_THREADS + threadIdx.x;
	const bool in = i < n;
	const uint32_t lane = mdb_lane();
	uint64_t b1 = 0;
	uint32_t g1 = MDB_GROUP_NONE;
	bool v1 = false;
	if (in) {
		const uint32_t sp = perm[i];
		g1 = gid ? gid[sp] : 0u;
		v1 = mdb_stream_cell(c, sp, &b1);
		if (v1)
			(void)mdb_set_canonical(c.type, &b1);
	}
	uint64_t b0 = (uint64_t)__shfl_up((unsigned long long)b1, 1u, MDB_WAVE);
	uint32_t g0 = (uint32_t)__shfl_up((int)g1, 1u, MDB_WAVE);
	bool v0 = __shfl_up((int)v1, 1u, MDB_WAVE) != 0;
	if (lane == 0) {
		g0 = MDB_GROUP_NONE;
		v0 = false;
		if (in && i) {
			const uint32_t sp = perm[i - 1];
			g0 = gid ? gid[sp] : 0u;
			b0 = 0;
			v0 = mdb_stream_cell(c, sp, &b0);
			if (v0)
				(void)mdb_set_canonical(c.type, &b0);
		}
	}
	const bool head = in && v1 && g1 < G && (i == 0 || g0 != g1 || !v0 || b0 != b1);
	const unsigned long long heads = __ballot(head);
	const bool seg_start = lane == 0 || g1 != (uint32_t)__shfl_up((int)g1, 1u, MDB_WAVE);
	const unsigned long long starts = __ballot(seg_start);
	if (seg_start && in && g1 < G) {
		const unsigned long long above = lane == MDB_WAVE - 1u ? 0ull : starts & (~0ull << (lane + 1u));
		const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 1u : MDB_WAVE;	/* the segment is lanes [lane, end) */
		const unsigned long long upto = end == MDB_WAVE ? ~0ull : (1ull << end) - 1ull;
		const uint32_t cnt = (uint32_t)__popcll(heads & upto & (~0ull << lane));
		if (cnt)
			atomicAdd(out + g1, (unsigned long long)cnt);
	}
}

/* ------------------------------------------------------------------ form 3: group i = row i */
__global__ __launch_bounds__(CD_THREADS) void k_cd_identity(mdb_stream_col c, uint64_t n, int64_t *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * CD_THREADS + threadIdx.x;
	if (i >= n)
		return;
	uint64_t bits = 0;
	out[i] = mdb_stream_cell(c, i, &bits) ? 1 : 0;
}

/* ------------------------------------------------------------------ host side */

static mdb_stream_col cd_col_of(const struct mdb_count_distinct *a) { return mdb_stream_col_of(a->values, a->nullbits, a->rid, 0, a->type); }

static uint32_t cd_grid(uint64_t items)
{
	return (uint32_t)((items + CD_THREADS - 1u) / CD_THREADS);
}

/* step A1 */
static int cd_gid_lds(mdb_dev_ctx *ctx, const struct mdb_sort_key *key, uint64_t n, const uint32_t *first, uint64_t G, uint32_t *gid, uint32_t *status)
{
	cd_lds_args A;
	memset(&A, 0, sizeof(A));
	A.key = mdb_stream_col_of_key(key);
	A.n = n;
	A.first = first;
	A.G = (uint32_t)G;
	A.log2_slots = mdb_group_lds_log2(G);
	A.gid = gid;
	A.status = status;
	const size_t lds = mdb_group_lds_bytes(1ull << A.log2_slots);
	if (lds > MDB_GROUP_LDS_BUDGET)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "group_count_distinct: %llu groups do not fit the LDS table", (unsigned long long)G);
	MDB_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cd_gid_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	MDB_LAUNCH_LDS(ctx, "cd_gid_lds", k_cd_gid_lds, mdb_group_lds_grid(ctx, lds, n), CD_LDS_THREADS, lds, A);
	return mdb_groups_status(ctx, status, "group_count_distinct", "groups in LDS");
}

/* step A2 */
static int cd_gid_sorted(mdb_dev_ctx *ctx, const struct mdb_sort_key *keys, int nkeys, uint64_t n, const uint32_t *first, uint64_t G, uint32_t *gid)
{
	mdb_dev_tmp tmp(ctx);
	mdb_runs R;
	const int rc = mdb_runs_find(ctx, keys, nkeys, n, first, G, "group_count_distinct", "sorted runs", tmp, &R);
	if (rc)
		return rc;
	MDB_LAUNCH(ctx, "cd_run_scatter", k_cd_run_scatter, cd_grid(n), CD_THREADS, R.hb, R.base, R.perm, n, R.rungroup, gid);
	return MIDORIDB_OK;
}

/* whether form 1 takes the column, and its geometry: span values from min, wpg words per group */
static bool cd_bitmap_applies(const struct mdb_count_distinct *c, uint64_t G, uint64_t *span, uint64_t *wpg)
{
	if (c->type != MDB_T_INT64 || !c->has_range || c->max < c->min)
		return false;
	const uint64_t s = (uint64_t)c->max - (uint64_t)c->min + 1u;
	if (!s)	/* (max - min + 1 = 2^64) */
		return false;
	const uint64_t w = (s - 1u) / 64u + 1u;
	if (w > MDB_COUNT_DISTINCT_BITMAP_BITS / 64u || G > MDB_COUNT_DISTINCT_BITMAP_BITS / 64u / w)
		return false;
	*span = s;
	*wpg = w;
	return true;
}

/* form 1; *redo = a cell lay outside the promised range: nothing was written */
static int cd_form_bitmap(mdb_dev_ctx *ctx, const struct mdb_count_distinct *c, const uint32_t *gid, uint64_t n, uint64_t G, uint64_t span, uint64_t wpg,
			  uint32_t *status, bool *redo)
{
	mdb_dev_tmp tmp(ctx);
	int rc;
	unsigned long long *bitmap = (unsigned long long *)tmp.take(G * wpg * 8u);
	if (!bitmap)
		return mdb_set_err(ctx, -MIDORIDB_NOMEM, "group_count_distinct: no device memory for a bitmap of %llu words", (unsigned long long)(G * wpg));
	MDB_HIP(ctx, hipMemsetAsync(bitmap, 0, G * wpg * 8u, ctx->stream));
	MDB_HIP(ctx, hipMemsetAsync(status, 0, 4, ctx->stream));
	uint64_t grid = (n + CD_THREADS * 8u - 1u) / (CD_THREADS * 8u);	/* eight rows per thread, at most eight workgroups per CU */
	grid = grid < (uint64_t)ctx->num_cus * 8u ? grid : (uint64_t)ctx->num_cus * 8u;
	MDB_LAUNCH(ctx, "cd_mark", k_cd_mark, (uint32_t)(grid ? grid : 1u), CD_THREADS, cd_col_of(c), gid, n, G, c->min, span, wpg, bitmap, status);
	uint32_t flags = 0;
	if ((rc = mdb_groups_status(ctx, status, "group_count_distinct", "bitmap", &flags)))
		return rc;
	*redo = (flags & CD_ST_OUT_OF_RANGE) != 0;
	if (*redo)
		return MIDORIDB_OK;
	if (wpg <= CD_WAVE_WORDS)
		MDB_LAUNCH(ctx, "cd_popcount_wave", k_cd_popcount_wave, (uint32_t)((G + 3u) / 4u), CD_THREADS, (const unsigned long long *)bitmap, G, wpg, c->out);
	else
		MDB_LAUNCH(ctx, "cd_popcount_wg", k_cd_popcount_wg, (uint32_t)G, CD_THREADS, (const unsigned long long *)bitmap, wpg, c->out);
	return MIDORIDB_OK;
}

/* form 2; gid64 (NULL without keys) = the group numbers as an 8-byte column */
static int cd_form_sorted(mdb_dev_ctx *ctx, const struct mdb_count_distinct *c, const uint32_t *gid, const unsigned long long *gid64, uint64_t n,
			  uint64_t G)
{
	mdb_dev_tmp tmp(ctx);
	struct mdb_sort_key sk[2];
	int nk = 0, rc;
	uint32_t *perm = (uint32_t *)tmp.take(n * 4u + 16u);
	if (!perm)
		return mdb_set_err(ctx, -MIDORIDB_NOMEM, "group_count_distinct: no device memory for the permutation");
	memset(sk, 0, sizeof(sk));
	if (gid64) {
		sk[nk].values = gid64;
		sk[nk].type = MDB_T_INT64;
		nk++;
	}
	sk[nk].values = c->values;
	sk[nk].nullbits = c->nullbits;
	sk[nk].rid = c->rid;
	sk[nk].type = c->type;
	nk++;
	if ((rc = mdb_dev_sort_perm(ctx, sk, nk, n, perm)))
		return rc;
	MDB_HIP(ctx, hipMemsetAsync(c->out, 0, G * 8u, ctx->stream));
	MDB_LAUNCH(ctx, "cd_sorted_heads", k_cd_sorted_heads, cd_grid(n), CD_THREADS, cd_col_of(c), gid, (const uint32_t *)perm, n, G,
		   (unsigned long long *)c->out);
	return MIDORIDB_OK;
}

extern "C" int mdb_dev_group_count_distinct(mdb_dev_ctx *ctx, const struct mdb_sort_key *keys, int nkeys, uint64_t n, const uint32_t *first, uint64_t G,
					    const struct mdb_count_distinct *cols, int ncols, uint32_t *out_forms)
{
	if (!ctx)
		return -MIDORIDB_ERROR;
	for (int c = 0; out_forms && c < ncols && c < MDB_AGG_MAX_AGGS; c++)
		out_forms[c] = 0;
	if (!cols || ncols < 1 || ncols > MDB_AGG_MAX_AGGS)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct: 1 ... %d columns per call", MDB_AGG_MAX_AGGS);
	if (nkeys != MDB_AGG_IDENTITY && (nkeys < 0 || nkeys > MDB_SORT_MAX_KEYS || (nkeys && !keys)))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct: 0 ... %d group key columns", MDB_SORT_MAX_KEYS);
	if (n >= MDB_NO_ROW || G > n + (n ? 0u : 1u))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct: %llu groups over %llu rows", (unsigned long long)G, (unsigned long long)n);
	for (int c = 0; c < ncols; c++) {
		if (cols[c].type != MDB_T_INT64 && cols[c].type != MDB_T_DOUBLE)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct: column %d: unknown cell type %d", c, cols[c].type);
		if (!cols[c].out || (n && !cols[c].values))
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct: column %d: no cells or no place for the result", c);
	}
	if (nkeys == 0 && G != (n ? 1u : G))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct: without group keys the stream is one group");
	if (nkeys == MDB_AGG_IDENTITY && G != n)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct: the identity form takes as many groups as rows");
	if (nkeys > 0 && G && !first)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct: no first rows");
	if (!G)
		return MIDORIDB_OK;
	if (!n) {	/* (one group over no row: 0) */
		for (int c = 0; c < ncols; c++)
			MDB_HIP(ctx, hipMemsetAsync(cols[c].out, 0, G * 8u, ctx->stream));
		MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		return MIDORIDB_OK;
	}
	if (nkeys == MDB_AGG_IDENTITY) {
		for (int c = 0; c < ncols; c++) {
			MDB_LAUNCH(ctx, "cd_identity", k_cd_identity, cd_grid(n), CD_THREADS, cd_col_of(&cols[c]), n, cols[c].out);
			if (out_forms)
				out_forms[c] = 3;
		}
		MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		return MIDORIDB_OK;
	}

	mdb_dev_tmp tmp(ctx);
	int rc;
	uint32_t *status = (uint32_t *)tmp.take(256);
	uint32_t *gid = nkeys ? (uint32_t *)tmp.take(n * 4u + 16u) : NULL;
	unsigned long long *gid64 = NULL;
	if (!status || (nkeys && !gid))
		return mdb_set_err(ctx, -MIDORIDB_NOMEM, "group_count_distinct: no device memory for the groups of %llu rows", (unsigned long long)n);
	MDB_HIP(ctx, hipMemsetAsync(status, 0, 4, ctx->stream));
	if (nkeys == 1 && G <= mdb_dev_group_count_distinct_lds_groups())
		rc = cd_gid_lds(ctx, &keys[0], n, first, G, gid, status);
	else if (nkeys)
		rc = cd_gid_sorted(ctx, keys, nkeys, n, first, G, gid);
	else
		rc = MIDORIDB_OK;
	if (rc)
		return rc;

	const bool bitmap_on = !mdb_knob_off("MDB_COUNT_DISTINCT_BITMAP");
	for (int c = 0; c < ncols; c++) {
		uint64_t span = 0, wpg = 0;
		bool redo = false;
		uint32_t form = 2;
		if (bitmap_on && cd_bitmap_applies(&cols[c], G, &span, &wpg)) {
			if ((rc = cd_form_bitmap(ctx, &cols[c], gid, n, G, span, wpg, status, &redo)))
				return rc;
			form = redo ? 2 : 1;
		}
		if (form == 2) {
			if (gid && !gid64) {
				gid64 = (unsigned long long *)tmp.take(n * 8u);
				if (!gid64)
					return mdb_set_err(ctx, -MIDORIDB_NOMEM, "group_count_distinct: no device memory for the groups of %llu rows", (unsigned long long)n);
				MDB_LAUNCH(ctx, "cd_widen", k_cd_widen, cd_grid(n), CD_THREADS, (const uint32_t *)gid, n, gid64);
			}
			if ((rc = cd_form_sorted(ctx, &cols[c], gid, gid64, n, G)))
				return rc;
		}
		if (out_forms)
			out_forms[c] = form;
	}
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return MIDORIDB_OK;
}
