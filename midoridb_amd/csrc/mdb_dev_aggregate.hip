/*
 * mdb_dev_aggregate.hip - SUM / MIN / MAX / AVG per group (mdb_dev_group_aggregate): an extension - the reference's lexer knows COUNT( only
 * (src/parser/midorisql.l:139-142) and its executor counts rows and nothing else (inc_count_cols, src/engine/executor_select.c:1465-1524).
 *
 * The GROUP BY operators have delivered first[G] (the stream position of every group's first row, ascending) before this operator runs; it
 * folds the cells of every aggregate's column into the group of their row.  A cell that is NULL - its NULL bit, or a row id of MDB_NO_ROW -
 * is skipped; a group without a non-NULL cell is NULL.  Results are bit-exact and the same from call to call: there is no floating-point
 * atomic anywhere, and every floating-point sum is folded in an order that depends on n, the sort permutation and the launch geometry alone.
 *
 * An accumulator is a pair (acc, cnt) of 64-bit words: cnt = non-NULL cells folded, acc = their sum (integers: two's complement, wrapping;
 * DOUBLE: the bits of the sum) or the smallest / largest order-preserving image (mdb_order_image).  Cells, images, the LDS table and the
 * status flags are mdb_dev_stream.h's.
 *
 *   form 1  groups in LDS.  Every aggregate is order-free (integer cells, or MIN / MAX over DOUBLE), at most one 8-byte group key per row
 *           and G <= mdb_dev_group_aggregate_lds_groups(naggs): every workgroup builds the key -> group table from the keys at first[g]
 *           (mdb_group_lds_build), streams its share of the rows and
 *           updates accumulators in LDS with 64-bit integer atomics - as many copies of the accumulators as fit (at most AGG_MAX_COPIES),
 *           indexed by thread, so that a handful of groups does not send every lane to one address.  The workgroups' slabs are folded by
 *           k_agg_fold_slabs, a wave per accumulator.  MDB_AGG_LDS=0 turns the form off.
 *   form 2  sorted segments.  mdb_runs_find (mdb_dev_runs.hip) sorts the stream by the group keys and delivers the runs' heads and their
 *           groups.  Chunks of AGG_CHUNK sorted positions, one wave
 *           each, a strip of AGG_STRIP positions per lane: a lane folds its strip in order, the wave joins the strips with a segmented
 *           scan (shuffles), runs that begin and end inside a chunk are final there; a run that crosses a chunk boundary is finished by
 *           k_agg_seg_fin from the chunks' (part before the first head, part after the last head) records, in chunk order.
 *   form 3  the identity (nkeys == MDB_AGG_IDENTITY): group i is row i.
 */
#include "mdb_dev_internal.h"
#include "mdb_dev_stream.h"

#define AGG_LDS_THREADS 1024
#define AGG_MAX_COPIES 16u
#define AGG_CHUNK MDB_RUNS_CHUNK		/* sorted positions per wave of form 2 */
#define AGG_STRIP (AGG_CHUNK / MDB_WAVE)	/* ... per lane: 16, a quarter of a word of head bits */
#define AGG_SEG_THREADS 256
static_assert(AGG_STRIP == 16u, "a lane's strip is 16 head bits");

__host__ __device__ static inline bool agg_is_minmax(int op) { return op == MDB_AGG_MIN || op == MDB_AGG_MAX; }

/* value -> what is folded */
__device__ static inline uint64_t agg_to_acc(int op, int type, uint64_t bits) { return agg_is_minmax(op) ? mdb_order_image(bits, type) : bits; }

/* (a, na) then (b, nb): b is folded INTO a, in that order.  An empty side changes nothing (a group's first cell is taken as it is: the sum
 * of {-0.0} is -0.0) */
__device__ static inline void agg_fold(int op, int type, uint64_t &a, uint64_t &na, uint64_t b, uint64_t nb)
{
	if (!nb)
		return;
	if (!na) {
		a = b;
		na = nb;
		return;
	}
	if (op == MDB_AGG_MIN)
		a = b < a ? b : a;
	else if (op == MDB_AGG_MAX)
		a = b > a ? b : a;
	else if (type == MDB_T_DOUBLE)
		a = (uint64_t)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
	else
		a += b;
	na += nb;
}

/* ------------------------------------------------------------------ the result cells: every form ends here
 * rec[(s * per + g) * 2 + {0, 1}] = (acc, cnt) of group g in slab s (form 1: one slab per workgroup, folded in workgroup order; forms 2 and
 * 3: one).  One thread per group, a wave per word of NULL bits: every word of out_nullbits is written whole. */
__global__ __launch_bounds__(256) void k_agg_finish(const unsigned long long *__restrict__ rec, uint32_t nslab, uint64_t per, uint64_t G, int op, int type,
						     uint64_t *__restrict__ out, unsigned long long *__restrict__ out_nullbits)
{
	const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	uint64_t acc = 0, cnt = 0;
	if (g < G)
		for (uint32_t s = 0; s < nslab; s++) {
			const unsigned long long *r = rec + ((uint64_t)s * per + g) * 2u;
			agg_fold(op, type, acc, cnt, r[0], r[1]);
		}
	uint64_t res = 0;
	if (cnt) {
		if (agg_is_minmax(op))
			res = mdb_order_unimage(acc, type);
		else if (op == MDB_AGG_SUM)
			res = acc;
		else if (type == MDB_T_DOUBLE)
			res = (uint64_t)__double_as_longlong(__longlong_as_double((long long)acc) / (double)cnt);
		else
			res = (uint64_t)__double_as_longlong((double)(long long)acc / (double)cnt);
	}
	if (g < G)
		out[g] = res;
	const unsigned long long nb = __ballot(g < G && !cnt);
	if (mdb_lane() == 0 && (g & ~63ull) < G)
		out_nullbits[g >> 6] = nb;
}

/* form 1: the workgroups' slabs folded into one, a wave per (aggregate, group) - lane l takes slabs l, l + 64 ... in that order, the lanes are
 * folded pairwise in a fixed tree (integer sums and order images: the result does not depend on the order anyway) */
struct agg_ops {
	int32_t op[MDB_AGG_MAX_AGGS], type[MDB_AGG_MAX_AGGS];
};

__global__ __launch_bounds__(256) void k_agg_fold_slabs(const unsigned long long *__restrict__ slab, uint32_t nslab, uint64_t per, uint64_t G, agg_ops O,
							 unsigned long long *__restrict__ rec)
{
	const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
	if (i >= per)
		return;
	const int op = O.op[i / G], type = O.type[i / G];
	const uint32_t lane = mdb_lane();
	uint64_t acc = 0, cnt = 0;
	for (uint32_t s = lane; s < nslab; s += MDB_WAVE) {
		const unsigned long long *r = slab + ((uint64_t)s * per + i) * 2u;
		agg_fold(op, type, acc, cnt, r[0], r[1]);
	}
	for (uint32_t d = MDB_WAVE / 2; d; d >>= 1) {
		const uint64_t oa = (uint64_t)__shfl_down((unsigned long long)acc, d, MDB_WAVE);
		const uint64_t on = (uint64_t)__shfl_down((unsigned long long)cnt, d, MDB_WAVE);
		if (lane < d)
			agg_fold(op, type, acc, cnt, oa, on);
	}
	if (lane == 0) {
		rec[i * 2u] = acc;
		rec[i * 2u + 1u] = cnt;
	}
}

/* ------------------------------------------------------------------ form 3: group i = row i */
__global__ __launch_bounds__(256) void k_agg_identity(mdb_stream_col c, uint64_t n, unsigned long long *__restrict__ rec)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= n)
		return;
	uint64_t bits = 0;
	const bool ok = mdb_stream_cell(c, i, &bits);
	rec[i * 2u] = ok ? agg_to_acc(c.op, c.type, bits) : 0ull;
	rec[i * 2u + 1u] = ok ? 1ull : 0ull;
}

/* ------------------------------------------------------------------ form 1: groups in LDS */
struct agg_lds_args {
	mdb_stream_col a[MDB_AGG_MAX_AGGS];
	mdb_stream_col key;
	int naggs, has_key;
	uint64_t n;
	const uint32_t *first;
	uint32_t G, log2_slots, copies;
	unsigned long long *slab;	/* gridDim.x slabs of naggs * G accumulators */
	uint32_t *status;
};

/* dynamic LDS: [copies][naggs][G] accumulators of two words, then slots keys, then slots group numbers */
__global__ __launch_bounds__(AGG_LDS_THREADS) void k_agg_lds(agg_lds_args A)
{
	extern __shared__ unsigned long long s_mem[];
	const uint32_t slots = A.has_key ? 1u << A.log2_slots : 0u, G = A.G;
	const uint32_t per = (uint32_t)A.naggs * G;
	unsigned long long *s_acc = s_mem;

	for (uint32_t i = threadIdx.x; i < A.copies * per; i += AGG_LDS_THREADS) {
		const int op = A.a[(i % per) / G].op;
		s_acc[2u * i] = op == MDB_AGG_MIN ? ~0ull : 0ull;
		s_acc[2u * i + 1u] = 0ull;
	}
	const mdb_group_lds T = mdb_group_lds_build(s_acc + (size_t)A.copies * per * 2u, slots, A.log2_slots, A.key, A.first, G, AGG_LDS_THREADS);

	const uint32_t copy = threadIdx.x & (A.copies - 1u);
	bool missing = false;
	for (uint64_t i = ((uint64_t)blockIdx.x * AGG_LDS_THREADS + threadIdx.x) * 2u; i < A.n; i += (uint64_t)gridDim.x * AGG_LDS_THREADS * 2u) {
		const bool two = i + 1u < A.n;
		uint64_t kb[2] = { 0, 0 };
		bool kv[2] = { true, two };
		uint32_t grp[2] = { 0u, 0u };
		if (A.has_key) {
			mdb_stream_cell2(A.key, i, two, kb, kv);
#pragma unroll
			for (int r = 0; r < 2; r++) {
				grp[r] = r && !two ? MDB_GROUP_NONE : mdb_group_lds_find(T, kb[r], kv[r]);	/* (r && !two: no second row) */
				missing = missing || (grp[r] == MDB_GROUP_NONE && (!r || two));
			}
		}
		for (int a = 0; a < A.naggs; a++) {
			const mdb_stream_col &c = A.a[a];
			uint64_t vb[2];
			bool vv[2];
			mdb_stream_cell2(c, i, two, vb, vv);
#pragma unroll
			for (int r = 0; r < 2; r++) {
				if (!vv[r] || grp[r] == MDB_GROUP_NONE)
					continue;
				unsigned long long *at = s_acc + ((size_t)(copy * (uint32_t)A.naggs + (uint32_t)a) * G + grp[r]) * 2u;
				if (c.op == MDB_AGG_MIN)
					atomicMin(at, (unsigned long long)mdb_order_image(vb[r], c.type));
				else if (c.op == MDB_AGG_MAX)
					atomicMax(at, (unsigned long long)mdb_order_image(vb[r], c.type));
				else
					atomicAdd(at, (unsigned long long)vb[r]);
				atomicAdd(at + 1, 1ull);
			}
		}
	}
	if (missing)
		mdb_raise(A.status, MDB_GROUPS_ST_KEY_MISSING);
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < per; i += AGG_LDS_THREADS) {
		const mdb_stream_col &c = A.a[i / G];
		uint64_t acc = 0, cnt = 0;
		for (uint32_t k = 0; k < A.copies; k++)
			agg_fold(c.op, c.type, acc, cnt, s_acc[2u * ((size_t)k * per + i)], s_acc[2u * ((size_t)k * per + i) + 1u]);
		A.slab[((uint64_t)blockIdx.x * per + i) * 2u] = acc;
		A.slab[((uint64_t)blockIdx.x * per + i) * 2u + 1u] = cnt;
	}
}

static size_t agg_lds_bytes(uint32_t slots, uint32_t copies, int naggs, uint64_t G)
{
	return mdb_group_lds_bytes(slots) + (size_t)copies * (size_t)naggs * (size_t)G * 16u;
}

extern "C" uint64_t mdb_dev_group_aggregate_lds_groups(int naggs)
{
	uint64_t best = 0;
	if (naggs < 1 || naggs > MDB_AGG_MAX_AGGS)
		return 0;
	for (uint32_t lg = MDB_SET_MIN_LOG2; lg <= 16u; lg++) {
		const uint64_t slots = 1ull << lg;
		if (mdb_group_lds_bytes(slots) >= MDB_GROUP_LDS_BUDGET)
			break;
		uint64_t g = (MDB_GROUP_LDS_BUDGET - mdb_group_lds_bytes(slots)) / ((uint64_t)naggs * 16u);
		g = g < slots / 2u ? g : slots / 2u;
		best = g > best ? g : best;
	}
	return best;
}

/* ------------------------------------------------------------------ form 2: sorted segments */

/* One wave per chunk, one aggregate per launch.  A lane folds its strip in order; what it holds at the strip's end is the part of the run
 * that is open there.  Written: rec[g] for every run that begins and ends inside the chunk; pre[chunk] = the part of the chunk in front of
 * its first head (the whole chunk when it has none), tail[chunk] = the part from its last head on. */
__global__ __launch_bounds__(AGG_SEG_THREADS) void k_agg_seg(mdb_stream_col c, const uint32_t *__restrict__ perm, uint64_t n, uint64_t nchunks,
							      const unsigned long long *__restrict__ hb, const uint32_t *__restrict__ base,
							      const uint32_t *__restrict__ rungroup, unsigned long long *__restrict__ rec,
							      unsigned long long *__restrict__ pre, unsigned long long *__restrict__ tail)
{
	const uint64_t w = (uint64_t)blockIdx.x * (AGG_SEG_THREADS / MDB_WAVE) + (threadIdx.x >> 6);
	if (w >= nchunks)
		return;
	const uint32_t lane = mdb_lane();
	const uint32_t bits = (uint32_t)(hb[w * (AGG_CHUNK / 64u) + (lane >> 2)] >> ((lane & 3u) * AGG_STRIP)) & 0xFFFFu;
	const uint32_t nheads = (uint32_t)__popc(bits);
	uint32_t rank = base[w] + mdb_wave_incl_scan(nheads) - nheads;	/* run number of the strip's first head */
	const uint64_t p0 = w * AGG_CHUNK + (uint64_t)lane * AGG_STRIP;

	uint32_t sp[AGG_STRIP];
	for (uint32_t q = 0; q < AGG_STRIP; q += 4u) {
		if (perm && p0 + q + 3u < n) {
			const uint4 v = *reinterpret_cast<const uint4 *>(perm + p0 + q);	/* (p0 + q is a multiple of 4; perm is 16-byte aligned) */
			sp[q] = v.x;
			sp[q + 1] = v.y;
			sp[q + 2] = v.z;
			sp[q + 3] = v.w;
		} else {
			for (uint32_t j = q; j < q + 4u; j++)
				sp[j] = perm ? (p0 + j < n ? perm[p0 + j] : 0u) : (uint32_t)(p0 + j);
		}
	}
	uint64_t acc = 0, cnt = 0, pacc = 0, pcnt = 0;
	bool seen = false;
#pragma unroll
	for (uint32_t j = 0; j < AGG_STRIP; j++) {
		if (p0 + j >= n)
			break;
		if ((bits >> j) & 1u) {
			if (seen) {	/* a run that began in this strip ends here */
				const uint32_t g = rungroup[rank - 1u];
				rec[(uint64_t)g * 2u] = acc;
				rec[(uint64_t)g * 2u + 1u] = cnt;
			} else {
				pacc = acc;
				pcnt = cnt;
			}
			seen = true;
			rank++;
			acc = cnt = 0;
		}
		uint64_t vb = 0;
		if (mdb_stream_cell(c, sp[j], &vb))
			agg_fold(c.op, c.type, acc, cnt, agg_to_acc(c.op, c.type, vb), 1ull);
	}
	/* segmented inclusive scan over the lanes: (flag, value) (+) (flag', value') = (flag | flag', flag' ? value' : value + value') */
	uint32_t f = seen ? 1u : 0u;
	uint64_t va = acc, vn = cnt;
	for (uint32_t d = 1; d < MDB_WAVE; d <<= 1) {
		const uint32_t of = (uint32_t)__shfl_up((int)f, d, MDB_WAVE);
		uint64_t oa = (uint64_t)__shfl_up((unsigned long long)va, d, MDB_WAVE);
		uint64_t on = (uint64_t)__shfl_up((unsigned long long)vn, d, MDB_WAVE);
		if (lane >= d) {
			if (!f) {
				agg_fold(c.op, c.type, oa, on, va, vn);
				va = oa;
				vn = on;
			}
			f |= of;
		}
	}
	uint32_t ef = (uint32_t)__shfl_up((int)f, 1u, MDB_WAVE);
	uint64_t ea = (uint64_t)__shfl_up((unsigned long long)va, 1u, MDB_WAVE);
	uint64_t en = (uint64_t)__shfl_up((unsigned long long)vn, 1u, MDB_WAVE);
	if (lane == 0) {
		ef = 0;
		ea = en = 0;
	}
	const unsigned long long any = __ballot(seen);
	if (seen) {
		/* the run that is open at the strip's start ends at the strip's first head: what the lanes before hold of it, then this lane's part */
		agg_fold(c.op, c.type, ea, en, pacc, pcnt);
		if (ef) {
			const uint32_t g = rungroup[rank - nheads - 1u];
			rec[(uint64_t)g * 2u] = ea;
			rec[(uint64_t)g * 2u + 1u] = en;
		} else {
			pre[w * 2u] = ea;
			pre[w * 2u + 1u] = en;
		}
	}
	if (lane == MDB_WAVE - 1u) {
		unsigned long long *to = any ? tail : pre;
		to[w * 2u] = va;
		to[w * 2u + 1u] = vn;
	}
}

/* One wave per chunk that has a head: the run of its last head goes on through every chunk without a head up to the first head of a later
 * chunk (or the end).  Lane l folds the records of chunks w + 1 + l, w + 1 + l + 64 ... in that order, the lanes are folded pairwise in a
 * fixed tree, and the chunk's own tail goes in front. */
__global__ __launch_bounds__(AGG_SEG_THREADS) void k_agg_seg_fin(int op, int type, uint64_t nchunks, const uint32_t *__restrict__ base,
								  const uint32_t *__restrict__ rungroup, const unsigned long long *__restrict__ pre,
								  const unsigned long long *__restrict__ tail, unsigned long long *__restrict__ rec)
{
	const uint64_t w = (uint64_t)blockIdx.x * (AGG_SEG_THREADS / MDB_WAVE) + (threadIdx.x >> 6);
	if (w >= nchunks || base[w + 1] == base[w])
		return;
	const uint32_t lane = mdb_lane();
	uint64_t acc = 0, cnt = 0;
	for (uint64_t c0 = w + 1; c0 < nchunks; c0 += MDB_WAVE) {
		const uint64_t c = c0 + lane;
		const bool in = c < nchunks;
		const unsigned long long m = __ballot(in && base[c + 1] != base[c]);
		const uint32_t stop = m ? (uint32_t)__ffsll((long long)m) - 1u : MDB_WAVE;
		if (in && lane <= stop)
			agg_fold(op, type, acc, cnt, pre[c * 2u], pre[c * 2u + 1u]);
		if (m)
			break;
	}
	for (uint32_t d = MDB_WAVE / 2; d; d >>= 1) {
		const uint64_t oa = (uint64_t)__shfl_down((unsigned long long)acc, d, MDB_WAVE);
		const uint64_t on = (uint64_t)__shfl_down((unsigned long long)cnt, d, MDB_WAVE);
		if (lane < d)
			agg_fold(op, type, acc, cnt, oa, on);
	}
	if (lane == 0) {
		uint64_t ta = tail[w * 2u], tn = tail[w * 2u + 1u];
		agg_fold(op, type, ta, tn, acc, cnt);
		const uint32_t g = rungroup[base[w + 1] - 1u];
		rec[(uint64_t)g * 2u] = ta;
		rec[(uint64_t)g * 2u + 1u] = tn;
	}
}

/* ------------------------------------------------------------------ host side */

static mdb_stream_col agg_col_of(const struct mdb_agg *a) { return mdb_stream_col_of(a->values, a->nullbits, a->rid, a->op, a->type); }

static int agg_finish_all(mdb_dev_ctx *ctx, const unsigned long long *rec, uint32_t nslab, uint64_t G, const struct mdb_agg *aggs, int naggs)
{
	const uint64_t per = (uint64_t)naggs * G;
	for (int a = 0; a < naggs; a++)
		MDB_LAUNCH(ctx, "agg_finish", k_agg_finish, (uint32_t)((G + 255u) / 256u), 256, rec + (uint64_t)a * G * 2u, nslab, per, G, (int)aggs[a].op,
			   (int)aggs[a].type, (uint64_t *)aggs[a].out, (unsigned long long *)aggs[a].out_nullbits);
	return MIDORIDB_OK;
}

static int agg_form_lds(mdb_dev_ctx *ctx, const struct mdb_sort_key *keys, int nkeys, uint64_t n, const uint32_t *first, uint64_t G,
			const struct mdb_agg *aggs, int naggs)
{
	mdb_dev_tmp tmp(ctx);
	agg_lds_args A;
	memset(&A, 0, sizeof(A));
	for (int a = 0; a < naggs; a++)
		A.a[a] = agg_col_of(&aggs[a]);
	A.naggs = naggs;
	A.has_key = nkeys == 1;
	if (A.has_key)
		A.key = mdb_stream_col_of_key(&keys[0]);
	A.n = n;
	A.first = first;
	A.G = (uint32_t)G;
	A.log2_slots = A.has_key ? mdb_group_lds_log2(G) : MDB_SET_MIN_LOG2;
	const uint32_t slots = A.has_key ? 1u << A.log2_slots : 0u;
	A.copies = 1;
	while (A.copies < AGG_MAX_COPIES && agg_lds_bytes(slots, A.copies * 2u, naggs, G) <= MDB_GROUP_LDS_BUDGET)
		A.copies *= 2u;
	const size_t lds = agg_lds_bytes(slots, A.copies, naggs, G);
	if (lds > MDB_GROUP_LDS_BUDGET)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "group_aggregate: %llu groups do not fit the LDS form", (unsigned long long)G);
	const uint64_t grid = mdb_group_lds_grid(ctx, lds, n);
	const uint64_t per = (uint64_t)naggs * G;
	A.slab = (unsigned long long *)tmp.take(grid * per * 16u);
	A.status = (uint32_t *)tmp.take(256);
	unsigned long long *rec = (unsigned long long *)tmp.take(per * 16u);
	if (!A.slab || !A.status || !rec)
		return mdb_set_err(ctx, -MIDORIDB_NOMEM, "group_aggregate: no device memory for %llu slabs", (unsigned long long)grid);
	MDB_HIP(ctx, hipMemsetAsync(A.status, 0, 4, ctx->stream));
	MDB_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_agg_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	MDB_LAUNCH_LDS(ctx, "agg_lds", k_agg_lds, (uint32_t)grid, AGG_LDS_THREADS, lds, A);
	agg_ops O;
	memset(&O, 0, sizeof(O));
	for (int a = 0; a < naggs; a++) {
		O.op[a] = aggs[a].op;
		O.type[a] = aggs[a].type;
	}
	MDB_LAUNCH(ctx, "agg_fold_slabs", k_agg_fold_slabs, (uint32_t)((per + 3u) / 4u), 256, (const unsigned long long *)A.slab, (uint32_t)grid, per, G, O, rec);
	int rc = agg_finish_all(ctx, rec, 1u, G, aggs, naggs);
	if (rc)
		return rc;
	return mdb_groups_status(ctx, A.status, "group_aggregate", "groups in LDS");
}

static int agg_form_sorted(mdb_dev_ctx *ctx, const struct mdb_sort_key *keys, int nkeys, uint64_t n, const uint32_t *first, uint64_t G,
			   const struct mdb_agg *aggs, int naggs)
{
	mdb_dev_tmp tmp(ctx);
	mdb_runs R;
	int rc = mdb_runs_find(ctx, keys, nkeys, n, first, G, "group_aggregate", "sorted segments", tmp, &R);
	if (rc)
		return rc;
	const uint64_t nchunks = R.nchunks;
	unsigned long long *pre = (unsigned long long *)tmp.take(nchunks * 16u);
	unsigned long long *tail = (unsigned long long *)tmp.take(nchunks * 16u);
	unsigned long long *rec = (unsigned long long *)tmp.take((uint64_t)naggs * G * 16u);
	if (!pre || !tail || !rec)
		return mdb_set_err(ctx, -MIDORIDB_NOMEM, "group_aggregate: no device memory for %llu chunks", (unsigned long long)nchunks);
	const uint32_t seg_grid = (uint32_t)((nchunks + (AGG_SEG_THREADS / MDB_WAVE) - 1u) / (AGG_SEG_THREADS / MDB_WAVE));
	for (int a = 0; a < naggs; a++) {
		unsigned long long *r = rec + (uint64_t)a * G * 2u;
		MDB_LAUNCH(ctx, "agg_seg", k_agg_seg, seg_grid, AGG_SEG_THREADS, agg_col_of(&aggs[a]), R.perm, n, nchunks, R.hb, R.base, R.rungroup, r, pre, tail);
		MDB_LAUNCH(ctx, "agg_seg_fin", k_agg_seg_fin, seg_grid, AGG_SEG_THREADS, (int)aggs[a].op, (int)aggs[a].type, nchunks, R.base, R.rungroup,
			   (const unsigned long long *)pre, (const unsigned long long *)tail, r);
	}
	if ((rc = agg_finish_all(ctx, rec, 1u, G, aggs, naggs)))
		return rc;
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return MIDORIDB_OK;
}

extern "C" int mdb_dev_group_aggregate(mdb_dev_ctx *ctx, const struct mdb_sort_key *keys, int nkeys, uint64_t n, const uint32_t *first, uint64_t G,
				       const struct mdb_agg *aggs, int naggs, uint32_t *out_form)
{
	if (!ctx)
		return -MIDORIDB_ERROR;
	if (out_form)
		*out_form = 0;
	if (!aggs || naggs < 1 || naggs > MDB_AGG_MAX_AGGS)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_aggregate: 1 ... %d aggregates per call", MDB_AGG_MAX_AGGS);
	if (nkeys != MDB_AGG_IDENTITY && (nkeys < 0 || nkeys > MDB_SORT_MAX_KEYS || (nkeys && !keys)))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_aggregate: 0 ... %d group key columns", MDB_SORT_MAX_KEYS);
	if (n >= MDB_NO_ROW || G > n + (n ? 0u : 1u))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_aggregate: %llu groups over %llu rows", (unsigned long long)G, (unsigned long long)n);
	bool order_free = true;
	for (int a = 0; a < naggs; a++) {
		const struct mdb_agg *g = &aggs[a];
		if (g->op < MDB_AGG_SUM || g->op > MDB_AGG_AVG || (g->type != MDB_T_INT64 && g->type != MDB_T_DOUBLE))
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_aggregate: aggregate %d: unknown function %d or cell type %d", a, g->op, g->type);
		if (!g->out || !g->out_nullbits || (n && !g->values))
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_aggregate: aggregate %d: no cells or no place for the result", a);
		order_free = order_free && (g->type == MDB_T_INT64 || agg_is_minmax(g->op));
	}
	if (nkeys == 0 && G != (n ? 1u : G))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_aggregate: without group keys the stream is one group");
	if (nkeys == MDB_AGG_IDENTITY && G != n)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_aggregate: the identity form takes as many groups as rows");
	if (nkeys > 0 && G && !first)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_aggregate: no first rows");
	if (!G)
		return MIDORIDB_OK;
	if (!n) {	/* (one group over no row: NULL) */
		mdb_dev_tmp tmp(ctx);
		unsigned long long *rec = (unsigned long long *)tmp.take((uint64_t)naggs * G * 16u);
		if (!rec)
			return mdb_set_err(ctx, -MIDORIDB_NOMEM, "group_aggregate: no device memory");
		MDB_HIP(ctx, hipMemsetAsync(rec, 0, (uint64_t)naggs * G * 16u, ctx->stream));
		int rc = agg_finish_all(ctx, rec, 1u, G, aggs, naggs);
		if (rc)
			return rc;
		MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		return MIDORIDB_OK;
	}
	if (nkeys == MDB_AGG_IDENTITY) {
		mdb_dev_tmp tmp(ctx);
		unsigned long long *rec = (unsigned long long *)tmp.take((uint64_t)naggs * n * 16u);
		if (!rec)
			return mdb_set_err(ctx, -MIDORIDB_NOMEM, "group_aggregate: no device memory");
		for (int a = 0; a < naggs; a++)
			MDB_LAUNCH(ctx, "agg_identity", k_agg_identity, (uint32_t)((n + 255u) / 256u), 256, agg_col_of(&aggs[a]), n, rec + (uint64_t)a * n * 2u);
		int rc = agg_finish_all(ctx, rec, 1u, n, aggs, naggs);
		if (rc)
			return rc;
		MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (out_form)
			*out_form = 3;
		return MIDORIDB_OK;
	}
	const bool lds = order_free && nkeys <= 1 && G <= mdb_dev_group_aggregate_lds_groups(naggs) && !mdb_knob_off("MDB_AGG_LDS");
	const int rc = lds ? agg_form_lds(ctx, keys, nkeys, n, first, G, aggs, naggs) : agg_form_sorted(ctx, keys, nkeys, n, first, G, aggs, naggs);
	if (!rc && out_form)
		*out_form = lds ? 1u : 2u;
	return rc;
}
