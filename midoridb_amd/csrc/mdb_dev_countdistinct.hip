/*
 * mdb_dev_countdistinct.hip - COUNT(DISTINCT col) per group (mdb_dev_group_count_distinct): an extension, as SUM / MIN / MAX / AVG are
 * (mdb_dev_aggregate.hip) - the reference counts rows and nothing else.
 *
 * The GROUP BY operators have delivered first[G] before this operator runs.  Step A finds the group of every row once per call
 * (gid[n], shared by all columns; nothing for one group):
 *   A1  one 8-byte key and G <= mdb_dev_group_count_distinct_lds_groups(): every workgroup builds the key -> group table in LDS from the
 *       keys at first[g] - the table of the aggregate operator's LDS form: open addressing at load <= 1/2, mdb_set_slot_of, the NULL key
 *       in a slot of its own - and streams its rows through it.
 *   A2  otherwise: mdb_dev_sort_perm over the keys is stable, so every group is one run whose head is the group's first row; heads are
 *       marked and numbered by a scan, the run whose head sits at stream position p is the group g with first[g] == p (binary search).
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

#define CD_LDS_THREADS 1024
#define CD_LDS_BUDGET (160u * 1024u - 1024u)	/* bytes of dynamic LDS step A1 may take (the CU has 160 KiB; 1 KiB stays free) */
#define CD_THREADS 256
#define CD_EMPTY 0xFFFFFFFFu
#define CD_WAVE_WORDS 1024u			/* a group of up to this many bitmap words is counted by a wave, a longer one by a workgroup */
/* flags of the operator's own status word */
#define CD_ST_KEY_MISSING 1u	/* a row's group key is the key of no group / a run's head is nobody's first row: first[] does not belong to these keys */
#define CD_ST_RUNS_DIFFER 2u	/* more runs of equal keys than groups */
#define CD_ST_OUT_OF_RANGE 4u	/* form 1: a cell outside the promised [min, max] */
static_assert(mdb_flags_distinct({ CD_ST_KEY_MISSING, CD_ST_RUNS_DIFFER, CD_ST_OUT_OF_RANGE }), "count distinct: two status flags share a bit");

struct cd_col {
	const uint64_t *values;
	const uint64_t *nullbits;
	const uint32_t *rid;
	int32_t type;
};

struct cd_keys {
	cd_col k[MDB_SORT_MAX_KEYS];
	int nkeys;
};

/* the cell of stream position sp: false for a NULL cell and for "no row" (the aggregate operator's agg_cell) */
__device__ static inline bool cd_cell(const cd_col &c, uint64_t sp, uint64_t *bits)
{
	uint64_t row = sp;
	if (c.rid) {
		const uint32_t r = c.rid[sp];
		if (r == MDB_NO_ROW)
			return false;
		row = r;
	}
	if (c.nullbits && mdb_bit_is_set(c.nullbits, row))
		return false;
	*bits = c.values[row];
	return true;
}

/* the cells of stream positions i and i + 1 (i even; two: both exist): a column read without row ids takes one 16-byte load where its
 * address allows (a column that starts 8 bytes off a 16-byte boundary is read by 8-byte loads) and one look at the NULL word (agg_cell2) */
__device__ static inline void cd_cell2(const cd_col &c, uint64_t i, bool two, uint64_t bits[2], bool valid[2])
{
	if (c.rid) {
		valid[0] = cd_cell(c, i, &bits[0]);
		valid[1] = two && cd_cell(c, i + 1, &bits[1]);
		return;
	}
	const uint64_t *q = c.values + i;
	if (two && !((uintptr_t)q & 15u)) {
		const ulonglong2 w = *reinterpret_cast<const ulonglong2 *>(q);
		bits[0] = w.x;
		bits[1] = w.y;
	} else {
		bits[0] = q[0];
		bits[1] = two ? q[1] : 0;
	}
	const uint64_t nw = c.nullbits ? c.nullbits[i >> 6] >> (i & 63) : 0ull;	/* (i is even: i + 1 lies in the same word) */
	valid[0] = !(nw & 1ull);
	valid[1] = two && !(nw & 2ull);
}

/* ------------------------------------------------------------------ step A1: the key -> group table in LDS */
struct cd_lds_args {
	cd_col key;
	uint64_t n;
	const uint32_t *first;
	uint32_t G, log2_slots;
	uint32_t *gid;		/* n group numbers (8-byte aligned) */
	uint32_t *status;
};

/* dynamic LDS: slots keys, then slots group numbers */
__global__ __launch_bounds__(CD_LDS_THREADS) void k_cd_gid_lds(cd_lds_args A)
{
	extern __shared__ unsigned long long s_key[];
	__shared__ uint32_t s_nullgrp;
	const uint32_t slots = 1u << A.log2_slots, G = A.G;
	uint32_t *s_grp = reinterpret_cast<uint32_t *>(s_key + slots);

	for (uint32_t i = threadIdx.x; i < slots; i += CD_LDS_THREADS)
		s_grp[i] = CD_EMPTY;
	if (threadIdx.x == 0)
		s_nullgrp = CD_EMPTY;
	__syncthreads();
	for (uint32_t g = threadIdx.x; g < G; g += CD_LDS_THREADS) {
		uint64_t kb = 0;
		if (!cd_cell(A.key, A.first[g], &kb)) {
			s_nullgrp = g;
			continue;
		}
		uint32_t s = (uint32_t)mdb_set_slot_of(kb, A.log2_slots);
		for (uint32_t step = 0; step < slots; step++, s = (s + 1u) & (slots - 1u))
			if (atomicCAS(&s_grp[s], CD_EMPTY, g) == CD_EMPTY) {	/* (G <= slots / 2: a free slot exists) */
				s_key[s] = kb;
				break;
			}
	}
	__syncthreads();

	bool missing = false;
	for (uint64_t i = ((uint64_t)blockIdx.x * CD_LDS_THREADS + threadIdx.x) * 2u; i < A.n; i += (uint64_t)gridDim.x * CD_LDS_THREADS * 2u) {
		const bool two = i + 1u < A.n;
		uint64_t kb[2] = { 0, 0 };
		bool kv[2] = { true, two };
		uint32_t grp[2] = { CD_EMPTY, CD_EMPTY };
		cd_cell2(A.key, i, two, kb, kv);
#pragma unroll
		for (int r = 0; r < 2; r++) {
			if (r && !two)
				continue;
			uint32_t g = CD_EMPTY;
			if (!kv[r]) {
				g = s_nullgrp;
			} else {
				uint32_t s = (uint32_t)mdb_set_slot_of(kb[r], A.log2_slots);
				for (uint32_t step = 0; step < slots; step++, s = (s + 1u) & (slots - 1u)) {
					const uint32_t at = s_grp[s];
					if (at == CD_EMPTY)
						break;
					if (s_key[s] == kb[r]) {
						g = at;
						break;
					}
				}
			}
			grp[r] = g;
			missing = missing || g == CD_EMPTY;
		}
		if (two)
			*reinterpret_cast<uint2 *>(A.gid + i) = make_uint2(grp[0], grp[1]);	/* (i is even, gid is 8-byte aligned) */
		else
			A.gid[i] = grp[0];
	}
	if (missing)
		mdb_raise(A.status, CD_ST_KEY_MISSING);
}

static uint32_t cd_lds_log2_max(void)
{
	uint32_t lg = MDB_SET_MIN_LOG2;
	while ((2ull << lg) * 12u <= CD_LDS_BUDGET)
		lg++;
	return lg;
}

extern "C" uint64_t mdb_dev_group_count_distinct_lds_groups(void)
{
	return (1ull << cd_lds_log2_max()) / 2u;	/* 12 bytes per slot, load <= 1/2 */
}

extern "C" uint64_t mdb_dev_count_distinct_bitmap_bits(void)
{
	return MDB_COUNT_DISTINCT_BITMAP_BITS;
}

/* ------------------------------------------------------------------ step A2: the runs of the sorted stream */

/* flag[p] = 1 when sorted position p begins a run (position 0, or a key column differs from the row before: NULL equals NULL, values by
 * their bits), else 0 */
__global__ __launch_bounds__(CD_THREADS) void k_cd_run_heads(cd_keys K, const uint32_t *__restrict__ perm, uint64_t n, uint32_t *__restrict__ flag)
{
	const uint64_t p = (uint64_t)blockIdx.x * CD_THREADS + threadIdx.x;
	if (p >= n)
		return;
	bool head = p == 0;
	if (p) {
		const uint64_t s1 = perm[p], s0 = perm[p - 1];
		for (int k = 0; k < K.nkeys && !head; k++) {
			uint64_t b1 = 0, b0 = 0;
			const bool v1 = cd_cell(K.k[k], s1, &b1), v0 = cd_cell(K.k[k], s0, &b0);
			head = v0 != v1 || (v1 && b0 != b1);
		}
	}
	flag[p] = head ? 1u : 0u;
}

/* before[p] = heads in front of p (before[n] = runs): rungroup[r] = the group whose first row is the head of run r */
__global__ __launch_bounds__(CD_THREADS) void k_cd_run_groups(const uint32_t *__restrict__ before, const uint32_t *__restrict__ perm, uint64_t n,
							       const uint32_t *__restrict__ first, uint64_t G, uint32_t *__restrict__ rungroup, uint32_t *status)
{
	const uint64_t p = (uint64_t)blockIdx.x * CD_THREADS + threadIdx.x;
	if (p >= n || before[p + 1] == before[p])
		return;
	const uint32_t r = before[p];
	if (r >= G) {
		mdb_raise(status, CD_ST_RUNS_DIFFER);
		return;
	}
	const uint32_t sp = perm[p];
	uint64_t lo = 0, hi = G;
	while (lo < hi) {
		const uint64_t mid = (lo + hi) >> 1;
		if (first[mid] < sp)
			lo = mid + 1;
		else
			hi = mid;
	}
	if (lo >= G || first[lo] != sp) {
		mdb_raise(status, CD_ST_KEY_MISSING);
		return;
	}
	rungroup[r] = (uint32_t)lo;
}

/* (after the host has seen as many runs as groups and no flag: every run has its group) */
__global__ __launch_bounds__(CD_THREADS) void k_cd_run_scatter(const uint32_t *__restrict__ before, const uint32_t *__restrict__ perm, uint64_t n,
								const uint32_t *__restrict__ rungroup, uint32_t *__restrict__ gid)
{
	const uint64_t p = (uint64_t)blockIdx.x * CD_THREADS + threadIdx.x;
	if (p >= n)
		return;
	gid[perm[p]] = rungroup[before[p + 1] - 1u];	/* (position 0 is a head: before[p + 1] >= 1) */
}

/* ------------------------------------------------------------------ form 1: a bitmap per group */

/* every valid cell marks bit (value - min) of its group's words; gid == NULL: one group */
__global__ __launch_bounds__(CD_THREADS) void k_cd_mark(cd_col c, const uint32_t *__restrict__ gid, uint64_t n, uint64_t G, int64_t min, uint64_t span,
							 uint64_t wpg, unsigned long long *__restrict__ bitmap, uint32_t *status)
{
	bool outside = false;
	for (uint64_t i = ((uint64_t)blockIdx.x * CD_THREADS + threadIdx.x) * 2u; i < n; i += (uint64_t)gridDim.x * CD_THREADS * 2u) {
		const bool two = i + 1u < n;
		uint64_t vb[2] = { 0, 0 };
		bool vv[2] = { false, false };
		uint32_t g[2] = { 0u, 0u };
		cd_cell2(c, i, two, vb, vv);
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
__global__ __launch_bounds__(CD_THREADS) void k_cd_sorted_heads(cd_col c, const uint32_t *__restrict__ gid, const uint32_t *__restrict__ perm, uint64_t n,
								 uint64_t G, unsigned long long *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * CD_THREADS + threadIdx.x;
	const bool in = i < n;
	const uint32_t lane = mdb_lane();
	uint64_t b1 = 0;
	uint32_t g1 = CD_EMPTY;
	bool v1 = false;
	if (in) {
		const uint32_t sp = perm[i];
		g1 = gid ? gid[sp] : 0u;
		v1 = cd_cell(c, sp, &b1);
		if (v1)
			(void)mdb_set_canonical(c.type, &b1);
	}
	uint64_t b0 = (uint64_t)__shfl_up((unsigned long long)b1, 1u, MDB_WAVE);
	uint32_t g0 = (uint32_t)__shfl_up((int)g1, 1u, MDB_WAVE);
	bool v0 = __shfl_up((int)v1, 1u, MDB_WAVE) != 0;
	if (lane == 0) {
		g0 = CD_EMPTY;
		v0 = false;
		if (in && i) {
			const uint32_t sp = perm[i - 1];
			g0 = gid ? gid[sp] : 0u;
			b0 = 0;
			v0 = cd_cell(c, sp, &b0);
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
__global__ __launch_bounds__(CD_THREADS) void k_cd_identity(cd_col c, uint64_t n, int64_t *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * CD_THREADS + threadIdx.x;
	if (i >= n)
		return;
	uint64_t bits = 0;
	out[i] = cd_cell(c, i, &bits) ? 1 : 0;
}

/* ------------------------------------------------------------------ host side */

static cd_col cd_col_of(const struct mdb_count_distinct *a)
{
	cd_col c;
	c.values = (const uint64_t *)a->values;
	c.nullbits = a->nullbits;
	c.rid = a->rid;
	c.type = a->type;
	return c;
}

static cd_col cd_col_of_key(const struct mdb_sort_key *k)
{
	cd_col c;
	c.values = (const uint64_t *)k->values;
	c.nullbits = k->nullbits;
	c.rid = k->rid;
	c.type = k->type;
	return c;
}

struct cd_tmp {
	mdb_dev_ctx *ctx;
	void *p[16];
	int n;
	explicit cd_tmp(mdb_dev_ctx *c) : ctx(c), n(0) {}
	~cd_tmp()
	{
		for (int i = 0; i < n; i++)
			(void)mdb_cached_free(ctx, p[i]);
	}
	void *take(size_t bytes)
	{
		void *q = NULL;
		if (n == 16 || mdb_cached_alloc(ctx, bytes, &q))
			return NULL;
		p[n++] = q;
		return q;
	}
};

static uint32_t cd_grid(uint64_t items)
{
	return (uint32_t)((items + CD_THREADS - 1u) / CD_THREADS);
}

/* the flags of the status word; *out_of_range (may be NULL: then the flag is not expected) is the one that is no error */
static int cd_status(mdb_dev_ctx *ctx, const uint32_t *d_status, const char *what, bool *out_of_range)
{
	uint32_t h = 0;
	MDB_HIP(ctx, hipMemcpyAsync(&h, d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (h & CD_ST_RUNS_DIFFER)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct (%s): the keys form more runs than there are groups", what);
	if (h & CD_ST_KEY_MISSING)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct (%s): a row's key belongs to no group of first[]", what);
	if (out_of_range)
		*out_of_range = (h & CD_ST_OUT_OF_RANGE) != 0;
	return MIDORIDB_OK;
}

/* step A1 */
static int cd_gid_lds(mdb_dev_ctx *ctx, const struct mdb_sort_key *key, uint64_t n, const uint32_t *first, uint64_t G, uint32_t *gid, uint32_t *status)
{
	cd_lds_args A;
	memset(&A, 0, sizeof(A));
	A.key = cd_col_of_key(key);
	A.n = n;
	A.first = first;
	A.G = (uint32_t)G;
	uint32_t lg = MDB_SET_MIN_LOG2;
	while ((1ull << lg) < 2u * G)
		lg++;
	A.log2_slots = lg;
	A.gid = gid;
	A.status = status;
	const size_t lds = ((size_t)1u << lg) * 12u;
	if (lds > CD_LDS_BUDGET)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "group_count_distinct: %llu groups do not fit the LDS table", (unsigned long long)G);
	/* two workgroups per CU while their LDS allows, never more workgroups than 8192-row shares */
	uint64_t grid = (uint64_t)ctx->num_cus * (lds * 2u <= 160u * 1024u ? 2u : 1u);
	const uint64_t shares = (n + 8191u) / 8192u;
	grid = grid < shares ? grid : shares;
	grid = grid ? grid : 1;
	MDB_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cd_gid_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	MDB_LAUNCH_LDS(ctx, "cd_gid_lds", k_cd_gid_lds, (uint32_t)grid, CD_LDS_THREADS, lds, A);
	return cd_status(ctx, status, "groups in LDS", NULL);
}

/* step A2 */
static int cd_gid_sorted(mdb_dev_ctx *ctx, const struct mdb_sort_key *keys, int nkeys, uint64_t n, const uint32_t *first, uint64_t G, uint32_t *gid,
			 uint32_t *status)
{
	cd_tmp tmp(ctx);
	struct mdb_sort_key sk[MDB_SORT_MAX_KEYS];
	int rc;
	uint32_t *perm = (uint32_t *)tmp.take(n * 4u + 16u);
	uint32_t *before = (uint32_t *)tmp.take((n + 1u) * 4u);
	uint32_t *scan_tmp = (uint32_t *)tmp.take(mdb_scan_scratch_words(n + 1u) * 4u);
	uint32_t *rungroup = (uint32_t *)tmp.take(G * 4u);
	if (!perm || !before || !scan_tmp || !rungroup)
		return mdb_set_err(ctx, -MIDORIDB_NOMEM, "group_count_distinct: no device memory for the runs of %llu rows", (unsigned long long)n);
	cd_keys K;
	memset(&K, 0, sizeof(K));
	K.nkeys = nkeys;
	for (int k = 0; k < nkeys; k++) {
		sk[k] = keys[k];
		sk[k].desc = 0;
		K.k[k] = cd_col_of_key(&keys[k]);
	}
	if ((rc = mdb_dev_sort_perm(ctx, sk, nkeys, n, perm)))
		return rc;
	MDB_HIP(ctx, hipMemsetAsync(before + n, 0, 4, ctx->stream));
	MDB_LAUNCH(ctx, "cd_run_heads", k_cd_run_heads, cd_grid(n), CD_THREADS, K, (const uint32_t *)perm, n, before);
	if ((rc = mdb_scan_u32_inplace(ctx, before, n + 1u, scan_tmp)))
		return rc;
	MDB_LAUNCH(ctx, "cd_run_groups", k_cd_run_groups, cd_grid(n), CD_THREADS, (const uint32_t *)before, (const uint32_t *)perm, n, first, G, rungroup,
		   status);
	uint32_t runs = 0;
	MDB_HIP(ctx, hipMemcpyAsync(&runs, before + n, 4, hipMemcpyDeviceToHost, ctx->stream));
	if ((rc = cd_status(ctx, status, "sorted runs", NULL)))
		return rc;
	if (runs != G)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "group_count_distinct (sorted runs): %u runs of equal keys, %llu groups", runs, (unsigned long long)G);
	MDB_LAUNCH(ctx, "cd_run_scatter", k_cd_run_scatter, cd_grid(n), CD_THREADS, (const uint32_t *)before, (const uint32_t *)perm, n,
		   (const uint32_t *)rungroup, gid);
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
	cd_tmp tmp(ctx);
	int rc;
	unsigned long long *bitmap = (unsigned long long *)tmp.take(G * wpg * 8u);
	if (!bitmap)
		return mdb_set_err(ctx, -MIDORIDB_NOMEM, "group_count_distinct: no device memory for a bitmap of %llu words", (unsigned long long)(G * wpg));
	MDB_HIP(ctx, hipMemsetAsync(bitmap, 0, G * wpg * 8u, ctx->stream));
	MDB_HIP(ctx, hipMemsetAsync(status, 0, 4, ctx->stream));
	uint64_t grid = (n + CD_THREADS * 8u - 1u) / (CD_THREADS * 8u);	/* eight rows per thread, at most eight workgroups per CU */
	grid = grid < (uint64_t)ctx->num_cus * 8u ? grid : (uint64_t)ctx->num_cus * 8u;
	MDB_LAUNCH(ctx, "cd_mark", k_cd_mark, (uint32_t)(grid ? grid : 1u), CD_THREADS, cd_col_of(c), gid, n, G, c->min, span, wpg, bitmap, status);
	if ((rc = cd_status(ctx, status, "bitmap", redo)))
		return rc;
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
	cd_tmp tmp(ctx);
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

	cd_tmp tmp(ctx);
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
		rc = cd_gid_sorted(ctx, keys, nkeys, n, first, G, gid, status);
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
