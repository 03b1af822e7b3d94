/*
 * mdb_dev_rowset.hip - whole rows as set members: the device operators behind UNION [ALL], INTERSECT and EXCEPT (contracts:
 * include/mdb_dev.h, "row sets").
 *
 * mdb_dev_rows_semi() is a semi- / anti-join on ENTIRE rows of up to MDB_ROWS_MAX_COLS columns with NULL = NULL - what neither the device
 * sets (one column, NULLs skipped: mdb_dev_setbuild.hip) nor the joins (keys whose ranges fit 63 bits) offer.  The build rows go into an
 * open-addressing table in global memory whose 32-bit slots hold a BUILD ROW NUMBER and nothing else (ROWS_EMPTY: none); the cells stay where
 * they are and are read through the row number when two rows have to be compared.
 *
 * Passes (all through MDB_LAUNCH, each under a name of its own):
 *
 *   rows_insert   linear probing from the row hash's slot on.  The slot is READ first: empty - a 32-bit compare-and-swap (empty -> row
 *                 number) claims it; occupied - the two rows' cells are compared: equal means done (a duplicate costs loads only), different
 *                 means the next slot.  A slot changes exactly once and a build row's cells never change, so a slot is either empty or
 *                 complete: no thread ever waits for another.  A member is counted where the CAS succeeded (a ballot per wave, one atomic
 *                 per wave that found new members)
 *   rows_probe    the same path for every probe row, ending at an empty slot; one ballot per wave is one word of the hit bitmap, and every
 *                 workgroup leaves the number of its hits
 *   (scan)        mdb_scan_u32_inplace over the workgroups' counts
 *   rows_compact  the bitmap's set bits as ascending probe positions
 *
 * Every probe loop, in insert and in probe, ends after `slots` steps whatever the table holds: a wrong table gives a wrong answer, never a
 * spin.  The slot count is a power of two, at least 16 and at least twice the build rows, so a loop that runs out of steps is an internal error.
 *
 * mdb_dev_concat64() is the column of a UNION: the cells of up to MDB_CONCAT_MAX_PARTS parts one behind the other, their NULL bits moved to
 * bit offsets that are in general no multiple of 64, in one launch.
 */
#include "mdb_dev_internal.h"
#include "mdb_dev_stream.h"

#define ROWS_THREADS 256
#define ROWS_WAVES (ROWS_THREADS / MDB_WAVE)
#define ROWS_EMPTY 0xFFFFFFFFu
#define ROWS_ST_MEMBERS 0
#define ROWS_ST_NO_SLOT 1	/* a probe loop of the insertion ran its `slots` steps without a place */
#define ROWS_ST_WORDS 2
#define ROWS_NULL_WORD 0x6E756C6C4E554C4Cull	/* what a NULL cell contributes to the row hash instead of the bits under it */
#define ROWS_SEED 0x9E3779B97F4A7C15ull

struct rows_side {
	mdb_stream_col col[MDB_ROWS_MAX_COLS];
	unsigned long long n;
	int ncols;
};

/* cell i of a column (mdb_stream_cell): true = NULL (NULL bit or no row) and *bits = 0, else *bits = its 64 bits */
__device__ static inline bool rows_cell(const mdb_stream_col &c, unsigned long long i, unsigned long long *bits)
{
	uint64_t v = 0;
	const bool isnull = !mdb_stream_cell(c, i, &v);
	*bits = v;
	return isnull;
}

/* The row hash: every cell's word goes through fmix64 - a bijection, so all 64 bits of every column reach every bit of the hash, the top
 * ones that number the slot included - together with what the columns before it left; a NULL cell contributes ROWS_NULL_WORD and its flag,
 * never the bits under it.  The cells are kept for the comparisons that follow. */
__device__ static inline unsigned long long rows_hash(const rows_side &s, unsigned long long i, unsigned long long *cell, uint32_t *nullmask)
{
	unsigned long long h = ROWS_SEED;
	uint32_t nm = 0;
#pragma unroll 1
	for (int c = 0; c < s.ncols; c++) {
		unsigned long long v;
		const bool isnull = rows_cell(s.col[c], i, &v);
		cell[c] = v;
		nm |= (uint32_t)isnull << c;
		h = mdb_fmix64((h + (isnull ? 1ull : 0ull)) ^ (isnull ? ROWS_NULL_WORD : v)) + ROWS_SEED * (unsigned long long)(c + 1);
	}
	*nullmask = nm;
	return mdb_fmix64(h);
}

/* does build row b equal the row whose cells and NULL flags are given? */
__device__ static inline bool rows_equal(const rows_side &build, uint32_t b, const unsigned long long *cell, uint32_t nullmask)
{
#pragma unroll 1
	for (int c = 0; c < build.ncols; c++) {
		unsigned long long v;
		const bool isnull = rows_cell(build.col[c], b, &v);
		if (isnull != (bool)((nullmask >> c) & 1u) || v != cell[c])
			return false;
	}
	return true;
}

__global__ __launch_bounds__(ROWS_THREADS) void k_rows_insert(rows_side build, uint32_t *__restrict__ slots, unsigned log2,
							      unsigned long long *__restrict__ state)
{
	const unsigned long long nslots = 1ull << log2, mask = nslots - 1;
	/* (the bound is a multiple of the workgroup: all lanes of a wave make the same number of trips, the ballot sees whole waves) */
	const unsigned long long n_up = (build.n + ROWS_THREADS - 1) / ROWS_THREADS * ROWS_THREADS;
	for (unsigned long long i = (unsigned long long)blockIdx.x * ROWS_THREADS + threadIdx.x; i < n_up; i += (unsigned long long)gridDim.x * ROWS_THREADS) {
		int placed = 0;
		if (i < build.n) {
			unsigned long long cell[MDB_ROWS_MAX_COLS];
			uint32_t nullmask;
			unsigned long long s = rows_hash(build, i, cell, &nullmask) >> (64 - log2);
			placed = -1;
			for (unsigned long long step = 0; step < nslots; step++, s = (s + 1) & mask) {
				uint32_t cur = __hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if (cur == ROWS_EMPTY) {
					cur = atomicCAS(&slots[s], ROWS_EMPTY, (uint32_t)i);
					if (cur == ROWS_EMPTY) {
						placed = 1;
						break;
					}
				}
				/* (cur < build.n: a slot holds nothing but ROWS_EMPTY or a row number written here; the test keeps a wrong table from
				 * becoming a wild read) */
				if (cur < build.n && rows_equal(build, cur, cell, nullmask)) {
					placed = 0;
					break;
				}
			}
		}
		if (placed < 0)
			state[ROWS_ST_NO_SLOT] = 1;
		const unsigned long long fresh = __ballot(placed > 0);
		if (fresh && mdb_lane() == 0)
			atomicAdd(&state[ROWS_ST_MEMBERS], (unsigned long long)__popcll(fresh));
	}
}

/* one workgroup per ROWS_THREADS probe rows: wave w of workgroup b owns word b * ROWS_WAVES + w of the bitmap */
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_probe(rows_side probe, rows_side build, const uint32_t *__restrict__ slots, unsigned log2, int anti,
							     unsigned long long *__restrict__ bits, uint32_t *__restrict__ block_counts)
{
	__shared__ uint32_t s_cnt[ROWS_WAVES];
	const unsigned long long nslots = 1ull << log2, mask = nslots - 1;
	const unsigned long long i = (unsigned long long)blockIdx.x * ROWS_THREADS + threadIdx.x;
	bool hit = false;
	if (i < probe.n) {
		unsigned long long cell[MDB_ROWS_MAX_COLS];
		uint32_t nullmask;
		unsigned long long s = rows_hash(probe, i, cell, &nullmask) >> (64 - log2);
		bool found = false;
		for (unsigned long long step = 0; step < nslots; step++, s = (s + 1) & mask) {
			const uint32_t cur = slots[s];
			if (cur == ROWS_EMPTY)
				break;
			if (cur < build.n && rows_equal(build, cur, cell, nullmask)) {
				found = true;
				break;
			}
		}
		hit = found != (anti != 0);
	}
	const unsigned long long m = __ballot(hit);
	const uint32_t wave = threadIdx.x / MDB_WAVE;
	if (mdb_lane() == 0) {
		bits[(unsigned long long)blockIdx.x * ROWS_WAVES + wave] = m;
		s_cnt[wave] = (uint32_t)__popcll(m);
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t t = 0;
		for (int w = 0; w < ROWS_WAVES; w++)
			t += s_cnt[w];
		block_counts[blockIdx.x] = t;
	}
}

/* block_off: the exclusive prefix sums of k_rows_probe's block_counts */
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_compact(const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ block_off,
							       uint32_t *__restrict__ out_sel)
{
	const uint32_t wave = threadIdx.x / MDB_WAVE;
	const unsigned long long word0 = (unsigned long long)blockIdx.x * ROWS_WAVES;
	uint32_t before = block_off[blockIdx.x];
	for (uint32_t w = 0; w < wave; w++)
		before += (uint32_t)__popcll(bits[word0 + w]);
	const unsigned long long m = bits[word0 + wave];
	if ((m >> mdb_lane()) & 1ull)
		out_sel[before + (uint32_t)__popcll(m & mdb_lanemask_lt())] = (uint32_t)((word0 + wave) * MDB_WAVE + mdb_lane());
}

static unsigned rows_grid(const mdb_dev_ctx *ctx, unsigned long long items)
{
	const unsigned long long want = (items + ROWS_THREADS - 1) / ROWS_THREADS, most = (unsigned long long)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8u;
	return (unsigned)(want < 1 ? 1 : want < most ? want : most);
}

struct rows_scratch {
	void *d_slots, *d_state, *d_bits, *d_counts, *d_scan;
};

static int rows_run(mdb_dev_ctx *ctx, const rows_side &probe, const rows_side &build, int anti, uint32_t *out_sel, uint64_t *out_count,
		    struct mdb_dev_rows_info *info, rows_scratch *sc)
{
	unsigned log2 = 4;
	while ((1ull << log2) < 2 * build.n)
		log2++;
	const unsigned long long nslots = 1ull << log2;
	unsigned long long st[ROWS_ST_WORDS] = { 0 };
	int rc;

	if ((rc = mdb_dev_alloc(ctx, (size_t)nslots * 4, &sc->d_slots)) || (rc = mdb_dev_alloc(ctx, sizeof(st), &sc->d_state)))
		return rc;
	if ((rc = mdb_dev_memset(ctx, sc->d_slots, 0xFF, (size_t)nslots * 4)) || (rc = mdb_dev_memset(ctx, sc->d_state, 0, sizeof(st))))
		return rc;
	MDB_LAUNCH(ctx, "rows_insert", k_rows_insert, rows_grid(ctx, build.n), ROWS_THREADS, build, (uint32_t *)sc->d_slots, log2,
		   (unsigned long long *)sc->d_state);
	if ((rc = mdb_dev_d2h(ctx, st, sc->d_state, sizeof(st))))
		return rc;
	if (st[ROWS_ST_NO_SLOT])
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "rows_semi: a table of 2^%u slots had no place for one of %llu build rows", log2, build.n);
	info->members = st[ROWS_ST_MEMBERS];
	info->log2_slots = log2;
	if (!probe.n)
		return MIDORIDB_OK;

	const unsigned long long nblocks = (probe.n + ROWS_THREADS - 1) / ROWS_THREADS;
	if ((rc = mdb_dev_alloc(ctx, (size_t)nblocks * ROWS_WAVES * 8, &sc->d_bits)) || (rc = mdb_dev_alloc(ctx, (size_t)(nblocks + 1) * 4, &sc->d_counts)) ||
	    (rc = mdb_dev_alloc(ctx, mdb_scan_scratch_words(nblocks + 1) * 4, &sc->d_scan)))
		return rc;
	uint32_t *counts = (uint32_t *)sc->d_counts;
	if ((rc = mdb_dev_memset(ctx, counts + nblocks, 0, 4)))
		return rc;
	MDB_LAUNCH(ctx, "rows_probe", k_rows_probe, (unsigned)nblocks, ROWS_THREADS, probe, build, (const uint32_t *)sc->d_slots, log2, anti,
		   (unsigned long long *)sc->d_bits, counts);
	if ((rc = mdb_scan_u32_inplace(ctx, counts, nblocks + 1, (uint32_t *)sc->d_scan)))
		return rc;
	MDB_LAUNCH(ctx, "rows_compact", k_rows_compact, (unsigned)nblocks, ROWS_THREADS, (const unsigned long long *)sc->d_bits, (const uint32_t *)counts, out_sel);
	uint32_t total = 0;
	if ((rc = mdb_dev_d2h(ctx, &total, counts + nblocks, 4)))
		return rc;
	*out_count = total;
	return MIDORIDB_OK;
}

static int rows_side_from(mdb_dev_ctx *ctx, const struct mdb_sort_key *k, int ncols, uint64_t n, const char *which, rows_side *s)
{
	memset(s, 0, sizeof(*s));
	s->n = n;
	s->ncols = ncols;
	for (int c = 0; c < ncols; c++) {
		if (k[c].type != MDB_T_INT64 && k[c].type != MDB_T_DOUBLE)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "rows_semi: unknown value type %d of %s column %d", (int)k[c].type, which, c);
		if (n && !k[c].values)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "rows_semi: %s column %d has no values", which, c);
		s->col[c] = mdb_stream_col_of_key(&k[c]);
	}
	return MIDORIDB_OK;
}

extern "C" int mdb_dev_rows_semi(mdb_dev_ctx *ctx, const struct mdb_sort_key *probe, uint64_t n_probe, const struct mdb_sort_key *build, uint64_t n_build,
				 int ncols, int anti, uint32_t *out_sel, uint64_t *out_count, struct mdb_dev_rows_info *info)
{
	struct mdb_dev_rows_info local;
	if (!ctx)
		return -MIDORIDB_ERROR;
	if (!info)
		info = &local;
	memset(info, 0, sizeof(*info));
	info->form = 1;
	if (!out_count || (n_probe && !out_sel))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "rows_semi: no place for the selection");
	*out_count = 0;
	if (ncols < 1 || ncols > MDB_ROWS_MAX_COLS)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "rows_semi: %d columns, a row has 1 to %d", ncols, MDB_ROWS_MAX_COLS);
	if (!probe || !build)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "rows_semi: no columns");
	if (n_build > MDB_ROWS_MAX_BUILD)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "rows_semi: %llu build rows, the table takes at most %llu", (unsigned long long)n_build,
				   (unsigned long long)MDB_ROWS_MAX_BUILD);
	if (n_probe >= MDB_NO_ROW)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "rows_semi: %llu probe rows, a selection addresses at most 2^32 - 2", (unsigned long long)n_probe);
	for (int c = 0; c < ncols; c++)
		if (probe[c].type != build[c].type)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "rows_semi: column %d is of type %d on the probe side and of type %d on the build side", c,
					   (int)probe[c].type, (int)build[c].type);
	rows_side ps, bs;
	int rc;
	if ((rc = rows_side_from(ctx, probe, ncols, n_probe, "probe", &ps)) || (rc = rows_side_from(ctx, build, ncols, n_build, "build", &bs)))
		return rc;
	if (!n_build) {	/* nothing is a member: the empty selection, or every position */
		if (anti && n_probe && (rc = mdb_dev_iota32(ctx, out_sel, n_probe)))
			return rc;
		*out_count = anti ? n_probe : 0;
		return mdb_dev_sync(ctx);
	}
	rows_scratch sc = { NULL, NULL, NULL, NULL, NULL };
	rc = rows_run(ctx, ps, bs, anti, out_sel, out_count, info, &sc);
	if (rc)		/* whatever is still queued has to be over before its buffers go back to the allocator */
		(void)hipStreamSynchronize(ctx->stream);
	void *const bufs[] = { sc.d_slots, sc.d_state, sc.d_bits, sc.d_counts, sc.d_scan };
	for (void *b : bufs)
		if (b)
			mdb_dev_free(ctx, b);
	if (rc)
		*out_count = 0;
	return rc;
}

/* ------------------------------------------------------------------ mdb_dev_concat64 */

struct concat_parts {
	const unsigned long long *values[MDB_CONCAT_MAX_PARTS];
	const unsigned long long *nullbits[MDB_CONCAT_MAX_PARTS];
	unsigned long long end[MDB_CONCAT_MAX_PARTS];	/* the output position behind part k's last cell */
	int nparts;
};

/* thread i moves cell i; a wave's 64 cells are one word of the NULL bitmap: its ballot.  The bound is a multiple of the wave, so the last
 * word is written whole, with zero bits behind the last row */
__global__ __launch_bounds__(ROWS_THREADS) void k_concat64(concat_parts p, unsigned long long total, unsigned long long *__restrict__ dst,
							   unsigned long long *__restrict__ dst_nullbits)
{
	const unsigned long long n_up = (total + MDB_WAVE - 1) / MDB_WAVE * MDB_WAVE;
	/* (whole waves stay in the loop together: the stride is a multiple of the wave and so is the bound) */
	for (unsigned long long i = (unsigned long long)blockIdx.x * ROWS_THREADS + threadIdx.x; i < n_up; i += (unsigned long long)gridDim.x * ROWS_THREADS) {
		bool isnull = false;
		if (i < total) {
			int k = 0;
			while (k < p.nparts - 1 && i >= p.end[k])
				k++;
			const unsigned long long at = i - (k ? p.end[k - 1] : 0ull);
			isnull = p.nullbits[k] && mdb_bit_is_set((const uint64_t *)p.nullbits[k], at);
			dst[i] = p.values[k][at];
		}
		const unsigned long long m = __ballot(isnull);
		if (dst_nullbits && mdb_lane() == 0)
			dst_nullbits[i / MDB_WAVE] = m;
	}
}

extern "C" int mdb_dev_concat64(mdb_dev_ctx *ctx, const struct mdb_concat_part *parts, int nparts, void *dst, uint64_t *dst_nullbits)
{
	concat_parts p;
	unsigned long long total = 0;
	if (!ctx)
		return -MIDORIDB_ERROR;
	if (nparts < 0 || nparts > MDB_CONCAT_MAX_PARTS || (nparts && !parts))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "concat64: %d parts, a call takes at most %d", nparts, MDB_CONCAT_MAX_PARTS);
	memset(&p, 0, sizeof(p));
	p.nparts = nparts;
	for (int k = 0; k < nparts; k++) {
		if (parts[k].n && !parts[k].values)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "concat64: part %d has %llu rows and no values", k, (unsigned long long)parts[k].n);
		if (parts[k].nullbits && !dst_nullbits)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "concat64: part %d has a NULL bitmap, the destination has none", k);
		p.values[k] = (const unsigned long long *)parts[k].values;
		p.nullbits[k] = (const unsigned long long *)parts[k].nullbits;
		total += parts[k].n;
		p.end[k] = total;
	}
	if (!total)
		return MIDORIDB_OK;
	if (!dst)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "concat64: no destination");
	MDB_LAUNCH(ctx, "concat64", k_concat64, rows_grid(ctx, total), ROWS_THREADS, p, total, (unsigned long long *)dst, (unsigned long long *)dst_nullbits);
	return MIDORIDB_OK;
}
