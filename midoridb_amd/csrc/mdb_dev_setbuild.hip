/*
 * mdb_dev_setbuild.hip - a device set (MDB_P_IN_SET; image layout, hash and probe sequence: include/mdb_dev.h, "device sets") built ON the
 * device from a device column: the right side of  k IN (SELECT ...)  never visits the host.  mdb_dev_set_from_column() delivers the image
 * that the host builder (mdb_set.c) could have produced for the same members - the same EMPTY marker, the same slot count, every member
 * on its probe path; only the placement among colliding members is free - so no probe kernel knows which builder made its table.
 *
 * Passes (all through MDB_LAUNCH, each under a name of its own):
 *
 *   set_scan      every cell once: counts the valid, NULL and NaN cells and tests the canonical value of every valid cell against a batch
 *                 of 64 candidates of the marker sequence; the hits are ORed into one 64-bit mask (per workgroup in LDS, then one atomic
 *                 per workgroup).  The host takes the first candidate without a hit; when all 64 were hit the pass runs again with the
 *                 next 64 (n cells can hit n candidates at most: n / 64 + 1 rounds bound it, one round is the practical case)
 *   set_fill      a table of 2^log2 slots, all EMPTY, words 0 and 1 written: log2 = the sizing rule for the VALID cells, capped at
 *                 MDB_SET_MAX_LOG2
 *   set_insert    linear probing from mdb_set_slot_of() on.  The slot is READ first: a duplicate costs loads only, no atomic; where the
 *                 read shows the marker a 64-bit compare-and-swap (marker -> value) claims the slot.  A stale read of the marker is
 *                 harmless - a slot changes exactly once, from marker to a value, and the CAS result tells the truth.  A member is
 *                 counted where its CAS saw the marker (a ballot per wave, one atomic per wave that found new members); every wave
 *                 looks at that counter before each cell and stops once it exceeds the limit, so the load passes 1/2 by no more than
 *                 what is in flight.  Every probe loop ends after `slots` steps
 *   set_reinsert  when the sizing rule gives a smaller table for the MEMBERS than for the cells (duplicates, NaNs): the occupied slots
 *                 of the first table are inserted into one of that size - once: the members are distinct, the second size is final
 *
 * The state block (8 words of device memory) carries the counters; the host reads it after the scan and after each insertion.
 */
#include "mdb_dev_internal.h"
#include "mdb_dev_stream.h"

#define SB_THREADS 256
#define SB_ST_VALID 0
#define SB_ST_NULL 1
#define SB_ST_NAN 2
#define SB_ST_HITS 3		/* bit c: candidate c of the batch is the canonical value of a valid cell */
#define SB_ST_MEMBERS 4
#define SB_ST_NO_SLOT 5		/* a probe loop ran its `slots` steps without a place (a table that the limit let fill up) */
#define SB_ST_WORDS 8

struct sb_column {
	const unsigned long long *values;
	const unsigned long long *nullbits;
	const uint32_t *rid;
	unsigned long long n;
	int type;
};

struct sb_candidates {
	unsigned long long c[64];
};

/* the canonical bits of cell i; 0 = a valid member candidate, 1 = NULL (NULL bit or no row), 2 = NaN */
__device__ static inline int sb_cell(const sb_column &col, unsigned long long i, unsigned long long *bits)
{
	const mdb_stream_col c = { (const uint64_t *)col.values, (const uint64_t *)col.nullbits, col.rid, 0, col.type };
	uint64_t v = 0;
	if (!mdb_stream_cell(c, i, &v))
		return 1;
	if (!mdb_set_canonical(col.type, &v))
		return 2;
	*bits = v;
	return 0;
}

__global__ __launch_bounds__(SB_THREADS) void k_set_scan(sb_column col, sb_candidates cand, int count_cells, unsigned long long *__restrict__ state)
{
	__shared__ unsigned long long s_acc[4];
	if (threadIdx.x < 4)
		s_acc[threadIdx.x] = 0;
	__syncthreads();
	unsigned long long hits = 0;
	uint32_t n_valid = 0, n_null = 0, n_nan = 0;
	for (unsigned long long i = (unsigned long long)blockIdx.x * SB_THREADS + threadIdx.x; i < col.n; i += (unsigned long long)gridDim.x * SB_THREADS) {
		unsigned long long v = 0;
		const int k = sb_cell(col, i, &v);
		n_valid += k == 0;
		n_null += k == 1;
		n_nan += k == 2;
		if (k == 0) {
#pragma unroll
			for (int c = 0; c < 64; c++)
				hits |= (unsigned long long)(v == cand.c[c]) << c;
		}
	}
	if (hits)
		atomicOr(&s_acc[SB_ST_HITS], hits);
	if (count_cells) {
		if (n_valid)
			atomicAdd(&s_acc[SB_ST_VALID], (unsigned long long)n_valid);
		if (n_null)
			atomicAdd(&s_acc[SB_ST_NULL], (unsigned long long)n_null);
		if (n_nan)
			atomicAdd(&s_acc[SB_ST_NAN], (unsigned long long)n_nan);
	}
	__syncthreads();
	if (threadIdx.x < 4 && s_acc[threadIdx.x]) {
		if (threadIdx.x == SB_ST_HITS)
			atomicOr(&state[SB_ST_HITS], s_acc[SB_ST_HITS]);
		else
			atomicAdd(&state[threadIdx.x], s_acc[threadIdx.x]);
	}
}

__global__ __launch_bounds__(SB_THREADS) void k_set_fill(unsigned long long *__restrict__ words, unsigned long long nslots, unsigned long long marker)
{
	const unsigned long long total = nslots + 2;
	for (unsigned long long i = (unsigned long long)blockIdx.x * SB_THREADS + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * SB_THREADS)
		words[i] = i == 0 ? marker : i == 1 ? nslots : marker;
}

/* place v: 1 = this call claimed a slot (a new member), 0 = v was there already, -1 = no place within `slots` steps */
__device__ static inline int sb_place(unsigned long long *slots, unsigned log2, unsigned long long marker, unsigned long long v)
{
	const unsigned long long nslots = 1ull << log2, mask = nslots - 1;
	unsigned long long i = mdb_set_slot_of(v, log2);
	for (unsigned long long step = 0; step < nslots; step++, i = (i + 1) & mask) {
		unsigned long long cur = __hip_atomic_load(&slots[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == marker) {
			cur = atomicCAS(&slots[i], marker, v);
			if (cur == marker)
				return 1;
		}
		if (cur == v)
			return 0;
	}
	return -1;
}

__global__ __launch_bounds__(SB_THREADS) void k_set_insert(sb_column col, unsigned long long *__restrict__ words, unsigned log2, unsigned long long marker,
							  unsigned long long limit, unsigned long long *__restrict__ state)
{
	unsigned long long *slots = words + 2;
	/* (the bound is a multiple of the workgroup: all lanes of a wave make the same number of trips, the ballot sees whole waves) */
	const unsigned long long n_up = (col.n + SB_THREADS - 1) / SB_THREADS * SB_THREADS;
	for (unsigned long long i = (unsigned long long)blockIdx.x * SB_THREADS + threadIdx.x; i < n_up; i += (unsigned long long)gridDim.x * SB_THREADS) {
		if (__any(__hip_atomic_load(&state[SB_ST_MEMBERS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > limit))
			break;
		unsigned long long v = 0;
		int placed = 0;
		if (i < col.n && sb_cell(col, i, &v) == 0)
			placed = sb_place(slots, log2, marker, v);
		if (placed < 0)
			state[SB_ST_NO_SLOT] = 1;
		const unsigned long long fresh = __ballot(placed > 0);
		if (fresh && mdb_lane() == 0)
			atomicAdd(&state[SB_ST_MEMBERS], (unsigned long long)__popcll(fresh));
	}
}

__global__ __launch_bounds__(SB_THREADS) void k_set_reinsert(const unsigned long long *__restrict__ old_words, unsigned long long old_nslots,
							    unsigned long long *__restrict__ words, unsigned log2, unsigned long long marker,
							    unsigned long long *__restrict__ state)
{
	for (unsigned long long i = (unsigned long long)blockIdx.x * SB_THREADS + threadIdx.x; i < old_nslots; i += (unsigned long long)gridDim.x * SB_THREADS) {
		const unsigned long long v = old_words[2 + i];
		if (v != marker && sb_place(words + 2, log2, marker, v) < 0)
			state[SB_ST_NO_SLOT] = 1;
	}
}

static unsigned sb_grid(const mdb_dev_ctx *ctx, unsigned long long items)
{
	const unsigned long long want = (items + SB_THREADS - 1) / SB_THREADS, most = (unsigned long long)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8u;
	return (unsigned)(want < 1 ? 1 : want < most ? want : most);
}

static int sb_new_table(mdb_dev_ctx *ctx, unsigned log2, unsigned long long marker, void **d_words)
{
	const unsigned long long nslots = 1ull << log2;
	int rc = mdb_dev_alloc(ctx, (size_t)(2 + nslots) * 8, d_words);
	if (rc)
		return rc;
	MDB_LAUNCH(ctx, "set_fill", k_set_fill, sb_grid(ctx, nslots + 2), SB_THREADS, (unsigned long long *)*d_words, nslots, marker);
	return MIDORIDB_OK;
}

static int sb_build(mdb_dev_ctx *ctx, const sb_column &col, unsigned long long limit, unsigned long long *d_state, void **d_words, void **d_first,
		    struct mdb_dev_set_info *info, unsigned *log2_out)
{
	unsigned long long st[SB_ST_WORDS] = { 0 }, marker = MDB_SET_MARKER_FIRST;
	int rc = mdb_dev_memset(ctx, d_state, 0, sizeof(st));
	if (rc)
		return rc;
	if (col.n) {
		/* the marker: the first candidate that no valid cell holds */
		sb_candidates cand;
		unsigned long long next = MDB_SET_MARKER_FIRST;
		for (unsigned long long round = 0;; round++) {
			for (int c = 0; c < 64; c++, next = mdb_set_marker_next(next))
				cand.c[c] = next;
			MDB_LAUNCH(ctx, "set_scan", k_set_scan, sb_grid(ctx, col.n), SB_THREADS, col, cand, round == 0 ? 1 : 0, d_state);
			if ((rc = mdb_dev_d2h(ctx, st, d_state, sizeof(st))))
				return rc;
			if (st[SB_ST_HITS] != ~0ull) {
				marker = cand.c[__builtin_ctzll(~st[SB_ST_HITS])];
				break;
			}
			if (round > col.n / 64)
				return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "set_from_column: no EMPTY marker after %llu rounds over %llu cells", round + 1, col.n);
			if ((rc = mdb_dev_memset(ctx, d_state + SB_ST_HITS, 0, 8)))
				return rc;
		}
	}
	info->cells_null = st[SB_ST_NULL];
	info->cells_nan = st[SB_ST_NAN];
	const unsigned long long valid = st[SB_ST_VALID];
	unsigned log2 = mdb_set_slots_log2_for(valid);
	if ((rc = sb_new_table(ctx, log2, marker, d_words)))
		return rc;
	if (valid) {
		MDB_LAUNCH(ctx, "set_insert", k_set_insert, sb_grid(ctx, col.n), SB_THREADS, col, (unsigned long long *)*d_words, log2, marker, limit, d_state);
		if ((rc = mdb_dev_d2h(ctx, st, d_state, sizeof(st))))
			return rc;
	} else {
		MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	}
	const unsigned long long members = st[SB_ST_MEMBERS];
	if (members > limit) {	/* (the count at which the insertion stopped: the column may hold more) */
		info->members = members;
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "set_from_column: %llu distinct values, a set takes at most %llu", members, limit);
	}
	if (st[SB_ST_NO_SLOT])
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "set_from_column: a table of 2^%u slots had no place for one of %llu cells", log2, valid);
	info->members = members;
	const unsigned want = mdb_set_slots_log2_for(members);
	if (want < log2) {
		*d_first = *d_words;
		*d_words = NULL;
		if ((rc = sb_new_table(ctx, want, marker, d_words)))
			return rc;
		MDB_LAUNCH(ctx, "set_reinsert", k_set_reinsert, sb_grid(ctx, 1ull << log2), SB_THREADS, (const unsigned long long *)*d_first, 1ull << log2,
			   (unsigned long long *)*d_words, want, marker, d_state);
		if ((rc = mdb_dev_d2h(ctx, st, d_state, sizeof(st))))
			return rc;
		if (st[SB_ST_NO_SLOT])
			return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "set_from_column: the table of 2^%u slots had no place for one of %llu members", want, members);
		info->rebuilt = 1;
		log2 = want;
	}
	info->log2_slots = log2;
	*log2_out = log2;
	return MIDORIDB_OK;
}

extern "C" int mdb_dev_set_from_column(mdb_dev_ctx *ctx, const void *values, const uint64_t *nullbits, const uint32_t *rid, uint64_t n, int type,
				       uint64_t max_members, mdb_dev_set **set, struct mdb_dev_set_info *info)
{
	struct mdb_dev_set_info local;
	if (!ctx || !set || (n && !values))
		return ctx ? mdb_set_err(ctx, -MIDORIDB_ERROR, "set_from_column: no column or no place for the set") : -MIDORIDB_ERROR;
	*set = NULL;
	if (!info)
		info = &local;
	memset(info, 0, sizeof(*info));
	if (type != MDB_T_INT64 && type != MDB_T_DOUBLE)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "set_from_column: unknown value type %d", type);
	if (n >= MDB_NO_ROW)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "set_from_column: %llu cells, a row-id vector addresses fewer than 2^32 - 1", (unsigned long long)n);
	const unsigned long long limit = max_members && max_members < MDB_SET_MAX_VALUES ? max_members : MDB_SET_MAX_VALUES;
	mdb_dev_set *s = (mdb_dev_set *)calloc(1, sizeof(*s));
	if (!s)
		return mdb_set_err(ctx, -MIDORIDB_NOMEM, "set_from_column: out of memory");
	void *d_state = NULL, *d_words = NULL, *d_first = NULL;
	unsigned log2 = 0;
	int rc = mdb_dev_alloc(ctx, SB_ST_WORDS * 8, &d_state);
	if (!rc) {
		const sb_column col = { (const unsigned long long *)values, (const unsigned long long *)nullbits, rid, n, type };
		rc = sb_build(ctx, col, limit, (unsigned long long *)d_state, &d_words, &d_first, info, &log2);
	}
	if (rc)		/* whatever is still queued has to be over before its buffers go back to the allocator */
		(void)hipStreamSynchronize(ctx->stream);
	if (d_first)
		mdb_dev_free(ctx, d_first);
	if (d_state)
		mdb_dev_free(ctx, d_state);
	if (rc) {
		if (d_words)
			mdb_dev_free(ctx, d_words);
		free(s);
		return rc;
	}
	s->d_words = d_words;
	s->slots = 1ull << log2;
	s->members = info->members;
	s->log2_slots = log2;
	s->type = type;
	*set = s;
	return MIDORIDB_OK;
}
