/*
 * mdb_dev_outer.hip - outer completion: the device pass of LEFT / RIGHT OUTER JOIN (mdb_dev_outer_complete, include/mdb_dev.h).
 *
 * The pair operators deliver the matched pairs (p, o) in ascending order of p, the position on the preserved side.  SQL wants
 * every preserved position that occurs in no pair once more, with "no row" (MDB_NO_ROW) as its partner, at its own place in
 * that order.  With H(j) = the number of j' <= j whose p differs from its predecessor's (run heads) and D(j) = j + 1 - H(j)
 * (the pairs up to j that REPEAT a position), everything is "own position + repeats before it":
 *
 *     pair j                                   goes to  p_j + D(j)
 *     unmatched position i behind pair j       goes to  i + D(j)        (j the last pair with p_j < i)
 *     unmatched position i before every pair   goes to  i
 *
 * so one prefix count over the pairs places them all - no bitmap of matched rows, no atomics, no search:
 *
 *   outer_heads   run heads per chunk of OUTER_CHUNK pairs (reads pairs_p once); their exclusive scan (mdb_scan_u32_inplace)
 *                 gives every chunk's H and, read back, U = n_p - heads: the outputs are sized exactly
 *   outer_place   reads both pair columns once, writes pair j to p_j + D(j) (monotone in j: streaming stores).  The last pair
 *                 of a run also writes the unmatched positions behind it up to the end of its 64-position word (at most 63),
 *                 and leaves per word w of the position space: low[w] = the lowest matched position of the word, and D at the
 *                 word's first and last pair (head_d / tail_d: 4 bytes each per 64 positions)
 *   outer_words   repeats inside a word = tail_d - head_d (0 for a word no pair touches); scanned, E[w] = D in front of word w
 *   outer_fill    the unmatched positions that no pair of their word precedes - (i & 63) < low[w] - go to i + E[w]: 64
 *                 consecutive stores per wave
 *
 * Memory: 12 J bytes read (pairs_p twice), 8 (J + U) written, n_p / 64 * 9 bytes of bookkeeping written and read twice.
 * Every store is bounds-checked against the output size and the word count: pairs that are not ascending or not below n_p set
 * a status word and the call fails, they cannot write outside the buffers.
 */
#include "mdb_dev_internal.h"
#include "mdb_dev.h"

#define OUTER_THREADS 256
#define OUTER_ITERS 8
#define OUTER_TILE (OUTER_THREADS * 4)			/* pairs per workgroup and iteration: four per thread, one 16-byte load per column */
#define OUTER_CHUNK ((uint64_t)OUTER_TILE * OUTER_ITERS)	/* pairs per workgroup */

/* v[0..4) = src[j4 ... j4 + 3], MDB_NO_ROW behind the end (it differs from every valid position) */
__device__ static inline void outer_load4(const uint32_t *__restrict__ src, uint64_t j4, uint64_t J, bool vec, uint32_t v[4])
{
	if (vec && j4 + 4 <= J) {
		const uint4 q = *reinterpret_cast<const uint4 *>(src + j4);
		v[0] = q.x;
		v[1] = q.y;
		v[2] = q.z;
		v[3] = q.w;
	} else {
#pragma unroll
		for (int e = 0; e < 4; e++)
			v[e] = j4 + e < J ? src[j4 + e] : MDB_NO_ROW;
	}
}

__global__ __launch_bounds__(OUTER_THREADS) void k_outer_heads(const uint32_t *__restrict__ pairs_p, uint64_t J, int vec,
								uint32_t *__restrict__ chunk_heads)
{
	__shared__ uint32_t tmp[32];
	const uint64_t base = (uint64_t)blockIdx.x * OUTER_CHUNK;
	uint32_t heads = 0;
#pragma unroll 2
	for (int it = 0; it < OUTER_ITERS; it++) {
		const uint64_t j4 = base + (uint64_t)it * OUTER_TILE + 4u * threadIdx.x;
		if (j4 < J) {
			uint32_t p[4];
			outer_load4(pairs_p, j4, J, vec != 0, p);
			uint32_t prev = j4 ? pairs_p[j4 - 1] : MDB_NO_ROW;
#pragma unroll
			for (int e = 0; e < 4; e++) {
				heads += (j4 + e < J && p[e] != prev) ? 1u : 0u;
				prev = p[e];
			}
		}
	}
	uint32_t total;
	(void)mdb_block_excl_scan(heads, tmp, &total);
	if (threadIdx.x == 0)
		chunk_heads[blockIdx.x] = total;
}

__global__ __launch_bounds__(OUTER_THREADS) void k_outer_place(const uint32_t *__restrict__ pairs_p, const uint32_t *__restrict__ pairs_o,
								uint64_t J, uint64_t n_p, uint64_t total, int vec,
								const uint32_t *__restrict__ chunk_heads, uint32_t *__restrict__ out_p,
								uint32_t *__restrict__ out_o, uint32_t *__restrict__ head_d,
								uint32_t *__restrict__ tail_d, uint8_t *__restrict__ low, uint32_t *status)
{
	__shared__ uint32_t tmp[32];
	const uint64_t base = (uint64_t)blockIdx.x * OUTER_CHUNK;
	uint32_t carry = chunk_heads[blockIdx.x];	/* run heads in front of this chunk */
	bool bad = false;
	for (int it = 0; it < OUTER_ITERS; it++) {	/* (uniform: the scan holds barriers) */
		const uint64_t j4 = base + (uint64_t)it * OUTER_TILE + 4u * threadIdx.x;
		uint32_t p[4] = { MDB_NO_ROW, MDB_NO_ROW, MDB_NO_ROW, MDB_NO_ROW }, o[4] = { 0, 0, 0, 0 };
		uint32_t prev = MDB_NO_ROW, next = MDB_NO_ROW, mine = 0;
		bool head[4];
		if (j4 < J) {
			outer_load4(pairs_p, j4, J, vec != 0, p);
			outer_load4(pairs_o, j4, J, vec != 0, o);
			if (j4)
				prev = pairs_p[j4 - 1];
			if (j4 + 4 < J)
				next = pairs_p[j4 + 4];
		}
		{
			uint32_t q = prev;
#pragma unroll
			for (int e = 0; e < 4; e++) {
				head[e] = j4 + e < J && p[e] != q;
				mine += head[e] ? 1u : 0u;
				q = p[e];
			}
		}
		uint32_t tile_heads;
		uint32_t H = carry + mdb_block_excl_scan(mine, tmp, &tile_heads);
		carry += tile_heads;
#pragma unroll
		for (int e = 0; e < 4; e++) {
			const uint64_t j = j4 + e;
			if (j >= J)
				continue;
			H += head[e] ? 1u : 0u;
			const uint32_t before = e ? p[e - 1] : prev, after = e < 3 ? p[e + 1] : next;	/* (MDB_NO_ROW at either end of the pairs) */
			const uint64_t pe = p[e];
			if (pe >= n_p || (j && before > p[e])) {
				bad = true;
				continue;
			}
			const uint64_t d = j + 1 - H, pos = pe + d, w = pe >> 6;
			if (pos < total) {
				out_p[pos] = p[e];
				out_o[pos] = o[e];
			} else {
				bad = true;
			}
			if (j == 0 || (before >> 6) != w) {
				head_d[w] = (uint32_t)d;
				low[w] = (uint8_t)(pe & 63);
			}
			if (j + 1 == J || (after >> 6) != w)
				tail_d[w] = (uint32_t)d;
			if (j + 1 == J || after != p[e]) {
				/* the unmatched positions behind this run, inside its word */
				uint64_t end = (pe | 63) + 1;
				end = end < n_p ? end : n_p;
				if (j + 1 < J && after < end)
					end = after;
				for (uint64_t i = pe + 1; i < end; i++)
					if (i + d < total) {
						out_p[i + d] = (uint32_t)i;
						out_o[i + d] = MDB_NO_ROW;
					}
			}
		}
	}
	if (bad)
		mdb_raise(status, MDB_FLAG_SET);
}

__global__ __launch_bounds__(OUTER_THREADS) void k_outer_words(uint32_t *__restrict__ head_d, const uint32_t *__restrict__ tail_d, uint64_t words)
{
	const uint64_t w = (uint64_t)blockIdx.x * OUTER_THREADS + threadIdx.x;
	if (w < words)
		head_d[w] = tail_d[w] - head_d[w];
}

/* one thread per preserved position: a wave covers one word */
__global__ __launch_bounds__(OUTER_THREADS) void k_outer_fill(const uint32_t *__restrict__ word_d, const uint8_t *__restrict__ low, uint64_t n_p,
							       uint64_t total, uint32_t *__restrict__ out_p, uint32_t *__restrict__ out_o)
{
	const uint64_t i = (uint64_t)blockIdx.x * OUTER_THREADS + threadIdx.x;
	if (i >= n_p)
		return;
	const uint64_t w = i >> 6;
	if ((uint32_t)(i & 63) < (uint32_t)low[w]) {
		const uint64_t pos = i + word_d[w];
		if (pos < total) {
			out_p[pos] = (uint32_t)i;
			out_o[pos] = MDB_NO_ROW;
		}
	}
}

extern "C" int mdb_dev_outer_complete(mdb_dev_ctx *ctx, const uint32_t *pairs_p, const uint32_t *pairs_o, uint64_t J, uint64_t n_p,
				      uint32_t **out_p, uint32_t **out_o, uint64_t *out_count)
{
	if (!ctx || !out_p || !out_o || !out_count)
		return -MIDORIDB_ERROR;
	*out_p = *out_o = NULL;
	*out_count = 0;
	if (J && (!pairs_p || !pairs_o))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete: %llu pairs but no pair columns", (unsigned long long)J);
	if (n_p >= MDB_NO_ROW || J >= MDB_NO_ROW)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete: 2^32 - 1 rows or pairs and more cannot be addressed");
	if (n_p == 0)
		return J ? mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete: pairs over an empty preserved side") : MIDORIDB_OK;

	const uint64_t words = (n_p + 63) / 64, chunks = (J + OUTER_CHUNK - 1) / OUTER_CHUNK;
	const uint64_t scan_len = words > chunks + 1 ? words : chunks + 1;
	const int vec = (((uintptr_t)pairs_p | (uintptr_t)pairs_o) & 15) == 0;
	uint32_t *chunk_heads = NULL, *head_d = NULL, *tail_d = NULL, *scan_tmp = NULL, *op = NULL, *oo = NULL;
	uint8_t *low = NULL;
	uint32_t h[2] = { 0, 0 };	/* run heads, status */
	int rc;
	if ((rc = mdb_cached_alloc(ctx, (chunks + 2) * 4, (void **)&chunk_heads)) || (rc = mdb_cached_alloc(ctx, words * 4, (void **)&head_d)) ||
	    (rc = mdb_cached_alloc(ctx, words * 4, (void **)&tail_d)) || (rc = mdb_cached_alloc(ctx, words, (void **)&low)) ||
	    (rc = mdb_cached_alloc(ctx, mdb_scan_scratch_words(scan_len) * 4, (void **)&scan_tmp)))
		goto done;
	rc = [&]() -> int {
		/* chunk_heads[chunks] = 0 becomes the total under the exclusive scan; chunk_heads[chunks + 1] is the status word */
		MDB_HIP(ctx, hipMemsetAsync(chunk_heads + chunks, 0, 8, ctx->stream));
		if (J) {
			MDB_LAUNCH(ctx, "outer_heads", k_outer_heads, (uint32_t)chunks, OUTER_THREADS, pairs_p, J, vec, chunk_heads);
			int src = mdb_scan_u32_inplace(ctx, chunk_heads, chunks + 1, scan_tmp);
			if (src)
				return src;
			MDB_HIP(ctx, hipMemcpyAsync(&h[0], chunk_heads + chunks, 4, hipMemcpyDeviceToHost, ctx->stream));
			MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		}
		if (h[0] > n_p)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete: the pairs name more positions than the preserved side has");
		const uint64_t U = n_p - h[0], total = J + U;
		if (total >= MDB_NO_ROW)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete: %llu result rows cannot be addressed by 32-bit positions",
					   (unsigned long long)total);
		int arc = mdb_dev_alloc(ctx, total * 4, (void **)&op);
		if (!arc)
			arc = mdb_dev_alloc(ctx, total * 4, (void **)&oo);
		if (arc)
			return arc;
		MDB_HIP(ctx, hipMemsetAsync(head_d, 0, words * 4, ctx->stream));
		MDB_HIP(ctx, hipMemsetAsync(tail_d, 0, words * 4, ctx->stream));
		MDB_HIP(ctx, hipMemsetAsync(low, 64, words, ctx->stream));
		if (J) {
			MDB_LAUNCH(ctx, "outer_place", k_outer_place, (uint32_t)chunks, OUTER_THREADS, pairs_p, pairs_o, J, n_p, total, vec,
				   (const uint32_t *)chunk_heads, op, oo, head_d, tail_d, low, chunk_heads + chunks + 1);
			MDB_LAUNCH(ctx, "outer_words", k_outer_words, (uint32_t)((words + OUTER_THREADS - 1) / OUTER_THREADS), OUTER_THREADS, head_d,
				   (const uint32_t *)tail_d, words);
			int src = mdb_scan_u32_inplace(ctx, head_d, words, scan_tmp);
			if (src)
				return src;
		}
		if (U)
			MDB_LAUNCH(ctx, "outer_fill", k_outer_fill, (uint32_t)((n_p + OUTER_THREADS - 1) / OUTER_THREADS), OUTER_THREADS,
				   (const uint32_t *)head_d, (const uint8_t *)low, n_p, total, op, oo);
		MDB_HIP(ctx, hipMemcpyAsync(&h[1], chunk_heads + chunks + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
		MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (h[1])
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete: the preserved positions of the pairs are not ascending and below %llu",
					   (unsigned long long)n_p);
		*out_count = total;
		return MIDORIDB_OK;
	}();
done:
	if (rc) {
		if (op)
			mdb_dev_free(ctx, op);
		if (oo)
			mdb_dev_free(ctx, oo);
	} else {
		*out_p = op;
		*out_o = oo;
	}
	if (chunk_heads)
		(void)mdb_cached_free(ctx, chunk_heads);
	if (head_d)
		(void)mdb_cached_free(ctx, head_d);
	if (tail_d)
		(void)mdb_cached_free(ctx, tail_d);
	if (low)
		(void)mdb_cached_free(ctx, low);
	if (scan_tmp)
		(void)mdb_cached_free(ctx, scan_tmp);
	return rc;
}
