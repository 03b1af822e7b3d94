/*
 * mdb_dev_outer.hip - outer completion: the device pass of LEFT / RIGHT OUTER JOIN (mdb_dev_outer_complete, include/mdb_dev.h) and of
 * FULL OUTER JOIN (mdb_dev_outer_complete_full: the same, and behind it the OTHER side's rows that occur in no pair).
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
 *
 * FULL OUTER JOIN preserves the other side too: behind the J + U entries above come the positions i in [0, n_o) that pairs_o never
 * names, ascending, as (MDB_NO_ROW, i).  pairs_o is in no order, so these need a set of the named positions:
 *
 *   outer_mark       reads pairs_o once (16-byte loads) and stores 1 into flags[o], ONE BYTE per position of the other side
 *   outer_unmatched  a workgroup's span of OUTER_SPAN flag bytes, 16 per thread and load: the zero bytes in front of n_o as a bit mask,
 *                    counted (__popc), summed in the block; the span totals' exclusive scan (mdb_scan_u32_inplace) gives every span's
 *                    place in the tail and U_o, which travels to the host with the run heads: no synchronisation of its own
 *   outer_tail       the same masks again, scanned in the block (mdb_block_excl_scan): the unmatched positions of a tile of 4096, ascending,
 *                    are staged in LDS and leave as consecutive 4-byte stores per wave to out_o[J + U + r], MDB_NO_ROW to out_p[J + U + r].
 *                    Both outputs were allocated at J + U + U_o: no second buffer, no concatenating copy
 *
 * Bytes, not bits: the flag form was chosen by what the memory system does with it, neither form has been timed against the other.
 * A bit per position needs atomicOr, and pairs_o comes out of a hash join in no order: nothing combines in a wave, every lane's
 * atomic is a memory request of its own that is executed behind the L2 and leaves nothing in it - J scattered read-modify-writes.
 * A byte per position is a plain store of the same value whoever writes it: no atomic, no ordering between writers, repeats merge in
 * the L2 line they hit, the result does not depend on arrival order.  The price is the larger array: n_o bytes cleared, written
 * at random and read twice, against n_o / 8.
 * Memory of the tail: 4 J bytes read (pairs_o a second time) and J one-byte stores; per position of the other side 1 byte cleared and
 * 2 bytes read (outer_unmatched, outer_tail); 8 U_o bytes written; 4 bytes per OUTER_SPAN positions of bookkeeping.
 * A partner position at or above n_o sets a status word of its own in outer_mark, where it is compared and never used as an index, and the
 * call fails before the outputs are allocated; every store of outer_tail is checked against the output size.
 */
#include "mdb_dev_internal.h"
#include "mdb_dev.h"

#define OUTER_THREADS 256
#define OUTER_ITERS 8
#define OUTER_TILE (OUTER_THREADS * 4)			/* pairs per workgroup and iteration: four per thread, one 16-byte load per column */
#define OUTER_CHUNK ((uint64_t)OUTER_TILE * OUTER_ITERS)	/* pairs per workgroup */

#define OUTER_SPAN_ITERS 4
#define OUTER_SPAN_TILE (OUTER_THREADS * 16)		/* positions of the other side per workgroup and iteration: 16 flag bytes per thread, one 16-byte load */
#define OUTER_SPAN ((uint64_t)OUTER_SPAN_TILE * OUTER_SPAN_ITERS)	/* positions of the other side per workgroup */

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

/* FULL: flags[o] = 1 for every partner position the pairs name */
__global__ __launch_bounds__(OUTER_THREADS) void k_outer_mark(const uint32_t *__restrict__ pairs_o, uint64_t J, int vec, uint64_t n_o,
							       uint8_t *__restrict__ flags, uint32_t *status)
{
	const uint64_t base = (uint64_t)blockIdx.x * OUTER_CHUNK;
	bool bad = false;
#pragma unroll 2
	for (int it = 0; it < OUTER_ITERS; it++) {
		const uint64_t j4 = base + (uint64_t)it * OUTER_TILE + 4u * threadIdx.x;
		if (j4 < J) {
			uint32_t o[4];
			outer_load4(pairs_o, j4, J, vec != 0, o);
#pragma unroll
			for (int e = 0; e < 4; e++) {
				if (j4 + e >= J)
					continue;
				if ((uint64_t)o[e] < n_o)
					flags[o[e]] = 1;
				else
					bad = true;
			}
		}
	}
	if (bad)
		mdb_raise(status, MDB_FLAG_SET);
}

/* bit e set: position i0 + e (i0 a multiple of 16) is below n_o and its flag byte is 0.  The flag array is a multiple of 16 bytes long. */
__device__ static inline uint32_t outer_zero_mask16(const uint8_t *__restrict__ flags, uint64_t i0, uint64_t n_o)
{
	if (i0 >= n_o)
		return 0;
	const uint4 q = *reinterpret_cast<const uint4 *>(flags + i0);
	const uint32_t w[4] = { q.x, q.y, q.z, q.w };
	uint32_t ones = 0;
#pragma unroll
	for (int k = 0; k < 4; k++)	/* bytes of 0 or 1: bit 0 of every byte, gathered into four bits */
		ones |= ((w[k] & 1u) | ((w[k] >> 7) & 2u) | ((w[k] >> 14) & 4u) | ((w[k] >> 21) & 8u)) << (4 * k);
	const uint32_t valid = n_o - i0 >= 16 ? 0xFFFFu : (1u << (uint32_t)(n_o - i0)) - 1u;	/* (nothing behind n_o ever counts) */
	return ~ones & valid;
}

__global__ __launch_bounds__(OUTER_THREADS) void k_outer_unmatched(const uint8_t *__restrict__ flags, uint64_t n_o, uint32_t *__restrict__ span_zeros)
{
	__shared__ uint32_t tmp[32];
	const uint64_t base = (uint64_t)blockIdx.x * OUTER_SPAN;
	uint32_t zeros = 0;
#pragma unroll
	for (int it = 0; it < OUTER_SPAN_ITERS; it++)
		zeros += __popc(outer_zero_mask16(flags, base + (uint64_t)it * OUTER_SPAN_TILE + 16u * threadIdx.x, n_o));
	uint32_t total;
	(void)mdb_block_excl_scan(zeros, tmp, &total);
	if (threadIdx.x == 0)
		span_zeros[blockIdx.x] = total;
}

/* span_at[b] = unmatched positions in front of span b (the scanned span totals); off = J + U, where the tail begins */
__global__ __launch_bounds__(OUTER_THREADS) void k_outer_tail(const uint8_t *__restrict__ flags, uint64_t n_o, const uint32_t *__restrict__ span_at,
							       uint64_t off, uint64_t total, uint32_t *__restrict__ out_p, uint32_t *__restrict__ out_o)
{
	__shared__ uint32_t tmp[32];
	__shared__ uint32_t stage[OUTER_SPAN_TILE];
	const uint64_t base = (uint64_t)blockIdx.x * OUTER_SPAN;
	uint64_t at = off + span_at[blockIdx.x];
	for (int it = 0; it < OUTER_SPAN_ITERS; it++) {	/* (uniform: the scan holds barriers, which also part one tile's use of `stage` from the next) */
		const uint64_t i0 = base + (uint64_t)it * OUTER_SPAN_TILE + 16u * threadIdx.x;
		uint32_t m = outer_zero_mask16(flags, i0, n_o), tile_zeros;
		uint32_t r = mdb_block_excl_scan(__popc(m), tmp, &tile_zeros);
		while (m) {
			const uint32_t e = (uint32_t)__ffs((int)m) - 1u;
			m &= m - 1u;
			if (r < OUTER_SPAN_TILE)
				stage[r] = (uint32_t)(i0 + e);
			r++;
		}
		__syncthreads();
		for (uint32_t k = threadIdx.x; k < tile_zeros && k < OUTER_SPAN_TILE; k += OUTER_THREADS)
			if (at + k < total) {
				out_p[at + k] = MDB_NO_ROW;
				out_o[at + k] = stage[k];
			}
		at += tile_zeros;
	}
}

/* both entry points behind their argument checks.  full: the other side has n_o positions and its unmatched ones follow (FULL); the
 * synchronisations are the same two either way (one when J == 0: nothing has to come back before the outputs are sized) */
static int outer_complete_body(mdb_dev_ctx *ctx, const uint32_t *pairs_p, const uint32_t *pairs_o, uint64_t J, uint64_t n_p, bool full, uint64_t n_o,
			       uint32_t **out_p, uint32_t **out_o, uint64_t *out_count, uint64_t *out_unmatched_o)
{
	const uint64_t words = (n_p + 63) / 64, chunks = (J + OUTER_CHUNK - 1) / OUTER_CHUNK;
	const uint64_t spans = full ? (n_o + OUTER_SPAN - 1) / OUTER_SPAN : 0, flag_bytes = full ? (n_o + 15) / 16 * 16 : 0;
	uint64_t scan_len = words > chunks + 1 ? words : chunks + 1;
	scan_len = scan_len > spans + 1 ? scan_len : spans + 1;
	const int vec = (((uintptr_t)pairs_p | (uintptr_t)pairs_o) & 15) == 0;
	uint32_t *chunk_heads = NULL, *head_d = NULL, *tail_d = NULL, *scan_tmp = NULL, *op = NULL, *oo = NULL, *span_zeros = NULL;
	uint8_t *low = NULL, *flags = NULL;
	uint32_t h[2] = { 0, 0 };	/* run heads, status */
	uint32_t t[2] = { 0, 0 };	/* FULL: unmatched positions of the other side, status of pairs_o */
	int rc;
	if ((rc = mdb_cached_alloc(ctx, (chunks + 2) * 4, (void **)&chunk_heads)) || (rc = mdb_cached_alloc(ctx, words * 4, (void **)&head_d)) ||
	    (rc = mdb_cached_alloc(ctx, words * 4, (void **)&tail_d)) || (rc = mdb_cached_alloc(ctx, words, (void **)&low)) ||
	    (rc = mdb_cached_alloc(ctx, mdb_scan_scratch_words(scan_len) * 4, (void **)&scan_tmp)))
		goto done;
	if (full && ((rc = mdb_cached_alloc(ctx, flag_bytes, (void **)&flags)) || (rc = mdb_cached_alloc(ctx, (spans + 2) * 4, (void **)&span_zeros))))
		goto done;
	rc = [&]() -> int {
		/* chunk_heads[chunks] = 0 becomes the total under the exclusive scan; chunk_heads[chunks + 1] is the status word */
		MDB_HIP(ctx, hipMemsetAsync(chunk_heads + chunks, 0, 8, ctx->stream));
		if (full) {
			/* span_zeros[spans] and [spans + 1]: the same for the other side's unmatched positions and the status of pairs_o */
			MDB_HIP(ctx, hipMemsetAsync(span_zeros + spans, 0, 8, ctx->stream));
			if (flag_bytes)
				MDB_HIP(ctx, hipMemsetAsync(flags, 0, flag_bytes, ctx->stream));
		}
		if (J) {
			MDB_LAUNCH(ctx, "outer_heads", k_outer_heads, (uint32_t)chunks, OUTER_THREADS, pairs_p, J, vec, chunk_heads);
			int src = mdb_scan_u32_inplace(ctx, chunk_heads, chunks + 1, scan_tmp);
			if (src)
				return src;
			if (full)
				MDB_LAUNCH(ctx, "outer_mark", k_outer_mark, (uint32_t)chunks, OUTER_THREADS, pairs_o, J, ((uintptr_t)pairs_o & 15) == 0 ? 1 : 0, n_o,
					   flags, span_zeros + spans + 1);
		}
		if (spans) {
			MDB_LAUNCH(ctx, "outer_unmatched", k_outer_unmatched, (uint32_t)spans, OUTER_THREADS, (const uint8_t *)flags, n_o, span_zeros);
			int src = mdb_scan_u32_inplace(ctx, span_zeros, spans + 1, scan_tmp);
			if (src)
				return src;
		}
		t[0] = (uint32_t)n_o;	/* (without pairs every position of the other side is unmatched: nothing to wait for) */
		if (J) {
			MDB_HIP(ctx, hipMemcpyAsync(&h[0], chunk_heads + chunks, 4, hipMemcpyDeviceToHost, ctx->stream));
			if (full)
				MDB_HIP(ctx, hipMemcpyAsync(&t[0], span_zeros + spans, 8, hipMemcpyDeviceToHost, ctx->stream));
			MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		}
		if (t[1])
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete_full: the pairs name positions of the other side that are not below %llu",
					   (unsigned long long)n_o);
		if (h[0] > n_p)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete: the pairs name more positions than the preserved side has");
		const uint64_t U = n_p - h[0], U_o = full ? t[0] : 0, total = J + U + U_o;
		if (total >= MDB_NO_ROW)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete: %llu result rows cannot be addressed by 32-bit positions",
					   (unsigned long long)total);
		if (!total)	/* (FULL over two empty sides) */
			return MIDORIDB_OK;
		int arc = mdb_dev_alloc(ctx, total * 4, (void **)&op);
		if (!arc)
			arc = mdb_dev_alloc(ctx, total * 4, (void **)&oo);
		if (arc)
			return arc;
		if (words) {
			MDB_HIP(ctx, hipMemsetAsync(head_d, 0, words * 4, ctx->stream));
			MDB_HIP(ctx, hipMemsetAsync(tail_d, 0, words * 4, ctx->stream));
			MDB_HIP(ctx, hipMemsetAsync(low, 64, words, ctx->stream));
		}
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
		if (U_o)
			MDB_LAUNCH(ctx, "outer_tail", k_outer_tail, (uint32_t)spans, OUTER_THREADS, (const uint8_t *)flags, n_o, (const uint32_t *)span_zeros,
				   J + U, total, op, oo);
		MDB_HIP(ctx, hipMemcpyAsync(&h[1], chunk_heads + chunks + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
		MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (h[1])
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete: the preserved positions of the pairs are not ascending and below %llu",
					   (unsigned long long)n_p);
		*out_count = total;
		if (out_unmatched_o)
			*out_unmatched_o = U_o;
		ctx->plan.outer_form = full ? 2 : 1;
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
	if (flags)
		(void)mdb_cached_free(ctx, flags);
	if (span_zeros)
		(void)mdb_cached_free(ctx, span_zeros);
	return rc;
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
	return outer_complete_body(ctx, pairs_p, pairs_o, J, n_p, false, 0, out_p, out_o, out_count, NULL);
}

extern "C" int mdb_dev_outer_complete_full(mdb_dev_ctx *ctx, const uint32_t *pairs_p, const uint32_t *pairs_o, uint64_t J, uint64_t n_p, uint64_t n_o,
					   uint32_t **out_p, uint32_t **out_o, uint64_t *out_count, uint64_t *out_unmatched_o)
{
	if (!ctx || !out_p || !out_o || !out_count || !out_unmatched_o)
		return -MIDORIDB_ERROR;
	*out_p = *out_o = NULL;
	*out_count = *out_unmatched_o = 0;
	if (J && (!pairs_p || !pairs_o))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete_full: %llu pairs but no pair columns", (unsigned long long)J);
	if (n_p >= MDB_NO_ROW || n_o >= MDB_NO_ROW || J >= MDB_NO_ROW)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete_full: 2^32 - 1 rows or pairs and more cannot be addressed");
	if (J && n_p == 0)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "outer_complete_full: pairs over an empty preserved side");
	return outer_complete_body(ctx, pairs_p, pairs_o, J, n_p, true, n_o, out_p, out_o, out_count, out_unmatched_o);
}

