/*
 * mdb_dev_window.hip - window functions (mdb_dev_window): ROW_NUMBER / RANK / DENSE_RANK / COUNT(*) / SUM / MIN / MAX / AVG / LAG / LEAD /
 * FIRST_VALUE / LAST_VALUE / NTILE ... OVER (PARTITION BY ... ORDER BY ...).  An extension: the reference's grammar has no OVER clause (src/parser/midorisql.y) and its executor no
 * per-row function of a row's neighbours.
 *
 * The stream is sorted once, stably, by the partition keys and then the order keys (mdb_dev_sort_perm): a partition is a run of equal
 * partition keys, a peer group a run of equal order keys inside it.  Everything else is a segmented scan over the sorted positions:
 *
 *   k_win_heads      one thread per sorted position asks mdb_stream_head_of (mdb_dev_stream.h, with the cells and the order images); one
 *                    ballot per wave and bitmap: ph = partition heads, gh = peer heads (gh contains ph)
 *   k_win_scan<0>    chunks of WIN_CHUNK positions, one workgroup each, a strip of WIN_STRIP positions per thread: every thread folds its
 *                    strip, the strips are scanned by shuffles inside a wave and across the four waves through LDS, the workgroup's
 *                    total is the chunk's summary - the last partition head (b1), the last peer head (g1), the peer heads since the last
 *                    partition head (d), the chunk's first peer head (fh1) and first partition head (fp1), and per aggregate the open
 *                    (accumulator, cell count) pair
 *   k_win_carry      ONE workgroup scans the summaries: carry[c] = what is open in front of chunk c, nexth[c] = the first peer head behind
 *                    it, nextp[c] = the first partition head behind it
 *   k_win_scan<1>    the same chunks again, with their carry: ROW_NUMBER / RANK / DENSE_RANK are final here and written to out[stream
 *                    position]; every aggregate leaves its running pair T[q] = fold of the partition's cells up to q; COUNT(*), LAG,
 *                    FIRST_VALUE and NTILE leave b
 *   k_win_ends       e = the position behind a row's peer group (from gh, or nexth): SQL's default frame ends at e - 1, so the value of an
 *                    aggregate is T[e - 1] and COUNT(*) is e - b
 *   k_win_nav        LAG / LEAD / FIRST_VALUE / LAST_VALUE / NTILE: pe = the position behind a row's partition (from ph, or nextp) as e comes
 *                    from gh; the value is the argument column's cell at p - k, p + k, b or e - 1 - one gather through the permutation -
 *                    or the default outside [b, pe); NTILE is arithmetic on p, b and pe.  The cell's 8 bytes are copied, never interpreted
 *   k_win_pack       the NULL flags, written per stream position as bytes, become whole words of out_nullbits (one ballot per word)
 *
 * Carries between workgroups travel through these separate launches only.  Integer arithmetic and order images throughout (SUM / AVG over
 * DOUBLE cells are refused), plain stores: the same input gives the same bytes.
 */
#include "mdb_dev_internal.h"
#include "mdb_dev_stream.h"

#define WIN_THREADS 256u
#define WIN_STRIP 16u				/* sorted positions per thread: a quarter of a word of head bits */
#define WIN_CHUNK (WIN_THREADS * WIN_STRIP)	/* ... per workgroup: 4096, 64 words of head bits */
#define WIN_WORDS (WIN_CHUNK / 64u)
#define WIN_WAVES (WIN_THREADS / MDB_WAVE)
static_assert(WIN_STRIP == 16u && WIN_CHUNK % 64u == 0, "a thread's strip is 16 head bits of one word");
/* (the status word holds one flag, MDB_GROUPS_ST_PERM_RANGE of mdb_dev_stream.h) */

#define WIN_MAX_FNS MDB_WIN_MAX_FNS
struct win_fns {
	mdb_stream_col c[WIN_MAX_FNS];
	uint64_t *out[WIN_MAX_FNS];		/* n cells in stream order */
	uint8_t *nf[WIN_MAX_FNS];		/* aggregates, LAG ... LAST_VALUE: n NULL flags in stream order */
	unsigned long long *T[WIN_MAX_FNS];	/* aggregates: n running (accumulator, cells) pairs in sorted order */
	int nfns;
};

/* what is open at a sorted position, of the structure: positions are kept + 1, 0 = none in the range */
struct win_st {
	uint32_t b1, g1;	/* last partition head, last peer head */
	uint32_t d;		/* peer heads since the last partition head (all of the range when it has none) */
	uint32_t fh1;		/* first peer head of the range (summaries only) */
	uint32_t fp1;		/* first partition head of the range (summaries only) */
};

struct win_ag {
	uint64_t acc, cnt;
};

__host__ __device__ static inline bool win_is_agg(int op) { return op >= MDB_WIN_SUM && op <= MDB_WIN_AVG; }
__host__ __device__ static inline bool win_is_nav(int op) { return op >= MDB_WIN_LAG && op <= MDB_WIN_NTILE; }
/* ... that copies a cell of its argument column (NTILE reads none) */
__host__ __device__ static inline bool win_is_gather(int op) { return op >= MDB_WIN_LAG && op <= MDB_WIN_LAST_VALUE; }
__host__ __device__ static inline bool win_is_minmax(int op) { return op == MDB_WIN_MIN || op == MDB_WIN_MAX; }

/* left then right: right is folded INTO left, in that order; an empty side changes nothing */
__device__ static inline win_ag win_fold(int op, win_ag l, win_ag r)
{
	if (!r.cnt)
		return l;
	if (!l.cnt)
		return r;
	if (op == MDB_WIN_MIN)
		l.acc = r.acc < l.acc ? r.acc : l.acc;
	else if (op == MDB_WIN_MAX)
		l.acc = r.acc > l.acc ? r.acc : l.acc;
	else
		l.acc += r.acc;		/* (integer cells: two's complement, wrapping) */
	l.cnt += r.cnt;
	return l;
}

/* the structure of a range on the left joined with the range behind it (rhasp: the right range holds a partition head) */
__device__ static inline win_st win_join(win_st l, win_st r)
{
	win_st o;
	o.b1 = r.b1 ? r.b1 : l.b1;
	o.g1 = r.g1 ? r.g1 : l.g1;
	o.d = r.b1 ? r.d : l.d + r.d;
	o.fh1 = l.fh1 ? l.fh1 : r.fh1;
	o.fp1 = l.fp1 ? l.fp1 : r.fp1;
	return o;
}

/* exclusive scans over the WIN_THREADS threads of a workgroup, left operand first: inside a wave by shuffles (six steps, no barrier), the
 * waves' totals joined through WIN_WAVES entries of LDS (two barriers per scan).  Returned: what the threads before this one hold, joined in
 * thread order; *total = all threads' */
__device__ static inline win_st win_shfl_up_st(win_st v, uint32_t d)
{
	win_st o;
	o.b1 = (uint32_t)__shfl_up((int)v.b1, d, MDB_WAVE);
	o.g1 = (uint32_t)__shfl_up((int)v.g1, d, MDB_WAVE);
	o.d = (uint32_t)__shfl_up((int)v.d, d, MDB_WAVE);
	o.fh1 = (uint32_t)__shfl_up((int)v.fh1, d, MDB_WAVE);
	o.fp1 = (uint32_t)__shfl_up((int)v.fp1, d, MDB_WAVE);
	return o;
}

__device__ static inline win_st win_block_scan_st(win_st v, win_st *lds /* [WIN_WAVES] */, win_st *total)
{
	const uint32_t lane = mdb_lane(), wave = threadIdx.x >> 6;
	const win_st none = {0, 0, 0, 0, 0};
	win_st incl = v;
	for (uint32_t d = 1; d < MDB_WAVE; d <<= 1) {
		const win_st o = win_shfl_up_st(incl, d);
		if (lane >= d)
			incl = win_join(o, incl);
	}
	win_st excl = win_shfl_up_st(incl, 1u);
	if (lane == 0)
		excl = none;
	if (lane == MDB_WAVE - 1u)
		lds[wave] = incl;
	__syncthreads();
	win_st pre = none, all = none;
	for (uint32_t w = 0; w < WIN_WAVES; w++) {
		if (w == wave)
			pre = all;
		all = win_join(all, lds[w]);
	}
	*total = all;
	__syncthreads();	/* (the entries are free for the next scan) */
	return win_join(pre, excl);
}

/* ... of an aggregate's pairs; hasp: this thread's range holds a partition head (what lies before it is not folded in) */
struct win_agf {
	win_ag a;
	uint32_t hasp;
};

__device__ static inline win_agf win_shfl_up_ag(win_agf v, uint32_t d)
{
	win_agf o;
	o.a.acc = (uint64_t)__shfl_up((unsigned long long)v.a.acc, d, MDB_WAVE);
	o.a.cnt = (uint64_t)__shfl_up((unsigned long long)v.a.cnt, d, MDB_WAVE);
	o.hasp = (uint32_t)__shfl_up((int)v.hasp, d, MDB_WAVE);
	return o;
}

/* the range on the left, then the range behind it: behind a partition head nothing of the left range is open any more */
__device__ static inline win_agf win_join_ag(int op, win_agf l, win_agf r)
{
	if (!r.hasp)
		r.a = win_fold(op, l.a, r.a);
	r.hasp |= l.hasp;
	return r;
}

__device__ static inline win_ag win_block_scan_ag(int op, win_ag v, bool hasp, win_agf *lds /* [WIN_WAVES] */, win_agf *total)
{
	const uint32_t lane = mdb_lane(), wave = threadIdx.x >> 6;
	win_agf none;
	none.a.acc = none.a.cnt = 0;
	none.hasp = 0;
	win_agf incl;
	incl.a = v;
	incl.hasp = hasp ? 1u : 0u;
	for (uint32_t d = 1; d < MDB_WAVE; d <<= 1) {
		const win_agf o = win_shfl_up_ag(incl, d);
		if (lane >= d)
			incl = win_join_ag(op, o, incl);
	}
	win_agf excl = win_shfl_up_ag(incl, 1u);
	if (lane == 0)
		excl = none;
	if (lane == MDB_WAVE - 1u)
		lds[wave] = incl;
	__syncthreads();
	win_agf pre = none, all = none;
	for (uint32_t w = 0; w < WIN_WAVES; w++) {
		if (w == wave)
			pre = all;
		all = win_join_ag(op, all, lds[w]);
	}
	*total = all;
	__syncthreads();	/* (the entries are free for the next scan) */
	return win_join_ag(op, pre, excl).a;
}

/* ------------------------------------------------------------------ the two head bitmaps
 * ph bit p = "sorted position p begins a partition" (position 0, or a partition key differs from the row before: NULL equals NULL, values
 * by their bits), gh bit p = "... a peer group" (a partition head, or an order key differs).  Both bitmaps were cleared by the caller;
 * every wave that holds a position below n writes its word of each. */
__global__ __launch_bounds__(WIN_THREADS) void k_win_heads(mdb_stream_keys K, const uint32_t *__restrict__ perm, uint64_t n, unsigned long long *__restrict__ ph,
							    unsigned long long *__restrict__ gh, uint32_t *status)
{
	const uint64_t p = (uint64_t)blockIdx.x * WIN_THREADS + threadIdx.x;
	const mdb_stream_head h = mdb_stream_head_of(K, perm, n, p, status);
	const unsigned long long bp = __ballot(h.part), bg = __ballot(h.peer);
	if (mdb_lane() == 0 && (p & ~63ull) < n) {
		ph[p >> 6] = bp;
		gh[p >> 6] = bg;
	}
}

/* ------------------------------------------------------------------ the segmented scan over one chunk */
struct win_scan_args {
	win_fns F;
	const uint32_t *perm;
	uint64_t n, nchunks;
	const unsigned long long *ph, *gh;
	win_st *st_sum;			/* [nchunks] */
	win_ag *ag_sum;			/* [nfns][nchunks]: the aggregates' slots only */
	uint32_t *hasp_sum;		/* [nchunks]: the chunk holds a partition head */
	const win_st *st_carry;		/* APPLY: what is open in front of the chunk */
	const win_ag *ag_carry;
	uint32_t *B32;			/* APPLY, with COUNT(*), LAG, FIRST_VALUE or NTILE: b of every sorted position */
	uint32_t *status;
};

template <bool APPLY> __global__ __launch_bounds__(WIN_THREADS) void k_win_scan(win_scan_args A)
{
	__shared__ win_st s_st[WIN_WAVES];
	__shared__ win_agf s_ag[WIN_WAVES];
	const uint64_t c = blockIdx.x, n = A.n;
	const uint32_t t = threadIdx.x;
	const uint64_t p0 = c * WIN_CHUNK + (uint64_t)t * WIN_STRIP;
	const uint32_t shift = (uint32_t)(p0 & 63u);
	const uint32_t pb = p0 < n ? (uint32_t)(A.ph[p0 >> 6] >> shift) & 0xFFFFu : 0u;
	const uint32_t gb = p0 < n ? (uint32_t)(A.gh[p0 >> 6] >> shift) & 0xFFFFu : 0u;

	/* the strip's stream positions: needed where cells are read (aggregates) and where results are written (APPLY) */
	uint32_t sp[WIN_STRIP];
	bool need_sp = APPLY;
	for (int f = 0; f < A.F.nfns; f++)
		need_sp = need_sp || win_is_agg(A.F.c[f].op);
	if (need_sp) {
		bool bad = false;
		for (uint32_t q = 0; q < WIN_STRIP; q += 4u) {
			if (A.perm && p0 + q + 3u < n) {
				const uint4 v = *reinterpret_cast<const uint4 *>(A.perm + p0 + q);	/* (p0 + q is a multiple of 4; perm is 16-byte aligned) */
				sp[q] = v.x;
				sp[q + 1] = v.y;
				sp[q + 2] = v.z;
				sp[q + 3] = v.w;
			} else {
				for (uint32_t j = q; j < q + 4u; j++)
					sp[j] = A.perm ? (p0 + j < n ? A.perm[p0 + j] : 0u) : (uint32_t)(p0 + j < n ? p0 + j : 0u);
			}
		}
#pragma unroll
		for (uint32_t j = 0; j < WIN_STRIP; j++)
			if (sp[j] >= n) {	/* (never read a cell or write a result beyond the stream) */
				bad = bad || p0 + j < n;
				sp[j] = 0xFFFFFFFFu;
			}
		if (bad)
			mdb_raise(A.status, MDB_GROUPS_ST_PERM_RANGE);
	}

	/* ---- the structure: b, g and the peer heads since b */
	win_st mine = {0, 0, 0, 0, 0};
#pragma unroll
	for (uint32_t j = 0; j < WIN_STRIP; j++) {
		if (p0 + j >= n)
			continue;
		if ((pb >> j) & 1u) {
			mine.b1 = (uint32_t)(p0 + j) + 1u;
			mine.d = 0;
			if (!mine.fp1)
				mine.fp1 = (uint32_t)(p0 + j) + 1u;
		}
		if ((gb >> j) & 1u) {
			mine.g1 = (uint32_t)(p0 + j) + 1u;
			mine.d++;
			if (!mine.fh1)
				mine.fh1 = (uint32_t)(p0 + j) + 1u;
		}
	}
	win_st total;
	win_st before = win_block_scan_st(mine, s_st, &total);
	if (!APPLY) {
		if (t == 0) {
			A.st_sum[c] = total;
			A.hasp_sum[c] = total.b1 ? 1u : 0u;
		}
	} else {
		win_st cur = win_join(A.st_carry[c], before);
#pragma unroll
		for (uint32_t j = 0; j < WIN_STRIP; j++) {
			const uint64_t p = p0 + j;
			if (p >= n)
				continue;
			if ((pb >> j) & 1u) {
				cur.b1 = (uint32_t)p + 1u;
				cur.d = 0;
			}
			if ((gb >> j) & 1u) {
				cur.g1 = (uint32_t)p + 1u;
				cur.d++;
			}
			/* (position 0 is a head of both kinds: b1 and g1 are set from there on) */
			const uint32_t b = cur.b1 - 1u, g = cur.g1 - 1u;
			if (A.B32)
				A.B32[p] = b;
			if (sp[j] == 0xFFFFFFFFu)
				continue;
			for (int f = 0; f < A.F.nfns; f++) {
				const int op = A.F.c[f].op;
				if (op == MDB_WIN_ROW_NUMBER)
					A.F.out[f][sp[j]] = (uint64_t)((uint32_t)p - b) + 1u;
				else if (op == MDB_WIN_RANK)
					A.F.out[f][sp[j]] = (uint64_t)(g - b) + 1u;
				else if (op == MDB_WIN_DENSE_RANK)
					A.F.out[f][sp[j]] = (uint64_t)cur.d;
			}
		}
	}

	/* ---- the aggregates: the running pair of the partition's cells */
	int slot = 0;
	for (int f = 0; f < A.F.nfns; f++) {
		const mdb_stream_col &col = A.F.c[f];
		if (!win_is_agg(col.op))
			continue;
		const bool mm = win_is_minmax(col.op);
		win_ag acc;
		acc.acc = acc.cnt = 0;
#pragma unroll
		for (uint32_t j = 0; j < WIN_STRIP; j++) {
			if (p0 + j >= n)
				continue;
			if ((pb >> j) & 1u)
				acc.acc = acc.cnt = 0;
			uint64_t vb = 0;
			if (sp[j] != 0xFFFFFFFFu && mdb_stream_cell(col, sp[j], &vb)) {
				win_ag one;
				one.acc = mm ? mdb_order_image(vb, col.type) : vb;
				one.cnt = 1;
				acc = win_fold(col.op, acc, one);
			}
		}
		win_agf tot;
		win_ag pre = win_block_scan_ag(col.op, acc, pb != 0u, s_ag, &tot);
		if (!APPLY) {
			if (t == 0)
				A.ag_sum[(uint64_t)slot * A.nchunks + c] = tot.a;
		} else {
			/* what is open in front of the strip: the chunk's carry unless a partition began in the chunk before this strip */
			win_ag cur = before.b1 ? pre : win_fold(col.op, A.ag_carry[(uint64_t)slot * A.nchunks + c], pre);
			unsigned long long *T = A.F.T[f];
#pragma unroll
			for (uint32_t j = 0; j < WIN_STRIP; j++) {
				const uint64_t p = p0 + j;
				if (p >= n)
					continue;
				if ((pb >> j) & 1u)
					cur.acc = cur.cnt = 0;
				uint64_t vb = 0;
				if (sp[j] != 0xFFFFFFFFu && mdb_stream_cell(col, sp[j], &vb)) {
					win_ag one;
					one.acc = mm ? mdb_order_image(vb, col.type) : vb;
					one.cnt = 1;
					cur = win_fold(col.op, cur, one);
				}
				*reinterpret_cast<ulonglong2 *>(T + p * 2u) = make_ulonglong2(cur.acc, cur.cnt);
			}
		}
		slot++;
	}
}

/* ------------------------------------------------------------------ the chunk summaries, one workgroup: thread t takes a run of consecutive
 * chunks, folds it, the runs are scanned through LDS, and the thread walks its run again: carry[c] = everything in front of chunk c.
 * nexth[c] = the first peer head of a chunk behind c, n when there is none; nextp[c] = the first partition head there, likewise. */
struct win_carry_args {
	uint64_t n, nchunks;
	int nslots;
	int32_t op[WIN_MAX_FNS];	/* of the aggregates' slots */
	const win_st *st_sum;
	const win_ag *ag_sum;
	const uint32_t *hasp_sum;
	win_st *st_carry;
	win_ag *ag_carry;
	uint32_t *nexth, *nextp;
};

__global__ __launch_bounds__(WIN_THREADS) void k_win_carry(win_carry_args A)
{
	__shared__ win_st s_st[WIN_WAVES];
	__shared__ win_agf s_ag[WIN_WAVES];
	__shared__ uint32_t s_first[WIN_THREADS], s_firstp[WIN_THREADS];
	const uint32_t t = threadIdx.x;
	const uint64_t per = (A.nchunks + WIN_THREADS - 1u) / WIN_THREADS;
	const uint64_t c0 = (uint64_t)t * per < A.nchunks ? (uint64_t)t * per : A.nchunks;
	const uint64_t c1 = c0 + per < A.nchunks ? c0 + per : A.nchunks;

	win_st mine = {0, 0, 0, 0, 0};
	for (uint64_t c = c0; c < c1; c++)
		mine = win_join(mine, A.st_sum[c]);
	win_st total;
	win_st cur = win_block_scan_st(mine, s_st, &total);
	for (uint64_t c = c0; c < c1; c++) {
		A.st_carry[c] = cur;
		cur = win_join(cur, A.st_sum[c]);
	}
	/* the first peer head behind every chunk */
	s_first[t] = mine.fh1;
	s_firstp[t] = mine.fp1;
	__syncthreads();
	uint32_t nx = (uint32_t)A.n, np = (uint32_t)A.n;
	for (uint32_t u = t + 1u; u < WIN_THREADS; u++)
		if (s_first[u]) {
			nx = s_first[u] - 1u;
			break;
		}
	for (uint32_t u = t + 1u; u < WIN_THREADS; u++)
		if (s_firstp[u]) {
			np = s_firstp[u] - 1u;
			break;
		}
	for (uint64_t c = c1; c > c0; c--) {
		A.nexth[c - 1u] = nx;
		A.nextp[c - 1u] = np;
		if (A.st_sum[c - 1u].fh1)
			nx = A.st_sum[c - 1u].fh1 - 1u;
		if (A.st_sum[c - 1u].fp1)
			np = A.st_sum[c - 1u].fp1 - 1u;
	}
	__syncthreads();

	for (int s = 0; s < A.nslots; s++) {
		const int op = A.op[s];
		const win_ag *sum = A.ag_sum + (uint64_t)s * A.nchunks;
		win_ag *carry = A.ag_carry + (uint64_t)s * A.nchunks;
		win_ag acc;
		acc.acc = acc.cnt = 0;
		bool hasp = false;
		for (uint64_t c = c0; c < c1; c++) {
			if (A.hasp_sum[c]) {	/* (the chunk's summary is what is open at its END: the part from its last partition head on) */
				acc = sum[c];
				hasp = true;
			} else {
				acc = win_fold(op, acc, sum[c]);
			}
		}
		win_agf tot;
		win_ag open = win_block_scan_ag(op, acc, hasp, s_ag, &tot);
		for (uint64_t c = c0; c < c1; c++) {
			carry[c] = open;
			open = A.hasp_sum[c] ? sum[c] : win_fold(op, open, sum[c]);
		}
	}
}

/* ------------------------------------------------------------------ the functions whose value lies at the END of the row's peer group */
struct win_ends_args {
	win_fns F;
	const uint32_t *perm;
	uint64_t n;
	const unsigned long long *gh;
	const uint32_t *nexth;
	const uint32_t *B32;
};

__global__ __launch_bounds__(WIN_THREADS) void k_win_ends(win_ends_args A)
{
	__shared__ unsigned long long s_w[WIN_WORDS];
	__shared__ uint32_t s_nx[WIN_WORDS];	/* the first peer head in the chunk's words behind word w, or behind the chunk */
	const uint64_t c = blockIdx.x, n = A.n, base = c * WIN_CHUNK;
	const uint32_t t = threadIdx.x;
	if (t < WIN_WORDS)
		s_w[t] = base + (uint64_t)t * 64u < n ? A.gh[(base >> 6) + t] : 0ull;
	__syncthreads();
	if (t == 0) {
		uint32_t nx = A.nexth[c];
		for (uint32_t w = WIN_WORDS; w > 0; w--) {
			s_nx[w - 1u] = nx;
			if (s_w[w - 1u])
				nx = (uint32_t)(base + (uint64_t)(w - 1u) * 64u) + (uint32_t)__ffsll((long long)s_w[w - 1u]) - 1u;
		}
	}
	__syncthreads();
	for (uint32_t k = 0; k < WIN_STRIP; k++) {
		const uint64_t p = base + (uint64_t)k * WIN_THREADS + t;
		if (p >= n)
			break;
		const uint32_t w = (uint32_t)(p - base) >> 6, bit = (uint32_t)p & 63u;
		const unsigned long long above = bit == 63u ? 0ull : s_w[w] >> (bit + 1u);
		const uint64_t e = above ? p + (uint64_t)__ffsll((long long)above) : (uint64_t)s_nx[w];	/* (p < e <= n) */
		const uint64_t sp = A.perm ? A.perm[p] : p;
		if (sp >= n)
			continue;	/* (k_win_scan has raised MDB_GROUPS_ST_PERM_RANGE) */
		for (int f = 0; f < A.F.nfns; f++) {
			const mdb_stream_col &col = A.F.c[f];
			if (col.op == MDB_WIN_COUNT) {
				A.F.out[f][sp] = e - (uint64_t)A.B32[p];
				continue;
			}
			if (!win_is_agg(col.op))
				continue;
			const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(A.F.T[f] + (e - 1u) * 2u);
			uint64_t res = 0;
			if (v.y) {
				if (win_is_minmax(col.op))
					res = mdb_order_unimage(v.x, col.type);
				else if (col.op == MDB_WIN_SUM)
					res = v.x;
				else
					res = (uint64_t)__double_as_longlong((double)(long long)v.x / (double)v.y);
			}
			A.F.out[f][sp] = res;
			A.F.nf[f][sp] = v.y ? 0u : 1u;
		}
	}
}

/* ------------------------------------------------------------------ the navigation functions: the cell of another row of the partition.
 * As k_win_ends, with the chunk's words of BOTH bitmaps in LDS: e from gh / nexth, pe = the position behind the row's partition from ph /
 * nextp, b from B32.  One gather per function and row: perm[q], then the cell.  Plain stores; the NULL flags go through k_win_pack. */
struct win_nav_args {
	win_fns F;
	uint64_t arg[WIN_MAX_FNS], dflt[WIN_MAX_FNS];
	uint32_t dnull[WIN_MAX_FNS];
	const uint32_t *perm;
	uint64_t n;
	const unsigned long long *ph, *gh;
	const uint32_t *nexth, *nextp;
	const uint32_t *B32;		/* NULL when no function of the call asks for b */
};

/* the first set bit of word w's bits above `bit` as a position, or nx[w] */
__device__ static inline uint64_t win_next_head(const unsigned long long *s_w, const uint32_t *s_nx, uint64_t p, uint32_t w, uint32_t bit)
{
	const unsigned long long above = bit == 63u ? 0ull : s_w[w] >> (bit + 1u);
	return above ? p + (uint64_t)__ffsll((long long)above) : (uint64_t)s_nx[w];
}

__global__ __launch_bounds__(WIN_THREADS) void k_win_nav(win_nav_args A)
{
	__shared__ unsigned long long s_w[2][WIN_WORDS];	/* 0: gh, 1: ph */
	__shared__ uint32_t s_nx[2][WIN_WORDS];			/* the first head in the chunk's words behind word w, or behind the chunk */
	const uint64_t c = blockIdx.x, n = A.n, base = c * WIN_CHUNK;
	const uint32_t t = threadIdx.x;
	if (t < 2u * WIN_WORDS) {
		const uint32_t which = t / WIN_WORDS, w = t % WIN_WORDS;
		s_w[which][w] = base + (uint64_t)w * 64u < n ? (which ? A.ph : A.gh)[(base >> 6) + w] : 0ull;
	}
	__syncthreads();
	if (t < 2u) {
		uint32_t nx = t ? A.nextp[c] : A.nexth[c];
		for (uint32_t w = WIN_WORDS; w > 0; w--) {
			s_nx[t][w - 1u] = nx;
			if (s_w[t][w - 1u])
				nx = (uint32_t)(base + (uint64_t)(w - 1u) * 64u) + (uint32_t)__ffsll((long long)s_w[t][w - 1u]) - 1u;
		}
	}
	__syncthreads();
	for (uint32_t k = 0; k < WIN_STRIP; k++) {
		const uint64_t p = base + (uint64_t)k * WIN_THREADS + t;
		if (p >= n)
			break;
		const uint32_t w = (uint32_t)(p - base) >> 6, bit = (uint32_t)p & 63u;
		const uint64_t e = win_next_head(s_w[0], s_nx[0], p, w, bit);	/* (p < e <= pe <= n) */
		const uint64_t pe = win_next_head(s_w[1], s_nx[1], p, w, bit);
		const uint64_t sp = A.perm ? A.perm[p] : p;
		if (sp >= n)
			continue;	/* (k_win_scan has raised MDB_GROUPS_ST_PERM_RANGE) */
		const uint64_t b = A.B32 ? (uint64_t)A.B32[p] : 0ull;	/* (b <= p) */
		for (int f = 0; f < A.F.nfns; f++) {
			const mdb_stream_col &col = A.F.c[f];
			const uint64_t a = A.arg[f];
			if (col.op == MDB_WIN_NTILE) {
				const uint64_t s = pe - b, r = p - b, q = s / a, m = s % a;	/* (a != 0: checked by the host) */
				const uint64_t big = m * (q + 1u);	/* (below s + a: no overflow) */
				A.F.out[f][sp] = r < big ? r / (q + 1u) + 1u : (q ? m + (r - big) / q + 1u : m);
				continue;
			}
			if (!win_is_gather(col.op))
				continue;
			uint64_t q = 0;
			bool in = true;
			if (col.op == MDB_WIN_LAG) {
				in = a <= p - b;
				q = p - (in ? a : 0u);
			} else if (col.op == MDB_WIN_LEAD) {
				in = a < pe - p;
				q = p + (in ? a : 0u);
			} else if (col.op == MDB_WIN_FIRST_VALUE) {
				q = b;
			} else {
				q = e - 1u;
			}
			uint64_t bits = 0;
			bool valid;
			if (in) {	/* (b <= q < pe <= n) */
				const uint64_t sq = A.perm ? A.perm[q] : q;
				valid = sq < n && mdb_stream_cell(col, sq, &bits);
			} else {
				bits = A.dflt[f];
				valid = !A.dnull[f];
			}
			A.F.out[f][sp] = valid ? bits : 0ull;
			A.F.nf[f][sp] = valid ? 0u : 1u;
		}
	}
}

/* one thread per stream position, a wave per word of NULL bits: every word of out_nullbits is written whole */
__global__ __launch_bounds__(WIN_THREADS) void k_win_pack(const uint8_t *__restrict__ nf, uint64_t n, unsigned long long *__restrict__ out_nullbits)
{
	const uint64_t i = (uint64_t)blockIdx.x * WIN_THREADS + threadIdx.x;
	const unsigned long long nb = __ballot(i < n && nf[i] != 0);
	if (mdb_lane() == 0 && (i & ~63ull) < n)
		out_nullbits[i >> 6] = nb;
}

/* ------------------------------------------------------------------ host side */

extern "C" int mdb_dev_window(mdb_dev_ctx *ctx, const struct mdb_sort_key *part, int npart, const struct mdb_sort_key *order, int norder, uint64_t n,
			      const struct mdb_window_fn *fns, int nfns, uint32_t *out_form)
{
	if (!ctx)
		return -MIDORIDB_ERROR;
	if (out_form)
		*out_form = 0;
	if (!fns || nfns < 1 || nfns > MDB_WIN_MAX_FNS)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "window: 1 ... %d functions per call", MDB_WIN_MAX_FNS);
	if (npart < 0 || norder < 0 || npart + norder > MDB_SORT_MAX_KEYS || (npart && !part) || (norder && !order))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "window: 0 ... %d partition and order key columns together", MDB_SORT_MAX_KEYS);
	if (n >= MDB_NO_ROW)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "window: %llu rows, a stream holds fewer than 2^32 - 1", (unsigned long long)n);
	const int nkeys = npart + norder;
	struct mdb_sort_key sk[MDB_SORT_MAX_KEYS];
	for (int k = 0; k < nkeys; k++) {
		sk[k] = k < npart ? part[k] : order[k - npart];
		if (k < npart)
			sk[k].desc = 0;
		if ((sk[k].type != MDB_T_INT64 && sk[k].type != MDB_T_DOUBLE) || (n && !sk[k].values))
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "window: key column %d: no cells, or unknown cell type %d", k, sk[k].type);
	}
	win_fns F;
	memset(&F, 0, sizeof(F));
	F.nfns = nfns;
	int nslots = 0, nnav = 0;
	bool has_count = false, need_b = false;
	win_nav_args N;
	memset(&N, 0, sizeof(N));
	for (int f = 0; f < nfns; f++) {
		const struct mdb_window_fn *w = &fns[f];
		if (w->op < MDB_WIN_ROW_NUMBER || w->op > MDB_WIN_NTILE || (w->op > MDB_WIN_AVG && w->op < MDB_WIN_LAG))
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "window: function %d: unknown function %d", f, w->op);
		if (!w->out || !w->out_nullbits)
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "window: function %d: no place for the result", f);
		F.c[f].op = w->op;
		F.out[f] = (uint64_t *)w->out;
		has_count = has_count || w->op == MDB_WIN_COUNT;
		need_b = need_b || w->op == MDB_WIN_COUNT || w->op == MDB_WIN_LAG || w->op == MDB_WIN_FIRST_VALUE || w->op == MDB_WIN_NTILE;
		if (win_is_nav(w->op)) {
			if (w->op == MDB_WIN_NTILE && !w->arg)
				return mdb_set_err(ctx, -MIDORIDB_ERROR, "window: function %d: NTILE(0): the number of buckets must be at least 1", f);
			nnav++;
			N.arg[f] = w->arg;
			N.dflt[f] = w->dflt;
			N.dnull[f] = w->dflt_null ? 1u : 0u;
			if (!win_is_gather(w->op))
				continue;
			if (n && !w->values)
				return mdb_set_err(ctx, -MIDORIDB_ERROR, "window: function %d: no cells", f);
			F.c[f] = mdb_stream_col_of(w->values, w->nullbits, w->rid, w->op, w->type);	/* (cells are copied: any type) */
			continue;
		}
		if (!win_is_agg(w->op))
			continue;
		if ((w->type != MDB_T_INT64 && w->type != MDB_T_DOUBLE) || (n && !w->values))
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "window: function %d: no cells, or unknown cell type %d", f, w->type);
		if (w->type == MDB_T_DOUBLE && !win_is_minmax(w->op))
			return mdb_set_err(ctx, -MIDORIDB_ERROR, "window: function %d: SUM / AVG over DOUBLE cells are not served (a scan's order of summation)", f);
		F.c[f] = mdb_stream_col_of(w->values, w->nullbits, w->rid, w->op, w->type);
		nslots++;
	}
	const uint32_t form = nkeys ? 2u : 1u;
	if (!n) {
		if (out_form)
			*out_form = form;
		return MIDORIDB_OK;
	}

	mdb_dev_tmp tmp(ctx);
	const uint64_t nchunks = (n + WIN_CHUNK - 1u) / WIN_CHUNK, words = (n + 63u) / 64u;
	uint32_t *perm = NULL;
	int rc;
	if (nkeys) {
		perm = (uint32_t *)tmp.take(n * 4u + 16u);
		if (!perm)
			return mdb_set_err(ctx, -MIDORIDB_NOMEM, "window: no device memory for the permutation");
		if ((rc = mdb_dev_sort_perm(ctx, sk, nkeys, n, perm)))
			return rc;
	}
	unsigned long long *ph = (unsigned long long *)tmp.take(nchunks * WIN_WORDS * 8u * 2u);
	win_st *st_sum = (win_st *)tmp.take(nchunks * sizeof(win_st) * 2u);
	win_ag *ag_sum = (win_ag *)tmp.take((uint64_t)(nslots ? nslots : 1) * nchunks * sizeof(win_ag) * 2u);
	uint32_t *hasp_sum = (uint32_t *)tmp.take(nchunks * 4u * 3u);
	uint32_t *B32 = need_b ? (uint32_t *)tmp.take(n * 4u) : NULL;
	uint32_t *status = (uint32_t *)tmp.take(256);
	if (!ph || !st_sum || !ag_sum || !hasp_sum || (need_b && !B32) || !status)
		return mdb_set_err(ctx, -MIDORIDB_NOMEM, "window: no device memory for %llu chunks", (unsigned long long)nchunks);
	unsigned long long *gh = ph + nchunks * WIN_WORDS;
	win_st *st_carry = st_sum + nchunks;
	win_ag *ag_carry = ag_sum + (uint64_t)(nslots ? nslots : 1) * nchunks;
	uint32_t *nexth = hasp_sum + nchunks, *nextp = nexth + nchunks;
	for (int f = 0; f < nfns; f++) {
		if (win_is_gather(F.c[f].op)) {
			F.nf[f] = (uint8_t *)tmp.take(n);
			if (!F.nf[f])
				return mdb_set_err(ctx, -MIDORIDB_NOMEM, "window: no device memory for the NULL flags of %llu rows", (unsigned long long)n);
		}
		if (!win_is_agg(F.c[f].op))
			continue;
		F.T[f] = (unsigned long long *)tmp.take(n * 16u);
		F.nf[f] = (uint8_t *)tmp.take(n);
		if (!F.T[f] || !F.nf[f])
			return mdb_set_err(ctx, -MIDORIDB_NOMEM, "window: no device memory for the running values of %llu rows", (unsigned long long)n);
	}

	mdb_stream_keys K;
	memset(&K, 0, sizeof(K));
	K.npart = npart;
	K.nkeys = nkeys;
	for (int k = 0; k < nkeys; k++)
		K.k[k] = mdb_stream_col_of_key(&sk[k]);
	MDB_HIP(ctx, hipMemsetAsync(status, 0, 4, ctx->stream));
	MDB_HIP(ctx, hipMemsetAsync(ph, 0, nchunks * WIN_WORDS * 8u * 2u, ctx->stream));
	MDB_LAUNCH(ctx, "win_heads", k_win_heads, (uint32_t)((n + WIN_THREADS - 1u) / WIN_THREADS), WIN_THREADS, K, (const uint32_t *)perm, n, ph, gh, status);

	win_scan_args S;
	memset(&S, 0, sizeof(S));
	S.F = F;
	S.perm = perm;
	S.n = n;
	S.nchunks = nchunks;
	S.ph = ph;
	S.gh = gh;
	S.st_sum = st_sum;
	S.ag_sum = ag_sum;
	S.hasp_sum = hasp_sum;
	S.st_carry = st_carry;
	S.ag_carry = ag_carry;
	S.B32 = B32;
	S.status = status;
	MDB_LAUNCH(ctx, "win_scan_local", k_win_scan<false>, (uint32_t)nchunks, WIN_THREADS, S);

	win_carry_args C;
	memset(&C, 0, sizeof(C));
	C.n = n;
	C.nchunks = nchunks;
	for (int f = 0; f < nfns; f++)
		if (win_is_agg(F.c[f].op))
			C.op[C.nslots++] = F.c[f].op;
	C.st_sum = st_sum;
	C.ag_sum = ag_sum;
	C.hasp_sum = hasp_sum;
	C.st_carry = st_carry;
	C.ag_carry = ag_carry;
	C.nexth = nexth;
	C.nextp = nextp;
	MDB_LAUNCH(ctx, "win_carry", k_win_carry, 1, WIN_THREADS, C);
	MDB_LAUNCH(ctx, "win_scan_apply", k_win_scan<true>, (uint32_t)nchunks, WIN_THREADS, S);

	if (nslots || has_count) {
		win_ends_args E;
		memset(&E, 0, sizeof(E));
		E.F = F;
		E.perm = perm;
		E.n = n;
		E.gh = gh;
		E.nexth = nexth;
		E.B32 = B32;
		MDB_LAUNCH(ctx, "win_ends", k_win_ends, (uint32_t)nchunks, WIN_THREADS, E);
	}
	if (nnav) {
		N.F = F;
		N.perm = perm;
		N.n = n;
		N.ph = ph;
		N.gh = gh;
		N.nexth = nexth;
		N.nextp = nextp;
		N.B32 = B32;
		MDB_LAUNCH(ctx, "win_nav", k_win_nav, (uint32_t)nchunks, WIN_THREADS, N);
	}
	for (int f = 0; f < nfns; f++) {
		if (win_is_agg(F.c[f].op) || win_is_gather(F.c[f].op))
			MDB_LAUNCH(ctx, "win_pack", k_win_pack, (uint32_t)((n + WIN_THREADS - 1u) / WIN_THREADS), WIN_THREADS, (const uint8_t *)F.nf[f], n,
				   (unsigned long long *)fns[f].out_nullbits);
		else	/* (a rank, a count or a bucket is never NULL) */
			MDB_HIP(ctx, hipMemsetAsync(fns[f].out_nullbits, 0, words * 8u, ctx->stream));
	}
	{
		uint32_t h = 0;
		MDB_HIP(ctx, hipMemcpyAsync(&h, status, 4, hipMemcpyDeviceToHost, ctx->stream));
		MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (h & MDB_GROUPS_ST_PERM_RANGE)
			return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "window: the sort's permutation names a row beyond the stream");
	}
	if (out_form)
		*out_form = form;
	return MIDORIDB_OK;
}

extern "C" uint64_t mdb_dev_window_fn_size(void) { return sizeof(struct mdb_window_fn); }
