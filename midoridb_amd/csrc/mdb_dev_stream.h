/*
 * mdb_dev_stream.h - what the operators over a tuple stream share (aggregate, COUNT(DISTINCT), window, row sets, the set builder, the sorts):
 * the cell of a stream position, the order-preserving image of a value, the test "does this sorted position begin a run", the key -> group
 * table in LDS, the group of a first row, the groups' status flags and scoped temporaries.  Every one of them exists here and nowhere else.
 */
#ifndef MDB_DEV_STREAM_H
#define MDB_DEV_STREAM_H

#include "mdb_dev_common.h"

/* ------------------------------------------------------------------ a column read along the stream: row i reads values[rid ? rid[i] : i] */
struct mdb_stream_col {
	const uint64_t *values;
	const uint64_t *nullbits;
	const uint32_t *rid;
	int32_t op, type;	/* op: the operator's own function code (0: a key column) */
};

struct mdb_stream_keys {
	mdb_stream_col k[MDB_SORT_MAX_KEYS];
	int npart, nkeys;	/* k[0 .. npart): partition keys, k[npart .. nkeys): order keys (no order keys: npart == nkeys) */
};

static inline mdb_stream_col mdb_stream_col_of(const void *values, const uint64_t *nullbits, const uint32_t *rid, int op, int type)
{
	mdb_stream_col c;
	c.values = (const uint64_t *)values;
	c.nullbits = nullbits;
	c.rid = rid;
	c.op = op;
	c.type = type;
	return c;
}

static inline mdb_stream_col mdb_stream_col_of_key(const struct mdb_sort_key *k) { return mdb_stream_col_of(k->values, k->nullbits, k->rid, 0, k->type); }

#define MDB_GROUP_NONE 0xFFFFFFFFu	/* no group: an empty slot of the LDS table, a key or a first row that belongs to no group */

/* flags of a grouped operator's status word; an operator's own flags (CD_ST_OUT_OF_RANGE) take other bits of the same word */
#define MDB_GROUPS_ST_KEY_MISSING 1u	/* a row's group key is the key of no group / a run's head is nobody's first row: first[] does not belong to these keys */
#define MDB_GROUPS_ST_RUNS_DIFFER 2u	/* more runs of equal keys than groups */
#define MDB_GROUPS_ST_PERM_RANGE 8u	/* the sort's permutation names a stream position at or beyond n: that row is skipped, the call fails */
static_assert(mdb_flags_distinct({ MDB_GROUPS_ST_KEY_MISSING, MDB_GROUPS_ST_RUNS_DIFFER, MDB_GROUPS_ST_PERM_RANGE }), "groups: two status flags share a bit");

/* The order-preserving image of a cell - INT64 with the sign bit flipped, DOUBLE by the IEEE total-order trick, so -0.0 lies before +0.0;
 * desc: the complement, for a descending key - and its inverse (of the ascending image) */
__host__ __device__ static inline uint64_t mdb_order_image(uint64_t bits, int type, int desc = 0)
{
	const uint64_t sign = 0x8000000000000000ull;
	uint64_t u;
	if (type == MDB_T_DOUBLE)
		u = (bits >> 63) ? ~bits : (bits ^ sign);
	else
		u = bits ^ sign;
	return desc ? ~u : u;
}

__host__ __device__ static inline uint64_t mdb_order_unimage(uint64_t u, int type)
{
	const uint64_t bits = mdb_order_image(u, MDB_T_INT64);	/* (the sign bit flipped back) */
	return type == MDB_T_DOUBLE && (bits >> 63) ? ~u : bits;
}

/* ------------------------------------------------------------------ scoped temporaries over mdb_cached_alloc: room for the window operator's
 * worst case (16 buffers and two per function); a request of no bytes still gets a buffer of its own */
struct mdb_dev_tmp {
	mdb_dev_ctx *ctx;
	void *p[16 + 2 * MDB_WIN_MAX_FNS];
	int n;
	explicit mdb_dev_tmp(mdb_dev_ctx *c) : ctx(c), n(0) {}
	mdb_dev_tmp(const mdb_dev_tmp &) = delete;
	mdb_dev_tmp &operator=(const mdb_dev_tmp &) = delete;
	~mdb_dev_tmp()
	{
		for (int i = 0; i < n; i++)
			(void)mdb_cached_free(ctx, p[i]);
	}
	void *take(size_t bytes)
	{
		void *q = NULL;
		if (n == (int)(sizeof(p) / sizeof(p[0])) || mdb_cached_alloc(ctx, bytes ? bytes : 8, &q))
			return NULL;
		p[n++] = q;
		return q;
	}
};

/* ------------------------------------------------------------------ the key -> group table in LDS, host side: 2^log2 slots of an 8-byte key
 * and a 4-byte group number, open addressing (mdb_set_slot_of) at load <= 1/2 */
#define MDB_GROUP_LDS_BUDGET (160u * 1024u - 1024u)	/* bytes of dynamic LDS a workgroup may take (the CU has 160 KiB; 1 KiB stays free) */

static inline uint32_t mdb_group_lds_log2(uint64_t G)
{
	uint32_t lg = MDB_SET_MIN_LOG2;
	while ((1ull << lg) < 2u * G)
		lg++;
	return lg;
}

static inline size_t mdb_group_lds_bytes(uint64_t slots) { return (size_t)slots * 12u; }

/* two workgroups per CU while their LDS allows, never more workgroups than 8192-row shares */
static inline uint32_t mdb_group_lds_grid(const mdb_dev_ctx *ctx, size_t lds, uint64_t n)
{
	uint64_t grid = (uint64_t)ctx->num_cus * (lds * 2u <= 160u * 1024u ? 2u : 1u);
	const uint64_t shares = (n + 8191u) / 8192u;
	grid = grid < shares ? grid : shares;
	return (uint32_t)(grid ? grid : 1);
}

#ifdef __HIPCC__

/* ------------------------------------------------------------------ cells */

/* the cell of stream position sp: false - and *bits untouched - for a NULL cell and for "no row" */
__device__ static inline bool mdb_stream_cell(const mdb_stream_col &c, uint64_t sp, uint64_t *bits)
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
 * address allows (a column that starts 8 bytes off a 16-byte boundary is read by 8-byte loads) and one look at the NULL word */
__device__ static inline void mdb_stream_cell2(const mdb_stream_col &c, uint64_t i, bool two, uint64_t bits[2], bool valid[2])
{
	if (c.rid) {
		valid[0] = mdb_stream_cell(c, i, &bits[0]);
		valid[1] = two && mdb_stream_cell(c, i + 1, &bits[1]);
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

/* ------------------------------------------------------------------ runs of a sorted stream
 * Does sorted position p (stream position perm[p]; perm == NULL: p itself) begin a run?  part: position 0, or one of the keys [0, npart)
 * differs from the row before - NULL equals NULL, values by their bits -, peer: part, or one of the other keys differs.  Every position
 * gathers ITS key cells once; the row before is the lane before (a shuffle) - only a wave's first lane gathers it: ALL lanes of a wave call
 * this, with consecutive p.  Where perm names a position at or beyond n no key cell beyond the stream is read: MDB_GROUPS_ST_PERM_RANGE is
 * raised in the caller's status word. */
struct mdb_stream_head {
	bool part, peer;
};

__device__ static inline mdb_stream_head mdb_stream_head_of(const mdb_stream_keys &K, const uint32_t *__restrict__ perm, uint64_t n, uint64_t p, uint32_t *status)
{
	const bool in = p < n, first_lane = in && p && mdb_lane() == 0;
	uint64_t s1 = in ? (perm ? perm[p] : p) : 0, s0 = first_lane ? (perm ? perm[p - 1] : p - 1) : 0;
	if (s1 >= n || s0 >= n) {
		if (in)
			mdb_raise(status, MDB_GROUPS_ST_PERM_RANGE);
		s1 = s1 >= n ? 0 : s1;
		s0 = s0 >= n ? 0 : s0;
	}
	mdb_stream_head h;
	h.part = in && p == 0;
	h.peer = false;
	for (int k = 0; k < K.nkeys; k++) {
		uint64_t b1 = 0;
		const bool v1 = in && mdb_stream_cell(K.k[k], s1, &b1);
		uint64_t b0 = (uint64_t)__shfl_up((unsigned long long)b1, 1u, MDB_WAVE);
		bool v0 = __shfl_up((int)v1, 1u, MDB_WAVE) != 0;
		if (first_lane) {
			b0 = 0;
			v0 = mdb_stream_cell(K.k[k], s0, &b0);
		}
		if (in && p) {
			const bool differs = v0 != v1 || (v1 && b0 != b1);
			if (k < K.npart)
				h.part = h.part || differs;
			else
				h.peer = h.peer || differs;
		}
	}
	h.peer = h.peer || h.part;
	return h;
}

/* the group g with first[g] == sp (first[] ascending), or MDB_GROUP_NONE */
__device__ static inline uint32_t mdb_first_group_of(const uint32_t *__restrict__ first, uint64_t G, uint32_t sp)
{
	uint64_t lo = 0, hi = G;
	while (lo < hi) {
		const uint64_t mid = (lo + hi) >> 1;
		if (first[mid] < sp)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo < G && first[lo] == sp ? (uint32_t)lo : MDB_GROUP_NONE;
}

/* what mdb_runs_find (mdb_dev_runs.hip) leaves: hb bit p = "sorted position p begins a run", base[c] = heads in front of chunk c of
 * MDB_RUNS_CHUNK positions (hb holds whole chunks).  -> the heads in front of position p, in two forms.  One thread on its own (the few
 * positions that are heads): it counts the chunk's words in front of its own, at most 15. */
#define MDB_RUNS_CHUNK 1024u
__device__ static inline uint32_t mdb_runs_heads_before(const unsigned long long *__restrict__ hb, const uint32_t *__restrict__ base, uint64_t p)
{
	const uint64_t chunk = p / MDB_RUNS_CHUNK;
	uint32_t r = base[chunk] + (uint32_t)__popcll(hb[p >> 6] & ((1ull << (p & 63)) - 1ull));
	for (uint64_t q = chunk * (MDB_RUNS_CHUNK / 64u); q < (p >> 6); q++)
		r += (uint32_t)__popcll(hb[q]);
	return r;
}

/* ... for EVERY position: ALL lanes of a wave call this, lane l with p = a multiple of 64 + l - the words in front of the wave's word are
 * counted a lane each and added up in the wave */
__device__ static inline uint32_t mdb_runs_heads_before_wave(const unsigned long long *__restrict__ hb, const uint32_t *__restrict__ base, uint64_t p)
{
	const uint32_t lane = mdb_lane();
	const uint64_t chunk = p / MDB_RUNS_CHUNK, word0 = chunk * (MDB_RUNS_CHUNK / 64u);
	const uint32_t mine = word0 + lane < (p >> 6) ? (uint32_t)__popcll(hb[word0 + lane]) : 0u;
	const uint32_t words = (uint32_t)__shfl((int)mdb_wave_incl_scan(mine), MDB_WAVE - 1, MDB_WAVE);
	return base[chunk] + words + (uint32_t)__popcll(hb[p >> 6] & ((1ull << lane) - 1ull));
}

/* ------------------------------------------------------------------ the key -> group table in LDS, device side
 * mem: mdb_group_lds_bytes(slots) bytes of LDS - slots keys, then slots group numbers; the NULL key has a word of its own. */
struct mdb_group_lds {
	unsigned long long *key;
	uint32_t *grp, *nullgrp;
	uint32_t slots, log2_slots;
};

/* All `threads` threads of the workgroup: the table of the keys at first[0 .. G) (slots == 0: no key column, an empty table).  Begins and
 * ends with a barrier of its own, so what the caller initialised in LDS before the call is visible after it. */
__device__ static inline mdb_group_lds mdb_group_lds_build(unsigned long long *mem, uint32_t slots, uint32_t log2_slots, const mdb_stream_col &key,
							    const uint32_t *__restrict__ first, uint32_t G, uint32_t threads)
{
	__shared__ uint32_t s_nullgrp;
	mdb_group_lds T;
	T.key = mem;
	T.grp = reinterpret_cast<uint32_t *>(mem + slots);
	T.nullgrp = &s_nullgrp;
	T.slots = slots;
	T.log2_slots = log2_slots;
	for (uint32_t i = threadIdx.x; i < slots; i += threads)
		T.grp[i] = MDB_GROUP_NONE;
	if (threadIdx.x == 0)
		s_nullgrp = MDB_GROUP_NONE;
	__syncthreads();
	if (slots)
		for (uint32_t g = threadIdx.x; g < G; g += threads) {
			uint64_t kb = 0;
			if (!mdb_stream_cell(key, first[g], &kb)) {
				s_nullgrp = g;
				continue;
			}
			uint32_t s = (uint32_t)mdb_set_slot_of(kb, log2_slots);
			for (uint32_t step = 0; step < slots; step++, s = (s + 1u) & (slots - 1u))
				if (atomicCAS(&T.grp[s], MDB_GROUP_NONE, g) == MDB_GROUP_NONE) {	/* (G <= slots / 2: a free slot exists) */
					T.key[s] = kb;
					break;
				}
		}
	__syncthreads();
	return T;
}

/* the group of a key cell (valid == false: the NULL key), or MDB_GROUP_NONE */
__device__ static inline uint32_t mdb_group_lds_find(const mdb_group_lds &T, uint64_t bits, bool valid)
{
	uint32_t g = MDB_GROUP_NONE;
	if (!valid) {
		g = *T.nullgrp;
	} else {
		uint32_t s = (uint32_t)mdb_set_slot_of(bits, T.log2_slots);
		for (uint32_t step = 0; step < T.slots; step++, s = (s + 1u) & (T.slots - 1u)) {
			const uint32_t at = T.grp[s];
			if (at == MDB_GROUP_NONE)
				break;
			if (T.key[s] == bits) {
				g = at;
				break;
			}
		}
	}
	return g;
}

#endif /* __HIPCC__ */
#endif /* MDB_DEV_STREAM_H */
