/*
 * mdb_dev_partition.hip - LDS-staged MSD radix partitioning of a key column by the top
 * bits of fmix64(key).  This is the bandwidth-dominant stage of the join / GROUP BY pipeline.
 *
 * Why it exists: the reference joins by comparing every pair of rows (reference
 * src/engine/executor_select.c:1096-1141, O(nA*nB)) and groups by comparing every pair of
 * surviving rows (:1542-1583, O(n^2)).  Here both tables are split into 2^bits "leaves" whose
 * build side fits one CU's LDS; equal keys always land in the same leaf, so each leaf is joined /
 * grouped independently by one workgroup (mdb_dev_join_leaf.hip, mdb_dev_leaf_wide.hip).
 *
 * The default ("FAST") form has NO histogram pass: every child owns a fixed-capacity region and each (tile, digit)
 * run reserves its place with one global atomic on the region's cursor (first level: 8 sub-regions per digit, one
 * per XCD, cursors laid out so that a tile's 256 atomics fall into 8 lines private to its XCD); an overflowing
 * region (skew) is flagged on the device and the caller redoes the operator with the exact form below, which is
 * also what the stable variant (materialising N:M join) and the destination partition (multi-GPU) use.
 *
 * Exact form, one level = histogram -> exclusive scan -> scatter, all tile based (MDB_TILE = 4096 keys):
 *
 *   k_part_hist     per tile: LDS histogram of the level's digit, written digit-major
 *   (scan)          one exclusive scan over [segment][digit][tile] gives every tile its output
 *                   offset per digit and, as a by-product, the exact start of every child segment
 *   k_part_scatter  per tile: one LDS atomic per key gives its rank inside its digit, keys are
 *                   staged sorted-by-digit in LDS, then written out as contiguous runs per digit
 *                   (coalesced; TILE/R keys per run)
 *
 * Level 0 reads the raw int64 keys (+ NULL bits, NULL rows are dropped - a NULL key never joins,
 * executor_select.c:557-579), hashes them, and attaches the row id; later levels move (hash, rid).
 * Order inside a leaf is unspecified; the consumers restore the reference's orders from the row ids.
 *
 * Memory traffic per level and key: hist reads 8 B, scatter reads 8(+4) B and writes 8(+4) B.
 * Blocks are mapped to tiles XCD-contiguously (blockIdx % 8 selects the XCD) so that adjacent
 * tiles - which extend each other's output runs - meet in the same 4 MiB L2.
 */
#include <stdlib.h>
#include <type_traits>
#include "mdb_dev_internal.h"

#define PART_ST_OWN_RANGE_BROKEN 1024u	/* status flag of mdb_dev_partition_by_dest_pruned alone (beside MDB_ST_KEY_OUTSIDE): a key outside the range promised for its column */
static_assert(mdb_flags_distinct({ MDB_ST_REGION_FULL, MDB_ST_LIST_FULL, MDB_ST_KEY_OUTSIDE, PART_ST_OWN_RANGE_BROKEN }), "partition: two status flags share a bit");

#define PART_THREADS 512
#define PART_WAVES (PART_THREADS / MDB_WAVE)
#define PART_ITEMS (MDB_TILE / PART_THREADS)		/* 8 keys per thread */
#define PART_WAVE_SPAN (MDB_TILE / PART_WAVES)		/* 512 consecutive keys per wave */
#define PART_MAX_R (1u << MDB_MAX_RADIX_BITS)
#define PART_FEW_DIGITS 4u	/* up to this many digits (destination GPUs) a wave ranks its keys with ballots, not one atomic per key */
#define PART_INVALID 0xFFFFFFFFu

struct mdb_level_args {
	/* level 0 input */
	const int64_t *keys;
	const uint64_t *nullbits;
	uint64_t n;
	/* level >= 1 input */
	const uint64_t *hv_in;
	const uint32_t *rid_in;
	const mdb_tile_desc *tiles;	/* NULL for level 0 (computed arithmetically) */
	/* output */
	uint64_t *hv_out;
	uint32_t *rid_out;		/* NULL = row ids not wanted */
	uint32_t *hist;			/* counts in, scanned offsets out */
	uint32_t ntiles;		/* tiles to cover (upper bound for level >= 1) */
	uint32_t R;			/* digits at this level */
	uint32_t shift;			/* RADIX mode: digit = (hv >> shift) & (R - 1) */
	uint32_t mbits;			/* bits needed to tell digits apart (ballot rounds of the STABLE form) */
	uint32_t mode;			/* enum mdb_digit_mode */
	uint32_t inverse_out;		/* write fmix64^-1(hv) (= the original key) instead of hv; 2 = as int32 (4-byte wire format) */
	/* FAST (histogram-free) form: child (seg, digit) owns the fixed-capacity region [child*cap, child*cap+cap) */
	uint32_t *cursor;		/* per child: elements placed so far (zeroed before the launch) */
	uint32_t cap;
	uint32_t skip_zero;		/* raw sort keys: a zero word is a gap in the input list, not a key */
	uint32_t nsub;			/* > 0: first level, child = digit * nsub + (block % nsub) sub-region; 0: child = seg * R + digit */
	uint32_t *status;		/* bit 1 set when a child overflowed its region */
	/* level 0, narrow form: every key must lie within 2^31 of narrow_base (otherwise bit 7 of *status is raised and the caller
	 * redoes the operator in the wide form); the word written is fmix32(low 32 bits of the key) << 32, plus the row id in
	 * the low half when narrow == 1 - hash and row id then travel as ONE 8-byte word and no row-id array exists - or
	 * the hash once more when narrow == 2 */
	uint32_t narrow;
	int64_t narrow_base;		/* narrow form: centre of the 2^32-wide window of key values that the 32-bit words can tell apart
					 * (compact form, narrow_kbits != 0: the window's LOW end) */
	uint32_t narrow_kbits;		/* compact narrow form: every key must lie in [narrow_base, narrow_base + 2^narrow_kbits); the 32-bit
					 * hash is mixk(key - narrow_base) in the TOP narrow_kbits bits of the field, zeros below */
	uint32_t keys32;		/* level 0: `keys` is an array of int32 (keys that crossed xGMI in the 4-byte wire format) */
	/* semi-join filter (second level, left side of a join in the compact narrow form; mdb_part_request.bits): the slice of
	 * first-level digit td.seg is words [seg * filter_words, ...); a row whose bit (hash32 >> filter_shift, masked to the
	 * slice) is clear can join nothing and is dropped before it is ranked */
	const uint32_t *filter;
	uint32_t filter_words, filter_shift;
	/* min-max pruning (first level, compact narrow form): the RIGHT table's launch leaves the smallest and the largest
	 * key - window base it saw in minmax_out[0..1] (atomics; the caller has stored 0xFFFFFFFF, 0 there), the LEFT table's
	 * launch - later on the same stream - reads them through range_in and drops every row outside: such a row can join
	 * nothing.  Exact, and free: one compare per row, no extra pass, no host round trip */
	uint32_t *minmax_out;
	uint32_t *minmax_final;	/* with minmax_out: the two words the reduce kernel's workgroups meet in - preset here (no key: lo > hi) */
	const uint32_t *range_in;
	/* the same for the 64-bit form (keys that fit no 2^32 window: hashes, snowflake ids - R64 instances): per-tile pairs of the
	 * smallest / largest key as order-preserving unsigned images (key ^ 2^63; the largest stored inverted) / the other table's
	 * range [lo, hi] as two signed keys in device memory */
	unsigned long long *minmax64_out;
	const long long *range64_in;
	/* PAY instance (first level of a join that carries payload cells through its one partition level): up to two 8-byte columns of
	 * the table, read at the row's own index and written at the row's place in the regions, beside its word */
	const uint64_t *pay_in[2];
	uint64_t *pay_out[2];
	uint32_t npay;
	/* first level: rows whose key lies outside [keep_lo, keep_hi] are dropped (keep_on; partition by destination: the other
	 * table's global key range is known before the exchange - nothing outside it can join on any GPU) */
	uint32_t keep_on;
	int64_t keep_lo, keep_hi;
	uint32_t own_on;		/* every key of this table was promised to lie in [own_lo, own_hi]: one that does not raises status bit 10 */
	int64_t own_lo, own_hi;
	uint32_t out16_shift;		/* OUT16 instance (first level only, compact narrow form, 4-byte words): what is WRITTEN is the 16-bit word
					 * (uint16_t)(hash32 >> out16_shift) - the hash bits below the digit, all the one-level leaf kernel needs */
	uint32_t fold64;		/* raw 4-byte words: the input is still the list of 8-byte records, folded on the fly (record >> 32 | low
					 * half: the caller knows that the two parts do not overlap) */
};

/* level-0 word of one key */
/* CF: the compact narrow form of an int64 column, known at COMPILE time (RIDW: the word's low half is the row id, else the
 * hash once more).  The generic body below picks the form per row from run-time fields - uniform branches and selects that
 * made the first-level kernels issue-bound (75 vector + 40 scalar instructions per row, profiles/r02). */
template <bool CF = false, bool RIDW = false>
__device__ static inline uint64_t part_hash_key(const mdb_level_args &a, uint64_t key, uint32_t rid, bool *bad, uint64_t *rel = nullptr)
{
	if (CF) {
		key -= (uint64_t)a.narrow_base;
		if (rel)
			*rel = key;
		*bad = *bad || (key >> a.narrow_kbits);
		const uint32_t h = mdb_mixk((uint32_t)key, a.narrow_kbits) << (32u - a.narrow_kbits);
		return ((uint64_t)h << 32) | (RIDW ? rid : h);
	}
	if (!a.narrow)
		return mdb_fmix64(key);
	key -= (uint64_t)a.narrow_base;		/* (wraps: the tests below are on the 64-bit difference) */
	if (rel)
		*rel = a.narrow_kbits ? key : key + 0x80000000ull;	/* a valid key's value is below 2^32 in both forms */
	uint32_t h;
	if (a.narrow_kbits) {
		*bad = *bad || (key >> a.narrow_kbits);
		h = mdb_mixk((uint32_t)key, a.narrow_kbits) << (32u - a.narrow_kbits);
	} else {
		*bad = *bad || (key + 0x80000000ull) >> 32;
		h = mdb_fmix32((uint32_t)key);
	}
	return ((uint64_t)h << 32) | (a.narrow == 1 ? rid : h);
}

template <bool CF = false, typename W>
__device__ static inline uint32_t part_digit(const mdb_level_args &a, W hv)
{
	if (CF || a.mode == MDB_DIGIT_RADIX)
		return (uint32_t)(hv >> a.shift) & (a.R - 1);	/* a.shift counts from the width of W */
	return (a.R & (a.R - 1)) == 0 ? (uint32_t)hv & (a.R - 1) : (uint32_t)hv % a.R;	/* 2, 4, 8 GPUs: no integer division */
}

/* XCD-contiguous block -> tile map: blocks b and b+8 share an XCD (round-robin dispatch), so give
 * each XCD one contiguous run of tiles.  The grid is rounded up to a multiple of 8. */
__device__ static inline uint32_t part_tile_of_block(void)
{
	const uint32_t per = gridDim.x >> 3;
	return (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
}

template <uint32_t TILE = MDB_TILE>
__device__ static inline mdb_tile_desc part_get_tile(const mdb_level_args &a, uint32_t t)
{
	mdb_tile_desc d;
	if (t >= a.ntiles) {
		d.start = d.len = d.hbase = d.nt = d.seg = 0;
		return d;
	}
	if (a.tiles)
		return a.tiles[t];
	const uint64_t start = (uint64_t)t * TILE;
	d.start = (uint32_t)start;
	d.len = start < a.n ? (uint32_t)((a.n - start) < TILE ? (a.n - start) : TILE) : 0;
	d.hbase = t;
	d.nt = a.ntiles;
	d.seg = 0;
	return d;
}

/* Load element i of the tile: returns false for a NULL key (level 0 only). */
template <bool LEVEL0>
__device__ static inline bool part_load(const mdb_level_args &a, const mdb_tile_desc &td, uint32_t i, uint64_t *hv,
					uint32_t *rid)
{
	const uint64_t g = (uint64_t)td.start + i;
	if (LEVEL0) {
		if (a.nullbits && mdb_bit_is_set(a.nullbits, g))
			return false;
		bool bad = false;
		const int64_t key = a.keys32 ? (int64_t)reinterpret_cast<const int32_t *>(a.keys)[g] : a.keys[g];
		*hv = part_hash_key(a, (uint64_t)key, (uint32_t)g, &bad);
		*rid = (uint32_t)g;
	} else {
		*hv = a.hv_in[g];
		*rid = a.rid_in ? a.rid_in[g] : 0;
	}
	return true;
}

/* Load the two adjacent elements 2p, 2p+1 (relative to the even-aligned base of the tile) with one 16-byte
 * access when both belong to the tile (8-byte accesses reach only ~0.6x of the 16-byte rate,
 * MI355X_MICROARCH.md).  lead = 1 when the tile starts on an odd element.  valid[k] = element exists and is
 * not NULL. */
template <bool LEVEL0, bool HAS_RID, bool RAW = false, bool INV = false, bool KEEP = true /* compile the key-range tests (by-destination kernels) */,
	  bool CF = false, bool RIDW = false /* see part_hash_key */>
__device__ static inline void part_load2(const mdb_level_args &a, const mdb_tile_desc &td, uint32_t p, uint64_t hv[2],
					 uint32_t rid[2], bool valid[2], uint64_t *rel = nullptr /* [2]: key - narrow_base (narrow forms) */,
					 const ulonglong2 *pre = nullptr /* the pair, already loaded (full, 16-byte aligned tiles: the caller
									  * issues a tile's loads together - see part_preload2) */,
					 int64_t *raw_out = nullptr /* [2]: the keys themselves (level 0; the 64-bit form's key-range tests) */)
{
	const uint32_t lead = td.start & 1u;
	const uint64_t base2 = (uint64_t)(td.start - lead);
	const uint32_t e0 = 2 * p, e1 = 2 * p + 1;
	const bool in0 = pre || (e0 >= lead && e0 < lead + td.len);
	const bool in1 = pre || e1 < lead + td.len;	/* e1 >= 1 >= lead always */
	const uint64_t g0 = base2 + e0;
	bool bad[2] = { false, false };
	int64_t raw_key[2] = { 0, 0 };
	hv[0] = hv[1] = 0;
	rid[0] = rid[1] = 0;
	valid[0] = in0;
	valid[1] = in1;
	if (in0 && in1) {
		if (LEVEL0) {
			ulonglong2 k;
			if (pre) {
				k = *pre;
			} else if (!CF && a.keys32) {
				const int2 q = *reinterpret_cast<const int2 *>(reinterpret_cast<const int32_t *>(a.keys) + g0);
				k.x = (uint64_t)(int64_t)q.x;
				k.y = (uint64_t)(int64_t)q.y;
			} else {
				/* (a non-temporal load here made the first-level kernels 3-8 % faster and the kernel that reads their output
				 * 10-20 % slower: +-1 % per query, same-box A/B) */
				k = *reinterpret_cast<const ulonglong2 *>(a.keys + g0);
			}
			raw_key[0] = (int64_t)k.x;
			raw_key[1] = (int64_t)k.y;
			hv[0] = INV ? k.x : part_hash_key<CF, RIDW>(a, k.x, (uint32_t)g0, &bad[0], rel ? &rel[0] : nullptr);	/* INV: the caller keeps the key itself */
			hv[1] = INV ? k.y : part_hash_key<CF, RIDW>(a, k.y, (uint32_t)g0 + 1, &bad[1], rel ? &rel[1] : nullptr);
			rid[0] = (uint32_t)g0;
			rid[1] = (uint32_t)g0 + 1;
		} else {
			const ulonglong2 k = pre ? *pre : *reinterpret_cast<const ulonglong2 *>(a.hv_in + g0);
			hv[0] = k.x;
			hv[1] = k.y;
			if (HAS_RID) {
				const uint2 q = *reinterpret_cast<const uint2 *>(a.rid_in + g0);
				rid[0] = q.x;
				rid[1] = q.y;
			}
		}
	} else if (in0 || in1) {
		const int k = in0 ? 0 : 1;
		const uint64_t g = g0 + (uint64_t)k;
		if (LEVEL0) {
			const int64_t key = (!CF && a.keys32) ? (int64_t)reinterpret_cast<const int32_t *>(a.keys)[g] : a.keys[g];
			raw_key[k] = key;
			hv[k] = INV ? (uint64_t)key : part_hash_key<CF, RIDW>(a, (uint64_t)key, (uint32_t)g, &bad[k], rel ? &rel[k] : nullptr);
			rid[k] = (uint32_t)g;
		} else {
			hv[k] = a.hv_in[g];
			if (HAS_RID)
				rid[k] = a.rid_in[g];
		}
	}
	if (LEVEL0 && raw_out) {
		raw_out[0] = raw_key[0];
		raw_out[1] = raw_key[1];
	}
	if (LEVEL0 && a.nullbits) {
		if (valid[0] && mdb_bit_is_set(a.nullbits, g0))
			valid[0] = false;
		if (valid[1] && mdb_bit_is_set(a.nullbits, g0 + 1))
			valid[1] = false;
	}
	if (LEVEL0 && KEEP && a.own_on && ((valid[0] && (raw_key[0] < a.own_lo || raw_key[0] > a.own_hi)) ||
				   (valid[1] && (raw_key[1] < a.own_lo || raw_key[1] > a.own_hi))))
		mdb_raise(a.status, PART_ST_OWN_RANGE_BROKEN);
	if (LEVEL0 && KEEP && a.keep_on) {
		valid[0] = valid[0] && raw_key[0] >= a.keep_lo && raw_key[0] <= a.keep_hi;
		valid[1] = valid[1] && raw_key[1] >= a.keep_lo && raw_key[1] <= a.keep_hi;
	}
	/* (with min-max pruning - range_in - a key outside the window is outside the right table's range, which lies inside the
	 * window: the caller drops the row, nothing to report) */
	if (LEVEL0 && !a.range_in && ((bad[0] && valid[0]) || (bad[1] && valid[1])))
		mdb_raise(a.status, MDB_ST_KEY_OUTSIDE);	/* a key outside the int32 range: the narrow form does not apply */
	if (RAW && a.skip_zero) {
		valid[0] = valid[0] && hv[0] != 0;
		valid[1] = valid[1] && hv[1] != 0;
	}
}

/* A full tile that starts on an even element: every thread's pairs exist, and their loads can be issued TOGETHER, ahead of
 * the hashing and ranking.  Inside part_load2's range tests each load sits in its own branch, the compiler waits for it
 * (s_waitcnt vmcnt(0)) before the next one is issued, and a thread has ONE 16-byte load in flight: the first-level kernels
 * ran at 3.6 TB/s where the copy rate is 5. */
template <bool LEVEL0, int PAIRS>
__device__ static inline void part_preload2(const mdb_level_args &a, const mdb_tile_desc &td, ulonglong2 pre[PAIRS])
{
	const uint64_t *const src = (LEVEL0 ? reinterpret_cast<const uint64_t *>(a.keys) : a.hv_in) + td.start;
#pragma unroll
	for (int r = 0; r < PAIRS; r++) {
		if (LEVEL0) {	/* a key column is read once: non-temporal, so that it does not push the regions' half-written lines out of the L2s */
			typedef unsigned long long ull2_nt __attribute__((ext_vector_type(2)));
			const ull2_nt v = __builtin_nontemporal_load(reinterpret_cast<const ull2_nt *>(src + 2u * ((uint32_t)r * PART_THREADS + threadIdx.x)));
			pre[r] = make_ulonglong2(v.x, v.y);
		} else {
			pre[r] = *reinterpret_cast<const ulonglong2 *>(src + 2u * ((uint32_t)r * PART_THREADS + threadIdx.x));
		}
	}
}

/* 4-byte words (the right side of the narrow form beyond level 0): the four adjacent elements 4p .. 4p+3 relative to
 * the 4-aligned base of the tile, one 16-byte access when all belong to the tile */
__device__ static inline void part_load4_w32(const mdb_level_args &a, const mdb_tile_desc &td, uint32_t p, uint32_t hv[4], bool valid[4],
					      const uint4 *pre = nullptr /* the four words, already loaded (full aligned tiles) */)
{
	const uint32_t lead = td.start & 3u;
	const uint32_t *src = reinterpret_cast<const uint32_t *>(a.hv_in) + (uint64_t)(td.start - lead) + 4 * (uint64_t)p;
	const uint32_t e0 = 4 * p, end = lead + td.len;
	if (pre || (e0 >= lead && e0 + 3 < end)) {
		const uint4 q = pre ? *pre : *reinterpret_cast<const uint4 *>(src);
		hv[0] = q.x;
		hv[1] = q.y;
		hv[2] = q.z;
		hv[3] = q.w;
		valid[0] = valid[1] = valid[2] = valid[3] = true;
	} else {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			valid[k] = e0 + k >= lead && e0 + k < end;
			hv[k] = valid[k] ? src[k] : 0u;
		}
	}
	if (a.skip_zero) {
#pragma unroll
		for (int k = 0; k < 4; k++)
			valid[k] = valid[k] && hv[k] != 0u;
	}
}

template <bool LEVEL0, bool RAW = false>
__global__ __launch_bounds__(PART_THREADS) void k_part_hist(mdb_level_args a)
{
	__shared__ uint32_t s_h[PART_MAX_R];
	const mdb_tile_desc td = part_get_tile(a, part_tile_of_block());
	if (td.len == 0)
		return;
	for (uint32_t d = threadIdx.x; d < a.R; d += PART_THREADS)
		s_h[d] = 0;
	__syncthreads();
	const bool full = td.len == MDB_TILE && !(td.start & 1u) && !(LEVEL0 && a.keys32);	/* (uniform) the tile's loads are issued together */
	ulonglong2 pre[PART_ITEMS / 2];
	if (full)
		part_preload2<LEVEL0, PART_ITEMS / 2>(a, td, pre);
#pragma unroll
	for (int r = 0; r < PART_ITEMS / 2; r++) {
		uint64_t hv[2];
		uint32_t rid[2];
		bool valid[2];
		if (full)
			part_load2<LEVEL0, false, RAW>(a, td, (uint32_t)r * PART_THREADS + threadIdx.x, hv, rid, valid, nullptr, &pre[r]);
		else
			part_load2<LEVEL0, false, RAW>(a, td, (uint32_t)r * PART_THREADS + threadIdx.x, hv, rid, valid);
		if (LEVEL0 && a.R <= PART_FEW_DIGITS) {	/* few destinations: one add per wave and digit (see k_part_scatter) */
			for (int k = 0; k < 2; k++) {
				const uint32_t dg = valid[k] ? part_digit(a, hv[k]) : PART_INVALID;
				for (uint32_t d = 0; d < a.R; d++) {
					const uint64_t m = __ballot(dg == d);
					if (m && mdb_lane() == (uint32_t)__ffsll((long long)m) - 1u)
						atomicAdd(&s_h[d], (uint32_t)__popcll(m));
				}
			}
			continue;
		}
		if (valid[0])
			atomicAdd(&s_h[part_digit(a, hv[0])], 1u);
		if (valid[1])
			atomicAdd(&s_h[part_digit(a, hv[1])], 1u);
	}
	__syncthreads();
	for (uint32_t d = threadIdx.x; d < a.R; d += PART_THREADS)
		a.hist[(uint64_t)td.hbase + (uint64_t)d * td.nt] = s_h[d];
}

/*
 * Scatter: the tile is ranked with LDS atomics (one ds_add_rtn per key returns the key's rank inside
 * its digit), staged in LDS sorted by digit, and written out as one contiguous run per digit.
 * Order inside a digit is arrival order, i.e. unspecified: no consumer depends on it (group order is
 * restored from row ids with atomicMin).  STABLE = true instead ranks with wave-level ballot
 * matching and keeps input order inside every digit; rocprofv3 showed that form issue-bound (SIMD
 * ~100 % busy at 2.3 TB/s vs 3.7 TB/s, profiles/r01/), so it is used only where order matters: the
 * right side of the materialising join, whose per-key row-id lists must come out ascending.
 *
 * LDS: hv 32 KiB (+ rid 16 KiB when row ids travel) + 3 KiB of per-digit words => 4 (3) workgroups/CU
 * (+16 KiB for STABLE).
 */
/* The rows of one thread in a FULL tile of the compact narrow form, no NULL bitmap: straight-line code, no per-row branch
 * (the generic loop below spends ~25 scalar branches per pair of rows on conditions that are the same for the whole launch).
 * MODE 1 (the one in use): min-max pruning, the left table - rows outside [range_lo, range_hi] are dropped (a key outside the
 * window is outside the range: nothing to report); 0: plain; 2: the right table of a pruned join - the smallest / largest
 * key - window base is recorded.  -> a key outside the window was seen (modes 0 and 2). */
template <bool W32v, int MODE, typename W, int ITEMS = PART_ITEMS>
__device__ static inline bool part_cf_rows(const mdb_level_args &a, const ulonglong2 *pre, uint32_t row0, W *hv, uint32_t *dig, uint64_t range_lo,
					   uint64_t range_hi, uint32_t &seen_min, uint32_t &seen_max)
{
	bool any_bad = false;
	const uint32_t dshift = a.shift - (W32v ? 0u : 32u);	/* the digit's place inside the 32-bit hash */
#pragma unroll
	for (int r = 0; r < ITEMS / 2; r++) {
#pragma unroll
		for (int e = 0; e < 2; e++) {
			const uint64_t key = (e ? pre[r].y : pre[r].x) - (uint64_t)a.narrow_base;
			bool ok = true;
			if (MODE == 1)
				ok = key >= range_lo && key <= range_hi;
			else
				any_bad = any_bad || (key >> a.narrow_kbits);
			if (MODE == 2) {
				seen_min = min(seen_min, (uint32_t)key);
				seen_max = max(seen_max, (uint32_t)key);
			}
			const uint32_t h = mdb_mixk((uint32_t)key, a.narrow_kbits) << (32u - a.narrow_kbits);
			const uint32_t rid = row0 + 2u * (uint32_t)r * PART_THREADS + (uint32_t)e;
			hv[2 * r + e] = W32v ? (W)h : (W)(((uint64_t)h << 32) | rid);
			dig[2 * r + e] = ok ? ((h >> dshift) & (a.R - 1u)) : PART_INVALID;
		}
	}
	return any_bad;
}

/* One instance of the scatter kernel = one of these structs: what the instance knows at compile time.
 *   LEVEL0  reads the key column (hashes, drops NULLs); otherwise the previous level's words through tile descriptors
 *   HAS_RID row ids travel in an array of their own (the 64-bit form's left side); STABLE keeps the input order inside a digit
 *   FAST    histogram-free: fixed-capacity regions + cursors (otherwise exact offsets from a histogram pass)
 *   RAW     the input words are ready-made sort keys (ordering of group records); W32: 4-byte words; OUT16: 2-byte words out
 *   INV     partition by destination GPU: what is written is the KEY (and the key-range tests are compiled in)
 *   FILT    second level with the semi-join bitmap; CF: first level of the compact narrow form over an int64 column
 * The struct's name is what a profiler shows as the kernel's template argument. */
struct pf_base {
	static constexpr bool LEVEL0 = false, HAS_RID = false, STABLE = false, FAST = false, RAW = false, W32 = false, INV = false, FILT = false,
			      OUT16 = false, CF = false, R64 = false, MM64 = false, PAY = false;
	static constexpr uint32_t TMUL = 1;	/* tile = TMUL x MDB_TILE rows (a histogram-free pass that cuts its own tiles: large tables) */
};
struct pf_word_hist : pf_base {  };
struct pf_word_hist_raw : pf_base { static constexpr bool RAW = true; };
struct pf_word : pf_base { static constexpr bool FAST = true; };
struct pf_word_semi : pf_base { static constexpr bool FAST = true; static constexpr bool FILT = true; };
struct pf_word_w32 : pf_base { static constexpr bool FAST = true; static constexpr bool W32 = true; };
struct pf_word_w32_out16 : pf_base { static constexpr bool FAST = true; static constexpr bool W32 = true; static constexpr bool OUT16 = true; };
struct pf_word_raw : pf_base { static constexpr bool FAST = true; static constexpr bool RAW = true; };
struct pf_word_raw_w32 : pf_base { static constexpr bool FAST = true; static constexpr bool RAW = true; static constexpr bool W32 = true; };
struct pf_word_rid_hist : pf_base { static constexpr bool HAS_RID = true; };
struct pf_word_rid : pf_base { static constexpr bool HAS_RID = true; static constexpr bool FAST = true; };
struct pf_word_rid_stable_hist : pf_base { static constexpr bool HAS_RID = true; static constexpr bool STABLE = true; };
struct pf_key_hist : pf_base { static constexpr bool LEVEL0 = true; };
struct pf_key_hist_dest : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool INV = true; };
struct pf_key : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool FAST = true; };
struct pf_key_cf : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool FAST = true; static constexpr bool CF = true; };
struct pf_key_w32 : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool FAST = true; static constexpr bool W32 = true; };
struct pf_key_w32_cf : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool FAST = true; static constexpr bool W32 = true; static constexpr bool CF = true; };
struct pf_key_w32_out16 : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool FAST = true; static constexpr bool W32 = true; static constexpr bool OUT16 = true; };
struct pf_key_w32_out16_cf : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool FAST = true; static constexpr bool W32 = true; static constexpr bool OUT16 = true; static constexpr bool CF = true; };
struct pf_word_pay : pf_base { static constexpr bool FAST = true; static constexpr bool PAY = true; };	/* second level of a join that carries payload cells */
struct pf_key_cf_pay : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool FAST = true; static constexpr bool CF = true; static constexpr bool PAY = true; };
struct pf_key_rid_hist : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool HAS_RID = true; };
struct pf_key_rid_hist_dest : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool HAS_RID = true; static constexpr bool INV = true; };
struct pf_key_rid : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool HAS_RID = true; static constexpr bool FAST = true; };
struct pf_key_rid_stable_hist : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool HAS_RID = true; static constexpr bool STABLE = true; };
/* the same with tiles of 2 x MDB_TILE rows (tables of 2^25 rows and more: half the cursor atomics, runs twice as long - whole 32-byte sectors of
 * 2-byte words; 10^8 rows: the right table's pass 0.241 -> 0.222 ms, the ordering sort's first level 0.174 -> 0.155, same-box A/B.  Smaller tables
 * keep MDB_TILE: fewer tiles than workgroup slots leave CUs idle).  4 x MDB_TILE at PART_THREADS means 32 rows per thread, and those cost the
 * registers that keep every wave slot filled: the right table's pass in 16384-row tiles is <pf_key_w32_out16_cf_t4>, 1024 threads of 16 rows -
 * 0.232 -> 0.207 ms, same-box A/B; the same body with 512 threads of 32 rows (105 registers, half the wave slots) 0.236:
 * profiles/micro/right_pass_tile4/ab.txt) */
#ifndef PART_TMUL
#define PART_TMUL 2u
#endif
struct pf_key_cf_t2 : pf_key_cf { static constexpr uint32_t TMUL = PART_TMUL; };
struct pf_key_w32_out16_cf_t2 : pf_key_w32_out16_cf { static constexpr uint32_t TMUL = PART_TMUL; };
struct pf_word_raw_w32_t2 : pf_word_raw_w32 { static constexpr uint32_t TMUL = PART_TMUL; };
/* the pruned left table of a join known to be selective: a body of its own (part_sel_tile, after the generic kernel) */
struct pf_key_cf_sel : pf_key_cf {  };
struct pf_key_cf_sel_t2 : pf_key_cf_sel { static constexpr uint32_t TMUL = PART_TMUL; };
/* the right table of the one-level join in tiles of 4 x MDB_TILE rows, 1024 threads: a body of its own (after the selective first level) */
struct pf_key_w32_out16_cf_t4 : pf_key_w32_out16_cf { static constexpr uint32_t TMUL = 4u; };
/* min-max pruning in the 64-bit form: the right table's first level records its key range (mm64), the left table's drops the rows outside (r64) */
struct pf_key_mm64 : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool FAST = true; static constexpr bool MM64 = true; };
struct pf_key_rid_r64 : pf_base { static constexpr bool LEVEL0 = true; static constexpr bool HAS_RID = true; static constexpr bool FAST = true; static constexpr bool R64 = true; };

template <typename F /* one of the pf_* structs above */>
__global__ __launch_bounds__(PART_THREADS) void k_part_scatter(mdb_level_args a)
{
	constexpr bool LEVEL0 = F::LEVEL0, HAS_RID = F::HAS_RID, STABLE = F::STABLE, FAST = F::FAST, RAW = F::RAW, W32 = F::W32, INV = F::INV, FILT = F::FILT,
		       OUT16 = F::OUT16, CF = F::CF, R64 = F::R64, MM64 = F::MM64, PAY = F::PAY;
	static_assert(!PAY || (FAST && !W32 && !HAS_RID && !RAW && !INV && !FILT && (CF || !LEVEL0)),
		      "payload cells travel with the compact narrow form's 8-byte hash | row id words: its first level, or a second level over them");
	static_assert(!(R64 || MM64) || (LEVEL0 && FAST && !RAW && !INV && !W32 && !CF && !STABLE), "64-bit key range: first level of the 64-bit form only");
	static_assert(!CF || (LEVEL0 && FAST && !RAW && !INV && !HAS_RID && !STABLE), "compact-form instance: first level of the narrow join forms only");
	static_assert(!OUT16 || (W32 && !RAW), "2-byte words out: the 4-byte form only");
	static_assert(!FILT || (!LEVEL0 && !HAS_RID && !STABLE && FAST && !RAW && !W32 && !INV), "semi-join filter: second level of the narrow left side only");
	/* INV (destination partition for the exchange): what is staged and written is the KEY, not its hash - the digit is
	 * taken from the hash once, at load time, and found again at write-out from the staged position (the tile-local
	 * digit starts are in LDS anyway), instead of hashing back and forth */
	static_assert(!INV || (LEVEL0 && !STABLE && !FAST && !RAW && !W32), "INV: unordered exact level-0 form only");
	/* W32: the words staged and written are 4-byte hashes (narrow form, right side: level 0 reads 8-byte keys and
	 * writes 4-byte words, level 1 reads and writes 4-byte words); never with row ids */
	static_assert(!W32 || (!HAS_RID && !STABLE && FAST && !(LEVEL0 && RAW)), "4-byte words: unordered FAST form without row ids only");
	constexpr uint32_t TILE = MDB_TILE * F::TMUL;
	constexpr int ITEMS = (int)(PART_ITEMS * F::TMUL);
	static_assert(F::TMUL == 1 || (FAST && !STABLE && !HAS_RID && !INV && !FILT && !PAY && !R64 && !MM64), "larger tiles: histogram-free passes that cut their own tiles only");
	typedef typename std::conditional<W32, uint32_t, uint64_t>::type W;
	/* Row ids are staged through the SAME LDS as the hashes, after the hashes have been written out (unordered
	 * form only): 35 KiB instead of 51 KiB per workgroup = 4 instead of 3 workgroups per CU, worth ~25 % of the
	 * kernel's time (occupancy is what hides the HBM latency of the scattered runs) */
	constexpr bool RID_SHARES_LDS = HAS_RID && !STABLE;
	__shared__ W s_hv[TILE];
	__shared__ uint32_t s_rid_own[(HAS_RID && !RID_SHARES_LDS) ? TILE : 1];
	uint32_t *const s_rid = RID_SHARES_LDS ? reinterpret_cast<uint32_t *>(s_hv) : s_rid_own;
	__shared__ uint32_t s_cnt[PART_MAX_R];		/* per-digit counters, then tile-local digit starts */
	__shared__ int32_t s_delta[PART_MAX_R];	/* global start of the digit's run minus its tile-local start */
	__shared__ uint32_t s_wcnt[STABLE ? PART_WAVES * PART_MAX_R : 1];	/* STABLE: per-wave digit counts, then bases */
	__shared__ uint8_t s_ok[FAST ? PART_MAX_R : 1];			/* FAST: the digit's run fits its region */
	__shared__ uint32_t s_tmp[32];

	if (LEVEL0 && FAST && !RAW && !INV && !HAS_RID && a.minmax_final && blockIdx.x == 0 && threadIdx.x == 0) {
		a.minmax_final[0] = 0xFFFFFFFFu;
		a.minmax_final[1] = 0u;
	}
	const mdb_tile_desc td = part_get_tile<TILE>(a, part_tile_of_block());
	if (td.len == 0)
		return;
	const uint32_t R = a.R;
	const uint32_t wave = threadIdx.x >> 6, lane = mdb_lane();

	for (uint32_t d = threadIdx.x; d < R; d += PART_THREADS)
		s_cnt[d] = 0;
	if (STABLE)
		for (uint32_t i = threadIdx.x; i < PART_WAVES * PART_MAX_R; i += PART_THREADS)
			s_wcnt[i] = 0;
	/* min-max pruning: the other table's key range (left side) / what this launch sees (right side) */
	uint64_t range_lo = 0, range_hi = ~0ull;
	uint32_t seen_min = 0xFFFFFFFFu, seen_max = 0u;
	__shared__ uint32_t s_mm[2 * PART_WAVES];
	if (LEVEL0 && a.range_in) {
		range_lo = a.range_in[0];
		range_hi = a.range_in[1];
	}
	/* 64-bit form: the keys' order-preserving unsigned images (key ^ 2^63) */
	uint64_t seen_min64 = ~0ull, seen_max64 = 0ull, r64_lo = 0ull, r64_hi = ~0ull;
	uint64_t *const s_mm64 = reinterpret_cast<uint64_t *>(s_delta);	/* (2 x PART_WAVES words of a buffer that step 3 fills later) */
	if (R64 && a.range64_in) {	/* the other table's key range, left there by its own first level earlier on this stream */
		r64_lo = (uint64_t)a.range64_in[0] ^ 0x8000000000000000ull;
		r64_hi = (uint64_t)a.range64_in[1] ^ 0x8000000000000000ull;
	}
	/* the filter slice of this tile's first-level digit lives in the staging buffer until the rows are ranked (the
	 * barrier after the load separates its last read from the first staged word) */
	uint32_t *const s_flt = reinterpret_cast<uint32_t *>(s_hv);
	if (FILT) {
		const uint4 *src = reinterpret_cast<const uint4 *>(a.filter + (size_t)td.seg * a.filter_words);
		for (uint32_t w = threadIdx.x; w < a.filter_words / 4; w += PART_THREADS)
			reinterpret_cast<uint4 *>(s_flt)[w] = src[w];
		__syncthreads();
	}

	/* 1. load (coalesced).  STABLE: wave w owns the 512 consecutive keys [w*512, w*512+512), so that
	 *    (wave, round, lane) order is input order; otherwise consecutive threads, consecutive keys. */
	W hv[ITEMS];
	uint32_t rid[ITEMS];
	uint32_t dig[ITEMS];
	uint32_t rank[ITEMS];
	if (STABLE) {
#pragma unroll
		for (int r = 0; r < ITEMS; r++) {
			const uint32_t i = wave * PART_WAVE_SPAN + (uint32_t)r * MDB_WAVE + lane;
			bool valid = i < td.len;
			uint64_t h = 0;
			rid[r] = 0;
			if (valid)
				valid = part_load<LEVEL0>(a, td, i, &h, &rid[r]);
			hv[r] = (W)h;
			dig[r] = valid ? part_digit(a, hv[r]) : PART_INVALID;
		}
	} else if (W32 && RAW && a.fold64) {
		/* group records on their way into the 4-byte ordering sort: 8-byte words in, folded */
		const bool full = td.len == TILE && !(td.start & 1u);	/* (uniform) */
		ulonglong2 pre[ITEMS / 2];
		if (full)
			part_preload2<false, ITEMS / 2>(a, td, pre);
#pragma unroll
		for (int r = 0; r < ITEMS / 2; r++) {
			bool valid[2];
			uint64_t h2[2];
			if (full)
				part_load2<false, false, true>(a, td, (uint32_t)r * PART_THREADS + threadIdx.x, h2, &rid[2 * r], valid, nullptr, &pre[r]);
			else
				part_load2<false, false, true>(a, td, (uint32_t)r * PART_THREADS + threadIdx.x, h2, &rid[2 * r], valid);
#pragma unroll
			for (int k = 0; k < 2; k++) {
				hv[2 * r + k] = (W)((uint32_t)(h2[k] >> 32) | (uint32_t)h2[k]);
				dig[2 * r + k] = valid[k] ? part_digit(a, hv[2 * r + k]) : PART_INVALID;
			}
		}
	} else if (W32 && !LEVEL0) {
		const bool full = td.len == TILE && !(td.start & 3u);	/* (uniform) */
		uint4 pre[ITEMS / 4];
		if (full) {
			const uint32_t *const src = reinterpret_cast<const uint32_t *>(a.hv_in) + td.start;
#pragma unroll
			for (int r = 0; r < ITEMS / 4; r++)
				pre[r] = *reinterpret_cast<const uint4 *>(src + 4u * ((uint32_t)r * PART_THREADS + threadIdx.x));
		}
#pragma unroll
		for (int r = 0; r < ITEMS / 4; r++) {
			uint32_t h4[4];
			bool valid[4];
			if (full)
				part_load4_w32(a, td, (uint32_t)r * PART_THREADS + threadIdx.x, h4, valid, &pre[r]);
			else
				part_load4_w32(a, td, (uint32_t)r * PART_THREADS + threadIdx.x, h4, valid);
#pragma unroll
			for (int k = 0; k < 4; k++) {
				hv[4 * r + k] = (W)h4[k];
				rid[4 * r + k] = 0;
				dig[4 * r + k] = valid[k] ? part_digit(a, hv[4 * r + k]) : PART_INVALID;
			}
		}
	} else {
		constexpr bool PRE_OK = LEVEL0 || !HAS_RID;	/* (row-id arrays beyond the first level: the wide form keeps part_load2's own loads) */
		const bool full = PRE_OK && td.len == TILE && !(td.start & 1u) && !(LEVEL0 && !CF && a.keys32);	/* (uniform) */
		ulonglong2 pre[ITEMS / 2];
		if (full)
			part_preload2<LEVEL0, ITEMS / 2>(a, td, pre);
		/* (uniform) the pruned left table only: for the right table - with or without its key range recorded - the same
		 * straight-line code measured equal (0.247 ms) or slower (0.235 -> 0.258 ms) than the loop below */
		const bool straight = CF && !W32 && !PAY && full && !a.nullbits && a.range_in;
		if (straight)
			(void)part_cf_rows<W32, 1, W, ITEMS>(a, pre, td.start + 2u * threadIdx.x, hv, dig, range_lo, range_hi, seen_min, seen_max);
#pragma unroll
		for (int r = 0; r < ITEMS / 2 && !straight; r++) {
			bool valid[2];
			uint64_t h2[2];
			constexpr bool RANGE = LEVEL0 && FAST && !RAW && !INV && !HAS_RID;	/* (the narrow forms' first level) */
			uint64_t rel2[2] = { 0, 0 };
			/* (the key-range tests of the by-destination partition are compiled into its own instance only: as run-time
			 * branches they cost the join's first-level kernels 0.05 ms per 10^8 rows) */
			int64_t raw2[2] = { 0, 0 };
			if (full)
				part_load2<LEVEL0, HAS_RID, RAW, INV, INV, CF, !W32>(a, td, (uint32_t)r * PART_THREADS + threadIdx.x, h2, &rid[2 * r], valid,
										     RANGE ? rel2 : nullptr, &pre[r], (R64 || MM64) ? raw2 : nullptr);
			else
				part_load2<LEVEL0, HAS_RID, RAW, INV, INV, CF, !W32>(a, td, (uint32_t)r * PART_THREADS + threadIdx.x, h2, &rid[2 * r], valid,
										     RANGE ? rel2 : nullptr, nullptr, (R64 || MM64) ? raw2 : nullptr);
			if (R64 || MM64) {	/* (order-preserving unsigned images) */
				rel2[0] = (uint64_t)raw2[0] ^ 0x8000000000000000ull;
				rel2[1] = (uint64_t)raw2[1] ^ 0x8000000000000000ull;
			}
			if (R64) {
				valid[0] = valid[0] && rel2[0] >= r64_lo && rel2[0] <= r64_hi;
				valid[1] = valid[1] && rel2[1] >= r64_lo && rel2[1] <= r64_hi;
			}
			if (MM64) {
#pragma unroll
				for (int k = 0; k < 2; k++)
					if (valid[k]) {
						seen_min64 = rel2[k] < seen_min64 ? rel2[k] : seen_min64;
						seen_max64 = rel2[k] > seen_max64 ? rel2[k] : seen_max64;
					}
			}
			if (RANGE && a.range_in) {		/* (uniform) */
				valid[0] = valid[0] && rel2[0] >= range_lo && rel2[0] <= range_hi;
				valid[1] = valid[1] && rel2[1] >= range_lo && rel2[1] <= range_hi;
			}
			if (RANGE && a.minmax_out) {
#pragma unroll
				for (int k = 0; k < 2; k++)
					if (valid[k]) {		/* (a valid row of a narrow form: rel < 2^32) */
						seen_min = rel2[k] < seen_min ? (uint32_t)rel2[k] : seen_min;
						seen_max = rel2[k] > seen_max ? (uint32_t)rel2[k] : seen_max;
					}
			}
			if (FILT) {		/* (narrow words: hash32 in the upper half) */
#pragma unroll
				for (int k = 0; k < 2; k++) {
					const uint32_t bit = ((uint32_t)(h2[k] >> 32) >> a.filter_shift) & (a.filter_words * 32u - 1u);
					valid[k] = valid[k] && ((s_flt[bit >> 5] >> (bit & 31u)) & 1u);
				}
			}
			hv[2 * r] = (W)h2[0];		/* W32 at level 0: the narrow word holds the hash in both halves */
			hv[2 * r + 1] = (W)h2[1];
			dig[2 * r] = valid[0] ? part_digit<CF>(a, INV ? (W)mdb_fmix64(h2[0]) : hv[2 * r]) : PART_INVALID;
			dig[2 * r + 1] = valid[1] ? part_digit<CF>(a, INV ? (W)mdb_fmix64(h2[1]) : hv[2 * r + 1]) : PART_INVALID;
		}
	}
	if (LEVEL0 && FAST && !RAW && !INV && !HAS_RID && a.minmax_out) {
#pragma unroll
		for (int o = MDB_WAVE / 2; o > 0; o >>= 1) {
			const uint32_t omin = (uint32_t)__shfl_xor((int)seen_min, o, MDB_WAVE), omax = (uint32_t)__shfl_xor((int)seen_max, o, MDB_WAVE);
			seen_min = omin < seen_min ? omin : seen_min;
			seen_max = omax > seen_max ? omax : seen_max;
		}
		if (lane == 0) {
			s_mm[2 * wave] = seen_min;
			s_mm[2 * wave + 1] = seen_max;
		}
	}
	if (MM64) {
#pragma unroll
		for (int o = MDB_WAVE / 2; o > 0; o >>= 1) {
			const uint64_t omin = ((uint64_t)(uint32_t)__shfl_xor((int)(seen_min64 >> 32), o, MDB_WAVE) << 32) | (uint32_t)__shfl_xor((int)seen_min64, o, MDB_WAVE);
			const uint64_t omax = ((uint64_t)(uint32_t)__shfl_xor((int)(seen_max64 >> 32), o, MDB_WAVE) << 32) | (uint32_t)__shfl_xor((int)seen_max64, o, MDB_WAVE);
			seen_min64 = omin < seen_min64 ? omin : seen_min64;
			seen_max64 = omax > seen_max64 ? omax : seen_max64;
		}
		if (lane == 0) {
			s_mm64[2 * wave] = seen_min64;
			s_mm64[2 * wave + 1] = seen_max64;
		}
	}
	__syncthreads();
	if (MM64 && threadIdx.x == 0) {
		uint64_t mn = ~0ull, mx = 0ull;
#pragma unroll
		for (int w = 0; w < PART_WAVES; w++) {
			mn = s_mm64[2 * w] < mn ? s_mm64[2 * w] : mn;
			mx = s_mm64[2 * w + 1] > mx ? s_mm64[2 * w + 1] : mx;
		}
		const uint32_t t = part_tile_of_block();
		a.minmax64_out[2 * t] = mn;
		a.minmax64_out[2 * t + 1] = ~mx;	/* (stored inverted) */
	}
	if (LEVEL0 && FAST && !RAW && !INV && !HAS_RID && a.minmax_out && threadIdx.x == 0) {
		/* one pair of plain stores per tile, reduced by k_part_minmax_reduce: atomics on two words from every wave of every
		 * tile (2 x 10^5 of them on the same address) cost 4 ms, coherent loads of "the best so far" 0.2 ms */
		uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
		for (int w = 0; w < PART_WAVES; w++) {
			mn = s_mm[2 * w] < mn ? s_mm[2 * w] : mn;
			mx = s_mm[2 * w + 1] > mx ? s_mm[2 * w + 1] : mx;
		}
		const uint32_t t = part_tile_of_block();
		a.minmax_out[2 * t] = mn;
		a.minmax_out[2 * t + 1] = ~mx;		/* (stored inverted) */
	}

	/* 2. rank inside the digit */
	if (STABLE) {
		/* lanes with the same digit find each other with `mbits` ballots; the lowest such lane bumps
		 * the wave-private LDS counter: rank = keys of the digit earlier in this wave's span */
		volatile uint32_t *wc = &s_wcnt[wave * PART_MAX_R];
		const uint64_t lt = mdb_lanemask_lt();
#pragma unroll
		for (int r = 0; r < ITEMS; r++) {
			const bool valid = dig[r] != PART_INVALID;
			const uint32_t d = dig[r];
			uint64_t peers = __ballot(valid);
			for (uint32_t b = 0; b < a.mbits; b++) {
				const bool bit = (d >> b) & 1u;
				const uint64_t m = __ballot(valid && bit);
				peers &= bit ? m : ~m;
			}
			const uint32_t before = (uint32_t)__popcll(peers & lt);
			const uint32_t cnt = (uint32_t)__popcll(peers);
			uint32_t prev = 0;
			if (valid)
				prev = wc[d];
			if (valid && before == 0)
				wc[d] = prev + cnt;
			rank[r] = prev + before;
			__builtin_amdgcn_wave_barrier();
		}
		__syncthreads();
		/* per digit: per-wave counts -> per-wave bases, digit total */
		if (threadIdx.x < R) {
			uint32_t run = 0;
#pragma unroll
			for (int w = 0; w < PART_WAVES; w++) {
				const uint32_t t = s_wcnt[w * PART_MAX_R + threadIdx.x];
				s_wcnt[w * PART_MAX_R + threadIdx.x] = run;
				run += t;
			}
			s_cnt[threadIdx.x] = run;
		}
	} else if (INV && R <= PART_FEW_DIGITS) {
		/* 1, 2, 4 destination GPUs: a wave's 64 keys would meet on one or two LDS words (32- to 64-way serialisation of the
		 * returning atomics: the two by-destination kernels took 1.7 ms per 2 x 10^8 keys at one destination).  The lanes of
		 * a digit find each other with one ballot per digit; the lowest of them takes the wave's share of the counter */
		const uint64_t lt = mdb_lanemask_lt();
#pragma unroll
		for (int r = 0; r < ITEMS; r++) {
			rank[r] = 0u;
			for (uint32_t d = 0; d < R; d++) {
				const uint64_t m = __ballot(dig[r] == d);
				if (!m)
					continue;
				const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
				uint32_t base = 0;
				if (lane == leader)
					base = atomicAdd(&s_cnt[d], (uint32_t)__popcll(m));
				base = __shfl(base, (int)leader, MDB_WAVE);
				if (dig[r] == d)
					rank[r] = base + (uint32_t)__popcll(m & lt);
			}
		}
	} else {
		/* one returning LDS atomic per key; order inside a digit = arrival order (unspecified) */
#pragma unroll
		for (int r = 0; r < ITEMS; r++)
			rank[r] = dig[r] != PART_INVALID ? atomicAdd(&s_cnt[dig[r]], 1u) : 0u;
	}
	__syncthreads();

	/* 3. digit totals -> tile-local starts; remember where each digit's run begins globally */
	const uint32_t total_d = threadIdx.x < R ? s_cnt[threadIdx.x] : 0u;
	uint32_t tile_total;
	const uint32_t off_d = mdb_block_excl_scan(total_d, s_tmp, &tile_total);
	uint32_t fast_base = 0, fast_child = 0;
	if (threadIdx.x < R) {
		s_cnt[threadIdx.x] = off_d;
		if (FAST) {
			/* no histogram pass: reserve the run's place in the child's fixed-capacity region with one
			 * global atomic per (tile, digit).  The returned base is only needed for the write-out, so
			 * the atomic's round trip overlaps the LDS staging below. */
			/* first level: 8 sub-regions per digit, picked by blockIdx % 8 (= the XCD under round-robin
			 * dispatch, so an XCD's partial lines meet in its own L2) keep the contention per cursor low */
			fast_child = a.nsub ? threadIdx.x * a.nsub + (blockIdx.x % a.nsub) : td.seg * R + threadIdx.x;
			/* first-level cursors are laid out sub-major (cursor[sub * R + digit]): the 256 atomics of one tile
			 * fall into 8 consecutive 128-byte lines that only this XCD's tiles touch, instead of 64 lines
			 * shared by every XCD (atomics on one line serialise) */
			const uint32_t cidx = a.nsub ? (blockIdx.x % a.nsub) * R + threadIdx.x : fast_child;
			fast_base = total_d ? atomicAdd(&a.cursor[cidx], total_d) : 0u;
		} else {
			s_delta[threadIdx.x] = (int32_t)(a.hist[(uint64_t)td.hbase + (uint64_t)threadIdx.x * td.nt] - off_d);
		}
	}
	__syncthreads();

	/* 4. stage sorted by digit */
#pragma unroll
	for (int r = 0; r < ITEMS; r++) {
		if (dig[r] != PART_INVALID) {
			uint32_t pos = s_cnt[dig[r]] + rank[r];
			if (STABLE)
				pos += s_wcnt[wave * PART_MAX_R + dig[r]];
			rank[r] = pos;		/* staged position (reused for the row ids below) */
			s_hv[pos] = hv[r];
			if (HAS_RID && !RID_SHARES_LDS)
				s_rid[pos] = rid[r];
		}
	}
	if (FAST && threadIdx.x < R) {
		const bool ok = fast_base + total_d <= a.cap;
		if (!ok)
			mdb_raise(a.status, MDB_ST_REGION_FULL);
		s_ok[threadIdx.x] = ok;
		s_delta[threadIdx.x] = (int32_t)(fast_child * a.cap + fast_base - off_d);
	}
	__syncthreads();

	/* 5. write out: consecutive threads write consecutive addresses inside each digit's run */
	uint32_t gpos[ITEMS];
#pragma unroll
	for (int k = 0; k < ITEMS; k++) {
		const uint32_t i = threadIdx.x + (uint32_t)k * PART_THREADS;
		gpos[k] = PART_INVALID;
		if (i >= tile_total)
			continue;
		const W h = s_hv[i];
		uint32_t d;
		if (INV) {	/* the last digit whose tile-local start is <= i (s_cnt[0] = 0) */
			uint32_t lo = 0, hi = R;
			while (hi - lo > 1) {
				const uint32_t mid = (lo + hi) >> 1;
				if (s_cnt[mid] <= i)
					lo = mid;
				else
					hi = mid;
			}
			d = lo;
		} else {
			d = part_digit<CF>(a, h);
		}
		if (FAST && !s_ok[d])
			continue;	/* overflowed child: the whole operator is re-run on the exact path */
		const uint32_t g = (uint32_t)((int32_t)i + s_delta[d]);
		gpos[k] = g;
		if (W32 && OUT16)
			reinterpret_cast<uint16_t *>(a.hv_out)[g] = (uint16_t)((uint32_t)h >> a.out16_shift);
		else if (W32)
			reinterpret_cast<uint32_t *>(a.hv_out)[g] = (uint32_t)h;
		else if (INV && a.inverse_out == 2) {
			if (((uint64_t)h + 0x80000000ull) >> 32)
				mdb_raise(a.status, MDB_ST_KEY_OUTSIDE);	/* the caller's promise (column statistics) does not hold: reported, not truncated */
			reinterpret_cast<int32_t *>(a.hv_out)[g] = (int32_t)(int64_t)h;	/* 4-byte wire format */
		}
		else if (INV)
			a.hv_out[g] = h;
		else if (a.inverse_out == 2)
			reinterpret_cast<int32_t *>(a.hv_out)[g] = (int32_t)(int64_t)mdb_fmix64_inv(h);
		else
			a.hv_out[g] = a.inverse_out ? mdb_fmix64_inv(h) : h;
		if (HAS_RID && !RID_SHARES_LDS)
			a.rid_out[g] = s_rid[i];
	}
	if (PAY) {
		/* the payload cells take the hashes' way through the same LDS buffer, one column after the other: read at the row's own
		 * index (consecutive threads, consecutive pairs of rows), staged at the row's rank, written beside its word */
		uint64_t *const s_pay = reinterpret_cast<uint64_t *>(s_hv);
		for (uint32_t c = 0; c < a.npay; c++) {	/* (uniform) */
			/* (element r of this thread = pair r / 2 of the tile, relative to its even-aligned base - part_load2's addressing) */
			const uint64_t base2 = (uint64_t)td.start - (td.start & 1u);
			uint64_t pv[ITEMS];
#pragma unroll
			for (int r = 0; r < ITEMS; r++)
				pv[r] = dig[r] != PART_INVALID ? a.pay_in[c][base2 + 2u * ((uint32_t)(r >> 1) * PART_THREADS + threadIdx.x) + (uint32_t)(r & 1)] : 0ull;
			__syncthreads();	/* every word of the previous round has been read */
#pragma unroll
			for (int r = 0; r < ITEMS; r++)
				if (dig[r] != PART_INVALID)
					s_pay[rank[r]] = pv[r];
			__syncthreads();
#pragma unroll
			for (int k = 0; k < ITEMS; k++)
				if (gpos[k] != PART_INVALID)
					a.pay_out[c][gpos[k]] = s_pay[threadIdx.x + (uint32_t)k * PART_THREADS];
		}
	}
	if (RID_SHARES_LDS) {
		__syncthreads();	/* every hash has been read: the buffer now takes the row ids */
#pragma unroll
		for (int r = 0; r < ITEMS; r++)
			if (dig[r] != PART_INVALID)
				s_rid[rank[r]] = rid[r];
		__syncthreads();
#pragma unroll
		for (int k = 0; k < ITEMS; k++)
			if (gpos[k] != PART_INVALID)
				a.rid_out[gpos[k]] = s_rid[threadIdx.x + (uint32_t)k * PART_THREADS];
	}
}

/* ---- selective first level: the pruned left table (compact narrow form, no NULL bitmap) of a join in which few rows survive ------
 *
 * The generic body above is sized for a tile whose every row survives: a staging buffer of TILE words and four per-row register
 * arrays that stay live across its barriers - 70 KiB of LDS and 90 registers in the 8192-row form, two workgroups per CU.  Where the
 * right table's key range keeps one left row in 16 (the benchmark's variant D) the pass is a streaming read, and what hides a stream's
 * HBM latency is residency.  Here a row is tested as its key arrives; only a survivor is hashed, ranked in its digit (returning LDS
 * atomic) and appended to a list of PART_SEL_CAP entries - its word, its digit and its rank.  After one cursor atomic per non-empty
 * digit every entry goes straight to its place in its region (no digit scan: the rank is the offset inside the run; no staging by
 * digit: the runs average under two words).  28 KiB of LDS: four workgroups per CU, as the right table's pass has.
 *
 * Same tiles, grid, words, regions, cursors and overflow flag as the generic body.  A tile with more survivors than the list holds
 * is redone in rounds of PART_SEL_CAP rows, which cannot overflow it, with a flush after each - exact for any tile; so are partial
 * tiles and a column that starts 8 bytes off a 16-byte boundary (every 16-byte load is aligned: positions count from the aligned
 * address below the column's first key). */
#define PART_SEL_CAP 2048u
static_assert(MDB_TILE % PART_SEL_CAP == 0 && PART_SEL_CAP % (2u * PART_THREADS) == 0, "selective first level: rounds of whole pairs per thread");

struct part_sel_lds {
	uint64_t word[PART_SEL_CAP];
	uint32_t meta[PART_SEL_CAP];		/* digit << 16 | rank inside the digit */
	uint32_t cnt[PART_MAX_R];
	uint32_t base[PART_MAX_R];		/* where the digit's run begins in hv_out (PART_INVALID: its region is full) */
	uint32_t n;				/* survivors so far (may pass PART_SEL_CAP: the entries beyond are not kept) */
};

/* a survivor into its slot of the list: hashed, ranked in its digit */
__device__ static inline void part_sel_append(const mdb_level_args &a, part_sel_lds &s, uint32_t slot, uint64_t rel, uint32_t rid, uint32_t dshift)
{
	const uint32_t h = mdb_mixk((uint32_t)rel, a.narrow_kbits) << (32u - a.narrow_kbits);
	const uint32_t d = (h >> dshift) & (a.R - 1u);
	const uint32_t rank = atomicAdd(&s.cnt[d], 1u);
	s.word[slot] = ((uint64_t)h << 32) | rid;
	s.meta[slot] = (d << 16) | rank;
}

/* two adjacent rows (row ids rid, rid + 1): every lane of the wave calls - the wave's survivors take their slots with ONE atomic */
__device__ static inline void part_sel_pair(const mdb_level_args &a, part_sel_lds &s, uint64_t key0, uint64_t key1, uint32_t rid, bool in0, bool in1,
					    uint64_t range_lo, uint64_t range_hi, uint32_t dshift)
{
	const uint64_t rel0 = key0 - (uint64_t)a.narrow_base, rel1 = key1 - (uint64_t)a.narrow_base;
	const bool ok0 = in0 && rel0 >= range_lo && rel0 <= range_hi, ok1 = in1 && rel1 >= range_lo && rel1 <= range_hi;
	const uint64_t m0 = __ballot(ok0), m1 = __ballot(ok1);
	if (!(m0 | m1))
		return;		/* (uniform) */
	const uint32_t leader = (uint32_t)__ffsll((long long)(m0 | m1)) - 1u, n0 = (uint32_t)__popcll(m0);
	uint32_t first = 0;
	if (mdb_lane() == leader)
		first = atomicAdd(&s.n, n0 + (uint32_t)__popcll(m1));
	first = (uint32_t)__builtin_amdgcn_readlane((int)first, (int)leader);
	const uint64_t lt = mdb_lanemask_lt();
	const uint32_t slot0 = first + (uint32_t)__popcll(m0 & lt), slot1 = first + n0 + (uint32_t)__popcll(m1 & lt);
	if (ok0 && slot0 < PART_SEL_CAP)
		part_sel_append(a, s, slot0, rel0, rid, dshift);
	if (ok1 && slot1 < PART_SEL_CAP)
		part_sel_append(a, s, slot1, rel1, rid + 1u, dshift);
}

/* scan-free flush of the list's first n entries (called behind a barrier): reserve, write */
__device__ static inline void part_sel_flush(const mdb_level_args &a, part_sel_lds &s, uint32_t n)
{
	for (uint32_t d = threadIdx.x; d < a.R; d += PART_THREADS) {
		const uint32_t total = s.cnt[d];
		uint32_t base = PART_INVALID;
		if (total) {
			const uint32_t sub = blockIdx.x % a.nsub, child = d * a.nsub + sub;
			const uint32_t at = atomicAdd(&a.cursor[sub * a.R + d], total);	/* (sub-major cursors: see the generic body) */
			if (at + total <= a.cap)
				base = child * a.cap + at;
			else
				mdb_raise(a.status, MDB_ST_REGION_FULL);
		}
		s.base[d] = base;
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < n; i += PART_THREADS) {
		const uint32_t meta = s.meta[i], base = s.base[meta >> 16];
		if (base != PART_INVALID)
			a.hv_out[base + (meta & 0xFFFFu)] = s.word[i];
	}
}

template <uint32_t TMUL>
__device__ static inline void part_sel_tile(const mdb_level_args &a)
{
	constexpr uint32_t TILE = MDB_TILE * TMUL;
	constexpr int PAIRS = (int)(TILE / (2u * PART_THREADS));
	__shared__ part_sel_lds s;
	const uint32_t t = part_tile_of_block();
	if (t >= a.ntiles)
		return;
	/* positions count from the 16-byte aligned address at or below the first key: row id = position - lead */
	const uint32_t lead = (uint32_t)(((uintptr_t)a.keys >> 3) & 1u);
	const uint64_t *const src = reinterpret_cast<const uint64_t *>(a.keys) - lead;
	const uint64_t start = (uint64_t)t * TILE, end = (uint64_t)lead + a.n;
	const uint64_t range_lo = a.range_in[0], range_hi = a.range_in[1];
	const uint32_t dshift = a.shift - 32u;	/* the digit's place inside the 32-bit hash */
	const bool full = start >= lead && start + TILE <= end;	/* (uniform) */
	if (full) {
		ulonglong2 pre[PAIRS];
		typedef unsigned long long ull2_nt __attribute__((ext_vector_type(2)));
#pragma unroll
		for (int r = 0; r < PAIRS; r++) {	/* the tile's loads together (see part_preload2) */
			const ull2_nt v = __builtin_nontemporal_load(reinterpret_cast<const ull2_nt *>(src + start + 2u * ((uint32_t)r * PART_THREADS + threadIdx.x)));
			pre[r] = make_ulonglong2(v.x, v.y);
		}
		for (uint32_t d = threadIdx.x; d < a.R; d += PART_THREADS)
			s.cnt[d] = 0;
		if (threadIdx.x == 0)
			s.n = 0;
		__syncthreads();
		const uint32_t rid0 = (uint32_t)start - lead + 2u * threadIdx.x;
#pragma unroll
		for (int r = 0; r < PAIRS; r++) {
			part_sel_pair(a, s, pre[r].x, pre[r].y, rid0 + 2u * (uint32_t)r * PART_THREADS, true, true, range_lo, range_hi, dshift);
		}
		__syncthreads();
		const uint32_t n = s.n;
		if (n <= PART_SEL_CAP) {	/* (uniform) */
			part_sel_flush(a, s, n);
			return;
		}
		__syncthreads();	/* more survivors than the list holds: every thread has read s.n - the tile is redone in rounds */
	}
	for (uint32_t round = 0; round < TILE / PART_SEL_CAP; round++) {
		const uint64_t rstart = start + (uint64_t)round * PART_SEL_CAP;
		if (rstart >= end)
			break;		/* (uniform) */
		for (uint32_t d = threadIdx.x; d < a.R; d += PART_THREADS)
			s.cnt[d] = 0;
		if (threadIdx.x == 0)
			s.n = 0;
		__syncthreads();
#pragma unroll
		for (uint32_t q = 0; q < PART_SEL_CAP / (2u * PART_THREADS); q++) {
			const uint64_t p0 = rstart + 2u * (q * PART_THREADS + threadIdx.x);
			const bool in0 = p0 >= lead && p0 < end, in1 = p0 + 1u < end;
			uint64_t k0 = 0, k1 = 0;
			if (in0 && in1) {
				const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(src + p0);
				k0 = v.x;
				k1 = v.y;
			} else if (in0) {
				k0 = src[p0];
			} else if (in1) {
				k1 = src[p0 + 1u];
			}
			part_sel_pair(a, s, k0, k1, (uint32_t)p0 - lead, in0, in1, range_lo, range_hi, dshift);
		}
		__syncthreads();
		part_sel_flush(a, s, s.n);	/* (at most PART_SEL_CAP rows went in) */
		__syncthreads();		/* the list and the counters have been read */
	}
}

template <>
__global__ __launch_bounds__(PART_THREADS) void k_part_scatter<pf_key_cf_sel>(mdb_level_args a)
{
	part_sel_tile<1u>(a);
}

template <>
__global__ __launch_bounds__(PART_THREADS) void k_part_scatter<pf_key_cf_sel_t2>(mdb_level_args a)
{
	part_sel_tile<PART_TMUL>(a);
}

/* ---- the right table's first level in tiles of 16384 rows (compact narrow form over an int64 column, no NULL bitmap, 2-byte words out) --
 *
 * What bounds the right table's pass is its runs: with 512 digits a (tile, digit) run of an 8192-row tile is 16 two-byte words
 * that begin on any 2-byte boundary - most runs straddle two 32-byte sectors and fill neither.  A tile of 16384 rows makes a run 64 bytes and
 * halves the cursor atomics.  The generic body takes its thread count from PART_THREADS, and 32 rows per thread cost it its registers; here
 * PART_T4_THREADS = 1024 threads keep 16 rows each, and a row is its hash and its rank - the digit is found again from the hash, a bit per
 * row says whether it takes part: 64 KiB of staging + 5 KiB of per-digit words, two workgroups per CU = every wave slot.
 *
 * Same words, regions, cursors, status flags and per-tile (min, ~max) pairs as <pf_key_w32_out16_cf_t2>, for full and partial tiles: the steps
 * below carry the numbers of the generic body's steps they restate (1 load - with the minmax_final preset and the per-tile pair that follow it
 * there -, 2 rank, 3 scan and cursor atomic, 4 stage and MDB_ST_REGION_FULL, 5 write-out).  A change to the region / cursor protocol or to the
 * status flags is made there, in part_sel_flush and here. */
#define PART_T4_THREADS 1024
#define PART_T4_TILE (4u * MDB_TILE)
#define PART_T4_ITEMS ((int)(PART_T4_TILE / PART_T4_THREADS))
#define PART_T4_WAVES (PART_T4_THREADS / MDB_WAVE)
static_assert(PART_T4_ITEMS % 2 == 0 && PART_T4_ITEMS <= 32 && PART_MAX_R <= PART_T4_THREADS, "16384-row tiles: whole pairs per thread, one valid bit per row, a thread per digit");

template <>
__global__ __launch_bounds__(PART_T4_THREADS) void k_part_scatter<pf_key_w32_out16_cf_t4>(mdb_level_args a)
{
	constexpr uint32_t TILE = PART_T4_TILE;
	constexpr int ITEMS = PART_T4_ITEMS;
	__shared__ uint32_t s_hv[TILE];
	__shared__ uint32_t s_cnt[PART_MAX_R];		/* per-digit counters, then tile-local digit starts */
	__shared__ int32_t s_delta[PART_MAX_R];	/* global start of the digit's run minus its tile-local start */
	__shared__ uint8_t s_ok[PART_MAX_R];		/* the digit's run fits its region */
	__shared__ uint32_t s_tmp[32];
	__shared__ uint32_t s_mm[2 * PART_T4_WAVES];

	if (a.minmax_final && blockIdx.x == 0 && threadIdx.x == 0) {
		a.minmax_final[0] = 0xFFFFFFFFu;
		a.minmax_final[1] = 0u;
	}
	const uint32_t t = part_tile_of_block();
	const uint64_t start = (uint64_t)t * TILE;
	if (t >= a.ntiles || start >= a.n)
		return;
	const uint32_t len = (a.n - start) < TILE ? (uint32_t)(a.n - start) : TILE;
	const uint32_t R = a.R;
	const uint32_t wave = threadIdx.x >> 6, lane = mdb_lane();
	if (threadIdx.x < R)
		s_cnt[threadIdx.x] = 0;

	/* 1. load: the tile starts on an even row of a 16-byte aligned column; a full tile's loads are issued together (see part_preload2) */
	const uint64_t *const src = reinterpret_cast<const uint64_t *>(a.keys) + start;
	ulonglong2 pre[ITEMS / 2];
	uint32_t in = 0;	/* bit r: row r of this thread exists */
	if (len == TILE) {	/* (uniform) */
		typedef unsigned long long ull2_nt __attribute__((ext_vector_type(2)));
#pragma unroll
		for (int r = 0; r < ITEMS / 2; r++) {
			const ull2_nt v = __builtin_nontemporal_load(reinterpret_cast<const ull2_nt *>(src + 2u * ((uint32_t)r * PART_T4_THREADS + threadIdx.x)));
			pre[r] = make_ulonglong2(v.x, v.y);
		}
		in = ITEMS == 32 ? 0xFFFFFFFFu : (1u << (ITEMS & 31)) - 1u;
	} else {
#pragma unroll
		for (int r = 0; r < ITEMS / 2; r++) {
			const uint32_t e0 = 2u * ((uint32_t)r * PART_T4_THREADS + threadIdx.x);
			pre[r] = make_ulonglong2(0ull, 0ull);
			if (e0 + 1u < len) {
				pre[r] = *reinterpret_cast<const ulonglong2 *>(src + e0);
				in |= 3u << (2 * r);
			} else if (e0 < len) {
				pre[r].x = src[e0];
				in |= 1u << (2 * r);
			}
		}
	}
	uint64_t range_lo = 0, range_hi = ~0ull;
	if (a.range_in) {
		range_lo = a.range_in[0];
		range_hi = a.range_in[1];
	}
	uint32_t hv[ITEMS];
	uint32_t seen_min = 0xFFFFFFFFu, seen_max = 0u;
	bool any_bad = false;
#pragma unroll
	for (int r = 0; r < ITEMS; r++) {
		const uint64_t rel = ((r & 1) ? pre[r / 2].y : pre[r / 2].x) - (uint64_t)a.narrow_base;
		bool valid = (in >> r) & 1u;
		any_bad = any_bad || (valid && (rel >> a.narrow_kbits));
		hv[r] = mdb_mixk((uint32_t)rel, a.narrow_kbits) << (32u - a.narrow_kbits);
		if (a.range_in)		/* (uniform) */
			valid = valid && rel >= range_lo && rel <= range_hi;
		if (a.minmax_out && valid) {	/* (a valid row of a narrow form: rel < 2^32) */
			seen_min = rel < seen_min ? (uint32_t)rel : seen_min;
			seen_max = rel > seen_max ? (uint32_t)rel : seen_max;
		}
		if (!valid)
			in &= ~(1u << r);
	}
	/* (with min-max pruning - range_in - a key outside the window is outside the other table's range: dropped, nothing to report) */
	if (any_bad && !a.range_in)
		mdb_raise(a.status, MDB_ST_KEY_OUTSIDE);
	if (a.minmax_out) {
#pragma unroll
		for (int o = MDB_WAVE / 2; o > 0; o >>= 1) {
			const uint32_t omin = (uint32_t)__shfl_xor((int)seen_min, o, MDB_WAVE), omax = (uint32_t)__shfl_xor((int)seen_max, o, MDB_WAVE);
			seen_min = omin < seen_min ? omin : seen_min;
			seen_max = omax > seen_max ? omax : seen_max;
		}
		if (lane == 0) {
			s_mm[2 * wave] = seen_min;
			s_mm[2 * wave + 1] = seen_max;
		}
	}
	__syncthreads();
	if (a.minmax_out && threadIdx.x == 0) {		/* one pair of plain stores per tile, reduced by k_part_minmax_reduce */
		uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
		for (int w = 0; w < PART_T4_WAVES; w++) {
			mn = s_mm[2 * w] < mn ? s_mm[2 * w] : mn;
			mx = s_mm[2 * w + 1] > mx ? s_mm[2 * w + 1] : mx;
		}
		a.minmax_out[2 * t] = mn;
		a.minmax_out[2 * t + 1] = ~mx;		/* (stored inverted) */
	}

	/* 2. rank inside the digit: one returning LDS atomic per row */
	uint32_t rank[ITEMS];
#pragma unroll
	for (int r = 0; r < ITEMS; r++)
		rank[r] = ((in >> r) & 1u) ? atomicAdd(&s_cnt[part_digit<true>(a, hv[r])], 1u) : 0u;
	__syncthreads();

	/* 3. digit totals -> tile-local starts; one cursor atomic per non-empty digit reserves the run's place in sub-region blockIdx % nsub
	 *    (sub-major cursors: see the generic body) */
	const uint32_t total_d = threadIdx.x < R ? s_cnt[threadIdx.x] : 0u;
	uint32_t tile_total;
	const uint32_t off_d = mdb_block_excl_scan(total_d, s_tmp, &tile_total);
	uint32_t fast_base = 0;
	const uint32_t sub = blockIdx.x % a.nsub;
	if (threadIdx.x < R) {
		s_cnt[threadIdx.x] = off_d;
		fast_base = total_d ? atomicAdd(&a.cursor[sub * R + threadIdx.x], total_d) : 0u;
	}
	__syncthreads();

	/* 4. stage sorted by digit */
#pragma unroll
	for (int r = 0; r < ITEMS; r++)
		if ((in >> r) & 1u)
			s_hv[s_cnt[part_digit<true>(a, hv[r])] + rank[r]] = hv[r];
	if (threadIdx.x < R) {
		const bool ok = fast_base + total_d <= a.cap;
		if (!ok)
			mdb_raise(a.status, MDB_ST_REGION_FULL);
		s_ok[threadIdx.x] = ok;
		s_delta[threadIdx.x] = (int32_t)((threadIdx.x * a.nsub + sub) * a.cap + fast_base - off_d);
	}
	__syncthreads();

	/* 5. write out: consecutive threads write consecutive 2-byte words inside each digit's run */
	uint16_t *const out = reinterpret_cast<uint16_t *>(a.hv_out);
#pragma unroll
	for (int k = 0; k < ITEMS; k++) {
		const uint32_t i = threadIdx.x + (uint32_t)k * PART_T4_THREADS;
		if (i >= tile_total)
			continue;
		const uint32_t h = s_hv[i];
		const uint32_t d = part_digit<true>(a, h);
		if (!s_ok[d])
			continue;	/* overflowed child: the whole operator is re-run on the exact path */
		out[(uint32_t)((int32_t)i + s_delta[d])] = (uint16_t)(h >> a.out16_shift);
	}
}

/* ---- segment bookkeeping between levels -------------------------------------------------------
 *
 * After a level's scan, child segment q = (parent p, digit d) starts at scanned[tb[p]*R + d*nt_p].
 * k_part_children writes child starts (S*R + 1 entries, last = total) and each child's tile count
 * (S*R + 1 entries, last = 0; exclusive-scanned afterwards into the child tile bases).
 */
__global__ void k_part_children(const uint32_t *__restrict__ scanned, const uint32_t *__restrict__ tb, uint32_t S, uint32_t R,
				uint32_t *__restrict__ child_start, uint32_t *__restrict__ child_ntiles)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t nq = S * R;
	if (q > nq)
		return;
	auto start_of = [&](uint32_t qq) -> uint32_t {
		if (qq >= nq)
			return scanned[(uint64_t)tb[S] * R];	/* == grand total */
		const uint32_t p = qq / R, d = qq % R;
		const uint32_t ntp = tb[p + 1] - tb[p];
		return scanned[(uint64_t)tb[p] * R + (uint64_t)d * ntp];
	};
	const uint32_t s0 = start_of(q);
	child_start[q] = s0;
	if (q == nq) {
		child_ntiles[q] = 0;
	} else {
		const uint32_t s1 = start_of(q + 1);
		/* tiles are cut at multiples of MDB_TILE from the segment's even-aligned base, so every tile but
		 * the first starts on an even element (16-byte loads) */
		child_ntiles[q] = s1 > s0 ? (s1 - (s0 & ~1u) + MDB_TILE - 1) / MDB_TILE : 0;
	}
}

/* tile descriptors of a level >= 1 from its segments (seg_start, tile bases tb), one thread per tile */
__global__ void k_part_build_tiles(const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ tb, uint32_t S, uint32_t R,
				   mdb_tile_desc *__restrict__ tiles, uint32_t max_tiles)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= max_tiles)
		return;
	mdb_tile_desc d;
	d.start = d.len = d.hbase = d.nt = d.seg = 0;
	if (t < tb[S]) {
		/* largest p with tb[p] <= t  (tb is non-decreasing, tb[S] > t) */
		uint32_t lo = 0, hi = S;
		while (hi - lo > 1) {
			const uint32_t mid = (lo + hi) >> 1;
			if (tb[mid] <= t)
				lo = mid;
			else
				hi = mid;
		}
		const uint32_t p = lo, tl = t - tb[p];
		const uint32_t seg0 = seg_start[p], s1 = seg_start[p + 1];
		const uint32_t lo_abs = (seg0 & ~1u) + tl * MDB_TILE;
		const uint32_t s0 = lo_abs > seg0 ? lo_abs : seg0;
		const uint32_t e0 = (lo_abs + MDB_TILE) < s1 ? (lo_abs + MDB_TILE) : s1;
		d.start = s0;
		d.len = e0 - s0;
		d.nt = tb[p + 1] - tb[p];
		d.hbase = tb[p] * R + tl;
		d.seg = p;
	}
	tiles[t] = d;
}

/* ---- histogram-free FIRST level: regions (digit, sub) of fixed capacity with atomic cursors -------------
 * region r = digit * nsub + sub lives at [r * cap, r * cap + min(cursor[r], cap)) and belongs to parent
 * partition r / nsub.  The next level's tiles are cut from the regions. */
/* FAST first level: tiles per region (a region = the filled part of a fixed-capacity sub-region) and their
 * exclusive scan, in one single-workgroup launch (there are only R * PART_NSUB + 1 entries). */
/* cursor of region r = digit * nsub + sub (sub-major cursor layout, see k_part_scatter) */
__device__ static inline uint32_t part_region_cursor(const uint32_t *cursor, uint32_t r, uint32_t nreg, uint32_t nsub)
{
	return cursor[(r % nsub) * (nreg / nsub) + r / nsub];
}

__global__ __launch_bounds__(1024) void k_part_region_tiles_scan(const uint32_t *__restrict__ cursor, uint32_t nreg, uint32_t cap,
								 uint32_t nsub, uint32_t *__restrict__ tb)
{
	__shared__ uint32_t s_tmp[32];
	uint32_t carry = 0;
	for (uint32_t base = 0; base <= nreg; base += 1024) {
		const uint32_t r = base + threadIdx.x;
		uint32_t c = 0;
		if (r < nreg) {
			c = part_region_cursor(cursor, r, nreg, nsub);
			c = c < cap ? c : cap;
		}
		const uint32_t nt = (c + MDB_TILE - 1) / MDB_TILE;
		uint32_t total;
		const uint32_t ex = mdb_block_excl_scan(nt, s_tmp, &total);
		if (r <= nreg)
			tb[r] = carry + ex;
		carry += total;
	}
}

__global__ void k_part_build_tiles_regions(const uint32_t *__restrict__ cursor, const uint32_t *__restrict__ tb, uint32_t nreg,
					   uint32_t cap, uint32_t nsub, mdb_tile_desc *__restrict__ tiles, uint32_t max_tiles)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= max_tiles)
		return;
	mdb_tile_desc d;
	d.start = d.len = d.hbase = d.nt = d.seg = 0;
	if (t < tb[nreg]) {
		uint32_t lo = 0, hi = nreg;
		while (hi - lo > 1) {
			const uint32_t mid = (lo + hi) >> 1;
			if (tb[mid] <= t)
				lo = mid;
			else
				hi = mid;
		}
		const uint32_t r = lo, tl = t - tb[r];
		uint32_t c = part_region_cursor(cursor, r, nreg, nsub);
		c = c < cap ? c : cap;
		d.start = r * cap + tl * MDB_TILE;		/* cap is a multiple of 64: every tile starts 16-byte aligned */
		d.len = (c - tl * MDB_TILE) < MDB_TILE ? (c - tl * MDB_TILE) : MDB_TILE;
		d.seg = r / nsub;
	}
	tiles[t] = d;
}

__global__ void k_part_seg0(uint32_t *seg_start, uint32_t *tb, uint32_t n, uint32_t ntiles)
{
	if (threadIdx.x == 0 && blockIdx.x == 0) {
		seg_start[0] = 0;
		seg_start[1] = n;
		tb[0] = 0;
		tb[1] = ntiles;
	}
}

/* the same for the 64-bit form: per-tile pairs of order-preserving images -> [lo, hi] as signed keys (an empty table: lo > hi) */
__global__ __launch_bounds__(1024) void k_part_minmax64_reduce(const unsigned long long *__restrict__ tile_mm, uint32_t ntiles, long long *__restrict__ out)
{
	__shared__ unsigned long long s_mn[16], s_mx[16];
	unsigned long long mn = ~0ull, mx = 0ull;
	for (uint32_t t = threadIdx.x; t < ntiles; t += 1024) {
		const unsigned long long a = tile_mm[2 * t], b = ~tile_mm[2 * t + 1];
		mn = a < mn ? a : mn;
		mx = b > mx ? b : mx;
	}
	for (int o = 32; o > 0; o >>= 1) {
		const unsigned long long omn = ((unsigned long long)(uint32_t)__shfl_xor((int)(mn >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)mn, o, 64);
		const unsigned long long omx = ((unsigned long long)(uint32_t)__shfl_xor((int)(mx >> 32), o, 64) << 32) | (uint32_t)__shfl_xor((int)mx, o, 64);
		mn = omn < mn ? omn : mn;
		mx = omx > mx ? omx : mx;
	}
	if ((threadIdx.x & 63u) == 0) {
		s_mn[threadIdx.x >> 6] = mn;
		s_mx[threadIdx.x >> 6] = mx;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 16; w++) {
			mn = s_mn[w] < mn ? s_mn[w] : mn;
			mx = s_mx[w] > mx ? s_mx[w] : mx;
		}
		out[0] = (long long)(mn ^ 0x8000000000000000ull);	/* (no key at all: lo = INT64_MAX > hi = INT64_MIN - every left row is dropped) */
		out[1] = (long long)(mx ^ 0x8000000000000000ull);
	}
}

/* per-tile (min, max) pairs of the right table's first level -> the two words the left table's first level reads.  One workgroup takes ~10 us
 * for the 195 KB of a 10^8-row table (what one CU can pull), so MM_GROUPS of them share the pairs and meet in the two words with one atomic pair per
 * wave; the words are preset by the scatter kernel's first workgroup (mdb_level_args.minmax_final) */
#define MM_GROUPS 64u
#define MM_THREADS 256u
__global__ __launch_bounds__(MM_THREADS) void k_part_minmax_reduce(const uint32_t *__restrict__ tile_mm, uint32_t ntiles, uint32_t *__restrict__ out)
{
	uint32_t mn = 0xFFFFFFFFu, mx = 0u;
	/* two pairs per 16-byte load, a workgroup's loads issued together where they are few */
	const uint4 *const mm2 = reinterpret_cast<const uint4 *>(tile_mm);
	const uint32_t n2 = ntiles / 2u;
	for (uint32_t t0 = blockIdx.x * MM_THREADS; t0 < n2; t0 += 4u * MM_GROUPS * MM_THREADS) {
		uint4 q[4];
#pragma unroll
		for (uint32_t u = 0; u < 4u; u++) {
			const uint32_t t = t0 + u * MM_GROUPS * MM_THREADS + threadIdx.x;
			q[u] = t < n2 ? mm2[t] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
		}
#pragma unroll
		for (uint32_t u = 0; u < 4u; u++) {
			mn = min(mn, min(q[u].x, q[u].z));
			mx = max(mx, max(~q[u].y, ~q[u].w));
		}
	}
	if ((ntiles & 1u) && blockIdx.x == 0 && threadIdx.x == 0) {
		mn = min(mn, tile_mm[2u * (ntiles - 1u)]);
		mx = max(mx, ~tile_mm[2u * (ntiles - 1u) + 1u]);
	}
#pragma unroll
	for (int o = MDB_WAVE / 2; o > 0; o >>= 1) {
		const uint32_t omin = (uint32_t)__shfl_xor((int)mn, o, MDB_WAVE), omax = (uint32_t)__shfl_xor((int)mx, o, MDB_WAVE);
		mn = omin < mn ? omin : mn;
		mx = omax > mx ? omax : mx;
	}
	if (mdb_lane() == 0 && mn <= mx) {	/* (a wave that saw no key has nothing to add) */
		atomicMin(&out[0], mn);
		atomicMax(&out[1], mx);
	}
}

/* ---- host orchestration ----------------------------------------------------------------------- */

struct part_carver {
	mdb_dev_ctx *ctx;
	bool dry;
	size_t bytes;
	bool failed;
	void *take(size_t b)
	{
		bytes += mdb_align_up(b ? b : 1);
		if (dry)
			return NULL;
		void *p = mdb_arena_take(ctx, b);
		if (!p)
			failed = true;
		return p;
	}
};

void mdb_choose_bits(uint64_t n, uint32_t target, int *bits1, int *bits2)
{
	uint64_t leaves = (n + target - 1) / target;
	int bits = 1;
	while (bits < 2 * MDB_MAX_RADIX_BITS && (1ull << bits) < leaves)
		bits++;
	if (bits <= 8) {
		*bits1 = bits;
		*bits2 = 0;
	} else if (bits <= 16) {
		*bits1 = 8;
		*bits2 = bits - 8;
	} else {
		*bits1 = 9;
		*bits2 = bits - 9;
	}
}

static inline uint32_t grid8(uint32_t tiles) { return ((tiles + 7u) / 8u) * 8u; }

#define PART_NSUB 8u		/* sub-regions per first-level digit in the FAST form */

/* capacity of one leaf region of the FAST form: 1.5 x the average leaf + 1024, rounded up to 64 */
static inline uint32_t part_fast_cap(uint64_t n, uint32_t nleaves)
{
	const uint64_t avg = (n + nleaves - 1) / nleaves;
	return (uint32_t)(((avg + avg / 2 + 1024) + 63) & ~63ull);
}

/* a request and what only the destination partition (mdb_dev_partition_by_dest_pruned) adds to one */
struct part_xrequest : mdb_part_request {
	uint32_t mode;		/* enum mdb_digit_mode of the first level */
	uint32_t n_dest;	/* MDB_DIGIT_MOD: its digits */
	bool inverse_out;	/* the last level writes the original keys (the inverse hash of the words) ... */
	bool keys32_out;	/* ... as 4-byte integers */
	uint64_t *final_hv_out;	/* the caller's buffers: the last level writes straight into them */
	uint32_t *final_rid_out;
	explicit part_xrequest(const mdb_part_request &rq) : mdb_part_request(rq), mode(MDB_DIGIT_RADIX), n_dest(0), inverse_out(false), keys32_out(false), final_hv_out(NULL), final_rid_out(NULL) {}
};

/* ---- the layout of a request: which levels, which form each takes, how large the regions are.  Pure - no context, no arena, no device */
struct part_layout {
	int nlevels;
	uint32_t R[2];		/* digits per level */
	uint32_t nleaves;	/* leaves of the whole partition */
	bool stop0;		/* first level only: the consumer walks the digits' sub-regions */
	bool out16;		/* ... whose words are the 16 hash bits below the digit */
	bool fast;		/* histogram-free last level (or only level, with stop0): one fixed-capacity region per leaf */
	bool fast0;		/* ... and first level: PART_NSUB fixed-capacity sub-regions per digit */
	bool fold32;		/* raw 8-byte records leave the first level as 4-byte words */
	bool w32;		/* 4-byte words from the first level's output on */
	int npay;		/* payload columns that travel with the words */
	uint32_t fast_cap;	/* words per leaf region */
	uint32_t cap0;		/* words per first-level sub-region */
	uint32_t nreg0;		/* first-level sub-regions (their cursors) ... */
	uint32_t nreg0_used;	/* ... and those of digits that can occur (their words): regions of digits that cannot occur are not allocated */
	bool selective_ok;	/* the selective first level can serve the request (MDB_SELECTIVE_L0 and the caller's hint decide: part_selective) */
	bool w32_unserved;	/* 4-byte words were asked for and the layout has none */
	bool stop0_unserved;	/* level0_only was asked for and the layout is another */
};

static part_layout part_layout_of(const part_xrequest &x)
{
	part_layout y;
	memset(&y, 0, sizeof(y));
	const uint32_t kbits = x.narrow ? x.narrow_kbits : 0u;
	y.nlevels = x.bits2 > 0 ? 2 : 1;
	y.stop0 = x.level0_only && y.nlevels == 1;
	y.out16 = y.stop0 && x.out16 && x.narrow == 2 && kbits && kbits - (uint32_t)x.bits1 <= 16u;
	y.R[0] = x.mode == MDB_DIGIT_MOD ? x.n_dest : (1u << x.bits1);
	y.R[1] = 1u << x.bits2;
	/* FAST applies to the last level only, and only while leaf * cap stays a 32-bit index */
	y.nleaves = y.nlevels == 2 ? y.R[0] * y.R[1] : y.R[0];
	y.fast_cap = x.leaf_cap ? x.leaf_cap : part_fast_cap(x.n, y.nleaves);
	y.fast = x.fast && !x.stable && (y.nlevels == 2 || y.stop0) && !x.final_hv_out && (uint64_t)y.nleaves * y.fast_cap < 0xFFFFFFFFull;
	/* ... and, with it, to the first level: PART_NSUB fixed-capacity sub-regions per digit */
	y.nreg0 = y.R[0] * PART_NSUB;
	/* raw sort keys need not cover the whole first digit range (row ids below n < 2^kbits): the regions are
	 * sized for the digits that can occur */
	y.nreg0_used = (x.digits0_used && x.digits0_used < y.R[0] ? x.digits0_used : y.R[0]) * PART_NSUB;
	uint64_t avg0 = (x.n + y.nreg0_used - 1) / y.nreg0_used;
	/* raw sort keys that are ROW IDS (the ordering of group records by first row): a first-level digit spans digit0_rows ids and every id
	 * occurs once at most, so min(n, digit0_rows) words is the most a digit can receive - and receives, where the first rows bunch
	 * (single-table GROUP BY over random duplicates: most groups' first rows lie in the first tenth of the table).  Regions sized for
	 * that never send the sort to its exact layout; the list's order has nothing to do with the row ids, so a digit's words spread
	 * evenly over its sub-regions */
	if (x.fast && x.digit0_rows) {
		const uint64_t most = x.n < x.digit0_rows ? x.n : x.digit0_rows, per_sub = (most + PART_NSUB - 1) / PART_NSUB;
		if (per_sub > avg0)
			avg0 = per_sub;
	}
	y.cap0 = x.region_cap ? x.region_cap : (uint32_t)((((x.level0_only && x.loose) ? avg0 * 3 / 2 : avg0 * 5 / 4) + 1024 + 63) & ~63ull);
	y.fast0 = y.fast && x.mode == MDB_DIGIT_RADIX && (uint64_t)y.nreg0_used * y.cap0 < 0xFFFFFFFFull;
	/* narrow form without row ids (right side of a join): 4-byte words from the first level's output on; only built for
	 * the histogram-free layout of both levels (callers ask mdb_partition_w32_applies() first) */
	y.fold32 = x.fold32 && x.raw_hv && y.fast0 && y.fast;
	y.w32 = (x.narrow == 2 && y.fast0 && y.fast) || y.fold32;
	y.w32_unserved = (x.narrow == 2 || x.fold32) && !y.w32;
	y.stop0_unserved = x.level0_only && !(y.stop0 && y.fast0);
	/* payload cells beside the words: one buffer per level, laid out like that level's words */
	y.npay = (y.fast0 && !y.w32 && (y.stop0 || (y.fast && y.nlevels == 2))) ? x.npay : 0;
	/* the pruned left table of the compact narrow form (hash | row id words over an int64 column, no NULL bitmap): k_part_scatter<pf_key_cf_sel> */
	y.selective_ok = y.fast0 && x.range_in && !x.nullbits && !x.raw_hv && !x.want_rid && !y.w32 && !y.npay && !x.minmax64_out && x.narrow == 1 && kbits &&
			 !x.keys32;
	return y;
}

/* ---- the knobs of the first level's choice of instance, read once per run */
struct part_knobs {
	long long selective_l0;	/* MDB_SELECTIVE_L0 - 0: never the selective first level, 1: where the caller knows the join is selective, 2: whatever it expects */
	long long tile2_min;	/* MDB_TILE2_MIN - rows from which the tiles of 2 x MDB_TILE rows are taken (default 2^25; tests: the form on small tables) */
	long long tile4_min;	/* MDB_TILE4_MIN - the same for the tiles of 4 x MDB_TILE rows */
	bool tile2_off;		/* MDB_TILE2=0: MDB_TILE rows everywhere */
	bool tile4_off;		/* MDB_TILE4=0: no tiles of 4 x MDB_TILE rows */
};

static part_knobs part_knobs_read(void)
{
	part_knobs kn;
	kn.selective_l0 = mdb_knob_int("MDB_SELECTIVE_L0", 1);
	kn.tile2_min = mdb_knob_int("MDB_TILE2_MIN", 0);
	kn.tile4_min = mdb_knob_int("MDB_TILE4_MIN", 0);
	kn.tile2_off = mdb_knob_off("MDB_TILE2") != 0;
	kn.tile4_off = mdb_knob_off("MDB_TILE4") != 0;
	return kn;
}

/* ... whether the selective first level runs - which reads a column from any 8-byte boundary; every other first level loads pairs of keys
 * from where the column starts */
static bool part_selective(const part_xrequest &x, const part_layout &y, const part_knobs &kn)
{
	return y.selective_ok && (kn.selective_l0 == 2 || (kn.selective_l0 != 0 && x.selective));
}

/* ---- one kernel launch of a level, as the ladders below choose it */
typedef void (*part_kernel)(mdb_level_args);
enum part_reduce { PART_RED_NONE = 0, PART_RED_MINMAX, PART_RED_MINMAX64 };	/* the per-tile (min, max) pairs a first level left behind, reduced after it */
struct part_launch {
	const char *name;	/* profiler name */
	part_kernel kernel;	/* NULL: no instance serves the request */
	uint32_t threads;
	uint32_t rows;		/* rows per tile */
	bool span16;		/* first level: tiles are counted from the 16-byte boundary at or below the first key */
	part_reduce reduce;
};

template <typename F>
static part_launch part_scatter(const char *name, uint32_t rows = MDB_TILE, uint32_t threads = PART_THREADS)
{
	const part_launch pl = { name, k_part_scatter<F>, threads, rows, false, PART_RED_NONE };
	return pl;
}

/* the histogram-free first level.  Tables of 2^25 rows and more: tiles of 2 x MDB_TILE rows in the instances that have them, and of
 * 4 x MDB_TILE rows, 1024 threads, for the 2-byte words of an int64 column without a NULL bitmap (MDB_TILE2=0 asks for MDB_TILE rows
 * everywhere: not these either) */
static part_launch part_first_launch(const part_xrequest &x, const part_layout &y, const part_knobs &kn, const mdb_level_args &a)
{
	const uint32_t rows2 = PART_TMUL * MDB_TILE;
	/* compact narrow form over an int64 column: the instances that know so at compile time */
	const bool cf = a.narrow && a.narrow_kbits && !x.keys32 && x.mode == MDB_DIGIT_RADIX && !x.raw_hv && !x.want_rid;
	const bool t2 = x.n >= (kn.tile2_min > 0 ? (uint64_t)kn.tile2_min : (1ull << 25)) && !kn.tile2_off;
	const bool t4 = cf && !x.nullbits && x.n >= (kn.tile4_min > 0 ? (uint64_t)kn.tile4_min : (1ull << 25)) && !kn.tile4_off && !kn.tile2_off;
	if (x.raw_hv)
		return (y.fold32 && t2) ? part_scatter<pf_word_raw_w32_t2>("sort_scatter_l0_w32", rows2)
		       : y.fold32 ? part_scatter<pf_word_raw_w32>("sort_scatter_l0_w32") : part_scatter<pf_word_raw>("sort_scatter_l0");
	if (y.w32) {
		part_launch pl = !y.out16 ? (cf ? part_scatter<pf_key_w32_cf>("part_scatter_l0_w32") : part_scatter<pf_key_w32>("part_scatter_l0_w32"))
				 : t4 ? part_scatter<pf_key_w32_out16_cf_t4>("part_scatter_l0_w32", PART_T4_TILE, PART_T4_THREADS)
				 : (cf && t2) ? part_scatter<pf_key_w32_out16_cf_t2>("part_scatter_l0_w32", rows2)
				 : cf ? part_scatter<pf_key_w32_out16_cf>("part_scatter_l0_w32")
				      : part_scatter<pf_key_w32_out16>("part_scatter_l0_w32");
		pl.reduce = a.minmax_out ? PART_RED_MINMAX : PART_RED_NONE;	/* (every tile of the launch leaves its pair) */
		return pl;
	}
	if (y.npay) {	/* (payload cells travel with the compact narrow form's hash | row id words only) */
		part_launch pl = part_scatter<pf_key_cf_pay>("part_scatter_l0_pay");
		if (!cf || a.narrow != 1u)
			pl.kernel = NULL;
		return pl;
	}
	if (x.want_rid)		/* (64-bit form, left table, min-max pruning: the first) */
		return a.range64_in ? part_scatter<pf_key_rid_r64>("part_scatter_l0_rid_pruned") : part_scatter<pf_key_rid>("part_scatter_l0_rid");
	if (a.minmax64_out) {			/* 64-bit form, right table: its key range recorded */
		part_launch pl = part_scatter<pf_key_mm64>("part_scatter_l0");
		pl.reduce = PART_RED_MINMAX64;
		return pl;
	}
	if (part_selective(x, y, kn)) {
		part_launch pl = t2 ? part_scatter<pf_key_cf_sel_t2>("part_scatter_l0_pruned", rows2) : part_scatter<pf_key_cf_sel>("part_scatter_l0_pruned");
		pl.span16 = true;
		return pl;
	}
	/* (the same instances under two names: a pruned pass's bytes differ - most rows are read, not written) */
	const char *name = a.range_in ? "part_scatter_l0_pruned" : "part_scatter_l0";
	return (cf && t2) ? part_scatter<pf_key_cf_t2>(name, rows2) : cf ? part_scatter<pf_key_cf>(name) : part_scatter<pf_key>(name);
}

/* tiles of a first level's launch over `span` rows.  (Kept as it was: over an empty table only the instances of MDB_TILE rows that
 * count from the first key run one - empty - tile; the others get a grid of none) */
static uint32_t part_first_tiles(const part_launch &pl, uint64_t span)
{
	const uint32_t t = (uint32_t)((span + pl.rows - 1) / pl.rows);
	return (t || pl.rows != MDB_TILE || pl.span16) ? t : 1u;
}

/* the histogram-free last level: one cursor per leaf, runs placed with global atomics */
static part_launch part_last_launch(const part_xrequest &x, const part_layout &y, const mdb_level_args &a)
{
	return y.npay ? part_scatter<pf_word_pay>("part_scatter_l1_pay")
	       : x.want_rid ? part_scatter<pf_word_rid>("part_scatter_l1_rid")
	       : (x.raw_hv && y.fold32) ? part_scatter<pf_word_raw_w32>("sort_scatter_l1_w32")
	       : x.raw_hv ? part_scatter<pf_word_raw>("sort_scatter_l1")
	       : y.w32 ? part_scatter<pf_word_w32>("part_scatter_l1_w32")
	       : a.filter ? part_scatter<pf_word_semi>("part_scatter_l1_semi")
			  : part_scatter<pf_word>("part_scatter_l1");
}

/* the exact layout: a level's histogram kernel, and its scatter kernel */
static part_launch part_hist_launch(const part_xrequest &x, int level)
{
	part_launch pl = { "part_hist_l1", k_part_hist<false>, PART_THREADS, MDB_TILE, false, PART_RED_NONE };
	if (level == 0 && x.raw_hv) {
		pl.name = "sort_hist_l0";
		pl.kernel = k_part_hist<false, true>;
	} else if (level == 0) {
		pl.name = x.mode == MDB_DIGIT_MOD ? "dest_hist" : "part_hist_l0";
		pl.kernel = k_part_hist<true>;
	}
	return pl;
}

static part_launch part_exact_launch(const part_xrequest &x, int level, const mdb_level_args &a)
{
	if (level != 0)
		return x.stable ? part_scatter<pf_word_rid_stable_hist>("part_scatter_l1_stable")
		       : x.want_rid ? part_scatter<pf_word_rid_hist>("part_scatter_l1") : part_scatter<pf_word_hist>("part_scatter_l1");
	return x.raw_hv ? part_scatter<pf_word_hist_raw>("sort_scatter_l0")
	       : x.stable ? part_scatter<pf_key_rid_stable_hist>("part_scatter_l0_stable")
	       : (a.inverse_out && x.want_rid) ? part_scatter<pf_key_rid_hist_dest>("dest_scatter")
	       : a.inverse_out ? part_scatter<pf_key_hist_dest>("dest_scatter")
	       : x.want_rid ? part_scatter<pf_key_rid_hist>("part_scatter_l0")
			    : part_scatter<pf_key_hist>("part_scatter_l0");
}

/* ---- what the levels hand on to each other.  The sizing pass (cv.dry) and the real one walk the same functions with the same carver:
 * they cannot disagree about what is taken from the arena */
struct part_walk {
	part_carver cv;
	uint64_t *hv_buf[2];	/* per level: its output words, row ids ... */
	uint32_t *rid_buf[2];
	uint64_t *pay_buf[2], *pay_buf1[2];	/* ... and payload cells (first level, last level) */
	uint32_t S;		/* segments of the current level's input */
	uint32_t *seg_start, *tb;	/* exact layout: their starts and tile bases */
	const mdb_tile_desc *tiles;	/* tile descriptors of the current level's input (NULL: level 0, computed arithmetically) ... */
	uint32_t ntiles;	/* ... and their number (an upper bound from level 1 on) */
	int used_bits;		/* hash bits consumed so far */
	uint32_t *leaf_cnt;	/* fast layout: the leaf cursors (with stop0: the first level's) */
};

/* the levels' output buffers and the first level's segment words */
static void part_carve_outputs(const part_xrequest &x, const part_layout &y, part_walk &w)
{
	for (int l = 0; l < y.nlevels; l++) {
		const uint64_t elems = (y.fast && l == 1) ? (uint64_t)y.nleaves * y.fast_cap
				       : ((y.fast0 && l == 0) ? (uint64_t)y.nreg0_used * y.cap0 : (x.n ? x.n : 1));
		const bool last = l == y.nlevels - 1;
		w.hv_buf[l] = (last && x.final_hv_out) ? x.final_hv_out : (uint64_t *)w.cv.take(elems * (y.w32 ? 4 : 8));
		if (x.want_rid)
			w.rid_buf[l] = (last && x.final_rid_out) ? x.final_rid_out : (uint32_t *)w.cv.take(elems * 4);
	}
	for (int c = 0; c < y.npay && c < 2; c++) {
		w.pay_buf[c] = (uint64_t *)w.cv.take((uint64_t)y.nreg0_used * y.cap0 * 8);
		if (!y.stop0)
			w.pay_buf1[c] = (uint64_t *)w.cv.take((uint64_t)y.nleaves * y.fast_cap * 8);
	}
	w.seg_start = (uint32_t *)w.cv.take(2 * 4);
	w.tb = (uint32_t *)w.cv.take(2 * 4);
}

/* the kernel arguments of level `l`, but for what belongs to the level's form (cursors and capacities, histogram, payload buffers) */
static mdb_level_args part_level_args(const part_xrequest &x, const part_layout &y, int l, const part_walk &w)
{
	mdb_dev_ctx *ctx = w.cv.ctx;
	mdb_level_args a;
	memset(&a, 0, sizeof(a));
	a.keys = x.keys;
	a.nullbits = x.nullbits;
	a.n = x.n;
	a.hv_in = l ? w.hv_buf[l - 1] : x.raw_hv;	/* raw_hv: level 0 reads ready-made 64-bit sort keys */
	a.skip_zero = (l == 0 && x.raw_hv && x.zero_is_gap) ? 1u : 0u;
	a.fold64 = (y.fold32 && l == 0 && x.fold32 != 2) ? 1u : 0u;
	a.rid_in = l ? w.rid_buf[l - 1] : NULL;
	a.tiles = w.tiles;
	a.hv_out = w.hv_buf[l];
	a.rid_out = w.rid_buf[l];
	a.ntiles = w.ntiles;
	a.R = y.R[l];
	a.mode = l == 0 ? x.mode : (uint32_t)MDB_DIGIT_RADIX;
	a.inverse_out = (x.inverse_out && l == y.nlevels - 1) ? (x.keys32_out ? 2u : 1u) : 0u;
	a.narrow = (l == 0 && (x.narrow == 1 || x.narrow == 2)) ? (uint32_t)x.narrow : 0u;
	a.status = ctx ? ctx->d_status : NULL;
	a.keys32 = x.keys32 ? 1u : 0u;
	a.narrow_base = x.narrow ? x.narrow_base : 0;
	a.narrow_kbits = a.narrow ? x.narrow_kbits : 0u;
	a.own_on = (l == 0 && x.own_on) ? 1u : 0u;
	a.own_lo = x.own_lo;
	a.own_hi = x.own_hi;
	a.keep_on = (l == 0 && x.keep_on) ? 1u : 0u;
	a.keep_lo = x.keep_lo;
	a.keep_hi = x.keep_hi;
	a.minmax_out = (l == 0 && x.minmax_out) ? x.minmax_tiles : NULL;	/* per-tile pairs, reduced after the launch */
	a.minmax_final = a.minmax_out ? x.minmax_out : NULL;
	a.range_in = l == 0 ? x.range_in : NULL;
	a.minmax64_out = (l == 0 && x.minmax64_out) ? x.minmax64_tiles : NULL;
	a.range64_in = l == 0 ? x.range64_in : NULL;
	a.filter = l == 1 ? x.bits : NULL;
	a.filter_words = x.words;
	a.filter_shift = x.shift;
	if (a.mode == MDB_DIGIT_RADIX) {
		const int b = l == 0 ? x.bits1 : x.bits2;
		a.shift = (uint32_t)((y.w32 ? 32 : 64) - w.used_bits - b);
		a.mbits = (uint32_t)b;
	} else {
		uint32_t mb = 1;
		while ((1u << mb) < a.R)
			mb++;
		a.shift = 0;
		a.mbits = mb;
	}
	return a;
}

/* the first level's launch, and the reduction of the key range it recorded */
static int part_first_run(mdb_dev_ctx *ctx, const part_xrequest &x, const part_layout &y, const part_knobs &kn, const part_walk &w, mdb_level_args &a)
{
	const part_launch pl = part_first_launch(x, y, kn, a);
	if (!pl.kernel)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "payload cells travel with the compact narrow form's hash | row id words only");
	if (!x.raw_hv && y.w32 && y.out16)
		a.out16_shift = 32u - a.narrow_kbits;
	if (!x.raw_hv && y.npay) {
		a.npay = (uint32_t)y.npay;
		for (int c = 0; c < y.npay; c++) {
			a.pay_in[c] = reinterpret_cast<const uint64_t *>(x.pay_in[c]);
			a.pay_out[c] = w.pay_buf[c];
		}
	}
	/* (the selective instance counts positions from the aligned address below the first key) */
	a.ntiles = part_first_tiles(pl, x.n + (pl.span16 ? (((uintptr_t)x.keys >> 3) & 1u) : 0u));
	MDB_LAUNCH(ctx, pl.name, pl.kernel, grid8(a.ntiles), pl.threads, a);
	if (pl.reduce == PART_RED_MINMAX)
		MDB_LAUNCH(ctx, "part_minmax", k_part_minmax_reduce, MM_GROUPS, MM_THREADS, (const uint32_t *)a.minmax_out, a.ntiles, x.minmax_out);
	if (pl.reduce == PART_RED_MINMAX64)
		MDB_LAUNCH(ctx, "part_minmax", k_part_minmax64_reduce, 1, 1024, (const unsigned long long *)a.minmax64_out, a.ntiles, x.minmax64_out);
	return MIDORIDB_OK;
}

/* histogram-free first level: PART_NSUB sub-regions per digit, then the tile descriptors of the level behind it */
static int part_level_first(const part_xrequest &x, const part_layout &y, const part_knobs *kn, part_walk &w)
{
	mdb_dev_ctx *ctx = w.cv.ctx;
	const bool dry = w.cv.dry;
	const bool cursor_ext = !dry && x.cursor0_ext && y.nreg0 <= x.cursor0_ext_words;
	uint32_t *cursor0 = cursor_ext ? x.cursor0_ext : (uint32_t *)w.cv.take((size_t)y.nreg0 * 4);
	uint32_t *reg_nt = (uint32_t *)w.cv.take(((size_t)y.nreg0 + 1) * 4);
	const uint32_t next_tiles = (uint32_t)(x.n / MDB_TILE) + y.nreg0 + 1;
	mdb_tile_desc *next_desc = y.stop0 ? NULL : (mdb_tile_desc *)w.cv.take((size_t)next_tiles * sizeof(mdb_tile_desc));
	if (w.cv.failed)
		return -MIDORIDB_INTERNAL;
	if (!dry) {
		mdb_level_args a = part_level_args(x, y, 0, w);
		a.cursor = cursor0;
		a.cap = y.cap0;
		a.nsub = PART_NSUB;
		if (!cursor_ext)
			MDB_HIP(ctx, hipMemsetAsync(cursor0, 0, (size_t)y.nreg0 * 4, ctx->stream));
		const int rc = part_first_run(ctx, x, y, *kn, w, a);
		if (rc)
			return rc;
		if (!y.stop0) {
			MDB_LAUNCH(ctx, "part_region_tiles", k_part_region_tiles_scan, 1, 1024, cursor0, y.nreg0, y.cap0, PART_NSUB, reg_nt);
			MDB_LAUNCH(ctx, "part_build_tiles", k_part_build_tiles_regions, (next_tiles + 255) / 256, 256, cursor0, reg_nt, y.nreg0, y.cap0,
				   PART_NSUB, next_desc, next_tiles);
		}
	}
	if (y.stop0) {
		w.leaf_cnt = cursor0;
		return MIDORIDB_OK;
	}
	uint32_t real_tiles = next_tiles;
	if (!dry && (x.range_in || x.range64_in) && x.expect_pruned) {
		/* min-max pruning may have dropped most rows: the second level is launched for the tiles that exist (one
		 * 4-byte read-back and a synchronisation, ~15 us) - 26 000 workgroups that find an empty descriptor and leave
		 * cost 0.09 ms at 10^8 rows */
		uint64_t *h = ctx->h_pinned;
		MDB_HIP(ctx, hipMemcpyAsync(&h[MDB_HP_PART_TILES], reg_nt + y.nreg0, 4, hipMemcpyDeviceToHost, ctx->stream));
		MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
		const uint32_t got = (uint32_t)h[MDB_HP_PART_TILES];
		real_tiles = got < next_tiles ? (got ? got : 1u) : next_tiles;
	}
	w.used_bits += x.bits1;
	w.seg_start = NULL;
	w.tb = NULL;
	w.S = y.R[0];
	w.tiles = next_desc;
	w.ntiles = real_tiles;
	return MIDORIDB_OK;
}

/* histogram-free last level: one fixed-capacity region and one cursor per leaf */
static int part_level_last(const part_xrequest &x, const part_layout &y, part_walk &w)
{
	mdb_dev_ctx *ctx = w.cv.ctx;
	const uint32_t nchild = w.S * y.R[1];
	w.leaf_cnt = (uint32_t *)w.cv.take((size_t)nchild * 4);
	if (w.cv.failed)
		return -MIDORIDB_INTERNAL;
	if (!w.cv.dry) {
		mdb_level_args a = part_level_args(x, y, 1, w);
		a.cursor = w.leaf_cnt;
		a.cap = y.fast_cap;
		MDB_HIP(ctx, hipMemsetAsync(w.leaf_cnt, 0, (size_t)nchild * 4, ctx->stream));
		if (y.npay) {
			a.npay = (uint32_t)y.npay;
			for (int c = 0; c < y.npay; c++) {
				a.pay_in[c] = w.pay_buf[c];
				a.pay_out[c] = w.pay_buf1[c];
			}
		}
		const part_launch pl = part_last_launch(x, y, a);
		MDB_LAUNCH(ctx, pl.name, pl.kernel, grid8(w.ntiles), pl.threads, a);
	}
	w.used_bits += x.bits2;
	w.S = nchild;
	w.seg_start = NULL;
	return MIDORIDB_OK;
}

/* exact level `l`: histogram, scan, scatter; the children's starts, and the tile descriptors of the level behind it */
static int part_level_exact(const part_xrequest &x, const part_layout &y, int l, part_walk &w)
{
	mdb_dev_ctx *ctx = w.cv.ctx;
	const uint32_t R = y.R[l], nchild = w.S * R, ntiles = w.ntiles;
	const uint64_t hlen = (uint64_t)ntiles * R + 1;
	uint32_t *hist = (uint32_t *)w.cv.take(hlen * 4);
	uint32_t *scan_tmp = (uint32_t *)w.cv.take(mdb_scan_scratch_words(hlen) * 4);
	uint32_t *child_start = (uint32_t *)w.cv.take(((size_t)nchild + 1) * 4);
	uint32_t *child_nt = (uint32_t *)w.cv.take(((size_t)nchild + 1) * 4);
	uint32_t *child_scan_tmp = (uint32_t *)w.cv.take(mdb_scan_scratch_words((uint64_t)nchild + 1) * 4);
	/* tile descriptors of the NEXT level (upper bound: every child adds at most two partial tiles) */
	const uint32_t next_tiles = (uint32_t)(x.n / MDB_TILE) + 2 * nchild + 1;
	const bool more = l + 1 < y.nlevels;
	mdb_tile_desc *next_desc = more ? (mdb_tile_desc *)w.cv.take((size_t)next_tiles * sizeof(mdb_tile_desc)) : NULL;
	if (w.cv.failed)
		return -MIDORIDB_INTERNAL;
	if (!w.cv.dry) {
		mdb_level_args a = part_level_args(x, y, l, w);
		a.hist = hist;
		MDB_HIP(ctx, hipMemsetAsync(hist, 0, hlen * 4, ctx->stream));
		const part_launch ph = part_hist_launch(x, l);
		MDB_LAUNCH(ctx, ph.name, ph.kernel, grid8(ntiles), ph.threads, a);
		int rc = mdb_scan_u32_inplace(ctx, hist, hlen, scan_tmp);
		if (rc)
			return rc;
		const part_launch ps = part_exact_launch(x, l, a);
		MDB_LAUNCH(ctx, ps.name, ps.kernel, grid8(ntiles), ps.threads, a);
		MDB_LAUNCH(ctx, "part_children", k_part_children, (nchild + 1 + 255) / 256, 256, hist, w.tb, w.S, R, child_start, child_nt);
		if (more) {
			rc = mdb_scan_u32_inplace(ctx, child_nt, (uint64_t)nchild + 1, child_scan_tmp);
			if (rc)
				return rc;
			MDB_LAUNCH(ctx, "part_build_tiles", k_part_build_tiles, (next_tiles + 255) / 256, 256, child_start, child_nt, nchild, y.R[l + 1],
				   next_desc, next_tiles);
		}
	}
	w.used_bits += (l == 0 ? x.bits1 : x.bits2);
	w.seg_start = child_start;
	w.tb = child_nt;
	w.S = nchild;
	w.tiles = next_desc;
	w.ntiles = next_tiles;
	return MIDORIDB_OK;
}

static void part_result_fill(const part_xrequest &x, const part_layout &y, const part_walk &w, mdb_part_result *out)
{
	const bool digits = y.stop0 && y.fast0;	/* the first level's sub-regions are the result */
	const int last = y.nlevels - 1;
	out->hv = w.hv_buf[last];
	out->rid = digits ? NULL : w.rid_buf[last];
	out->leaf_off = digits ? NULL : w.seg_start;
	out->leaf_cnt = w.leaf_cnt;
	out->leaf_cap = digits ? y.cap0 : (y.fast ? y.fast_cap : 0);
	out->nleaves = digits ? y.R[0] : w.S;
	out->bits_total = digits ? (uint32_t)x.bits1 : (uint32_t)w.used_bits;
	out->w32 = y.w32;
	out->w16 = digits && y.out16 && y.w32;
	out->nsub = digits ? PART_NSUB : 0;
	for (int c = 0; c < 2; c++)
		out->pay[c] = digits ? w.pay_buf[c] : (y.nlevels == 2 ? w.pay_buf1[c] : NULL);
}

/* one walk over the levels of a request: the real one, or - kn = NULL - the sizing pass: nothing is launched, *bytes is what the real
 * one would take from the arena */
static int part_run(mdb_dev_ctx *ctx, const part_xrequest &x, const part_knobs *kn, mdb_part_result *out, size_t *bytes = NULL)
{
	const bool dry = kn == NULL;
	const part_layout y = part_layout_of(x);
	part_walk w;
	memset(&w, 0, sizeof(w));
	w.cv.ctx = ctx;
	w.cv.dry = dry;
	w.S = 1;
	w.ntiles = x.n ? (uint32_t)((x.n + MDB_TILE - 1) / MDB_TILE) : 1u;
	if (y.w32_unserved && !dry)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "4-byte partition words need the two-level fast layout");
	if (y.stop0_unserved && !dry)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "first-level-only partition: histogram-free layout, one level");
	if (!dry && x.keys && !x.keys32 && ((uintptr_t)x.keys & 15) && !part_selective(x, y, *kn))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "key columns must be 16-byte aligned on the device (8-byte for int32 keys)");
	part_carve_outputs(x, y, w);
	if (w.cv.failed)
		return -MIDORIDB_INTERNAL;
	if (!dry && !y.fast0)	/* the FAST first level has no parent segments to describe */
		MDB_LAUNCH(ctx, "part_seg0", k_part_seg0, 1, 64, w.seg_start, w.tb, (uint32_t)x.n, w.ntiles);
	for (int l = 0; l < y.nlevels; l++) {
		const int rc = (y.fast0 && l == 0) ? part_level_first(x, y, kn, w) : (y.fast && l == 1) ? part_level_last(x, y, w) : part_level_exact(x, y, l, w);
		if (rc)
			return rc;
	}
	if (out)
		part_result_fill(x, y, w, out);
	if (bytes)
		*bytes = w.cv.bytes;
	return MIDORIDB_OK;
}

/* arena bytes of a request */
static size_t part_bytes(const part_xrequest &x)
{
	size_t bytes = 0;
	(void)part_run(NULL, x, NULL, NULL, &bytes);
	return bytes;
}

static int part_execute(mdb_dev_ctx *ctx, const part_xrequest &x, mdb_part_result *out)
{
	const part_knobs kn = part_knobs_read();
	return part_run(ctx, x, &kn, out);
}

/* what the sizing functions have in common */
static mdb_part_request part_sizing_request(uint64_t n, int bits1, int bits2, bool fast)
{
	mdb_part_request rq;
	memset(&rq, 0, sizeof(rq));
	rq.n = n;
	rq.bits1 = bits1;
	rq.bits2 = bits2;
	rq.fast = fast;
	return rq;
}

size_t mdb_partition_arena_bytes(uint64_t n, int bits1, int bits2, bool want_rid, bool fast, int npay)
{
	mdb_part_request rq = part_sizing_request(n, bits1, bits2, fast);
	rq.want_rid = want_rid;
	rq.npay = npay;
	return part_bytes(part_xrequest(rq)) + 4096 + (size_t)npay * 1024;
}

size_t mdb_partition_level0_arena_bytes(uint64_t n, int bits1, bool loose, int npay)
{
	mdb_part_request rq = part_sizing_request(n, bits1, 0, true);
	rq.level0_only = true;
	rq.loose = loose;
	rq.npay = npay;
	return part_bytes(part_xrequest(rq)) + 4096 + (size_t)npay * 512;
}

bool mdb_partition_w32_applies(uint64_t n, int bits1, int bits2, bool fast)
{
	mdb_part_request rq = part_sizing_request(n, bits1, bits2, fast);
	rq.narrow = 2;
	return part_layout_of(part_xrequest(rq)).w32;
}

static int part_request_check(mdb_dev_ctx *ctx, const mdb_part_request &rq)
{
	const bool stop0 = rq.level0_only, stable = rq.stable, want_rid = rq.want_rid, fast = rq.fast;
	const int narrow = rq.narrow, bits2 = rq.bits2;
	const uint32_t narrow_kbits = rq.narrow_kbits;
	if (stop0 && (!narrow || !narrow_kbits || want_rid || stable || !fast || bits2 != 0 || rq.bits))
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "first-level-only partition: compact narrow form, bits2 = 0, no bitmap");
	if (rq.bits && (narrow != 1 || !narrow_kbits || want_rid || stable || !fast || bits2 <= 0 || rq.words < 4 || rq.words > MDB_TILE * 2 ||
			(rq.words & (rq.words - 1))))
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "semi-join filter: left side of the compact narrow form, two fast levels, slices of 4 ... 8192 words");
	if ((rq.minmax_out || rq.range_in) && (!narrow || want_rid || stable || !fast || (bits2 <= 0 && !stop0) || (rq.minmax_out && (narrow != 2 || !rq.minmax_tiles))))
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "min-max pruning: narrow forms, two fast levels");
	if ((rq.minmax64_out || rq.range64_in) && (narrow || stable || !fast || bits2 <= 0 || (rq.minmax64_out && (want_rid || !rq.minmax64_tiles)) ||
						   (rq.range64_in && !want_rid)))
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "min-max pruning, 64-bit form: two fast levels, the right table without and the left with row ids");
	if (rq.npay && (narrow != 1 || !narrow_kbits || want_rid || stable || !fast || rq.npay < 0 || rq.npay > 2 || (bits2 <= 0 && !stop0)))
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "payload cells: compact narrow form with hash | row id words, histogram-free layout, at most two columns");
	if (narrow_kbits && (!narrow || narrow_kbits < 8 || narrow_kbits > 32 || (uint32_t)(rq.bits1 + bits2) > narrow_kbits))
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "compact narrow form: bad window width");
	if (narrow && (stable || want_rid))
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "narrow partitioning carries row ids inside the word");
	if (rq.n >= 0xFFFFFFFFull)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "table of %llu rows exceeds the 32-bit row-id limit of one GPU shard", (unsigned long long)rq.n);
	if (stable && !want_rid)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "stable partitioning is only built with row ids");
	if ((uintptr_t)rq.keys & 7)	/* (int64 columns: 16 bytes, unless the selective first level takes them - part_run) */
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "key columns must be 16-byte aligned on the device (8-byte for int32 keys)");
	return MIDORIDB_OK;
}

int mdb_partition_table(mdb_dev_ctx *ctx, const mdb_part_request &rq, mdb_part_result *out)
{
	const int rc = part_request_check(ctx, rq);
	return rc ? rc : part_execute(ctx, part_xrequest(rq), out);
}

size_t mdb_partition_raw_arena_bytes(uint64_t n, int bits1, int bits2, uint32_t leaf_cap, bool fast, uint32_t digits0_used, uint64_t digit0_rows)
{
	mdb_part_request rq = part_sizing_request(n, bits1, bits2, fast);
	rq.leaf_cap = leaf_cap;
	rq.digits0_used = digits0_used;
	rq.digit0_rows = digit0_rows;
	return part_bytes(part_xrequest(rq)) + 4096;
}

int mdb_partition_raw(mdb_dev_ctx *ctx, const mdb_part_request &rq, mdb_part_result *out)
{
	if (rq.fold32 && (!rq.fast || rq.bits2 <= 0 || !rq.zero_is_gap))
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "4-byte raw words need the two-level fast layout");
	return part_execute(ctx, part_xrequest(rq), out);
}

/* ---- one histogram-free radix level over 4-byte words in caller-described tiles (the receiver's second level of the
 * sharded operator, mdb_dev_shard.hip: its input regions came from several ranks) ------------------------------------- */
int mdb_partition_words_level(mdb_dev_ctx *ctx, const uint32_t *words_in, const mdb_tile_desc *tiles, uint32_t ntiles, int bits, uint32_t shift,
			      uint32_t *words_out, uint32_t *cursor, uint32_t nchild, uint32_t cap, uint32_t out16_shift)
{
	if (bits < 1 || bits > MDB_MAX_RADIX_BITS || !ntiles)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "words level: bad digit width");
	mdb_level_args a;
	memset(&a, 0, sizeof(a));
	a.hv_in = reinterpret_cast<const uint64_t *>(words_in);
	a.tiles = tiles;
	a.hv_out = reinterpret_cast<uint64_t *>(words_out);
	a.ntiles = ntiles;
	a.R = 1u << bits;
	a.mode = MDB_DIGIT_RADIX;
	a.shift = shift;
	a.mbits = (uint32_t)bits;
	a.cursor = cursor;
	a.cap = cap;
	a.nsub = 0;
	a.status = ctx->d_status;
	MDB_HIP(ctx, hipMemsetAsync(cursor, 0, (size_t)nchild * 4, ctx->stream));
	if (out16_shift) {	/* the children are leaves whose key bits fit 16: 2-byte words out, (uint16_t)(word >> out16_shift) */
		a.out16_shift = out16_shift;
		MDB_LAUNCH(ctx, "part_scatter_l1_w32", (k_part_scatter<pf_word_w32_out16>), grid8(ntiles), PART_THREADS, a);
	} else {
		MDB_LAUNCH(ctx, "part_scatter_l1_w32", (k_part_scatter<pf_word_w32>), grid8(ntiles), PART_THREADS, a);
	}
	return MIDORIDB_OK;
}

/* ---- one stable LSD radix pass (ORDER BY) --------------------------------------------------------
 *
 * (key_in, rid_in) -> (key_out, rid_out), stably ordered by the `bits`-wide digit at `shift`: the flat-tiled
 * histogram / scan / ballot-ranked scatter of the exact partition path (STABLE keeps the input order inside
 * every digit, which is what makes least-significant-digit-first sorting and multi-column ORDER BY work). */
size_t mdb_sort_pass_hist_words(uint64_t n)
{
	const uint64_t nt = (n + MDB_TILE - 1) / MDB_TILE;
	return (size_t)(nt ? nt : 1) * 256u + 1u;
}

int mdb_sort_pass(mdb_dev_ctx *ctx, const uint64_t *key_in, const uint32_t *rid_in, uint64_t n, uint32_t shift, uint32_t bits,
		  uint64_t *key_out, uint32_t *rid_out, uint32_t *hist, uint32_t *scan_tmp)
{
	if (n == 0)
		return MIDORIDB_OK;
	if (bits < 1 || bits > 8 || n >= 0xFFFFFFFFull)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "sort pass: bad digit width or too many rows");
	mdb_level_args a;
	memset(&a, 0, sizeof(a));
	a.n = n;
	a.hv_in = key_in;
	a.rid_in = rid_in;
	a.hv_out = key_out;
	a.rid_out = rid_out;
	a.ntiles = (uint32_t)((n + MDB_TILE - 1) / MDB_TILE);
	a.R = 1u << bits;
	a.mode = MDB_DIGIT_RADIX;
	a.shift = shift;
	a.mbits = bits;
	a.hist = hist;
	const uint64_t hlen = (uint64_t)a.ntiles * a.R;
	MDB_LAUNCH(ctx, "orderby_hist", k_part_hist<false>, grid8(a.ntiles), PART_THREADS, a);
	int rc = mdb_scan_u32_inplace(ctx, hist, hlen, scan_tmp);
	if (rc)
		return rc;
	MDB_LAUNCH(ctx, "orderby_scatter", (k_part_scatter<pf_word_rid_stable_hist>), grid8(a.ntiles), PART_THREADS, a);
	return MIDORIDB_OK;
}

/* ---- multi-GPU destination partition ------------------------------------------------------------ */

extern "C" int mdb_dev_partition_by_dest(mdb_dev_ctx *ctx, const int64_t *keys, const uint64_t *nullbits, uint64_t n,
					 uint32_t n_dest, int keys32, void *out_keys, uint32_t *out_rid, uint64_t *out_counts)
{
	return mdb_dev_partition_by_dest_pruned(ctx, keys, nullbits, n, n_dest, keys32, INT64_MIN, INT64_MAX, INT64_MIN, INT64_MAX, out_keys, out_rid,
						out_counts);
}

extern "C" int mdb_dev_partition_by_dest_pruned(mdb_dev_ctx *ctx, const int64_t *keys, const uint64_t *nullbits, uint64_t n,
						uint32_t n_dest, int keys32, int64_t keep_lo, int64_t keep_hi, int64_t own_lo, int64_t own_hi,
						void *out_keys, uint32_t *out_rid, uint64_t *out_counts)
{
	if (n_dest == 0 || n_dest > PART_MAX_R)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "partition_by_dest: n_dest must be in [1, %u]", PART_MAX_R);
	if (n >= 0xFFFFFFFFull)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "partition_by_dest: too many rows");
	if ((uintptr_t)keys & 15)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "key columns must be 16-byte aligned on the device");
	for (uint32_t d = 0; d < n_dest; d++)
		out_counts[d] = 0;
	if (n == 0)
		return MIDORIDB_OK;
	/* one exact level, digit = low32(hash) mod n_dest, original keys written back through the inverse hash - as 4-byte integers when the
	 * caller knows from the column's statistics that every key fits - source row ids beside them when asked for */
	mdb_part_request rq;
	memset(&rq, 0, sizeof(rq));
	rq.keys = keys;
	rq.nullbits = nullbits;
	rq.n = n;
	rq.bits1 = 1;
	rq.want_rid = out_rid != NULL;
	rq.keep_on = keep_lo != INT64_MIN || keep_hi != INT64_MAX;
	rq.keep_lo = keep_lo;
	rq.keep_hi = keep_hi;
	rq.own_on = own_lo != INT64_MIN || own_hi != INT64_MAX;
	rq.own_lo = own_lo;
	rq.own_hi = own_hi;
	part_xrequest x(rq);
	x.mode = MDB_DIGIT_MOD;
	x.n_dest = n_dest;
	x.inverse_out = true;
	x.keys32_out = keys32 != 0;
	x.final_hv_out = (uint64_t *)out_keys;
	x.final_rid_out = out_rid;
	int rc = mdb_arena_begin(ctx, part_bytes(x) + 4096);
	if (rc)
		return rc;
	mdb_part_result res;
	MDB_HIP(ctx, hipMemsetAsync(ctx->d_status, 0, 4, ctx->stream));
	rc = part_execute(ctx, x, &res);
	if (rc)
		return rc;
	uint32_t *h_off = (uint32_t *)ctx->h_pinned;
	MDB_HIP(ctx, hipMemcpyAsync(h_off, res.leaf_off, ((size_t)n_dest + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
	MDB_HIP(ctx, hipMemcpyAsync(h_off + n_dest + 1, ctx->d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (h_off[n_dest + 1] & PART_ST_OWN_RANGE_BROKEN)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "partition_by_dest: a key lies outside the range [%lld, %lld] promised for its column",
				   (long long)own_lo, (long long)own_hi);
	if (keys32 && (h_off[n_dest + 1] & MDB_ST_KEY_OUTSIDE))
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "partition_by_dest: a key does not fit the 4-byte wire format (keys32 needs every key in "
							 "the int32 range: check mdb_dev_key_range)");
	for (uint32_t d = 0; d < n_dest; d++)
		out_counts[d] = (uint64_t)h_off[d + 1] - h_off[d];
	return MIDORIDB_OK;
}
