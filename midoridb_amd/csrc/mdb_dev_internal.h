/*
 * mdb_dev_internal.h - host-side entry points shared between the device-layer translation units.
 */
#ifndef MDB_DEV_INTERNAL_H
#define MDB_DEV_INTERNAL_H

#include "mdb_dev_common.h"

/* ---- scan (mdb_dev_core.hip) ----------------------------------------------------------------
 * In-place exclusive prefix sum over data[0..len) (uint32).  data[len-1]'s exclusive prefix is the
 * last value written; callers that need the grand total append one zero element.  `block_sums`
 * is scratch of mdb_scan_scratch_words(len) uint32 words. */
#define MDB_SCAN_CHUNK 4096u
#define MDB_SCAN_SMALL 16384u	/* up to here the scan is one single-workgroup launch */
static inline size_t mdb_scan_scratch_words(uint64_t len) { return (size_t)((len + MDB_SCAN_CHUNK - 1) / MDB_SCAN_CHUNK) + 1; }
int mdb_scan_u32_inplace(mdb_dev_ctx *ctx, uint32_t *data, uint64_t len, uint32_t *block_sums);
/* dst[0..n] = exclusive prefix sums of src[0..n), dst[n] = total; one single-workgroup launch (n <= MDB_SCAN_FROM_MAX) */
#define MDB_SCAN_FROM_MAX 65536u
int mdb_scan_u32_small_from(mdb_dev_ctx *ctx, const uint32_t *src, uint32_t n, uint32_t *dst);

/* ---- radix partition (mdb_dev_partition.hip) ------------------------------------------------ */
#define MDB_TILE 4096u		/* elements per partition tile */
#define MDB_MAX_RADIX_BITS 9	/* up to 512-way per level */

/* one tile of a partition level's input (mdb_dev_partition.hip) */
struct mdb_tile_desc {
	uint32_t start;		/* first input element of the tile */
	uint32_t len;		/* elements in the tile (0 = unused tile) */
	uint32_t hbase;		/* histogram index of (segment, digit 0, this tile) */
	uint32_t nt;		/* tiles in this tile's segment = histogram stride between digits */
	uint32_t seg;		/* index of the segment (parent partition) the tile belongs to */
};

enum mdb_digit_mode {
	MDB_DIGIT_RADIX = 0,	/* digit = bit field of the hashed key (MSD levels) */
	MDB_DIGIT_MOD = 1,	/* digit = low32(hash) mod n_dest (multi-GPU destination) */
};

struct mdb_part_result {
	uint64_t *hv;		/* hashed keys grouped by leaf (or original keys when inverse_out) */
	uint32_t *rid;		/* row ids, same order (NULL when not requested) */
	uint32_t *leaf_off;	/* exact form: nleaves + 1 offsets into hv/rid (NULL in the fast form) */
	uint32_t *leaf_cnt;	/* fast form: rows of each leaf, leaf i lives at [i * leaf_cap, i * leaf_cap + leaf_cnt[i]) */
	uint32_t leaf_cap;	/* 0 = exact form */
	uint32_t nleaves;
	uint32_t bits_total;
	bool w32;		/* hv holds 4-byte words (narrow form without row ids) */
	bool w16;		/* ... 2-byte words: the hash bits below the first level's digit (mdb_part_request.out16) */
	uint64_t *pay[2];	/* mdb_part_request.npay: the payload cells, laid out like hv (the cell of hv[i] is pay[c][i]) */
	uint32_t nsub;		/* != 0: first level only (mdb_part_request.level0_only) - nleaves = 2^bits1 digits, digit d's rows lie in nsub
				 * regions: region r = d * nsub + s at [r * leaf_cap, r * leaf_cap + min(count, leaf_cap)), its count at
				 * leaf_cnt[s * nleaves + d] */
};

/* One partition request: what to partition, into how many leaves, in which form, and what the first and the second level do to the rows
 * on their way.  Callers zero the record and set the fields they mean by name; mdb_partition_table reads the key column's fields,
 * mdb_partition_raw the raw words', both the plan and the fields below them. */
struct mdb_part_request {
	/* ---- the key column (mdb_partition_table) */
	const int64_t *keys;	/* 16-byte aligned on the device (8 bytes do for int32 keys and for the selective first level) */
	const uint64_t *nullbits;	/* NULL keys are dropped (NULL: the column has none) */
	uint64_t n;		/* rows - or words of the raw list */
	bool keys32;		/* `keys` points to int32 values */
	/* ---- the plan: 2^(bits1 + bits2) leaves by the top bits of the hashed key (bits2 = 0: one level) */
	int bits1, bits2;
	bool want_rid;		/* row ids travel beside the words (mdb_part_result.rid) */
	bool stable;		/* keep input order inside every leaf (slower ballot ranking; needs want_rid and the exact layout), otherwise the
				 * order inside a leaf is unspecified */
	bool fast;		/* no histogram passes: every leaf is a fixed-capacity region, runs are placed with atomic cursors (two levels, or
				 * level0_only); a region that overflows raises MDB_ST_REGION_FULL and the caller redoes the operator with fast = false,
				 * the exact histogram layout */
	int narrow;		/* (want_rid must be false) every key is expected within 2^31 of narrow_base - a key outside raises MDB_ST_KEY_OUTSIDE
				 * and the caller redoes the operator wide.  1: hv[i] = fmix32(key) << 32 | row id; 2: hv is an array of 4-byte words
				 * fmix32(key) - only in the histogram-free layout of both levels, see mdb_partition_w32_applies() */
	int64_t narrow_base;	/* narrow: the keys are taken relative to this value (centre of their 2^32 window; compact form: its low end) */
	uint32_t narrow_kbits;	/* compact narrow form: keys in [narrow_base, narrow_base + 2^narrow_kbits), hash32 = mdb_mixk(key - narrow_base,
				 * narrow_kbits) << (32 - narrow_kbits): below the bits1 + bits2 partition bits only narrow_kbits - bits1 - bits2
				 * bits tell keys apart */
	/* ---- ready-made 64-bit sort keys instead of a column (mdb_partition_raw: no hashing, no NULLs) */
	const uint64_t *raw_hv;
	uint32_t leaf_cap;	/* != 0: rows per leaf region of the fast layout (the caller guarantees that no leaf holds more) */
	uint32_t digits0_used;	/* how many of the 2^bits1 first-level digits can occur at all (0 = every one): sizes the fast first-level regions */
	uint64_t digit0_rows;	/* the words are row ids and a first-level digit spans that many of them (0: not so): the fast first-level regions
				 * are sized for the most a digit can hold instead of the average */
	bool zero_is_gap;	/* zero words are gaps of a chunked list, not words */
	int fold32;		/* two fast levels only, with zero_is_gap.  1: the first level folds every 8-byte record w into the 4-byte word
				 * (w >> 32) | (uint32_t)w - the caller knows that the two parts share no bit - and everything after it moves 4-byte
				 * words (mdb_part_result.w32); 2: raw_hv already holds 4-byte words */
	/* ---- semi-join filter of the SECOND level (left side of a join in the compact narrow form, two fast levels): a bitmap of the hashed
	 * key values the OTHER table holds, one bit per 2^coarse adjacent values, laid out by first-level digit: digit d owns words
	 * [d * words, d * words + words).  The second level's workgroup loads its digit's slice into LDS and drops the rows whose bit is
	 * clear before they are ranked and written. */
	const uint32_t *bits;	/* NULL: no bitmap */
	uint32_t words;		/* per first-level digit: a power of two, 4 ... 8192 (32 KiB) */
	uint32_t shift;		/* bit index (before masking to the slice) = hash32 >> shift */
	/* ---- min-max pruning at the FIRST level (narrow forms): the right table's call passes minmax_out (two words the caller
	 * initialised to 0xFFFFFFFF, 0: smallest / largest key - window base seen), the left table's call, later on the same
	 * stream, passes the same words as range_in and drops the rows outside */
	uint32_t *minmax_out;
	uint32_t *minmax_tiles;	/* with minmax_out: scratch of mdb_part_minmax_words(n) words (a pair per first-level tile, reduced after the launch) */
	const uint32_t *range_in;
	/* the same in the 64-bit form (narrow = 0): the right table (no row ids) leaves [lo, hi] of its keys as two signed 64-bit words in
	 * minmax64_out (scratch: minmax64_tiles, mdb_part_minmax_words(n) * 2 uint32 words), the left table (with row ids) reads them
	 * through range64_in */
	long long *minmax64_out;
	unsigned long long *minmax64_tiles;
	const long long *range64_in;
	bool selective;		/* with range_in, compact narrow form: the caller KNOWS (the last join over these columns, or the caller's statistics)
				 * that few rows lie inside the range: the first level runs its selective instance (k_part_scatter<pf_key_cf_sel>) */
	bool expect_pruned;	/* with range_in / range64_in: the caller expects most rows to be dropped (key sample): the second level's grid is
				 * then sized by the tiles that exist (a 4-byte read-back + synchronisation) instead of by the table */
	/* ---- payload: narrow = 1, histogram-free layout, one level (level0_only) or two: up to two 8-byte columns of the table travel with
	 * the rows (mdb_part_result.pay) - a join that carries the right table's payload to the leaf instead of gathering it afterwards */
	const void *pay_in[2];
	int npay;
	/* ---- key ranges of the first level, any form (mdb_dev_partition_by_dest_pruned): keep only the rows whose KEY lies in
	 * [keep_lo, keep_hi] - the other table's global key range, known before an exchange */
	bool keep_on;
	int64_t keep_lo, keep_hi;
	bool own_on;		/* ... and verify that every key of THIS table lies in [own_lo, own_hi] (a promised range; an error otherwise) */
	int64_t own_lo, own_hi;
	/* ---- first level only */
	bool level0_only;	/* stop after the histogram-free first level (compact narrow form, bits2 = 0, fast): the consumer reads the digits'
				 * sub-regions itself (mdb_part_result.nsub; k_leaf_wide in mdb_dev_leaf_wide.hip) */
	bool loose;		/* with level0_only: regions of 1.5 x (instead of 1.25 x) the average size - a column of some 10^4 - 10^5 distinct
				 * values puts a few dozen of them, with thousands of rows each, into a region */
	bool out16;		/* with level0_only and narrow = 2: 2-byte words (mdb_part_result.w16) when the hash bits below the digit fit 16 bits */
	uint32_t region_cap;	/* with level0_only, != 0: words per first-level region (a multiple of 64) instead of 1.25 x the average + 1024 -
				 * the sharded operator, whose ranks must agree on it */
	uint32_t *cursor0_ext;	/* != NULL: the first level's region cursors live here (cursor0_ext_words of them at least), ALREADY ZERO - the caller's
				 * one memset covers them (ctx->d_status + MDB_ZERO_BLK_OFF) - instead of an arena block and a memset of its own */
	uint32_t cursor0_ext_words;
};
static inline size_t mdb_part_minmax_words(uint64_t n) { return (size_t)((n + MDB_TILE - 1) / MDB_TILE + 8) * 2; }

/* Partition rq.keys into 2^(bits1 + bits2) leaves by the top bits of fmix64(key), dropping NULL keys.  All temporaries and outputs are
 * carved from the arena (the caller has called mdb_arena_begin with enough room: mdb_partition_arena_bytes, or
 * mdb_partition_level0_arena_bytes for level0_only).  No host sync, except with expect_pruned. */
int mdb_partition_table(mdb_dev_ctx *ctx, const mdb_part_request &rq, mdb_part_result *out);
/* ... what it needs of the arena.  Sized for a less specific request than the one that runs (8-byte words where narrow = 2 moves 4). */
size_t mdb_partition_arena_bytes(uint64_t n, int bits1, int bits2, bool want_rid, bool fast, int npay = 0);
size_t mdb_partition_level0_arena_bytes(uint64_t n, int bits1, bool loose = false, int npay = 0);
/* whether narrow = 2 is served for a table of n rows: the histogram-free layout of both levels, with every region index in 32 bits */
bool mdb_partition_w32_applies(uint64_t n, int bits1, int bits2, bool fast);

/* MSD radix partition of rq.raw_hv by the top bits1 + bits2 bits of the words; with two levels and fast the last one uses the
 * fixed-capacity layout with rq.leaf_cap rows per leaf.  Orders GROUP BY results by first row id, and sorts (mdb_dev_sort.hip). */
int mdb_partition_raw(mdb_dev_ctx *ctx, const mdb_part_request &rq, mdb_part_result *out);
size_t mdb_partition_raw_arena_bytes(uint64_t n, int bits1, int bits2, uint32_t leaf_cap, bool fast, uint32_t digits0_used, uint64_t digit0_rows = 0);

/* one stable least-significant-digit radix pass over (key, row id) pairs: digit = (key >> shift) & (2^bits - 1),
 * bits <= 8.  hist = scratch of mdb_sort_pass_hist_words(n) uint32, scan_tmp = mdb_scan_scratch_words(of that). */
size_t mdb_sort_pass_hist_words(uint64_t n);
int mdb_sort_pass(mdb_dev_ctx *ctx, const uint64_t *key_in, const uint32_t *rid_in, uint64_t n, uint32_t shift, uint32_t bits,
		  uint64_t *key_out, uint32_t *rid_out, uint32_t *hist, uint32_t *scan_tmp);

/* One histogram-free radix level over 4-byte words that lie in caller-described tiles: word w of tile t belongs to segment
 * tiles[t].seg and goes to child seg * 2^bits + ((w >> shift) & (2^bits - 1)); child c owns words_out[c * cap, c * cap + cap),
 * cursor[c] (zeroed by the call) counts its words; MDB_ST_REGION_FULL is raised when a child overflows.  Tile starts
 * must be multiples of 4 words.  No host sync. */
int mdb_partition_words_level(mdb_dev_ctx *ctx, const uint32_t *words_in, const mdb_tile_desc *tiles, uint32_t ntiles, int bits, uint32_t shift,
			      uint32_t *words_out, uint32_t *cursor, uint32_t nchild, uint32_t cap,
			      uint32_t out16_shift = 0 /* != 0: the children receive 2-byte words (uint16_t)(word >> out16_shift); cap counts them */);

/* ---- the sharded join + GROUP BY with first-level regions on the wire (mdb_dev_shard.hip) ------------------------------
 *
 * Every rank partitions ITS rows of a table ONCE with the histogram-free first level of the compact narrow form (512 digits,
 * 8 per-XCD sub-regions each, fixed capacity, 4- or 2-byte words = the k-bit hash of key - window base); the digit's top
 * bits are the destination rank, so the regions of one destination are one contiguous block of a size every rank knows
 * beforehand: the blocks ARE the all-to-all, no counts have to reach a host before it is posted.  The receiver joins the
 * regions it got from all ranks - straight from them when the hash bits below the digit index an LDS table (one level), or
 * after one more partition level of its own - and emits (key, COUNT) pairs; no row ids travel and no result ordering runs
 * (across ranks SQL leaves the order open anyway). */
#define MDB_SHARD_MAX_TABS 4
/* flags of mdb_shard_join in word 0 of ctx->d_status beside the common ones (MDB_ST_REGION_FULL: a region overflowed, MDB_ST_LIST_FULL: cap too
 * small, MDB_ST_KEY_OUTSIDE: a right key outside the window), and the words behind it */
#define MDB_SHARD_ST_PRODUCT_WIDE 2048u	/* a product of the right tables' counts beyond 32 bits */
#define MDB_SHARD_ST_PEER_FAILED 16384u	/* a peer's region counters say that its first level failed (k_shard_regions; mdb_dist.hip sets it for its own rank) */
static_assert(mdb_flags_distinct({ MDB_ST_REGION_FULL, MDB_ST_LIST_FULL, MDB_ST_KEY_OUTSIDE, MDB_SHARD_ST_PRODUCT_WIDE, MDB_SHARD_ST_PEER_FAILED }),
	      "sharded join: two status flags share a bit");
#define MDB_SHARD_STW_GROUPS 1	/* number of groups written */
#define MDB_SHARD_STW_JOINED 2	/* [2..3] joined rows (u64) */
struct mdb_shard_plan {
	uint32_t world, rank;
	uint32_t dbits;			/* first-level digit bits: 9 (the join's own first level), or 12 (the wide fan-out form) */
	uint32_t D, Dp, nsub;		/* first-level digits, digits per destination, sub-regions per digit */
	uint32_t kbits;			/* key window [key_lo, key_lo + 2^kbits) */
	int64_t key_lo;
	uint32_t ntab;			/* tables: [0] the left one, [1] the right one, [2..] further right tables joined on the same key */
	uint32_t cap[MDB_SHARD_MAX_TABS];	/* words per first-level region of each table */
	uint32_t wbytes;		/* bytes per word on the wire: 4, or 2 when the hash bits below the digit fit */
	int b2;				/* receiver: bits of its own partition level (0: the regions are joined as they are) */
	uint32_t rem;			/* key bits that index the leaf tables */
	uint64_t block_words[MDB_SHARD_MAX_TABS];	/* words per destination block = Dp * nsub * cap */
	uint32_t leaf_cap[MDB_SHARD_MAX_TABS];		/* b2 > 0: words per leaf region of the receiver's level */
	bool right_only;		/* GROUP BY of ONE table (it plays the right table; the left one has no rows): a slot's group is its first row, COUNT = its rows */
	uint64_t l_rel_hi;		/* the left table keeps the rows with key - key_lo in [0, l_rel_hi] (= the right table's range) */
};
/* 0 = plan made; 1 = this shape is not served (window too wide, world not a power of two ...): the caller takes another path */
int mdb_shard_plan_make(uint32_t world, uint32_t rank, uint32_t ntab, const uint64_t *n_max /* [ntab]: the largest shard of each table */,
			int64_t l_lo, int64_t l_hi, int64_t r_lo, int64_t r_hi, mdb_shard_plan *plan);
size_t mdb_shard_arena_bytes(const mdb_shard_plan *plan);
/* sender: table 0 = left (rows outside the right table's range are dropped), 1 = right (a key outside the window is reported),
 * 2.. = further right tables (rows outside the window are dropped: they join nothing); *regions = the region buffer
 * (world * block_words[side] words of wbytes bytes, destination-major), *cursors = D * nsub region counters (sub-major).
 * The caller has begun the arena and cleared ctx->d_status[0..15].  No host sync. */
int mdb_shard_partition(mdb_dev_ctx *ctx, const mdb_shard_plan *plan, int side, const int64_t *keys, const uint64_t *nulls, uint64_t n,
			const void **regions, const uint32_t **cursors);
/* receiver: recv[x] = world blocks of block_words[x] words (source-major), cnt[x] = world cursor arrays of D * nsub counters;
 * out_key / out_count (capacity cap): the groups; their number, the joined rows and the flags in ctx->d_status (MDB_SHARD_ST*).  No host sync. */
int mdb_shard_join(mdb_dev_ctx *ctx, const mdb_shard_plan *plan, const void *const *recv, const uint32_t *const *cnt, int64_t *out_key,
		   int64_t *out_count, uint64_t cap, void *const *arrived = NULL /* [ntab] hipEvent_t or NULL: table x's blocks and counters
		   have arrived when arrived[x] has happened - the context's stream waits for it right before the first kernel that reads
		   table x, so the receiver's level over one table runs while the next table is still on the wire */);
/* one 4096-digit pass over a key column of the compact narrow form (mdb_dev_shard.hip): 2-byte words, or 4-byte row words with run headers */
uint32_t mdb_scatter4096_cap(const mdb_dev_ctx *ctx, uint64_t n, bool row_words);
size_t mdb_scatter4096_arena_bytes(const mdb_dev_ctx *ctx, uint64_t n, bool row_words);
int mdb_scatter4096(mdb_dev_ctx *ctx, const int64_t *keys, const uint64_t *nulls, uint64_t n, int64_t key_lo, uint32_t kbits, bool report, uint32_t rel_hi,
		    uint32_t cap, bool row_words, const char *name, void **regions, uint32_t **cursors);

/* ---- ordering of (row id, payload) records (mdb_dev_order.hip) ---------------------------------
 * rec[i] = (row id << (64 - kbits)) | payload (payload >= 1; zero words are gaps), kbits = bits of a row id as
 * returned by mdb_order_records_arena_bytes(); delivers out_first[] = row ids ascending, out_count[] = payloads. */
size_t mdb_order_records_arena_bytes(uint64_t cap, uint64_t n_rows, uint32_t *kbits_out);
int mdb_order_records_by_rowid(mdb_dev_ctx *ctx, const unsigned long long *rec, uint64_t list_len, uint64_t n_rows, uint32_t kbits,
			       uint32_t *out_first, int64_t *out_count);

/* (a, b) pairs of 32-bit ids (a < na, b < nb, unique as pairs; at least 2^18 of them) into ascending (a, b) order
 * (mdb_dev_sort.hip).  0 = done, 1 = not applicable (few pairs, or a's too unevenly spread): the caller sorts another way. */
int mdb_sort_pairs(mdb_dev_ctx *ctx, const uint32_t *a, const uint32_t *b, uint64_t n, uint64_t na, uint64_t nb, uint32_t *out_a,
		   uint32_t *out_b);

/* (key, COUNT) groups -> every key written COUNT times (mdb_dev_pairs.hip): *out = a device array of `joined` keys allocated with
 * mdb_dev_alloc.  joined = the sum of the counts (< 2^32).  Synchronises. */
int mdb_expand_keys_by_count(mdb_dev_ctx *ctx, const int64_t *key, const int64_t *count, uint64_t groups, uint64_t joined, int64_t **out);

/* group i = row i, COUNT 1 (mdb_dev_dense.hip): a GROUP BY over a column whose statistics say MDB_COL_DISTINCT */
int mdb_group_identity(mdb_dev_ctx *ctx, uint64_t n, uint32_t *out_first, int64_t *out_count);

/* ---- a set in device memory (MDB_P_IN_SET): made by mdb_dev_set_create (mdb_dev_filter.hip, from host values) and by
 * mdb_dev_set_from_column (mdb_dev_setbuild.hip, from a device column) */
struct mdb_dev_set {
	void *d_words;		/* the image (mdb_dev.h) in a buffer of mdb_dev_alloc */
	uint64_t slots, members;
	uint32_t log2_slots;
	int32_t type;
};

/* ---- the runs of a stream sorted by its group keys (mdb_dev_runs.hip; device side and the types: mdb_dev_stream.h) ----
 * mdb_dev_sort_perm over the keys (ascending) is stable: every group is one run of rows in stream order, and the run whose head sits at stream
 * position p is the group g with first[g] == p.  Delivered, in buffers of `tmp`: perm (NULL without keys: the stream is one run), hb - bit p =
 * "sorted position p begins a run" (position 0, or a key column differs from the row before: NULL equals NULL, values by their bits) -,
 * base[c] = heads in front of chunk c of MDB_RUNS_CHUNK positions (base[nchunks] = runs) and rungroup[r] = the group of run r.  n, G >= 1.
 * Fails "<op> (<what>): ..." when first[] does not belong to these keys (more runs than groups, a head that is nobody's first row, another
 * number of runs than groups) and "<op>: no device memory ..." when `tmp` cannot hold its buffers.  Synchronises once. */
struct mdb_dev_tmp;
struct mdb_runs {
	const uint32_t *perm;
	const unsigned long long *hb;
	const uint32_t *base;
	const uint32_t *rungroup;
	uint64_t nchunks;
};
int mdb_runs_find(mdb_dev_ctx *ctx, const struct mdb_sort_key *keys, int nkeys, uint64_t n, const uint32_t *first, uint64_t G, const char *op,
		  const char *what, mdb_dev_tmp &tmp, mdb_runs *out);
/* reads a grouped operator's status word (*word, may be NULL, = all of it: the operator's own flags) and fails "<op> (<what>): ..." for
 * the MDB_GROUPS_ST_ flags.  Synchronises. */
int mdb_groups_status(mdb_dev_ctx *ctx, const uint32_t *d_status, const char *op, const char *what, uint32_t *word = NULL);

/* choose level bits so that the average leaf holds about `target` keys */
void mdb_choose_bits(uint64_t n, uint32_t target, int *bits1, int *bits2);

#endif /* MDB_DEV_INTERNAL_H */
