/*
 * mdb_dev_common.h - internals shared by the HIP translation units of the device layer
 * (context, scratch arena, launch/profiling helpers, wave64 primitives).  gfx950 only.
 */
#ifndef MDB_DEV_COMMON_H
#define MDB_DEV_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include <string>
#include <unordered_map>
#include "mdb_dev.h"
#include "mdb_dev_memo.h"

#define MDB_WAVE 64

struct mdb_prof_rec {
	int name_id;
	hipEvent_t start, stop;
};

/* (the base: what the operators remember about key columns, mdb_dev_memo.h) */
struct mdb_dev_ctx : mdb_memo_store {
	int device;
	int num_cus;			/* compute units of the device (256 on MI355X) */
	hipStream_t stream;		/* stream every operator launches on */
	bool own_stream;
	hipStream_t aux_stream;		/* second stream: the two tables of a join are partitioned concurrently */
	hipEvent_t ev_fork, ev_join;
	hipEvent_t ev_status;		/* recorded behind a status copy that a kernel is queued behind: the host waits for the copy alone */
	bool stream_ordered;		/* mdb_dev_results_in_stream_order(): the caller reads result columns in the order of `stream` */
	bool last_return_early;		/* the last join + GROUP BY returned with its ordering kernel still queued (mdb_dev_last_return_was_early) */
	bool overlap;			/* false: everything on the main stream (isolated per-kernel timing) */
	bool last_left_dups_known, last_left_dups;	/* the last join ran through leaf kernels that tell whether a key with partners has several LEFT rows, and whether one has */
	int narrow_mode;		/* 32-bit hashes for int32-range join keys: 0 never, 1 sampled + verified (default), 2 always try */
	int unordered_no_counts;	/* set by mdb_dev_join_keys around its call of the any-order operator: group keys only, no COUNT column */
	/* the caller's MDB_KEYS_MAY_ALIAS / MDB_COUNTS_OPTIONAL of the current join + GROUP BY call (what became of them: plan) */
	bool key_alias_ok, counts_optional;
	void *pending_op;		/* state of a begun-but-unfinished split operator (mdb_dev_join.hip) */
	bool guess_remembered;		/* the last narrow-form decision came from the memo, not from a sample of the data */
	/* mdb_dev_call_stats(): the caller's statistics of the key columns of the calls that follow */
	bool cs_on, cs_has_r;
	const void *cs_kl, *cs_kr;
	struct mdb_dev_col_stats cs_l, cs_r;
	/* mdb_dev_last_plan() / mdb_dev_explain_*(): what the current / last operator did - every operator writes its facts here */
	struct mdb_dev_plan_info plan;
	int pl_depth;			/* operators that call operators: the outermost one's entry clears the plan (mdb_plan_scope) */
	/* mdb_dev_counters(): running totals since the context was created (what a slow call paid for) */
	uint64_t ct_calls, ct_retries, ct_samples, ct_arena_grows, ct_alloc_misses;
	/* mdb_dev_explain_*(): the operator's own decision code runs and stops in front of its first launch (a context without a device) */
	bool explaining;
	bool explain_as_sample;		/* ... as if the statistics were what a key sample found: the forms only a catalog's promise opens are not taken */
	/* mdb_dev_alloc / mdb_dev_free recycle buffers (stream-ordered reuse on the context's stream): a query
	 * allocates dozens of temporaries and hipMalloc/hipFree cost 0.1-0.3 ms each */
	std::unordered_map<void *, size_t> live;		/* buffers handed out -> size */
	std::unordered_map<void *, uint32_t> holders;		/* ... -> holders beyond the first (mdb_dev_retain) */
	std::vector<std::pair<void *, size_t>> cache;		/* released buffers kept for reuse */
	size_t cache_bytes;
	char err[512];
	/* scratch arena (grow-only, bump allocated per operator) */
	char *arena;
	size_t arena_cap;
	size_t arena_off;
	/* device-side status words: [0] = leaf hash-table overflow flag, [1..] scratch */
	uint32_t *d_status;
	/* pinned host mirror for small read-backs */
	uint64_t *h_pinned;
	/* profiling */
	bool prof_on;
	std::vector<std::string> prof_names;
	std::vector<std::vector<const void *>> prof_kernels;	/* per name: the kernel functions (template instances) launched under it */
	std::vector<mdb_prof_rec> prof_recs;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;
	size_t prof_pool_used;
};

int mdb_set_err(mdb_dev_ctx *ctx, int code, const char *fmt, ...);
/* MDB_* environment knobs - the library's ONE reader of the environment, kept per process (mdb_knob.c; mdb_host.h says what each returns) */
extern "C" int mdb_knob_set(const char *name);
extern "C" int mdb_knob_off(const char *name);
extern "C" long long mdb_knob_int(const char *name, long long dflt);
extern "C" int mdb_knob_str(const char *name, char *buf, size_t cap);

/* first statement of every public join / GROUP BY operator: what mdb_dev_last_plan() reports starts at the OUTERMOST operator's entry */
struct mdb_plan_scope {
	mdb_dev_ctx *c;
	explicit mdb_plan_scope(mdb_dev_ctx *ctx) : c(ctx)
	{
		if (c && c->pl_depth++ == 0) {
			memset(&c->plan, 0, sizeof(c->plan));
			c->last_return_early = false;
		}
	}
	~mdb_plan_scope()
	{
		if (c && --c->pl_depth == 0) {
			c->ct_calls++;
			c->ct_retries += c->plan.retries;
			c->ct_samples += c->plan.samples;
		}
	}
};

/* An operator that calls mdb_dev_join_group_count and then works on its result columns outside the context's stream (mdb_dist.hip's transfer
 * stream), or whose use of them has not been checked against mdb_dev_results_in_stream_order(): complete on return inside this scope */
struct mdb_complete_on_return {
	mdb_dev_ctx *c;
	bool was;
	explicit mdb_complete_on_return(mdb_dev_ctx *ctx) : c(ctx), was(ctx && ctx->stream_ordered)
	{
		if (c)
			c->stream_ordered = false;
	}
	~mdb_complete_on_return()
	{
		if (c)
			c->stream_ordered = was;
	}
};

/* mdb_dev_explain_* with as_sample: the statistics stand for what a raw caller's first key sample found */
static inline void mdb_explain_sampled(mdb_dev_ctx *ctx)
{
	if (ctx->explain_as_sample) {
		ctx->plan.from_stats = 0;
		ctx->plan.samples = 1;
	}
}

#define MDB_HIP(ctx, call)                                                                         \
	do {                                                                                       \
		hipError_t e__ = (call);                                                           \
		if (e__ != hipSuccess)                                                             \
			return mdb_set_err((ctx), -MIDORIDB_INTERNAL, "%s failed: %s (%s:%d)", #call, \
					   hipGetErrorString(e__), __FILE__, __LINE__);            \
	} while (0)

/* cached device allocations (mdb_dev_core.hip) */
int mdb_cached_alloc(mdb_dev_ctx *ctx, size_t bytes, void **dptr);
int mdb_cached_free(mdb_dev_ctx *ctx, void *dptr);

/* scratch arena */
int mdb_arena_begin(mdb_dev_ctx *ctx, size_t total_bytes);
void *mdb_arena_take(mdb_dev_ctx *ctx, size_t bytes);
/* behind the 128 status words of ctx->d_status: a block of counters that one memset clears together with them at the start of an
 * operator call - the first-level cursors of both tables (2 x 4096 words) and the ordering ranges' fills (2048 words) - instead of a
 * fill command each (5 us apiece between two kernels) */
#define MDB_ZERO_BLK_OFF 128u
#define MDB_ZERO_BLK_SLOT 4096u
#define MDB_ZERO_BLK_WORDS (2u * MDB_ZERO_BLK_SLOT + 2048u)
static inline size_t mdb_align_up(size_t x) { return (x + 255) & ~(size_t)255; }

/* ---- ctx->d_status: how every device operator reports to the host.  Word 0 holds flag bits (mdb_raise), the words behind it
 * counters and scratch values that each operator names for itself.  The flags below cross the translation units: the partition,
 * scatter and ordering kernels raise them, every operator reads them, and they mean the same wherever they appear.  What an
 * operator adds of its own has that operator's prefix (GC_ST_, PJ_ST_, RJ_ST_, SORT_ST_ ...) and a static_assert next to it
 * that none of its flags shares a bit with another or with these. */
#define MDB_ST_REGION_FULL 2u	/* a fixed-capacity region (histogram-free partition level, scatter pass, ordering range) overflowed: redo with the exact layout */
#define MDB_ST_LIST_FULL 8u	/* an output list sized by the caller is exhausted */
#define MDB_ST_KEY_OUTSIDE 128u	/* a key outside the window / the int32 range the caller's form assumes */
#define MDB_FLAG_SET 1u		/* a scratch word of its own used as ONE boolean (not word 0): "seen" */
#define MDB_STW_FLAGS 0		/* index of the flag word */
#define MDB_STW_UTIL 12		/* [12..15] scratch of the stand-alone utilities (mdb_dev_combine_counts, mdb_dev_key_range, the distinct scan): no operator is running */

/* every flag one bit, no bit twice */
template <size_t N> constexpr bool mdb_flags_distinct(const uint32_t (&f)[N])
{
	uint64_t sum = 0;
	uint32_t any = 0;
	for (size_t i = 0; i < N; i++) {
		if (!f[i] || (f[i] & (f[i] - 1u)))
			return false;
		sum += f[i];
		any |= f[i];
	}
	return sum == any;
}
static_assert(mdb_flags_distinct({ MDB_ST_REGION_FULL, MDB_ST_LIST_FULL, MDB_ST_KEY_OUTSIDE }), "common status flags share a bit");

/* ---- ctx->h_pinned (1024 8-byte words): the staging slots that may be in use at the same time, by 8-byte word.  A read-back stays
 * valid until the next copy into the same slot; host-to-device sources must stay untouched until the stream has passed them. */
#define MDB_HP_COUNT 0		/* one count read back on its own (or an operator's whole read-back when nothing else is in flight) */
#define MDB_HP_STATUS 1		/* [1..7] up to 56 bytes of d_status from word 0 on (struct gc_readback and its kin) */
#define MDB_HP_SORT_FLAGS 8	/* the ordering sort's look at the flag word while [1..7] are still being read */
#define MDB_HP_HOT 9		/* the hot-key path's number of hot leaves */
#define MDB_HP_SORT_OUTSIDE 12	/* the ORDER BY pack's count of keys outside the sampled range */
#define MDB_HP_PART_TILES 15	/* the pruned left pass's number of second-level tiles (read inside the operator, before its status) */
#define MDB_HP_SEND_SHARD 256	/* host -> device: the sharded operator's pruning range (two 4-byte words) */
#define MDB_HP_SEND_RANGE 260	/* host -> device: the fused operator's key window as a pruning range; the sharded operator's "a peer failed" flag word */
#define MDB_HP_SEND_FLAGS 264	/* host -> device: the fused operator's flag word with the retried bits taken out (the window may still be on its way) */

/* run the following launches on the auxiliary stream (after everything queued so far on the main
 * stream), and come back; between the two calls ctx->stream IS the auxiliary stream */
int mdb_aux_begin(mdb_dev_ctx *ctx, hipStream_t *saved_main);
int mdb_aux_end(mdb_dev_ctx *ctx, hipStream_t saved_main);	/* back to the main stream; marks the end of the aux work */
int mdb_aux_join(mdb_dev_ctx *ctx);				/* main stream waits for the marked aux work */

/* profiling hooks around one launch */
void mdb_prof_begin(mdb_dev_ctx *ctx, const char *name, const void *kernel);
void mdb_prof_end(mdb_dev_ctx *ctx);

#define MDB_LAUNCH(ctx, name, kernel, grid, block, ...)                                            \
	do {                                                                                       \
		mdb_prof_begin((ctx), (name), (const void *)(kernel));                             \
		hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (ctx)->stream, __VA_ARGS__); \
		mdb_prof_end((ctx));                                                               \
		hipError_t le__ = hipGetLastError();                                               \
		if (le__ != hipSuccess)                                                            \
			return mdb_set_err((ctx), -MIDORIDB_INTERNAL, "launch %s failed: %s", (name), \
					   hipGetErrorString(le__));                               \
	} while (0)

/* the same with dynamic LDS */
#define MDB_LAUNCH_LDS(ctx, name, kernel, grid, block, lds_bytes, ...)                             \
	do {                                                                                       \
		mdb_prof_begin((ctx), (name), (const void *)(kernel));                             \
		hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), (lds_bytes), (ctx)->stream, __VA_ARGS__); \
		mdb_prof_end((ctx));                                                               \
		hipError_t le__ = hipGetLastError();                                               \
		if (le__ != hipSuccess)                                                            \
			return mdb_set_err((ctx), -MIDORIDB_INTERNAL, "launch %s failed: %s", (name), \
					   hipGetErrorString(le__));                               \
	} while (0)

/* ------------------------------------------------------------------ device helpers */
#ifdef __HIPCC__

/* murmur3 fmix64: a bijection on 64-bit words (so the hashed value identifies the key),
 * fmix64(0) == 0. */
__host__ __device__ static inline uint64_t mdb_fmix64(uint64_t k)
{
	k ^= k >> 33;
	k *= 0xff51afd7ed558ccdULL;
	k ^= k >> 33;
	k *= 0xc4ceb9fe1a85ec53ULL;
	k ^= k >> 33;
	return k;
}

/* murmur3 fmix32: a bijection on 32-bit words, fmix32(0) == 0.  The narrow form of the join (every key of both
 * tables inside the int32 range) partitions and compares 32-bit hashes. */
__host__ __device__ static inline uint32_t mdb_fmix32(uint32_t h)
{
	h ^= h >> 16;
	h *= 0x85EBCA6Bu;
	h ^= h >> 13;
	h *= 0xC2B2AE35u;
	h ^= h >> 16;
	return h;
}

/* The same finaliser on k-bit words (8 <= k <= 32): x ^= x >> s and a multiplication by an odd constant modulo 2^k are
 * both bijections of [0, 2^k), so mixk is one, and mixk(0) == 0.  The compact narrow form uses it on key - window base: a
 * key column whose values span fewer than 2^k values hashes into k bits, the radix partition consumes the top bits and what
 * is left below them is small enough to INDEX a per-leaf table in LDS directly (mdb_dev_join_leaf.hip, k_leaf_direct). */
__host__ __device__ static inline uint32_t mdb_mixk(uint32_t x, uint32_t k)
{
	const uint32_t mask = k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);
	const uint32_t s = (k + 1) >> 1;
	x ^= x >> s;
	x = (x * 0x85EBCA6Bu) & mask;
	x ^= x >> s;
	x = (x * 0xC2B2AE35u) & mask;
	x ^= x >> s;
	return x;
}

/* inverse of mdb_mixk: x ^= x >> s is an involution on k-bit words (2 s >= k), the multipliers have inverses modulo 2^32
 * and therefore modulo 2^k */
__host__ __device__ static inline uint32_t mdb_unmixk(uint32_t x, uint32_t k)
{
	const uint32_t mask = k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);
	const uint32_t s = (k + 1) >> 1;
	x ^= x >> s;
	x = (x * 0x7ED1B41Du) & mask;		/* 0xC2B2AE35^-1 */
	x ^= x >> s;
	x = (x * 0xA5CB9243u) & mask;		/* 0x85EBCA6B^-1 */
	x ^= x >> s;
	return x;
}

/* inverse of mdb_fmix64 (modular inverses of the two odd multipliers; x ^= x >> 33 is an involution
 * on 64-bit words because 2*33 >= 64). */
__host__ __device__ static inline uint64_t mdb_fmix64_inv(uint64_t k)
{
	k ^= k >> 33;
	k *= 0x9cb4b2f8129337dbULL;
	k ^= k >> 33;
	k *= 0x4f74430c22a54005ULL;
	k ^= k >> 33;
	return k;
}

__device__ static inline uint32_t mdb_lane(void) { return threadIdx.x & (MDB_WAVE - 1); }
__device__ static inline uint64_t mdb_lanemask_lt(void) { return (1ull << mdb_lane()) - 1ull; }

/* inclusive scan across the 64 lanes of a wave: data-parallel-primitive moves inside the vector ALU (shifts by 1, 2, 4, 8 inside
 * every row of 16 lanes, then the last lane of a row broadcast to the next row, then lane 31 to the upper half) - six adds, no
 * trip through the LDS crossbar (six ds_bpermute round trips of ~60 cycles each before) */
__device__ static inline uint32_t mdb_wave_incl_scan(uint32_t v)
{
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xF, 0xF, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112 /* row_shr:2 */, 0xF, 0xF, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114 /* row_shr:4 */, 0xF, 0xF, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118 /* row_shr:8 */, 0xF, 0xF, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142 /* row_bcast:15 */, 0xA, 0xF, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143 /* row_bcast:31 */, 0xC, 0xF, false);
	return v;
}

/* Block-wide exclusive scan of one value per thread.  blockDim.x must be a multiple of 64 and
 * <= 1024; `tmp` is LDS scratch of at least 17 words.  Returns the exclusive prefix, *total the
 * block sum.  Contains __syncthreads(): call from uniform control flow.
 * Every wave scans the (at most 16) wave totals itself: two barriers and no serial walk by one thread (which cost 2 000 -
 * 4 000 cycles per call with 16 waves - a quarter of a partition tile's fixed costs). */
__device__ static inline uint32_t mdb_block_excl_scan(uint32_t v, uint32_t *tmp, uint32_t *total)
{
	const uint32_t wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6, lane = mdb_lane();
	const uint32_t incl = mdb_wave_incl_scan(v);
	__syncthreads();	/* protect tmp against a previous use */
	if (lane == MDB_WAVE - 1)
		tmp[wave] = incl;
	__syncthreads();
	const uint32_t pi = mdb_wave_incl_scan(lane < nwaves ? tmp[lane] : 0u);
	*total = (uint32_t)__shfl((int)pi, (int)nwaves - 1, MDB_WAVE);
	const uint32_t before = (uint32_t)__shfl((int)pi, wave ? (int)wave - 1 : 0, MDB_WAVE);
	return incl - v + (wave ? before : 0u);
}

/* Raise flag bits in a device status word.  The word is looked at first: a condition that holds for every row of a
 * table (duplicate keys under the unique-key join, wide keys under the narrow form) would otherwise send one global
 * atomic per row to a single address - 10^8 of them took 18 ms. */
__device__ static inline void mdb_raise(uint32_t *status, uint32_t bits)
{
	if ((*(volatile const uint32_t *)status & bits) != bits)
		atomicOr(status, bits);
}

__device__ static inline bool mdb_bit_is_set(const uint64_t *bits, uint64_t i)
{
	return (bits[i >> 6] >> (i & 63)) & 1ull;
}

#endif /* __HIPCC__ */
#endif /* MDB_DEV_COMMON_H */
