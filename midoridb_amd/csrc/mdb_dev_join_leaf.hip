/*
 * mdb_dev_join_leaf.hip - the per-leaf LDS kernels of the fused join + GROUP BY key + COUNT(*) operator and their launchers (split off
 * mdb_dev_join.hip; what the files share: mdb_dev_join_internal.h): hashed tables (k_leaf_group_count), direct-address tables of the
 * compact narrow form (k_leaf_direct), the semi-join bitmap (k_leaf_bitmap), hot keys across the whole chip (k_hot_*), the NULL group
 * (k_null_*).  The kernels that join a whole first-level digit per workgroup live in mdb_dev_leaf_wide.hip.  A launcher takes the
 * kernels' argument block and the few scalars its grid needs; the driver in mdb_dev_join.hip decides which one runs.
 *
 * After mdb_partition_table() every leaf holds all rows (of both tables) whose hashed key shares
 * the same top bits (in unspecified order; orders are restored from the row ids).  Persistent
 * workgroups walk the leaves: each builds an open-addressing hash table in LDS keyed by the 64-bit
 * hashed key (fmix64 is a bijection, so equal hash <=> equal key; the value 0 = "empty slot", the
 * single key that hashes to 0 is kept in a dedicated side slot) from the side with fewer rows, then
 * streams the other side through it.  All counters are LDS atomics; global memory is read once,
 * coalesced, and written once.  Groups leave as 64-bit records (first row id, COUNT) that a radix
 * sort + k_order_leaf put into the reference's order; hot keys take the k_hot_* path.
 */
#include "mdb_dev_join_internal.h"

/* ------------------------------------------------------------------ fused join + group count */

/*
 * Persistent form: gridDim.x workgroups (2 per CU) walk the leaves with stride gridDim.x.  The first
 * LEAF_BATCH keys per thread of BOTH sides of the next leaf are requested before the current leaf's
 * results are emitted and the tables re-initialised, so the HBM round trip overlaps LDS work instead of
 * being paid three times per leaf (offsets -> left keys -> right keys), which made the one-leaf-per-
 * workgroup version latency-bound (70 % of wave time in s_waitcnt, profiles/r01).
 */
struct gc_batch {
	uint64_t hv_l[LEAF_BATCH];
	uint32_t rid_l[LEAF_BATCH];
	uint64_t hv_r[LEAF_BATCH];
	uint32_t h32_r[LEAF_BATCH];	/* narrow form: the right side's 4-byte words */
};

/* the same in two steps, so that the words can be requested one whole leaf before they are needed */
__device__ static inline uint2 gc_leaf_raw(const uint32_t *off, const uint32_t *cnt, uint32_t cap, uint32_t leaf)
{
	/* The index is hidden from the uniformity analysis: a load the compiler knows to be wave-uniform is moved into
	 * scalar registers on arrival, i.e. waited for on the spot.  gc_leaf_decode() makes the words scalar again, one
	 * leaf later. */
	asm volatile("" : "+v"(leaf));
	uint2 w;
	if (cap) {
		w.x = cnt[leaf];
		w.y = 0;
	} else {
		w.x = off[leaf];
		w.y = off[leaf + 1];
	}
	return w;
}

__device__ static inline void gc_leaf_decode(uint2 w, uint32_t cap, uint32_t leaf, uint32_t *b, uint32_t *e)
{
	w.x = __builtin_amdgcn_readfirstlane(w.x);
	w.y = __builtin_amdgcn_readfirstlane(w.y);
	if (cap) {
		*b = leaf * cap;
		*e = *b + (w.x < cap ? w.x : cap);
	} else {
		*b = w.x;
		*e = w.y;
	}
}

/* NW: 0 = 64-bit hashes, 1 = narrow words, 2 = whatever gc_args.narrow says (the rarely taken hot-key kernels) */
template <int NW>
__device__ static inline bool gc_is_narrow(const gc_args &a)
{
	return NW == 2 ? a.narrow != 0 : NW == 1;
}

/* The batch keeps the words as loaded (a conversion at load time would make the prefetch wait for its own loads);
 * they are decoded where they are consumed. */
template <bool IS_L, int NW>
__device__ static inline uint64_t gc_batch_hv(const gc_args &a, const gc_batch &b, int u)
{
	if (!gc_is_narrow<NW>(a))
		return IS_L ? b.hv_l[u] : b.hv_r[u];
	if (IS_L)
		return gc_narrow_hv(b.hv_l[u]);
	return ((uint64_t)b.h32_r[u] << 32) | b.h32_r[u];	/* right side: 4-byte words */
}

template <int NW>
__device__ static inline uint32_t gc_batch_rid(const gc_args &a, const gc_batch &b, int u)
{
	return gc_is_narrow<NW>(a) ? (uint32_t)b.hv_l[u] : b.rid_l[u];
}

template <int NW>
__device__ static inline void gc_load_l(const gc_args &a, uint32_t base, uint32_t end, gc_batch &b)
{
#pragma unroll
	for (int u = 0; u < LEAF_BATCH; u++) {
		const uint32_t i = base + (uint32_t)u * GC_THREADS + threadIdx.x;
		b.hv_l[u] = 0;
		b.rid_l[u] = 0;
		if (i < end) {
			b.hv_l[u] = a.hv_l[i];
			if (!gc_is_narrow<NW>(a))
				b.rid_l[u] = a.rid_l[i];
		}
	}
}

template <int NW>
__device__ static inline void gc_load_r(const gc_args &a, uint32_t base, uint32_t end, gc_batch &b)
{
#pragma unroll
	for (int u = 0; u < LEAF_BATCH; u++) {
		const uint32_t j = base + (uint32_t)u * GC_THREADS + threadIdx.x;
		if (gc_is_narrow<NW>(a)) {
			b.h32_r[u] = 0;
			if (j < end)
				b.h32_r[u] = reinterpret_cast<const uint32_t *>(a.hv_r)[j];
		} else {
			b.hv_r[u] = j < end ? a.hv_r[j] : 0;
		}
	}
}

template <bool HAS_R, int NW>
__device__ static inline void gc_prefetch(const gc_args &a, uint32_t l0, uint32_t l1, uint32_t r0, uint32_t r1, gc_batch &b)
{
#pragma unroll
	for (int u = 0; u < LEAF_BATCH; u++) {
		const uint32_t i = l0 + (uint32_t)u * GC_THREADS + threadIdx.x;
		b.hv_l[u] = 0;
		b.rid_l[u] = 0;
		if (i < l1) {
			b.hv_l[u] = a.hv_l[i];
			if (!gc_is_narrow<NW>(a))
				b.rid_l[u] = a.rid_l[i];
		}
		if (HAS_R) {
			const uint32_t j = r0 + (uint32_t)u * GC_THREADS + threadIdx.x;
			if (gc_is_narrow<NW>(a)) {
				b.h32_r[u] = 0;
				if (j < r1)
					b.h32_r[u] = reinterpret_cast<const uint32_t *>(a.hv_r)[j];
			} else {
				b.hv_r[u] = j < r1 ? a.hv_r[j] : 0;
			}
		}
	}
}

/* One side of a leaf goes INTO the table (insert-or-find, count, first left row id) ... */
__device__ static inline uint32_t gc_wave_min_u32(uint32_t v)
{
#pragma unroll
	for (int d = 1; d < MDB_WAVE; d <<= 1) {
		const uint32_t o = (uint32_t)__shfl_xor((int)v, d, MDB_WAVE);
		v = o < v ? o : v;
	}
	return v;
}

/* MERGE (the plain GROUP BY instance): lanes of a wave that hold the same value are merged before the table is touched -
 * one insert + one counter update for the group instead of one per row on the same LDS address (GROUP BY over 10^4 - 10^6
 * distinct values: leaves with a few values and thousands of rows).  Given up after the first round that finds no
 * duplicates of the leader, so columns of distinct values pay one ballot. */
template <bool IS_L, int NW, bool MERGE = false>
__device__ static inline void gc_build_side(const gc_args &a, unsigned long long *s_key, unsigned long long *s_cnt, uint32_t *s_first,
					    gc_batch &b, uint32_t x0, uint32_t x1, uint32_t own[LEAF_BATCH])
{
	for (uint32_t base = x0; base < x1; base += GC_THREADS * LEAF_BATCH) {
		if (base != x0) {
			if (IS_L)
				gc_load_l<NW>(a, base, x1, b);
			else
				gc_load_r<NW>(a, base, x1, b);
		}
		/* first probe of every key of the batch issued back to back (the CAS round trips overlap);
		 * only keys whose first slot is taken by another key walk on, one after the other */
		uint32_t s_[LEAF_BATCH], step_[LEAF_BATCH];
		unsigned long long old_[LEAF_BATCH];
		bool act_[LEAF_BATCH];
		uint32_t mult_[LEAF_BATCH], rid_[LEAF_BATCH];
		bool drop_[LEAF_BATCH];
#pragma unroll
		for (int u = 0; u < LEAF_BATCH; u++) {
			const uint32_t i = base + (uint32_t)u * GC_THREADS + threadIdx.x;
			const uint64_t hv = gc_batch_hv<IS_L, NW>(a, b, u);
			mult_[u] = 1;
			rid_[u] = IS_L ? gc_batch_rid<NW>(a, b, u) : 0u;
			drop_[u] = false;
			if (MERGE && (a.merge_all || x1 - x0 > GC_THREADS * LEAF_BATCH)) {	/* (uniform) a leaf beyond one register batch holds
												 * duplicates for sure; merge_all: the sample says most do */
				const bool in = i < x1;
				uint64_t pending = __ballot(in);
				for (int round = 0; round < 8 && pending; round++) {
					const int leader = __ffsll((long long)pending) - 1;
					const uint32_t llo = (uint32_t)__shfl((int)(uint32_t)hv, leader, MDB_WAVE);
					const uint32_t lhi = (uint32_t)__shfl((int)(uint32_t)(hv >> 32), leader, MDB_WAVE);
					const bool same = in && !drop_[u] && (uint32_t)hv == llo && (uint32_t)(hv >> 32) == lhi;
					const uint64_t grp = __ballot(same);
					const uint32_t cnt = (uint32_t)__popcll(grp);
					if (cnt < 8)
						break;		/* few lanes per value: the LDS atomics cope, and a round costs more than it saves */
					const uint32_t rmin = IS_L ? gc_wave_min_u32(same ? rid_[u] : 0xFFFFFFFFu) : 0u;
					if (same) {
						if ((int)mdb_lane() == leader) {
							mult_[u] = cnt;
							rid_[u] = rmin;
						} else {
							drop_[u] = true;
						}
					}
					pending &= ~grp;
				}
			}
			if (base == x0)
				own[u] = 0xFFFFFFFFu;
			act_[u] = i < x1 && hv != 0 && !drop_[u];
			s_[u] = leaf_slot(hv, GC_SLOTS);
			step_[u] = leaf_step(hv, GC_SLOTS);
			old_[u] = act_[u] ? atomicCAS(&s_key[s_[u]], 0ull, (unsigned long long)hv) : 0ull;
		}
#pragma unroll
		for (int u = 0; u < LEAF_BATCH; u++) {
			const uint32_t i = base + (uint32_t)u * GC_THREADS + threadIdx.x;
			const uint64_t hv = gc_batch_hv<IS_L, NW>(a, b, u);
			if (i >= x1 || drop_[u])
				continue;
			uint32_t s = GC_SLOTS;		/* the key whose hash is 0 has the side slot */
			bool created = false;
			if (act_[u]) {
				s = s_[u];
				unsigned long long old = old_[u];
				uint32_t probe = 1;
				while (old != 0ull && old != hv) {
					if (probe++ >= GC_SLOTS) {
						s = 0xFFFFFFFFu;
						break;
					}
					s += step_[u];
					if (s >= GC_SLOTS)
						s -= GC_SLOTS;
					old = atomicCAS(&s_key[s], 0ull, (unsigned long long)hv);
				}
				created = old == 0ull;
			}
			if (s == 0xFFFFFFFFu) {
				mdb_raise(a.status, GC_ST_TABLE_FULL);
			} else {
				if (IS_L) {
					atomicAdd(&s_cnt[s], (unsigned long long)mult_[u]);
					atomicMin(&s_first[s], rid_[u]);
				} else {
					atomicAdd(&s_cnt[s], (unsigned long long)mult_[u] << 32);
				}
				if (created && base == x0)
					own[u] = s;	/* this thread emits (and clears) the group */
			}
		}
	}
}

/* ... and the other side only LOOKS UP: a key that is not in the table costs one LDS read */
template <bool IS_L, int NW>
__device__ static inline void gc_probe_side(const gc_args &a, const unsigned long long *s_key, unsigned long long *s_cnt, uint32_t *s_first,
					    gc_batch &b, uint32_t x0, uint32_t x1)
{
	for (uint32_t base = x0; base < x1; base += GC_THREADS * LEAF_BATCH) {
		if (base != x0) {
			if (IS_L)
				gc_load_l<NW>(a, base, x1, b);
			else
				gc_load_r<NW>(a, base, x1, b);
		}
		/* same shape as the build: the first slot of every key is read before any is examined */
		uint32_t ps_[LEAF_BATCH], pstep_[LEAF_BATCH];
		unsigned long long cur_[LEAF_BATCH];
#pragma unroll
		for (int u = 0; u < LEAF_BATCH; u++) {
			const uint64_t hv = gc_batch_hv<IS_L, NW>(a, b, u);
			ps_[u] = leaf_slot(hv, GC_SLOTS);
			pstep_[u] = leaf_step(hv, GC_SLOTS);
			cur_[u] = s_key[ps_[u]];
		}
#pragma unroll
		for (int u = 0; u < LEAF_BATCH; u++) {
			const uint32_t j = base + (uint32_t)u * GC_THREADS + threadIdx.x;
			const uint64_t hv = gc_batch_hv<IS_L, NW>(a, b, u);
			if (j >= x1)
				continue;
			uint32_t s = GC_SLOTS;
			if (hv != 0) {
				unsigned long long cur = cur_[u];
				uint32_t probe = 1;
				s = ps_[u];
				while (cur != hv) {
					if (cur == 0ull || probe++ >= GC_SLOTS) {
						s = 0xFFFFFFFFu;
						break;
					}
					s += pstep_[u];
					if (s >= GC_SLOTS)
						s -= GC_SLOTS;
					cur = s_key[s];
				}
			}
			if (s != 0xFFFFFFFFu) {
				if (IS_L) {
					atomicAdd(&s_cnt[s], 1ull);
					atomicMin(&s_first[s], gc_batch_rid<NW>(a, b, u));
				} else {
					atomicAdd(&s_cnt[s], 1ull << 32);
				}
			}
		}
	}
}

/* Hot keys.  A leaf that received tens of thousands of rows holds few distinct keys with very many duplicates
 * (more distinct keys than table slots is an error anyway), and one LDS atomic per row on the same slot serialises:
 * 2*10^7 rows of one key took 77 ms.  For such leaves (GC_HEAVY rows or more on the side at hand) the lanes of a wave
 * first merge their duplicates - leader's key, ballot of the lanes that hold the same key, one table operation for
 * the whole group - so the table sees one update per distinct key per wave instead of one per row. */

template <bool IS_L, bool INSERT, int NW = 2>
__device__ static inline void gc_side_heavy(const gc_args &a, unsigned long long *s_key, unsigned long long *s_cnt, uint32_t *s_first,
					    gc_batch &b, uint32_t x0, uint32_t x1)
{
	for (uint32_t base = x0; base < x1; base += GC_THREADS * LEAF_BATCH) {
		if (base != x0) {
			if (IS_L)
				gc_load_l<NW>(a, base, x1, b);
			else
				gc_load_r<NW>(a, base, x1, b);
		}
#pragma unroll
		for (int u = 0; u < LEAF_BATCH; u++) {
			const uint32_t i = base + (uint32_t)u * GC_THREADS + threadIdx.x;
			const uint64_t hv = gc_batch_hv<IS_L, NW>(a, b, u);
			const uint32_t rid = IS_L ? gc_batch_rid<NW>(a, b, u) : 0u;
			const bool active = i < x1;
			uint64_t pending = __ballot(active);
			while (pending) {	/* wave-uniform: one round per distinct key among the wave's rows */
				const int leader = __ffsll((long long)pending) - 1;
				const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)hv, leader, MDB_WAVE);
				const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(hv >> 32), leader, MDB_WAVE);
				const uint64_t lhv = ((uint64_t)hi << 32) | lo;
				const bool mine = active && hv == lhv;
				const uint64_t grp = __ballot(mine);
				const uint32_t rmin = IS_L ? gc_wave_min_u32(mine ? rid : 0xFFFFFFFFu) : 0u;
				if ((int)mdb_lane() == leader) {
					uint32_t s = GC_SLOTS;
					if (lhv != 0)
						s = INSERT ? leaf_insert(s_key, GC_SLOTS, lhv) : leaf_find(s_key, GC_SLOTS, lhv);
					if (s == 0xFFFFFFFFu) {
						if (INSERT)
							mdb_raise(a.status, GC_ST_TABLE_FULL);
					} else if (IS_L) {
						atomicAdd(&s_cnt[s], (unsigned long long)__popcll(grp));
						atomicMin(&s_first[s], rmin);
					} else {
						atomicAdd(&s_cnt[s], (unsigned long long)__popcll(grp) << 32);
					}
				}
				pending &= ~grp;
			}
		}
	}
}

template <bool HAS_R, bool BUILD_R, bool HEAVY, bool NARROW = false>
__global__ __launch_bounds__(GC_THREADS, 8) void k_leaf_group_count(gc_args a)
{
	constexpr int NW = HEAVY ? 2 : (NARROW ? 1 : 0);
	/* The HEAVY instance (single-workgroup fallback of the hot-key path) only works when the plain one met hot leaves. */
	if (HEAVY) {
		const uint32_t st = *(volatile const uint32_t *)a.status;
		if ((st & 2u) || !(st & 64u))
			return;
	}

	/* slot = hashed key (0 = empty) + packed counters (low 32 bits: left rows, high 32 bits: right rows)
	 * + first left row id.  The tables are zeroed once; afterwards the emit pass clears exactly the slots
	 * it reads as occupied, which halves the LDS traffic of a clear-everything-per-leaf loop. */
	__shared__ unsigned long long s_key[GC_SLOTS];
	__shared__ unsigned long long s_cnt[GC_SLOTS + 1];	/* [GC_SLOTS] = the key whose hash is 0 */
	__shared__ uint32_t s_first[GC_SLOTS + 1];
	__shared__ unsigned long long s_sum;
	__shared__ uint32_t s_chunk[4];		/* record list chunk of this workgroup: [0] base [1] used [2] size [3] valid records */

	for (uint32_t s = threadIdx.x; s <= GC_SLOTS; s += GC_THREADS) {
		if (s < GC_SLOTS)
			s_key[s] = 0ull;
		s_cnt[s] = 0ull;
		s_first[s] = 0xFFFFFFFFu;
	}
	if (threadIdx.x == 0)
		s_sum = 0ull;
	if (threadIdx.x < 4)
		s_chunk[threadIdx.x] = 0;	/* size 0: the first live leaf reserves a chunk */
	unsigned long long mine = 0;
	uint32_t nvalid = 0;

	uint32_t leaf = blockIdx.x;
	uint32_t l0 = 0, l1 = 0, r0 = 0, r1 = 0;
	gc_batch b;
	/* Leaf ranges are requested TWO leaves ahead and decoded one iteration later: read where they are needed (or one
	 * leaf ahead but converted at once) each of the two loads was followed by s_waitcnt vmcnt(0) - two exposed L2 round
	 * trips per leaf on the critical path of a kernel that has ~4 us per leaf. */
	uint2 raw_l = make_uint2(0, 0), raw_r = make_uint2(0, 0);	/* of leaf + gridDim.x */
	if (leaf < a.nleaves) {
		gc_leaf_range(a.off_l, a.cnt_l, a.cap_l, leaf, &l0, &l1);
		if (HAS_R)
			gc_leaf_range(a.off_r, a.cnt_r, a.cap_r, leaf, &r0, &r1);
		gc_prefetch<HAS_R, NW>(a, l0, l1, r0, r1, b);
		if (leaf + gridDim.x < a.nleaves) {
			raw_l = gc_leaf_raw(a.off_l, a.cnt_l, a.cap_l, leaf + gridDim.x);
			if (HAS_R)
				raw_r = gc_leaf_raw(a.off_r, a.cnt_r, a.cap_r, leaf + gridDim.x);
		}
	}
	__syncthreads();
	while (leaf < a.nleaves) {
		const uint32_t next = leaf + gridDim.x, next2 = next + gridDim.x;
		uint32_t nl0 = 0, nl1 = 0, nr0 = 0, nr1 = 0;
		if (next < a.nleaves) {		/* requested during the previous leaf */
			gc_leaf_decode(raw_l, a.cap_l, next, &nl0, &nl1);
			if (HAS_R)
				gc_leaf_decode(raw_r, a.cap_r, next, &nr0, &nr1);
		}
		if (next2 < a.nleaves) {	/* in flight during this leaf, decoded at the top of the next */
			raw_l = gc_leaf_raw(a.off_l, a.cnt_l, a.cap_l, next2);
			if (HAS_R)
				raw_r = gc_leaf_raw(a.off_r, a.cnt_r, a.cap_r, next2);
		}
		const bool nonempty = l0 != l1 && (!HAS_R || r0 != r1);	/* otherwise no group can come out of this leaf */
		const bool heavy_l = l1 - l0 >= a.heavy_l, heavy_r = HAS_R && r1 - r0 >= a.heavy_r;	/* hot keys: see gc_side_heavy */
		const bool hot = nonempty && (heavy_l || heavy_r);
		const bool live = HEAVY ? hot : (nonempty && !hot);
		if (!HEAVY && hot && threadIdx.x == 0)
			mdb_raise(a.status, GC_ST_HOT_LEAVES);	/* left to the hot-key path */
		/* a leaf whose left side fits one register batch (the normal case) is emitted by the threads that
		 * created its table slots; only oversized (skewed) leaves scan the whole table */
		const uint32_t build_rows = (HAS_R && BUILD_R) ? r1 - r0 : l1 - l0;
		const bool by_owner = build_rows <= GC_THREADS * LEAF_BATCH;
		uint32_t own[LEAF_BATCH];
		if (live && a.kbits) {
			/* Record list space: this leaf emits at most one record per left row (and per table slot).
			 * When the workgroup's current chunk cannot hold that, the unused tail is zero-filled (the
			 * ordering sort skips zero records) and a new chunk is reserved with ONE global atomic - i.e.
			 * one atomic per ~10-170 leaves instead of one on the critical path of every leaf. */
			const uint32_t rows = (HAS_R && (r1 - r0) < (l1 - l0)) ? r1 - r0 : l1 - l0;	/* a group needs a row on both sides */
			const uint32_t need = (rows < GC_SLOTS ? rows : GC_SLOTS) + 1;
			const uint32_t base = s_chunk[0], used = s_chunk[1], size = s_chunk[2];
			if (used + need > size) {		/* uniform: every thread read the same words */
				for (uint32_t i = used + threadIdx.x; i < size; i += GC_THREADS)
					a.rec[base + i] = 0ull;
				__syncthreads();		/* everyone has read s_chunk */
				if (threadIdx.x == 0) {
					const uint32_t want = need > GC_REC_CHUNK ? need : GC_REC_CHUNK;
					const uint32_t nb = atomicAdd(a.rec_count, want);
					if (nb + want > a.rec_cap) {
						mdb_raise(a.status, MDB_ST_LIST_FULL);	/* list capacity exhausted: sizing bug, reported as an error */
						s_chunk[0] = 0;
						s_chunk[2] = 0;
					} else {
						s_chunk[0] = nb;
						s_chunk[2] = want;
					}
					s_chunk[1] = 0;
				}
				/* visible to everyone after the barrier that ends the build phase */
			}
		}
		if (live) {
			/* The table is built from the side with fewer rows per leaf (the right one when it is not the
			 * larger table): with N:1 data (every left key unique, few of them matched) the left rows then
			 * cost one LDS read each instead of an insert, a count, a minimum and a clear. */
			if (HAS_R && BUILD_R) {
				if (HEAVY && heavy_r)
					gc_side_heavy<false, true>(a, s_key, s_cnt, s_first, b, r0, r1);
				else
					gc_build_side<false, NW>(a, s_key, s_cnt, s_first, b, r0, r1, own);
				__syncthreads();
				if (HEAVY && heavy_l)
					gc_side_heavy<true, false>(a, s_key, s_cnt, s_first, b, l0, l1);
				else
					gc_probe_side<true, NW>(a, s_key, s_cnt, s_first, b, l0, l1);
				__syncthreads();
			} else {
				if (HEAVY && heavy_l)
					gc_side_heavy<true, true>(a, s_key, s_cnt, s_first, b, l0, l1);
				else
					gc_build_side<true, NW, !HAS_R>(a, s_key, s_cnt, s_first, b, l0, l1, own);
				__syncthreads();
				if (HAS_R) {
					if (HEAVY && heavy_r)
						gc_side_heavy<false, false>(a, s_key, s_cnt, s_first, b, r0, r1);
					else
						gc_probe_side<false, NW>(a, s_key, s_cnt, s_first, b, r0, r1);
					__syncthreads();
				}
			}
		}

		/* request the next leaf's first batches now: they travel while this leaf is emitted */
		if (next < a.nleaves)
			gc_prefetch<HAS_R, NW>(a, nl0, nl1, nr0, nr1, b);

		if (live) {
			/* emit one COUNT(*) per group and clear the slot.  Record mode: the groups of this leaf are
			 * appended to one global list (a single atomic per leaf reserves the space) and ordered
			 * afterwards by a radix sort on the first row id; dense mode: COUNT(*) is scattered to the
			 * group's first row position (8-byte random writes, only kept as a fallback). */
			const uint32_t cbase = s_chunk[0], csize = s_chunk[2];
			/* owner mode: one round per register-batch element, plus one for the side slot of the hash-0 key in the
			 * single leaf that holds it (a wave that reads the flag after thread 0 cleared it has nothing to do there) */
			const int iters = by_owner ? (s_cnt[GC_SLOTS] != 0ull ? LEAF_BATCH + 1 : LEAF_BATCH) : GC_EMIT_ITERS;
#pragma unroll
			for (int it = 0; it < GC_EMIT_ITERS; it++) {
				if (it >= iters)
					break;
				unsigned long long recv = 0;
				uint32_t s = 0xFFFFFFFFu;
				if (by_owner) {
					/* slots created by this thread, plus (thread 0) the side slot of the hash-0 key */
					if (it < LEAF_BATCH)
						s = own[it];
					else if (it == LEAF_BATCH && threadIdx.x == 0)
						s = GC_SLOTS;
				} else {
					s = threadIdx.x + (uint32_t)it * GC_THREADS;
					if (s > GC_SLOTS)
						s = 0xFFFFFFFFu;
				}
				if (s != 0xFFFFFFFFu) {
					const unsigned long long c2 = s_cnt[s];
					const bool occupied = s < GC_SLOTS ? (by_owner || s_key[s] != 0ull) : c2 != 0ull;
					if (occupied) {
						const uint32_t cl = (uint32_t)c2, cr = (uint32_t)(c2 >> 32);
						const uint32_t first = s_first[s];
						if (s < GC_SLOTS)
							s_key[s] = 0ull;
						s_cnt[s] = 0ull;
						s_first[s] = 0xFFFFFFFFu;
						if (cl && (!HAS_R || cr)) {
							const unsigned long long c = HAS_R ? (unsigned long long)cl * cr : (unsigned long long)cl;
							mine += c;
							if (a.kbits) {
								if (c >> (64 - a.kbits))
									mdb_raise(a.status, GC_ST_COUNT_NOT_REC64);	/* COUNT(*) does not fit beside the row id */
								if (c >> (32 - (a.kbits < 32 ? a.kbits : 31)))
									mdb_raise(a.status, GC_ST_COUNT_NOT_REC32);	/* ... nor in a 4-byte record */
								recv = ((unsigned long long)first << (64 - a.kbits)) | c;
							} else {
								if (first < a.dense_n)
								a.dense_cnt[first] = (int64_t)c;
							}
						}
					}
				}
				if (a.kbits) {
					/* wave-level append: one LDS atomic per wave and iteration, no workgroup barrier */
					const uint64_t m = __ballot(recv != 0ull);
					if (m) {
						const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
						uint32_t wbase = 0;
						if (mdb_lane() == leader)
							wbase = atomicAdd(&s_chunk[1], (uint32_t)__popcll(m));
						wbase = __shfl(wbase, (int)leader, MDB_WAVE);
						if (recv) {
							const uint32_t pos = wbase + (uint32_t)__popcll(m & mdb_lanemask_lt());
							if (pos < csize)
								a.rec[cbase + pos] = recv;
							nvalid++;
						}
					}
				}
			}
			__syncthreads();	/* the next leaf builds into the cleared tables */
		}
		leaf = next;
		l0 = nl0;
		l1 = nl1;
		r0 = nr0;
		r1 = nr1;
	}
	if (a.kbits) {
		const uint32_t base = s_chunk[0], used = s_chunk[1], size = s_chunk[2];
		for (uint32_t i = used + threadIdx.x; i < size; i += GC_THREADS)
			a.rec[base + i] = 0ull;		/* unused tail of the last chunk */
		if (nvalid)
			atomicAdd(&s_chunk[3], nvalid);
	}
	if (mine)
		atomicAdd(&s_sum, mine);
	__syncthreads();
	if (threadIdx.x == 0 && s_sum)
		atomicAdd(a.joined, s_sum);
	if (threadIdx.x == 0 && a.kbits && s_chunk[3])
		atomicAdd(a.rec_valid, s_chunk[3]);
}

/* ------------------------------------------------------------------ direct-address leaves (compact narrow form)
 *
 * When the keys of both tables span fewer than 2^k values (k found from the key sample, verified for every key by the
 * first partition level), the 32-bit hash is mdb_mixk(key - base) in the top k bits of its field - a bijection of the
 * window - and the radix partition has consumed the top b1 + b2 of them: inside a leaf only rem = k - b1 - b2 bits tell
 * keys apart.  For rem <= LD_MAX_REM those bits INDEX the leaf's table: three plain arrays in LDS (right rows, left
 * rows, first left row per key) - no stored keys, no compare-and-swap, no probe chains, no "table full".  A right row
 * is ONE LDS add, a left row ONE LDS read (plus an add and a minimum when its key has right rows), and the emit pass
 * walks the arrays linearly.  The hashed kernel above spends ~120 wave instructions per 64 rows and is issue bound
 * (profiles/r01: 380 M vector + scalar instructions for 2 * 10^8 rows); this one is bound by the HBM stream of the
 * partitioned rows.  Hashing (instead of partitioning by key range) keeps the leaves evenly filled whatever part of the
 * window a table covers: the benchmark's right table holds the lowest sixteenth of the left table's key range.
 *
 * 512 threads, dynamic LDS of (12 << rem) + 32 bytes (24 KiB at rem = 11: four workgroups = 32 waves per CU).
 * Persistent: the first register round of both sides of the NEXT leaf is requested before the current leaf is emitted.
 */
/* ROUND = rows of either side in the first (register) round of a leaf: 2048 (24 prefetch registers in the two sets, 64 in
 * all).  4096 for the leaves of 2^12 entries (2 x 3052 rows on average at 10^8 rows) needs 80 registers + 11 spilled and
 * measured 1-3 % slower than 2048 with the remaining rows loaded in the loop. */

template <int THREADS, int ROUND>
struct ld_regs {
	static constexpr int RB = ROUND / (4 * THREADS);	/* 16-byte loads per thread, right side: 4 words each */
	static constexpr int RA = ROUND / (2 * THREADS);	/* ... left side: 2 words each */
	uint4 b[RB];
	ulonglong2 a[RA];
	uint32_t l1, r1;		/* ends of the requested leaf's two row ranges (they start at leaf * cap) */
	uint2 next_l, next_r;		/* row counts of the leaf this register set will take NEXT, as loaded (gc_leaf_decode) */
};

/* Row counts of `leaf`, to be decoded one leaf's work later. */
template <bool HAS_R, int THREADS, int ROUND>
__device__ static inline void ld_request_counts(const gc_args &a, uint32_t leaf, ld_regs<THREADS, ROUND> &q)
{
	q.next_l = make_uint2(0, 0);
	q.next_r = make_uint2(0, 0);
	if (leaf < a.nleaves) {
		q.next_l = gc_leaf_raw(a.off_l, a.cnt_l, a.cap_l, leaf);
		if (HAS_R)
			q.next_r = gc_leaf_raw(a.off_r, a.cnt_r, a.cap_r, leaf);
	}
}

/* First-round loads of `leaf` (whose counts were requested into q before), untouched until they are consumed: a
 * conversion at load time would make the request wait for itself (see gc_batch).  A leaf is requested TWO leaves ahead of
 * its turn, so its loads have a whole leaf's work to land in; its counts are requested two leaves before that, so that
 * only the rows that exist are fetched (whole rounds regardless of the count were 30 % more bytes and 15 % slower). */
template <bool HAS_R, int THREADS, int ROUND>
__device__ static inline void ld_request(const gc_args &a, uint32_t leaf, ld_regs<THREADS, ROUND> &q)
{
	uint32_t l0, r0 = 0;
	gc_leaf_decode(q.next_l, a.cap_l, leaf, &l0, &q.l1);
	q.r1 = 1;
	if (HAS_R)
		gc_leaf_decode(q.next_r, a.cap_r, leaf, &r0, &q.r1);
	ld_request_counts<HAS_R, THREADS, ROUND>(a, leaf + 2 * gridDim.x, q);
#pragma unroll
	for (int u = 0; u < ld_regs<THREADS, ROUND>::RA; u++) {
		const uint32_t i = l0 + 2u * ((uint32_t)u * THREADS + threadIdx.x);
		q.a[u] = make_ulonglong2(0ull, 0ull);
		if (i < q.l1)
			q.a[u] = *reinterpret_cast<const ulonglong2 *>(a.hv_l + i);
	}
	if (HAS_R) {
#pragma unroll
		for (int u = 0; u < ld_regs<THREADS, ROUND>::RB; u++) {
			const uint32_t j = r0 + 4u * ((uint32_t)u * THREADS + threadIdx.x);
			q.b[u] = make_uint4(0u, 0u, 0u, 0u);
			if (j < q.r1)
				q.b[u] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint32_t *>(a.hv_r) + j);
		}
	}
}

/* one left row: narrow word = hash32 << 32 | row id */
template <bool HAS_R>
__device__ static inline void ld_left_row(unsigned long long w, uint32_t shift, uint32_t mask, const uint32_t *s_cr, uint32_t *s_cl,
					  uint32_t *s_first)
{
	const uint32_t idx = ((uint32_t)(w >> 32) >> shift) & mask;
	if (!HAS_R || s_cr[idx]) {
		atomicAdd(&s_cl[idx], 1u);
		atomicMin(&s_first[idx], (uint32_t)w);
	}
}

struct ld_state {
	uint32_t *s_cr, *s_cl, *s_first, *s_chunk;
	uint32_t *s_cx;		/* nextra arrays of T counters: the further right tables */
	uint32_t T, mask, shift, rem;
	unsigned long long mine;
	uint32_t nvalid;
};

/* one leaf: count the right rows, look the left rows up, request leaf + 2 * gridDim.x into the registers just consumed, emit */
template <bool HAS_R, int THREADS, int ROUND>
__device__ static inline void ld_leaf(const gc_args &a, ld_state &st, uint32_t leaf, ld_regs<THREADS, ROUND> &q)
{
	uint32_t *const s_cr = st.s_cr, *const s_cl = st.s_cl, *const s_first = st.s_first, *const s_chunk = st.s_chunk;
	const uint32_t T = st.T, mask = st.mask, shift = st.shift;
	const uint32_t l0 = leaf * a.cap_l, l1 = q.l1, r0 = HAS_R ? leaf * a.cap_r : 0u, r1 = q.r1;
	const bool nonempty = l0 != l1 && (!HAS_R || r0 != r1);
	const bool hot = nonempty && (l1 - l0 >= a.heavy_l || (HAS_R && r1 - r0 >= a.heavy_r));
	const bool live = nonempty && !hot;
	if (hot && threadIdx.x == 0)
		mdb_raise(a.status, GC_ST_HOT_LEAVES);	/* left to the hot-key path (hashed tables in global memory) */
	if (live && a.kbits) {
		/* record list space, reserved a chunk at a time: one global atomic per ~10-170 leaves (see k_leaf_group_count).
		 * (Reserving for the DISTINCT right keys instead of the rows - counted with returning adds - left fewer zero-filled
		 * gaps in the list but cost the kernel 25 %: profiles/micro/leaf_direct_exp.sh) */
		const uint32_t rows = (HAS_R && (r1 - r0) < (l1 - l0)) ? r1 - r0 : l1 - l0;	/* a group needs a row on both sides */
		const uint32_t need = (rows < T ? rows : T) + 1;
		const uint32_t base = s_chunk[0], used = s_chunk[1], size = s_chunk[2];
		if (used + need > size) {		/* uniform: every thread read the same words */
			for (uint32_t i = used + threadIdx.x; i < size; i += THREADS) {
				if (a.rec32)
					reinterpret_cast<uint32_t *>(a.rec)[base + i] = 0u;
				else
					a.rec[base + i] = 0ull;
			}
			__syncthreads();		/* everyone has read s_chunk */
			if (threadIdx.x == 0) {
				const uint32_t want = need > GC_REC_CHUNK ? need : GC_REC_CHUNK;
				const uint32_t nb = atomicAdd(a.rec_count, want);
				if (nb + want > a.rec_cap) {
					mdb_raise(a.status, MDB_ST_LIST_FULL);
					s_chunk[0] = 0;
					s_chunk[2] = 0;
				} else {
					s_chunk[0] = nb;
					s_chunk[2] = want;
				}
				s_chunk[1] = 0;
			}
			/* visible to everyone after the barrier that ends the count phase */
		}
	}
	if (live) {
		if (HAS_R) {
			/* right rows: one LDS add each (r0 is a multiple of 64: the rounds start on the leaf's first row) */
			const uint32_t *const hv_r32 = reinterpret_cast<const uint32_t *>(a.hv_r);
#pragma unroll
			for (int u = 0; u < ld_regs<THREADS, ROUND>::RB; u++) {
				const uint32_t j = r0 + 4u * ((uint32_t)u * THREADS + threadIdx.x);
				const uint32_t w[4] = { q.b[u].x, q.b[u].y, q.b[u].z, q.b[u].w };
#pragma unroll
				for (int k = 0; k < 4; k++)
					if (j + k < r1)
						atomicAdd(&s_cr[(w[k] >> shift) & mask], 1u);
			}
			for (uint32_t j = r0 + 4u * (ld_regs<THREADS, ROUND>::RB * THREADS + threadIdx.x); j < r1; j += 4u * THREADS) {
				const uint4 v = *reinterpret_cast<const uint4 *>(hv_r32 + j);
				const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
				for (int k = 0; k < 4; k++)
					if (j + k < r1)
						atomicAdd(&s_cr[(w[k] >> shift) & mask], 1u);
			}
			if (a.nextra) {		/* (uniform) further right tables on the same key: their rows, then the product of the counts */
				for (uint32_t x = 0; x < a.nextra; x++) {
					uint32_t *const s_c = st.s_cx + x * T;
					const uint32_t x0 = leaf * a.cap_x[x], xc = a.cnt_x[x][leaf], x1 = x0 + (xc < a.cap_x[x] ? xc : a.cap_x[x]);
					for (uint32_t j = x0 + 4u * threadIdx.x; j < x1; j += 4u * THREADS) {
						const uint4 v = *reinterpret_cast<const uint4 *>(a.hv_x[x] + j);
						const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
						for (int k = 0; k < 4; k++)
							if (j + k < x1)
								atomicAdd(&s_c[(w[k] >> shift) & mask], 1u);
					}
				}
				__syncthreads();
				for (uint32_t sl = threadIdx.x; sl < T; sl += THREADS) {
					unsigned long long c = s_cr[sl];
					for (uint32_t x = 0; x < a.nextra; x++) {
						c *= st.s_cx[x * T + sl];
						st.s_cx[x * T + sl] = 0u;
						if (c >> 32) {		/* the product of the right counts no longer fits: reported, the caller chains 2-table operators */
							mdb_raise(a.status, GC_ST_PRODUCT_WIDE);
							c = 0;
						}
					}
					s_cr[sl] = (uint32_t)c;
				}
			}
			__syncthreads();
		}
		/* left rows: one LDS read each; rows whose key has right rows are counted and compete for "first" */
#pragma unroll
		for (int u = 0; u < ld_regs<THREADS, ROUND>::RA; u++) {
			const uint32_t i = l0 + 2u * ((uint32_t)u * THREADS + threadIdx.x);
			if (i < l1)
				ld_left_row<HAS_R>(q.a[u].x, shift, mask, s_cr, s_cl, s_first);
			if (i + 1 < l1)
				ld_left_row<HAS_R>(q.a[u].y, shift, mask, s_cr, s_cl, s_first);
		}
		for (uint32_t i = l0 + 2u * (ld_regs<THREADS, ROUND>::RA * THREADS + threadIdx.x); i < l1; i += 2u * THREADS) {
			const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(a.hv_l + i);
			ld_left_row<HAS_R>(v.x, shift, mask, s_cr, s_cl, s_first);
			if (i + 1 < l1)
				ld_left_row<HAS_R>(v.y, shift, mask, s_cr, s_cl, s_first);
		}
		__syncthreads();
	}

	/* these registers are free again: the leaf after next travels while this one is emitted and the next one processed */
	if (leaf + 2 * gridDim.x < a.nleaves)
		ld_request<HAS_R, THREADS, ROUND>(a, leaf + 2 * gridDim.x, q);

	if (live) {
		/* emit one record per key that has rows on both sides and clear what was touched (4-byte accesses, thread t takes
		 * entries t, t + THREADS, ...: four consecutive entries per thread with 16-byte LDS accesses measured 10 % slower
		 * when few entries are occupied and 4 % faster when all are - profiles/micro/leaf_direct_exp.sh) */
		const uint32_t cbase = s_chunk[0], csize = s_chunk[2];
		for (uint32_t s0 = 0; s0 < T; s0 += THREADS) {	/* uniform trip count */
			const uint32_t s = s0 + threadIdx.x;
			unsigned long long recv = 0;
			if (s < T) {
				const uint32_t cl = s_cl[s];
				uint32_t cr = 1u;
				if (HAS_R) {
					cr = s_cr[s];
					if (cr)
						s_cr[s] = 0u;
				}
				if (cl) {
					const uint32_t first = s_first[s];
					const unsigned long long c = (unsigned long long)cl * cr;
					s_cl[s] = 0u;
					s_first[s] = 0xFFFFFFFFu;
					st.mine += c;
					if (HAS_R && cl > 1u && cr)
						mdb_raise(a.status, GC_ST_LEFT_DUPS);	/* (a matched key with several left rows: mdb_dev_join_keys_ordered asks) */
					if (a.kbits && a.keyed_cbits) {
						if (c >> a.keyed_cbits)
							mdb_raise(a.status, GC_ST_COUNT_NOT_KEYED);	/* COUNT(*) does not fit a keyed record: redone with plain records */
						recv = ((unsigned long long)first << (64 - a.kbits)) |
						       ((unsigned long long)((leaf << st.rem) | s) << a.keyed_cbits) | c;
					} else if (a.kbits) {
						if (c >> (64 - a.kbits))
							mdb_raise(a.status, GC_ST_COUNT_NOT_REC64);	/* COUNT(*) does not fit beside the row id */
						if (c >> (32 - (a.kbits < 32 ? a.kbits : 31)))
							mdb_raise(a.status, GC_ST_COUNT_NOT_REC32);	/* ... nor in a 4-byte record (the ordering sort then moves 8-byte ones) */
						recv = a.rec32 ? (unsigned long long)(((uint32_t)first << (32 - a.kbits)) | (uint32_t)c)
							       : ((unsigned long long)first << (64 - a.kbits)) | c;
						if (a.rec32 && (c >> (32 - a.kbits)))
							mdb_raise(a.status, GC_ST_REC32_STALE);
					} else {
						if (first < a.dense_n)
								a.dense_cnt[first] = (int64_t)c;
					}
				}
			}
			if (a.kbits) {
				/* wave-level append: one LDS atomic per wave and iteration */
				const uint64_t m = __ballot(recv != 0ull);
				if (m) {
					const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
					uint32_t wbase = 0;
					if (mdb_lane() == leader)
						wbase = atomicAdd(&s_chunk[1], (uint32_t)__popcll(m));
					wbase = __shfl(wbase, (int)leader, MDB_WAVE);
					if (recv) {
						const uint32_t pos = wbase + (uint32_t)__popcll(m & mdb_lanemask_lt());
						if (pos < csize) {
							if (a.rec32)
								reinterpret_cast<uint32_t *>(a.rec)[cbase + pos] = (uint32_t)recv;
							else
								a.rec[cbase + pos] = recv;
						}
						st.nvalid++;
					}
				}
			}
		}
		__syncthreads();	/* the next leaf counts into the cleared arrays */
	}
}

template <bool HAS_R, int THREADS, int ROUND>
__global__ __launch_bounds__(THREADS, 4 * THREADS / 256) void k_leaf_direct	/* four workgroups per CU: at most 64 registers */(gc_args a, uint32_t rem, uint32_t shift)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t ld_lds[];
	ld_state st;
	st.T = 1u << rem;
	st.rem = rem;
	st.mask = st.T - 1u;
	st.shift = shift;
	st.s_cr = ld_lds;			/* right rows per key */
	st.s_cl = ld_lds + st.T;		/* left rows per key (joins: only of keys that have right rows) */
	st.s_first = ld_lds + 2 * st.T;		/* first left row per key */
	st.s_chunk = ld_lds + 3 * st.T;		/* record list chunk: [0] base [1] used [2] size [3] valid records; [4..7] see below */
	st.s_cx = ld_lds + 3 * st.T + 8;	/* (further right tables) */
	for (uint32_t s = threadIdx.x; s < a.nextra * st.T; s += THREADS)
		st.s_cx[s] = 0u;
	unsigned long long *const s_sum = reinterpret_cast<unsigned long long *>(ld_lds + 3 * st.T + 4);
	st.mine = 0;
	st.nvalid = 0;

	for (uint32_t s = threadIdx.x; s < st.T; s += THREADS) {
		st.s_cr[s] = 0u;
		st.s_cl[s] = 0u;
		st.s_first[s] = 0xFFFFFFFFu;
	}
	if (threadIdx.x < 8)
		st.s_chunk[threadIdx.x] = 0u;		/* [4..5] = s_sum, [6] = distinct right keys of the current leaf */

	/* two register sets: while leaf i is processed out of one, leaf i + 1 sits (or still travels) in the other */
	ld_regs<THREADS, ROUND> qa, qb;
	uint32_t leaf = blockIdx.x;
	ld_request_counts<HAS_R, THREADS, ROUND>(a, leaf, qa);
	ld_request_counts<HAS_R, THREADS, ROUND>(a, leaf + gridDim.x, qb);
	if (leaf < a.nleaves)
		ld_request<HAS_R, THREADS, ROUND>(a, leaf, qa);
	if (leaf + gridDim.x < a.nleaves)
		ld_request<HAS_R, THREADS, ROUND>(a, leaf + gridDim.x, qb);
	__syncthreads();
	while (leaf < a.nleaves) {
		ld_leaf<HAS_R, THREADS, ROUND>(a, st, leaf, qa);
		leaf += gridDim.x;
		if (leaf >= a.nleaves)
			break;
		ld_leaf<HAS_R, THREADS, ROUND>(a, st, leaf, qb);
		leaf += gridDim.x;
	}
	if (a.kbits) {
		const uint32_t base = st.s_chunk[0], used = st.s_chunk[1], size = st.s_chunk[2];
		for (uint32_t i = used + threadIdx.x; i < size; i += THREADS) {	/* unused tail of the last chunk */
			if (a.rec32)
				reinterpret_cast<uint32_t *>(a.rec)[base + i] = 0u;
			else
				a.rec[base + i] = 0ull;
		}
		if (st.nvalid)
			atomicAdd(&st.s_chunk[3], st.nvalid);
	}
	if (st.mine)
		atomicAdd(s_sum, st.mine);
	__syncthreads();
	if (threadIdx.x == 0 && *s_sum)
		atomicAdd(a.joined, *s_sum);
	if (threadIdx.x == 0 && a.kbits && st.s_chunk[3])
		atomicAdd(a.rec_valid, st.s_chunk[3]);
}

/* ------------------------------------------------------------------ semi-join filter (compact narrow form)
 *
 * Bitmap of the hashed key values the RIGHT table holds, one bit per 2^coarse adjacent values, built from its
 * partitioned form: the 2^rem values a leaf can hold are a contiguous slice of the bitmap, so ONE WAVE per leaf sets the
 * bits in LDS and writes the slice with coalesced stores (no global atomics); leaves are consecutive in the bitmap, so
 * the slices of a first-level digit are too - which is what the left table's second partition level loads. */
#define LB_WAVES 4u
__global__ __launch_bounds__(LB_WAVES * MDB_WAVE) void k_leaf_bitmap(const uint32_t *__restrict__ hv_r, const uint32_t *__restrict__ cnt_r, uint32_t cap_r,
								 uint32_t nleaves, uint32_t rem, uint32_t coarse, uint32_t shift,
								 uint32_t *__restrict__ bits)
{
	__shared__ uint32_t s_bits[LB_WAVES][(1u << LD_MAX_REM) / 32];
	const uint32_t wave = threadIdx.x / MDB_WAVE, lane = mdb_lane();
	const uint32_t words = 1u << (rem - coarse - 5u), mask = (1u << rem) - 1u;	/* rem - coarse >= 5: at least one word */
	const uint32_t rounds = (nleaves + gridDim.x * LB_WAVES - 1) / (gridDim.x * LB_WAVES);
	for (uint32_t k = 0; k < rounds; k++) {
		const uint32_t leaf = (k * gridDim.x + blockIdx.x) * LB_WAVES + wave;
		for (uint32_t w = lane; w < words; w += MDB_WAVE)
			s_bits[wave][w] = 0u;
		__syncthreads();
		if (leaf < nleaves) {
			const uint32_t c = cnt_r[leaf], r0 = leaf * cap_r, r1 = r0 + (c < cap_r ? c : cap_r);
			for (uint32_t j = r0 + 4u * lane; j < r1; j += 4u * MDB_WAVE) {
				const uint4 v = *reinterpret_cast<const uint4 *>(hv_r + j);	/* (regions start 16-byte aligned and are padded) */
				const uint32_t h[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
				for (int q = 0; q < 4; q++)
					if (j + q < r1) {
						const uint32_t idx = ((h[q] >> shift) & mask) >> coarse;
						atomicOr(&s_bits[wave][idx >> 5], 1u << (idx & 31u));
					}
			}
		}
		__syncthreads();
		if (leaf < nleaves)
			for (uint32_t w = lane; w < words; w += MDB_WAVE)
				bits[(size_t)leaf * words + w] = s_bits[wave][w];
		__syncthreads();
	}
}

/* ------------------------------------------------------------------ hot keys across the whole chip
 *
 * One workgroup streams a leaf at ~16 GB/s; a key with 10^7 duplicates would pin one workgroup for 10+ ms while the
 * other 511 idle.  Hot leaves (GC_HEAVY rows or more on a side; the plain kernel skips them and raises status bit 6)
 * are therefore cut into slices of HOT_SLICE rows that ALL resident workgroups share: every slice is merged into an
 * LDS table with gc_side_heavy (a wave's duplicates first collapse into one update), the table is flushed into the
 * leaf's table in global memory with one atomic triple per distinct key, and a last small kernel turns the global
 * tables into group records exactly like the emit phase of the plain kernel.  At most HOT_MAX hot leaves take this
 * path; beyond that the single-workgroup HEAVY instance of the leaf kernel does the work.
 */
#define HOT_MAX 64u
#define HOT_SLOTS 8191u		/* global table per hot leaf (prime; a leaf holds at most GC_SLOTS distinct keys) */
#define HOT_SLICE 65536u

struct hot_args {
	uint32_t *count;			/* number of hot leaves found */
	uint32_t *leaf;				/* [HOT_MAX] */
	unsigned long long *g_key;		/* [HOT_MAX][HOT_SLOTS] hashed key, 0 = empty */
	unsigned long long *g_cnt;		/* [HOT_MAX][HOT_SLOTS + 1] packed counts; [HOT_SLOTS] = the key whose hash is 0 */
	uint32_t *g_first;			/* [HOT_MAX][HOT_SLOTS + 1] */
};

template <bool HAS_R>
__global__ void k_hot_list(gc_args a, hot_args h)
{
	const uint32_t leaf = blockIdx.x * blockDim.x + threadIdx.x;
	if (leaf >= a.nleaves)
		return;
	uint32_t l0, l1, r0 = 0, r1 = 1;
	gc_leaf_range(a.off_l, a.cnt_l, a.cap_l, leaf, &l0, &l1);
	if (HAS_R)
		gc_leaf_range(a.off_r, a.cnt_r, a.cap_r, leaf, &r0, &r1);
	if (l0 == l1 || r0 == r1)
		return;
	if (l1 - l0 >= a.heavy_l || (HAS_R && r1 - r0 >= a.heavy_r)) {
		const uint32_t i = atomicAdd(h.count, 1u);
		if (i < HOT_MAX)
			h.leaf[i] = leaf;
	}
}

__global__ void k_hot_clear(hot_args h)
{
	const uint32_t nh = *h.count < HOT_MAX ? *h.count : HOT_MAX;
	const uint64_t total = (uint64_t)nh * (HOT_SLOTS + 1);
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t t = i / (HOT_SLOTS + 1), s = i % (HOT_SLOTS + 1);
		if (s < HOT_SLOTS)
			h.g_key[t * HOT_SLOTS + s] = 0ull;
		h.g_cnt[i] = 0ull;
		h.g_first[i] = 0xFFFFFFFFu;
	}
}

__device__ static inline uint32_t hot_insert(unsigned long long *keys, uint64_t hv)
{
	uint32_t s = leaf_slot(hv, HOT_SLOTS);
	const uint32_t step = leaf_step(hv, HOT_SLOTS);
	for (uint32_t probe = 0; probe < HOT_SLOTS; probe++) {
		const unsigned long long old = atomicCAS(&keys[s], 0ull, (unsigned long long)hv);
		if (old == 0ull || old == hv)
			return s;
		s += step;
		if (s >= HOT_SLOTS)
			s -= HOT_SLOTS;
	}
	return 0xFFFFFFFFu;
}

template <bool HAS_R>
__global__ __launch_bounds__(GC_THREADS, 8) void k_hot_slices(gc_args a, hot_args h)
{
	__shared__ unsigned long long s_key[GC_SLOTS];
	__shared__ unsigned long long s_cnt[GC_SLOTS + 1];
	__shared__ uint32_t s_first[GC_SLOTS + 1];
	for (uint32_t s = threadIdx.x; s <= GC_SLOTS; s += GC_THREADS) {
		if (s < GC_SLOTS)
			s_key[s] = 0ull;
		s_cnt[s] = 0ull;
		s_first[s] = 0xFFFFFFFFu;
	}
	__syncthreads();
	const uint32_t nh = *h.count;	/* <= HOT_MAX guaranteed by the host */
	uint32_t task = 0;
	gc_batch b;
	for (uint32_t t = 0; t < nh; t++) {
		const uint32_t leaf = h.leaf[t];
		uint32_t l0, l1, r0 = 0, r1 = 0;
		gc_leaf_range(a.off_l, a.cnt_l, a.cap_l, leaf, &l0, &l1);
		if (HAS_R)
			gc_leaf_range(a.off_r, a.cnt_r, a.cap_r, leaf, &r0, &r1);
		const uint32_t nsl = (l1 - l0 + HOT_SLICE - 1) / HOT_SLICE, nsr = (r1 - r0 + HOT_SLICE - 1) / HOT_SLICE;
		for (uint32_t k = 0; k < nsl + nsr; k++, task++) {
			if (task % gridDim.x != blockIdx.x)
				continue;	/* uniform */
			const bool is_l = k < nsl;
			const uint32_t x0 = is_l ? l0 + k * HOT_SLICE : r0 + (k - nsl) * HOT_SLICE;
			const uint32_t xe = is_l ? l1 : r1;
			const uint32_t x1 = x0 + HOT_SLICE < xe ? x0 + HOT_SLICE : xe;
			if (is_l) {
				gc_load_l<2>(a, x0, x1, b);
				gc_side_heavy<true, true>(a, s_key, s_cnt, s_first, b, x0, x1);
			} else {
				gc_load_r<2>(a, x0, x1, b);
				gc_side_heavy<false, true>(a, s_key, s_cnt, s_first, b, x0, x1);
			}
			__syncthreads();
			/* flush the slice's table into the leaf's global table and clear it */
			unsigned long long *gk = h.g_key + (uint64_t)t * HOT_SLOTS;
			unsigned long long *gc = h.g_cnt + (uint64_t)t * (HOT_SLOTS + 1);
			uint32_t *gf = h.g_first + (uint64_t)t * (HOT_SLOTS + 1);
			for (uint32_t s = threadIdx.x; s <= GC_SLOTS; s += GC_THREADS) {
				const unsigned long long c2 = s_cnt[s];
				if (!c2)
					continue;
				uint32_t g = HOT_SLOTS;
				if (s < GC_SLOTS) {
					g = hot_insert(gk, s_key[s]);
					s_key[s] = 0ull;
				}
				if (g == 0xFFFFFFFFu) {
					mdb_raise(a.status, GC_ST_TABLE_FULL);
				} else {
					atomicAdd(&gc[g], c2);
					if (is_l)
						atomicMin(&gf[g], s_first[s]);
				}
				s_cnt[s] = 0ull;
				s_first[s] = 0xFFFFFFFFu;
			}
			__syncthreads();
		}
	}
}

/* one workgroup per hot leaf: global table -> group records (or dense counts), like the emit phase of the leaf kernel */
template <bool HAS_R>
__global__ __launch_bounds__(1024) void k_hot_finish(gc_args a, hot_args h)
{
	__shared__ unsigned long long s_sum;
	__shared__ uint32_t s_valid;
	const uint32_t t = blockIdx.x;
	if (t >= *h.count)
		return;
	if (threadIdx.x == 0) {
		s_sum = 0ull;
		s_valid = 0;
	}
	__syncthreads();
	const unsigned long long *gc = h.g_cnt + (uint64_t)t * (HOT_SLOTS + 1);
	const uint32_t *gf = h.g_first + (uint64_t)t * (HOT_SLOTS + 1);
	unsigned long long mine = 0;
	uint32_t nvalid = 0;
	for (uint32_t s = threadIdx.x; s <= HOT_SLOTS; s += blockDim.x) {
		const unsigned long long c2 = gc[s];
		const uint32_t cl = (uint32_t)c2, cr = (uint32_t)(c2 >> 32);
		if (!cl || (HAS_R && !cr))
			continue;
		const unsigned long long c = HAS_R ? (unsigned long long)cl * cr : (unsigned long long)cl;
		const uint32_t first = gf[s];
		mine += c;
		if (a.kbits) {
			if (c >> (64 - a.kbits))
				mdb_raise(a.status, GC_ST_COUNT_NOT_REC64);
			if (c >> (32 - (a.kbits < 32 ? a.kbits : 31)))
				mdb_raise(a.status, GC_ST_COUNT_NOT_REC32);
			const uint32_t pos = atomicAdd(a.rec_count, 1u);
			if (pos < a.rec_cap)
				a.rec[pos] = ((unsigned long long)first << (64 - a.kbits)) | c;
			else
				mdb_raise(a.status, MDB_ST_LIST_FULL);
			nvalid++;
		} else {
			if (first < a.dense_n)
								a.dense_cnt[first] = (int64_t)c;
		}
	}
	if (mine)
		atomicAdd(&s_sum, mine);
	if (nvalid)
		atomicAdd(&s_valid, nvalid);
	__syncthreads();
	if (threadIdx.x == 0) {
		if (s_sum)
			atomicAdd(a.joined, s_sum);
		if (s_valid)
			atomicAdd(a.rec_valid, s_valid);
	}
}

/* ------------------------------------------------------------------ NULL-key group (plain GROUP BY only) */

__global__ __launch_bounds__(256) void k_null_stats(const uint64_t *__restrict__ nullbits, uint64_t n,
						    unsigned long long *cnt_first /* [0]=count [1]=first */)
{
	const uint64_t words = (n + 63) >> 6;
	unsigned long long c = 0, first = ~0ull;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t m = nullbits[w];
		if (w == words - 1 && (n & 63))
			m &= (1ull << (n & 63)) - 1ull;
		if (m) {
			c += (unsigned long long)__popcll(m);
			const unsigned long long f = (w << 6) + (unsigned long long)(__ffsll((long long)m) - 1);
			if (f < first)
				first = f;
		}
	}
	if (c) {
		atomicAdd(&cnt_first[0], c);
		atomicMin(&cnt_first[1], first);
	}
}

__global__ void k_null_poke(const unsigned long long *cnt_first, int64_t *dense_cnt)
{
	if (threadIdx.x == 0 && blockIdx.x == 0 && cnt_first[0])
		dense_cnt[cnt_first[1]] = (int64_t)cnt_first[0];
}

__global__ void k_null_rec(const unsigned long long *cnt_first, unsigned long long *rec, uint32_t *rec_count, uint32_t *rec_valid,
			   uint32_t rec_cap, uint32_t kbits, uint32_t *status)
{
	if (threadIdx.x == 0 && blockIdx.x == 0 && cnt_first[0]) {
		if (cnt_first[0] >> (64 - kbits))
			atomicOr(status, 4u);
		if (cnt_first[0] >> (32 - (kbits < 32 ? kbits : 31)))
			atomicOr(status, 16u);
		const uint32_t pos = atomicAdd(rec_count, 1u);
		if (pos < rec_cap) {
			rec[pos] = (cnt_first[1] << (64 - kbits)) | cnt_first[0];
			atomicAdd(rec_valid, 1u);
		} else {
			atomicOr(status, 8u);
		}
	}
}

__global__ void k_gather_i32(const int32_t *__restrict__ keys, const uint32_t *__restrict__ sel, uint64_t n, int64_t *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n)
		out[i] = (int64_t)keys[sel[i]];
}

/* ------------------------------------------------------------------ launchers (mdb_dev_join.hip: gc_partition_left, gc_launch_leaf, gc_hot_keys, gc_deliver_dense) */

/* the hashed leaves: a persistent grid, two 75 KiB workgroups per CU's 160 KiB of LDS */
int leaf_hashed_launch(mdb_dev_ctx *ctx, const gc_args &a, bool has_r, bool build_r, bool narrow)
{
	const uint32_t resident = 2u * (uint32_t)ctx->num_cus;
	const uint32_t grid = a.nleaves < resident ? a.nleaves : resident;
	if (has_r && build_r && narrow) {
		MDB_LAUNCH(ctx, "leaf_join_group_count", (k_leaf_group_count<true, true, false, true>), grid, GC_THREADS, a);
	} else if (has_r && build_r) {
		MDB_LAUNCH(ctx, "leaf_join_group_count", (k_leaf_group_count<true, true, false>), grid, GC_THREADS, a);
	} else if (has_r && narrow) {
		MDB_LAUNCH(ctx, "leaf_join_group_count", (k_leaf_group_count<true, false, false, true>), grid, GC_THREADS, a);
	} else if (has_r) {
		MDB_LAUNCH(ctx, "leaf_join_group_count", (k_leaf_group_count<true, false, false>), grid, GC_THREADS, a);
	} else if (narrow) {
		MDB_LAUNCH(ctx, "leaf_group_count", (k_leaf_group_count<false, false, false, true>), grid, GC_THREADS, a);
	} else {
		MDB_LAUNCH(ctx, "leaf_group_count", (k_leaf_group_count<false, false, false>), grid, GC_THREADS, a);
	}
	return MIDORIDB_OK;
}

/* compact narrow form: the leaf's table is indexed by the rem hash bits the partition left over */
int leaf_direct_launch(mdb_dev_ctx *ctx, const gc_args &a, uint32_t rem, uint32_t shift, bool has_r, int nextra)
{
	const size_t lds = ((size_t)(12 + 4 * nextra) << rem) + 32;
	/* four 512-thread workgroups = the CU's 32 waves (three measured the same, 256-thread workgroups 10-30 % slower) */
	uint32_t per_cu = (uint32_t)((size_t)(160 * 1024) / lds);
	per_cu = per_cu > 4 ? 4 : (per_cu < 1 ? 1 : per_cu);
	const uint32_t dgrid = a.nleaves < per_cu * (uint32_t)ctx->num_cus ? a.nleaves : per_cu * (uint32_t)ctx->num_cus;
	if (has_r) {
		MDB_LAUNCH_LDS(ctx, "leaf_join_direct", (k_leaf_direct<true, 512, 2048>), dgrid, 512, lds, a, rem, shift);
	} else {
		MDB_LAUNCH_LDS(ctx, "leaf_group_direct", (k_leaf_direct<false, 512, 2048>), dgrid, 512, lds, a, rem, shift);
	}
	return MIDORIDB_OK;
}

/* the right table's hashed keys (4-byte fixed-capacity leaves) as a bitmap */
int leaf_bitmap_launch(mdb_dev_ctx *ctx, const uint32_t *hv_r, const uint32_t *cnt_r, uint32_t cap_r, uint32_t nleaves, uint32_t rem, uint32_t coarse, uint32_t shift,
		       uint32_t *bits)
{
	const uint32_t groups = (nleaves + LB_WAVES - 1) / LB_WAVES, resident = 16u * (uint32_t)ctx->num_cus;
	MDB_LAUNCH(ctx, "leaf_bitmap", k_leaf_bitmap, groups < resident ? groups : resident, LB_WAVES * MDB_WAVE, hv_r, cnt_r, cap_r, nleaves, rem, coarse, shift, bits);
	return MIDORIDB_OK;
}

/* the NULL keys' group behind the leaf kernel: as a record (record mode) or poked into the dense counts */
int leaf_null_group_launch(mdb_dev_ctx *ctx, const gc_args &a, const uint64_t *null_l, uint64_t n_l)
{
	unsigned long long *d_nullst = (unsigned long long *)(ctx->d_status + GC_STW_NULL_STATS);
	MDB_HIP(ctx, hipMemsetAsync(d_nullst + 1, 0xFF, 8, ctx->stream));
	MDB_LAUNCH(ctx, "null_stats", k_null_stats, 256, 256, null_l, n_l, d_nullst);
	if (a.rec) {
		MDB_LAUNCH(ctx, "null_rec", k_null_rec, 1, 64, d_nullst, a.rec, a.rec_count, a.rec_valid, a.rec_cap, a.kbits, ctx->d_status);
	} else {
		MDB_LAUNCH(ctx, "null_poke", k_null_poke, 1, 64, d_nullst, a.dense_cnt);
	}
	return MIDORIDB_OK;
}

/* what leaf_hot_launch takes from the arena (only touched when needed) */
size_t leaf_hot_arena_bytes(void)
{
	return mdb_align_up((size_t)HOT_MAX * HOT_SLOTS * 8) + mdb_align_up((size_t)HOT_MAX * (HOT_SLOTS + 1) * 8) + mdb_align_up((size_t)HOT_MAX * (HOT_SLOTS + 1) * 4) + 4096;
}

/* hot keys - the plain kernel left the leaves with GC_HEAVY or more rows on a side to this path (one host round trip: their number) */
int leaf_hot_launch(mdb_dev_ctx *ctx, const gc_args &a, bool has_r, bool build_r)
{
	const uint32_t nleaves = a.nleaves;
	hot_args ha;
	ha.count = (uint32_t *)mdb_arena_take(ctx, 64);
	ha.leaf = (uint32_t *)mdb_arena_take(ctx, HOT_MAX * 4);
	ha.g_key = (unsigned long long *)mdb_arena_take(ctx, (size_t)HOT_MAX * HOT_SLOTS * 8);
	ha.g_cnt = (unsigned long long *)mdb_arena_take(ctx, (size_t)HOT_MAX * (HOT_SLOTS + 1) * 8);
	ha.g_first = (uint32_t *)mdb_arena_take(ctx, (size_t)HOT_MAX * (HOT_SLOTS + 1) * 4);
	if (!ha.count || !ha.leaf || !ha.g_key || !ha.g_cnt || !ha.g_first)
		return -MIDORIDB_INTERNAL;
	MDB_HIP(ctx, hipMemsetAsync(ha.count, 0, 4, ctx->stream));
	if (has_r) {
		MDB_LAUNCH(ctx, "hot_list", k_hot_list<true>, (nleaves + 255) / 256, 256, a, ha);
	} else {
		MDB_LAUNCH(ctx, "hot_list", k_hot_list<false>, (nleaves + 255) / 256, 256, a, ha);
	}
	uint64_t *h = ctx->h_pinned;
	MDB_HIP(ctx, hipMemcpyAsync(&h[MDB_HP_HOT], ha.count, 4, hipMemcpyDeviceToHost, ctx->stream));
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const uint32_t nhot = (uint32_t)h[MDB_HP_HOT];
	const uint32_t resident = 2u * (uint32_t)ctx->num_cus;
	if (nhot <= HOT_MAX) {
		MDB_LAUNCH(ctx, "hot_clear", k_hot_clear, 256, 256, ha);
		if (has_r) {
			MDB_LAUNCH(ctx, "hot_slices", k_hot_slices<true>, resident, GC_THREADS, a, ha);
			MDB_LAUNCH(ctx, "hot_finish", k_hot_finish<true>, nhot, 1024, a, ha);
		} else {
			MDB_LAUNCH(ctx, "hot_slices", k_hot_slices<false>, resident, GC_THREADS, a, ha);
			MDB_LAUNCH(ctx, "hot_finish", k_hot_finish<false>, nhot, 1024, a, ha);
		}
	} else {
		/* very many hot leaves: each is streamed by one workgroup (the HEAVY instance of the leaf kernel) */
		const uint32_t grid = nleaves < resident ? nleaves : resident;
		if (has_r && build_r) {
			MDB_LAUNCH(ctx, "leaf_hot_keys", (k_leaf_group_count<true, true, true>), grid, GC_THREADS, a);
		} else if (has_r) {
			MDB_LAUNCH(ctx, "leaf_hot_keys", (k_leaf_group_count<true, false, true>), grid, GC_THREADS, a);
		} else {
			MDB_LAUNCH(ctx, "leaf_hot_keys", (k_leaf_group_count<false, false, true>), grid, GC_THREADS, a);
		}
	}
	return MIDORIDB_OK;
}

int leaf_gather_i32_launch(mdb_dev_ctx *ctx, const int32_t *keys, const uint32_t *sel, uint64_t n, int64_t *out)
{
	MDB_LAUNCH(ctx, "gather_i32", k_gather_i32, (uint32_t)((n + 255) / 256), 256, keys, sel, n, out);
	return MIDORIDB_OK;
}
