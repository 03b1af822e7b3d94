/*
 * mdb_dev_runs.hip - the runs of a stream sorted by its group keys (mdb_runs_find; contract: mdb_dev_internal.h): step 2 of the aggregate
 * operator's sorted form and step A2 of COUNT(DISTINCT).  The head test, the binary search over first[] and the count of heads in front of
 * a position are mdb_dev_stream.h's.
 */
#include "mdb_dev_internal.h"
#include "mdb_dev_stream.h"

/* one workgroup per chunk: hb bit p = "sorted position p begins a run", cnt[chunk] = heads in the chunk */
__global__ __launch_bounds__(MDB_RUNS_CHUNK) void k_agg_heads(mdb_stream_keys K, const uint32_t *__restrict__ perm, uint64_t n, unsigned long long *__restrict__ hb,
							      uint32_t *__restrict__ cnt, uint32_t *status)
{
	__shared__ uint32_t s_cnt;
	if (threadIdx.x == 0)
		s_cnt = 0;
	__syncthreads();
	const uint64_t p = (uint64_t)blockIdx.x * MDB_RUNS_CHUNK + threadIdx.x;
	const mdb_stream_head h = mdb_stream_head_of(K, perm, n, p, status);
	const unsigned long long b = __ballot(h.part);
	if (mdb_lane() == 0) {
		hb[p >> 6] = b;
		if (b)
			atomicAdd(&s_cnt, (uint32_t)__popcll(b));
	}
	__syncthreads();
	if (threadIdx.x == 0)
		cnt[blockIdx.x] = s_cnt;
}

/* rungroup[r] = the group whose first row is the head of run r (first == NULL: one group) */
__global__ __launch_bounds__(MDB_RUNS_CHUNK) void k_agg_run_groups(const unsigned long long *__restrict__ hb, const uint32_t *__restrict__ base,
								   const uint32_t *__restrict__ perm, uint64_t n, const uint32_t *__restrict__ first, uint64_t G,
								   uint32_t *__restrict__ rungroup, uint32_t *status)
{
	const uint64_t p = (uint64_t)blockIdx.x * MDB_RUNS_CHUNK + threadIdx.x;
	if (p >= n || !((hb[p >> 6] >> (p & 63)) & 1ull))
		return;
	const uint32_t r = mdb_runs_heads_before(hb, base, p);
	if (r >= G) {
		mdb_raise(status, MDB_GROUPS_ST_RUNS_DIFFER);
		return;
	}
	const uint32_t g = first ? mdb_first_group_of(first, G, perm ? perm[p] : (uint32_t)p) : 0u;
	if (g == MDB_GROUP_NONE) {
		mdb_raise(status, MDB_GROUPS_ST_KEY_MISSING);
		return;
	}
	rungroup[r] = g;
}

int mdb_groups_status(mdb_dev_ctx *ctx, const uint32_t *d_status, const char *op, const char *what, uint32_t *word)
{
	uint32_t h = 0;
	MDB_HIP(ctx, hipMemcpyAsync(&h, d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
	MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (word)
		*word = h;
	if (h & MDB_GROUPS_ST_RUNS_DIFFER)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "%s (%s): the keys form more runs than there are groups", op, what);
	if (h & MDB_GROUPS_ST_KEY_MISSING)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "%s (%s): a row's key belongs to no group of first[]", op, what);
	if (h & MDB_GROUPS_ST_PERM_RANGE)
		return mdb_set_err(ctx, -MIDORIDB_INTERNAL, "%s (%s): the sort's permutation names a row beyond the stream", op, what);
	return MIDORIDB_OK;
}

int mdb_runs_find(mdb_dev_ctx *ctx, const struct mdb_sort_key *keys, int nkeys, uint64_t n, const uint32_t *first, uint64_t G, const char *op,
		  const char *what, mdb_dev_tmp &tmp, mdb_runs *out)
{
	const uint64_t nchunks = (n + MDB_RUNS_CHUNK - 1u) / MDB_RUNS_CHUNK;
	mdb_stream_keys K;
	uint32_t *perm = NULL;
	int rc;
	memset(&K, 0, sizeof(K));
	memset(out, 0, sizeof(*out));
	if (nkeys > 0) {
		struct mdb_sort_key sk[MDB_SORT_MAX_KEYS];
		if (!(perm = (uint32_t *)tmp.take(n * 4u + 16u)))
			return mdb_set_err(ctx, -MIDORIDB_NOMEM, "%s: no device memory for the permutation", op);
		for (int k = 0; k < nkeys; k++) {
			sk[k] = keys[k];
			sk[k].desc = 0;
			K.k[k] = mdb_stream_col_of_key(&keys[k]);
		}
		K.npart = K.nkeys = nkeys;
		if ((rc = mdb_dev_sort_perm(ctx, sk, nkeys, n, perm)))
			return rc;
	}
	out->perm = perm;
	unsigned long long *hb = (unsigned long long *)tmp.take(nchunks * (MDB_RUNS_CHUNK / 8u));
	uint32_t *base = (uint32_t *)tmp.take((nchunks + 1u) * 4u);
	uint32_t *scan_tmp = (uint32_t *)tmp.take(mdb_scan_scratch_words(nchunks + 1u) * 4u);
	uint32_t *rungroup = (uint32_t *)tmp.take(G * 4u);
	uint32_t *status = (uint32_t *)tmp.take(256);
	if (!hb || !base || !scan_tmp || !rungroup || !status)
		return mdb_set_err(ctx, -MIDORIDB_NOMEM, "%s: no device memory for the runs of %llu rows", op, (unsigned long long)n);
	MDB_HIP(ctx, hipMemsetAsync(status, 0, 4, ctx->stream));
	MDB_HIP(ctx, hipMemsetAsync(base + nchunks, 0, 4, ctx->stream));
	MDB_LAUNCH(ctx, "agg_heads", k_agg_heads, (uint32_t)nchunks, MDB_RUNS_CHUNK, K, (const uint32_t *)perm, n, hb, base, status);
	if ((rc = mdb_scan_u32_inplace(ctx, base, nchunks + 1u, scan_tmp)))
		return rc;
	MDB_LAUNCH(ctx, "agg_run_groups", k_agg_run_groups, (uint32_t)nchunks, MDB_RUNS_CHUNK, (const unsigned long long *)hb, (const uint32_t *)base,
		   (const uint32_t *)perm, n, first, G, rungroup, status);
	/* (a run nobody gave a group would leave its group's results unwritten: the checks make sure every group has its run) */
	uint32_t runs = 0;
	MDB_HIP(ctx, hipMemcpyAsync(&runs, base + nchunks, 4, hipMemcpyDeviceToHost, ctx->stream));
	if ((rc = mdb_groups_status(ctx, status, op, what)))
		return rc;
	if (runs != G)
		return mdb_set_err(ctx, -MIDORIDB_ERROR, "%s (%s): %u runs of equal keys, %llu groups", op, what, runs, (unsigned long long)G);
	out->hb = hb;
	out->base = base;
	out->rungroup = rungroup;
	out->nchunks = nchunks;
	return MIDORIDB_OK;
}
