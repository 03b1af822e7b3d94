/*
 * mdb_exec_setop.c - compound statements: SELECT ... { UNION [ALL] | INTERSECT | EXCEPT  SELECT ... } [ORDER BY] [LIMIT] - an extension
 * (the reference's grammar has one SELECT per statement).
 *
 * Every arm is an ordinary SELECT, resolved on its own and run through exec_select_one() with its result kept on the device (the pattern
 * of subqueries_eval, mdb_exec.c - its handling of one-row results that stay on the host and of empty results included).  The chain is
 * combined step by step, left to right; the arms' columns correspond by their select lists (setop_check):
 *
 *   L UNION ALL R   L's rows, then R's rows                                                  mdb_dev_concat64 per column
 *   L UNION R       the first occurrences in that concatenation, in its order                ... mdb_dev_distinct_sel, a gather
 *   L INTERSECT R   L's distinct rows, in first-occurrence order, that occur in R            mdb_dev_distinct_sel over L, mdb_dev_rows_semi with
 *   L EXCEPT R      L's distinct rows, in first-occurrence order, that do not occur in R     that selection as the probe's row ids, a gather
 *
 * Rows are equal as mdb_dev_distinct_sel has them equal: NULL = NULL, 8-byte cells by their bits (VARCHAR cells are ids of the database's
 * one dictionary: equal strings, equal ids, whichever arm they come from).  The compound's ORDER BY / LIMIT run over the last step's rows
 * with the statement tail's own choice between sort and top-k (order_perm, mdb_exec_tail.c).
 */
#include "mdb_exec_internal.h"

/* n rows of ncols device columns: an arm's result (the buffers are `backing`'s, or - a one-row result, which stays on the host - uploaded
 * cells of its own) or a step's output (buffers of its own) */
struct rowset {
	uint64_t n;
	int ncols;
	void **vals;
	uint64_t **nulls;		/* per column or NULL: no cell of it is NULL */
	bool *own_vals, *own_nulls;	/* the buffer is this rowset's to free */
	struct mdb_result *backing;	/* the arm's result the other buffers belong to: freed with the rowset */
};

struct setop {
	struct mdb_catalog *cat;
	mdb_dev_ctx *dev;
	char *err;
	size_t errlen;
	const int *type;		/* the result columns' column types (the first arm's; every arm's) */
};

static int so_dev_fail(struct setop *o, const char *what)
{
	snprintf(o->err, o->errlen, "execution phase: %s: %s\n", what, mdb_dev_last_error(o->dev));
	return -MIDORIDB_INTERNAL;
}

static void rowset_free(struct setop *o, struct rowset *r)
{
	for (int c = 0; r->vals && c < r->ncols; c++) {
		if (r->own_vals && r->own_vals[c] && r->vals[c])
			mdb_dev_free(o->dev, r->vals[c]);
		if (r->own_nulls && r->own_nulls[c] && r->nulls[c])
			mdb_dev_free(o->dev, r->nulls[c]);
	}
	free(r->vals);
	free(r->nulls);
	free(r->own_vals);
	free(r->own_nulls);
	mdb_result_free(r->backing);
	memset(r, 0, sizeof(*r));
}

static int rowset_init(struct setop *o, struct rowset *r, int ncols, uint64_t n)
{
	const size_t k = (size_t)(ncols ? ncols : 1);
	memset(r, 0, sizeof(*r));
	r->ncols = ncols;
	r->n = n;
	r->vals = calloc(k, sizeof(*r->vals));
	r->nulls = calloc(k, sizeof(*r->nulls));
	r->own_vals = calloc(k, sizeof(bool));
	r->own_nulls = calloc(k, sizeof(bool));
	if (!r->vals || !r->nulls || !r->own_vals || !r->own_nulls) {
		rowset_free(o, r);
		snprintf(o->err, o->errlen, "out of memory\n");
		return -MIDORIDB_NOMEM;
	}
	return MIDORIDB_OK;
}

/* column c of r gets buffers of its own: n cells and, when wanted, their NULL words */
static int rowset_alloc_column(struct setop *o, struct rowset *r, int c, bool with_nulls)
{
	if (mdb_dev_alloc(o->dev, (size_t)(r->n ? r->n : 1) * 8, &r->vals[c]))
		return so_dev_fail(o, "allocating a set operation's column");
	r->own_vals[c] = true;
	if (with_nulls) {
		void *nb = NULL;
		if (mdb_dev_alloc(o->dev, (size_t)((r->n + 63) / 64 + 1) * 8, &nb))
			return so_dev_fail(o, "allocating a set operation's column");
		r->nulls[c] = nb;
		r->own_nulls[c] = true;
	}
	return MIDORIDB_OK;
}

/* an arm's result as a rowset, which takes the result over (on failure too): column c of the rowset is the result's column col_of[c] */
static int rowset_from_result(struct setop *o, struct mdb_result *res, const int *col_of, struct rowset *r)
{
	int rc = rowset_init(o, r, res->ncols, res->nrows);
	if (rc) {
		mdb_result_free(res);
		return rc;
	}
	r->backing = res;
	for (int c = 0; !rc && res->nrows && c < res->ncols; c++) {
		const int from = col_of[c];
		if (res->d_data && res->d_data[from]) {
			r->vals[c] = res->d_data[from];
			r->nulls[c] = res->d_nullbits ? res->d_nullbits[from] : NULL;
		} else if (res->nrows == 1 && res->data && res->data[from]) {
			/* a result of one row stays on the host (a lone COUNT(*) or MAX(v), or any statement that found one row): its cell and NULL word, uploaded */
			const uint64_t cell = (uint64_t)res->data[from][0], nullword[2] = { res->nullbits && res->nullbits[from] ? res->nullbits[from][0] & 1u : 0u, 0u };
			if (!(rc = rowset_alloc_column(o, r, c, nullword[0] != 0)) &&
			    (mdb_dev_h2d(o->dev, r->vals[c], &cell, 8) || (nullword[0] && mdb_dev_h2d(o->dev, r->nulls[c], nullword, 16))))
				rc = so_dev_fail(o, "uploading a one-row arm of a set operation");
		} else {
			snprintf(o->err, o->errlen, "execution phase: internal error (set operation: an arm's column is nowhere)\n");
			rc = -MIDORIDB_INTERNAL;
		}
	}
	if (rc)
		rowset_free(o, r);
	return rc;
}

static void rowset_keys(const struct setop *o, const struct rowset *r, const uint32_t *rid, struct mdb_sort_key *k)
{
	for (int c = 0; c < r->ncols; c++) {
		k[c].values = r->vals[c];
		k[c].nullbits = r->nulls[c];
		k[c].rid = rid;
		k[c].type = o->type[c] == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
		k[c].desc = 0;
	}
}

/* out = the rows rid[0 .. m) of src, in that order (rid == NULL: the first m rows) */
static int rowset_gather(struct setop *o, const struct rowset *src, const uint32_t *rid, uint64_t m, struct rowset *out)
{
	int rc = rowset_init(o, out, src->ncols, m);
	for (int c0 = 0; !rc && m && c0 < src->ncols; c0 += MDB_GATHER_MAX_COLS) {
		struct mdb_gather_col gl[MDB_GATHER_MAX_COLS];
		const int nc = src->ncols - c0 < MDB_GATHER_MAX_COLS ? src->ncols - c0 : MDB_GATHER_MAX_COLS;
		for (int c = c0; !rc && c < c0 + nc; c++) {
			if ((rc = rowset_alloc_column(o, out, c, src->nulls[c] != NULL)))
				break;
			gl[c - c0].src = src->vals[c];
			gl[c - c0].src_nullbits = src->nulls[c];
			gl[c - c0].rid = rid;
			gl[c - c0].dst = out->vals[c];
			gl[c - c0].dst_nullbits = out->nulls[c];
		}
		if (!rc && mdb_dev_gather_cols(o->dev, gl, nc, m))
			rc = so_dev_fail(o, "set operation gather");
	}
	if (rc)
		rowset_free(o, out);
	return rc;
}

/* out = l's rows, then r's rows */
static int step_concat(struct setop *o, const struct rowset *l, const struct rowset *r, struct rowset *out)
{
	int rc = rowset_init(o, out, l->ncols, l->n + r->n);
	for (int c = 0; !rc && out->n && c < l->ncols; c++) {
		const struct mdb_concat_part parts[2] = { { l->vals[c], l->n ? l->nulls[c] : NULL, l->n }, { r->vals[c], r->n ? r->nulls[c] : NULL, r->n } };
		if ((rc = rowset_alloc_column(o, out, c, parts[0].nullbits || parts[1].nullbits)))
			break;
		if (mdb_dev_concat64(o->dev, parts, 2, out->vals[c], out->nulls[c]))
			rc = so_dev_fail(o, "UNION");
	}
	if (!rc && mdb_dev_sync(o->dev))
		rc = so_dev_fail(o, "UNION");
	if (rc)
		rowset_free(o, out);
	return rc;
}

/* the first occurrences among r's rows: *sel = their ascending positions (a device buffer of the caller's now; NULL: every row is one), *m
 * their number */
static int distinct_rows(struct setop *o, const struct rowset *r, uint32_t **sel, uint64_t *m)
{
	struct mdb_sort_key keys[MDB_ROWS_MAX_COLS];
	void *p = NULL;
	*sel = NULL;
	*m = r->n;
	if (r->n < 2)
		return MIDORIDB_OK;
	rowset_keys(o, r, NULL, keys);
	if (mdb_dev_alloc(o->dev, (size_t)r->n * 4, &p))
		return so_dev_fail(o, "allocating a set operation's selection");
	if (mdb_dev_distinct_sel(o->dev, keys, r->ncols, r->n, p, m)) {
		mdb_dev_free(o->dev, p);
		return so_dev_fail(o, "set operation DISTINCT");
	}
	if (*m == r->n) {	/* no row twice */
		mdb_dev_free(o->dev, p);
		return MIDORIDB_OK;
	}
	*sel = p;
	return MIDORIDB_OK;
}

static int step_union(struct setop *o, const struct rowset *l, const struct rowset *r, struct rowset *out)
{
	struct rowset all;
	uint32_t *sel = NULL;
	uint64_t m = 0;
	int rc = step_concat(o, l, r, &all);
	if (rc)
		return rc;
	if (!(rc = distinct_rows(o, &all, &sel, &m))) {
		if (!sel) {	/* the concatenation is the answer */
			*out = all;
			return MIDORIDB_OK;
		}
		rc = rowset_gather(o, &all, sel, m, out);
		mdb_dev_free(o->dev, sel);
	}
	rowset_free(o, &all);
	return rc;
}

/* INTERSECT (anti = 0) / EXCEPT (anti = 1): the distinct first makes the probe smaller */
static int step_semi(struct setop *o, const struct rowset *l, const struct rowset *r, int anti, struct rowset *out)
{
	struct mdb_sort_key probe[MDB_ROWS_MAX_COLS], build[MDB_ROWS_MAX_COLS];
	uint32_t *first = NULL;
	void *hit = NULL, *rid = NULL;
	uint64_t m = 0, k = 0;
	int rc = distinct_rows(o, l, &first, &m);
	if (rc)
		return rc;
	if (!m) {
		rc = rowset_init(o, out, l->ncols, 0);
		goto done;
	}
	rowset_keys(o, l, first, probe);
	rowset_keys(o, r, NULL, build);
	if (mdb_dev_alloc(o->dev, (size_t)m * 4, &hit)) {
		rc = so_dev_fail(o, "allocating a set operation's selection");
		goto done;
	}
	o->cat->setop_calls++;
	if (mdb_dev_rows_semi(o->dev, probe, m, build, r->n, l->ncols, anti, hit, &k, NULL)) {
		rc = so_dev_fail(o, anti ? "EXCEPT" : "INTERSECT");
		goto done;
	}
	/* the positions among l's first occurrences -> positions among l's rows */
	if (first && k) {
		if (mdb_dev_alloc(o->dev, (size_t)k * 4, &rid) || mdb_dev_gather32(o->dev, first, hit, k, rid)) {
			rc = so_dev_fail(o, anti ? "EXCEPT" : "INTERSECT");
			goto done;
		}
	}
	rc = rowset_gather(o, l, first ? rid : hit, k, out);
done:
	if (rid)
		mdb_dev_free(o->dev, rid);
	if (hit)
		mdb_dev_free(o->dev, hit);
	if (first)
		mdb_dev_free(o->dev, first);
	return rc;
}

/* the compound's ORDER BY / LIMIT over cur (order_col[i]: the result column of ORDER BY item i) */
static int setop_tail(struct setop *o, const struct mdb_select *s, const int *order_col, struct rowset *cur)
{
	void *perm = NULL;
	const uint32_t *rid = NULL;
	uint64_t m = cur->n;
	int rc = MIDORIDB_OK;

	if (s->nset_order && cur->n > 1) {
		struct mdb_sort_key keys[MDB_SORT_MAX_KEYS];
		for (int i = 0; i < s->nset_order; i++) {
			const int c = order_col[i];
			keys[i].values = cur->vals[c];
			keys[i].nullbits = cur->nulls[c];
			keys[i].rid = NULL;
			keys[i].type = o->type[c] == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
			keys[i].desc = s->set_order_desc[i];
		}
		m = order_rows_wanted(cur->n, s->set_has_limit, s->set_limit_off, s->set_limit_cnt);
		if (mdb_dev_alloc(o->dev, (size_t)(m ? m : 1) * 4, &perm))
			return so_dev_fail(o, "allocating the ORDER BY permutation");
		if (order_perm(o->dev, keys, s->nset_order, cur->n, m, perm)) {
			rc = so_dev_fail(o, m < cur->n ? "ORDER BY ... LIMIT" : "ORDER BY");
			goto done;
		}
		rid = perm;
	}
	uint64_t off = 0, cnt = m;
	if (s->set_has_limit)
		limit_window(m, s->set_limit_off, s->set_limit_cnt, &off, &cnt);
	if (rid || off || cnt < cur->n) {
		struct rowset out;
		if (!rid && cnt) {	/* LIMIT alone: the rows [off, off + cnt) */
			if (mdb_dev_alloc(o->dev, (size_t)(off + cnt) * 4, &perm) || mdb_dev_iota32(o->dev, perm, off + cnt)) {
				rc = so_dev_fail(o, "LIMIT");
				goto done;
			}
			rid = perm;
		}
		if ((rc = rowset_gather(o, cur, rid ? rid + off : NULL, cnt, &out)))
			goto done;
		rowset_free(o, cur);
		*cur = out;
	}
done:
	if (perm)
		mdb_dev_free(o->dev, perm);
	return rc;
}

/* the last rowset -> the statement's result: kept on the device (its buffers change hands) or brought to the host, as any result is */
static int setop_result(struct setop *o, struct rowset *cur, struct mdb_result *res)
{
	const size_t k = (size_t)(cur->ncols ? cur->ncols : 1);
	const bool keep = o->cat->results_on_device && cur->n > 1;
	res->nrows = cur->n;
	res->data = calloc(k, sizeof(*res->data));
	res->nullbits = calloc(k, sizeof(*res->nullbits));
	if (!res->data || !res->nullbits)
		return -MIDORIDB_NOMEM;
	res->fetched = !keep;
	if (keep) {
		res->dev = o->dev;
		res->d_data = calloc(k, sizeof(*res->d_data));
		res->d_nullbits = calloc(k, sizeof(*res->d_nullbits));
		if (!res->d_data || !res->d_nullbits)
			return -MIDORIDB_NOMEM;
		for (int c = 0; c < cur->ncols; c++) {	/* (a step's output: every buffer is the rowset's own) */
			res->d_data[c] = cur->vals[c];
			res->d_nullbits[c] = cur->nulls[c];
			cur->vals[c] = NULL;
			cur->nulls[c] = NULL;
		}
		return MIDORIDB_OK;
	}
	for (int c = 0; c < cur->ncols; c++) {
		res->data[c] = mdb_dev_host_alloc((size_t)(cur->n ? cur->n : 1) * 8);
		if (!res->data[c])
			return -MIDORIDB_NOMEM;
		res->data[c][0] = 0;
		if (result_column_to_host(o->dev, res, c, cur->vals[c], cur->nulls[c]))
			return so_dev_fail(o, "reading a result column");
	}
	return MIDORIDB_OK;
}

static const char *setop_name(int op)
{
	return op == MDB_SETOP_UNION ? "UNION" : op == MDB_SETOP_UNIONALL ? "UNION ALL" : op == MDB_SETOP_INTERSECT ? "INTERSECT" : "EXCEPT";
}

/* The semantic rules of a compound, from the statement and the catalog alone: every arm resolved, the same number of result columns, the same
 * column type at every position (no coercion), at most MDB_ROWS_MAX_COLS columns unless every operator is UNION ALL, the ORDER BY names
 * among the first arm's result columns and none of them VARCHAR.  The arms correspond by their SELECT LISTS - item i of one to item i of
 * the other, as SQL has it - while every result keeps its columns in the reference's order (R3): col_of[a][c] = the column of arm a's
 * result that belongs to column c of the first arm's (each an array of the caller's now).  *first = the first arm's signature (the caller
 * frees it) */
static int setop_check(struct mdb_catalog *cat, struct mdb_select *s, struct select_signature *first, int **col_of, int *order_col, char *err, size_t errlen)
{
	int rc;
	bool all_union_all = true;

	for (int a = 0; a <= s->nset; a++) {
		struct mdb_select *arm = a ? s->set_arm[a - 1] : s;
		if (!arm->resolved && (rc = resolve_select(cat, arm, err, errlen)))
			return rc;
		arm->resolved = true;
	}
	if ((rc = select_signature(s, first, err, errlen)))
		return rc;
	for (int a = 0; a <= s->nset; a++) {
		struct select_signature sig;
		const int op = a ? s->set_op[a - 1] : MDB_SETOP_UNIONALL;	/* (the first arm is compared with itself: no refusal names it) */
		all_union_all = all_union_all && op == MDB_SETOP_UNIONALL;
		if ((rc = select_signature(a ? s->set_arm[a - 1] : s, &sig, err, errlen)))
			return rc;
		if (sig.ncols != first->ncols) {
			ERR("%s: the first SELECT has %d result columns, SELECT %d has %d: all arms of a set operation must have the same number\n",
			    setop_name(op), first->ncols, a + 1, sig.ncols);
			rc = -MIDORIDB_ERROR;
		}
		for (int i = 0; !rc && i < sig.ncols; i++)
			if (sig.type[sig.at[i]] != first->type[first->at[i]]) {
				ERR("%s: column %d is %s in the first SELECT ('%.100s') and %s in SELECT %d ('%.100s'): both sides must have the same type\n",
				    setop_name(op), i + 1, coltype_name(first->type[first->at[i]]), first->name[first->at[i]],
				    coltype_name(sig.type[sig.at[i]]), a + 1, sig.name[sig.at[i]]);
				rc = -MIDORIDB_ERROR;
			}
		if (!rc && !(col_of[a] = calloc((size_t)(sig.ncols > 0 ? sig.ncols : 1), sizeof(int)))) {
			ERR("out of memory\n");
			rc = -MIDORIDB_NOMEM;
		}
		for (int i = 0; !rc && i < sig.ncols; i++)
			col_of[a][first->at[i]] = sig.at[i];
		select_signature_free(&sig);
		if (rc)
			return rc;
	}
	if (!all_union_all && first->ncols > MDB_ROWS_MAX_COLS) {
		ERR("UNION, INTERSECT and EXCEPT over more than %d columns are not supported (UNION ALL takes any number): %d result columns\n", MDB_ROWS_MAX_COLS,
		    first->ncols);
		return -MIDORIDB_ERROR;
	}
	for (int i = 0; i < s->nset_order; i++) {
		int at = -1;
		for (int c = 0; c < first->ncols && at < 0; c++) {
			const char *dot = strrchr(first->name[c], '.');
			if (!strcmp(first->name[c], s->set_order[i]) || (dot && !strcmp(dot + 1, s->set_order[i])))
				at = c;
		}
		if (at < 0) {
			ERR("ORDER BY behind a set operation: '%.100s' is no result column of the first SELECT (a column's name or an alias)\n", s->set_order[i]);
			return -MIDORIDB_ERROR;
		}
		if (first->type[at] == MDB_CT_VARCHAR) {	/* cells are dictionary ids: equality only, no collation order */
			const char *dot = strrchr(first->name[at], '.');
			if (dot)
				ERR("ORDER BY over the VARCHAR column '%.*s.%s' is not supported on the MI355X path\n", (int)(dot - first->name[at]), first->name[at], dot + 1);
			else
				ERR("ORDER BY over the VARCHAR column '%s' is not supported on the MI355X path\n", first->name[at]);
			return -MIDORIDB_ERROR;
		}
		order_col[i] = at;
	}
	return MIDORIDB_OK;
}

int exec_setop(struct mdb_catalog *cat, struct mdb_select *s, struct mdb_result **out, char *err, size_t errlen)
{
	struct setop o = { .cat = cat, .err = err, .errlen = errlen };
	struct select_signature first;
	struct rowset cur, rhs;
	struct mdb_result *res = NULL, *arm_res = NULL;
	int order_col[MDB_SORT_MAX_KEYS], *col_of[MDB_SETOP_MAX_ARMS] = { NULL }, rc;
	const bool on_device = cat->results_on_device;

	stmt_dict = &cat->dict;
	*out = NULL;
	memset(&first, 0, sizeof(first));
	memset(&cur, 0, sizeof(cur));
	memset(&rhs, 0, sizeof(rhs));
	if (cat->dist) {
		/* (known from the statement alone: every rank leaves here together, before anything is exchanged) */
		ERR("sharded mode: UNION / INTERSECT / EXCEPT is not executed (set operations run on one GPU)\n");
		return -MIDORIDB_ERROR;
	}
	if ((rc = setop_check(cat, s, &first, col_of, order_col, err, errlen)))
		goto out;
	if ((rc = mdb_catalog_device(cat, err, errlen)))
		goto out;
	o.dev = cat->dev;
	o.type = first.type;
	const double t0 = now_ms();

	/* the first arm; what the result is called and typed is its result's */
	cat->results_on_device = true;
	rc = exec_select_one(cat, s, &arm_res, err, errlen);
	cat->results_on_device = on_device;
	if (rc)
		goto out;
	if (arm_res->ncols != first.ncols) {
		ERR("execution phase: internal error (set operation: an arm delivered %d columns, %d were announced)\n", arm_res->ncols, first.ncols);
		mdb_result_free(arm_res);
		rc = -MIDORIDB_INTERNAL;
		goto out;
	}
	res = calloc(1, sizeof(*res));
	if (res) {
		const size_t k = (size_t)(first.ncols ? first.ncols : 1);
		res->ncols = first.ncols;
		res->colname = calloc(k, sizeof(*res->colname));
		res->coltype = calloc(k, sizeof(int));
		res->colprec = calloc(k, sizeof(int));
	}
	if (!res || !res->colname || !res->coltype || !res->colprec) {
		ERR("out of memory\n");
		mdb_result_free(arm_res);
		rc = -MIDORIDB_NOMEM;
		goto out;
	}
	for (int c = 0; c < first.ncols; c++) {
		memcpy(res->colname[c], arm_res->colname[c], MDB_NAME_LEN);
		res->coltype[c] = arm_res->coltype[c];
		res->colprec[c] = arm_res->colprec[c];
	}
	if ((rc = rowset_from_result(&o, arm_res, col_of[0], &cur)))
		goto out;

	for (int a = 0; a < s->nset; a++) {
		struct rowset next;
		cat->results_on_device = true;
		rc = exec_select_one(cat, s->set_arm[a], &arm_res, err, errlen);
		cat->results_on_device = on_device;
		if (rc)
			goto out;
		if (arm_res->ncols != first.ncols) {
			ERR("execution phase: internal error (set operation: an arm delivered %d columns, %d were announced)\n", arm_res->ncols, first.ncols);
			mdb_result_free(arm_res);
			rc = -MIDORIDB_INTERNAL;
			goto out;
		}
		for (int c = 0; c < first.ncols; c++)	/* (VARCHAR(n): the widest arm's n serves every string of the result) */
			if (arm_res->colprec[col_of[a + 1][c]] > res->colprec[c])
				res->colprec[c] = arm_res->colprec[col_of[a + 1][c]];
		if ((rc = rowset_from_result(&o, arm_res, col_of[a + 1], &rhs)))
			goto out;
		if (cur.n + rhs.n >= MDB_NO_ROW) {
			ERR("%s: %llu + %llu rows, an intermediate result of a set operation holds at most 2^32 - 2\n", setop_name(s->set_op[a]),
			    (unsigned long long)cur.n, (unsigned long long)rhs.n);
			rc = -MIDORIDB_ERROR;
			goto out;
		}
		switch (s->set_op[a]) {
		case MDB_SETOP_UNIONALL: rc = step_concat(&o, &cur, &rhs, &next); break;
		case MDB_SETOP_UNION: rc = step_union(&o, &cur, &rhs, &next); break;
		case MDB_SETOP_INTERSECT: rc = step_semi(&o, &cur, &rhs, 0, &next); break;
		default: rc = step_semi(&o, &cur, &rhs, 1, &next); break;
		}
		if (rc)
			goto out;
		rowset_free(&o, &cur);
		rowset_free(&o, &rhs);
		cur = next;
	}
	if ((rc = setop_tail(&o, s, order_col, &cur)))
		goto out;
	if ((rc = setop_result(&o, &cur, res))) {
		if (rc == -MIDORIDB_NOMEM)
			ERR("out of memory\n");
		goto out;
	}
	res->dict = &cat->dict;
	mdb_result_legacy_header(res);
	mdb_result_legacy_rows(res);
	res->exec_ms = now_ms() - t0;
	*out = res;
	res = NULL;
out:
	if (o.dev) {
		rowset_free(&o, &cur);
		rowset_free(&o, &rhs);
	}
	mdb_result_free(res);
	select_signature_free(&first);
	for (int a = 0; a < MDB_SETOP_MAX_ARMS; a++)
		free(col_of[a]);
	stmt_dict = &cat->dict;
	return rc;
}
