/*
 * mdb_exec.c - the SELECT executor: lowers a statement plan onto the device C-ABI (mdb_dev.h).
 *
 * This file is the MI355X replacement of executor_run_select_stmt() (reference
 * src/engine/executor_select.c:1655-1744) and keeps its phase order:
 *
 *   reference phase (file:line)                        here
 *   -------------------------------------------------  --------------------------------------------
 *   build_cols_hashtable/build_table_scafold :267-322  result column set + order (R3), host only
 *   proc_from_clause_table :1282-1343 (scan)           tuple stream = identity row ids (no copy)
 *   _join_nested_loop_tbl2tbl :1076-1149               mdb_dev_join_pairs (+ residual ON filter)
 *   _join_nested_loop_tbl2mat :1151-1232 (3-way)       the same operator applied to the joined
 *                                                      stream (true (A x B) x C; the reference's
 *                                                      own tbl2mat is defective)
 *   proc_where_clause :1435-1463                       mdb_dev_filter: conjuncts that read one table filter
 *                                                      it BEFORE the join (same rows for inner joins),
 *                                                      the rest run over the joined stream
 *   proc_groupby_clause :1526-1588                     mdb_dev_group_count over the gathered key
 *                                                      (several fields: mdb_dev_group_count_multi)
 *   proc_select_clause :1369-1433 (projection)         mdb_dev_gather64 of the selected columns only
 *   handle_countonly_case :1590-1653                   COUNT(*) = stream length
 *   table_vacuum :1726                                 nothing to do (streams are always compact)
 *
 * plus one fused plan for the north-star shape (JOIN ... ON l = r GROUP BY that key, COUNT(*)),
 * which never materialises the joined rows (mdb_dev_join_group_count); it is chained over further
 * tables joined on the same key and also answers SELECT COUNT(*) over such joins; over two tables it also runs on a
 * packed composite key (ON l.x = r.x AND l.y = r.y GROUP BY those keys: composite_fused_plan).  After the
 * reference's phases come the clauses it parses but never executes - HAVING, DISTINCT, ORDER BY,
 * LIMIT (select_tail, mdb_exec_tail.c).
 *
 * mdb_exec_select() at the end of the file is the driver: the result column plan and the statement's shape, then ONE of the plan
 * stages (plan_fused_chain, composite_fused_plan, plan_keys_only, plan_filter_project, plan_general) produces the stream - x->plan
 * says which kind -, then the tail clauses and the projection (mdb_exec_result.c).  One more table into the stream: mdb_exec_join.c.
 *
 * Early materialisation is replaced by late materialisation: a tuple stream is a set of uint32
 * row-id vectors (one per FROM table; NULL = identity), so joins / filters / grouping move 4-byte
 * ids and only the selected columns are gathered once at the end.
 *
 * The plan normalisation the reference does in its optimiser (optimiser_select.c:114-238: NAME ->
 * fully qualified FIELDNAME, alias -> table name, SELECT * expansion) and the checks of its
 * semantic phase that guard the executor (semantic_select.c: unknown table/column, duplicate
 * column names across FROM tables S1, operand types S2, GROUP BY rule S4) happen in
 * resolve_select() (mdb_exec_resolve.c).
 */
#include "mdb_exec_internal.h"

/* ------------------------------------------------------------------ device-side execution state */



int dev_fail(struct exec *x, const char *what)
{
	snprintf(x->err, x->errlen, "execution phase: %s: %s\n", what, mdb_dev_last_error(x->dev));
	return -MIDORIDB_INTERNAL;
}

/* ... and of the sharded mode's exchange handle (what == NULL: the handle's own text says what failed) */
int dist_fail(struct exec *x, const char *what)
{
	if (what)
		snprintf(x->err, x->errlen, "execution phase: %s: %s\n", what, mdb_dist_last_error(x->cat->dist));
	else
		snprintf(x->err, x->errlen, "execution phase: %s\n", mdb_dist_last_error(x->cat->dist));
	return -MIDORIDB_INTERNAL;
}

int track(struct exec *x, void *p)
{
	if (x->bufs.n == x->bufs.cap) {
		int nc = x->bufs.cap ? x->bufs.cap * 2 : 32;
		void **np = realloc(x->bufs.p, sizeof(void *) * (size_t)nc);
		if (!np)
			return -MIDORIDB_NOMEM;
		x->bufs.p = np;
		x->bufs.cap = nc;
	}
	x->bufs.p[x->bufs.n++] = p;
	return 0;
}

void *dalloc(struct exec *x, size_t bytes)
{
	void *p = NULL;
	if (mdb_dev_alloc(x->dev, bytes ? bytes : 8, &p))
		return NULL;
	if (track(x, p)) {
		mdb_dev_free(x->dev, p);
		return NULL;
	}
	return p;
}

void free_all(struct exec *x)
{
	for (int i = 0; i < x->bufs.n; i++)
		mdb_dev_free(x->dev, x->bufs.p[i]);
	free(x->bufs.p);
	x->bufs.p = NULL;
	x->bufs.n = x->bufs.cap = 0;
}

/* Re-map every row-id vector of the stream through `sel` (n_new positions into the old stream). */
int stream_select(struct exec *x, int ntabs_in_stream, const uint32_t *sel, uint64_t n_new)
{
	for (int t = 0; t < ntabs_in_stream; t++) {
		if (x->rid[t]) {
			uint32_t *nr = dalloc(x, n_new * 4);
			if (!nr)
				return dev_fail(x, "allocating row ids");
			if (n_new && mdb_dev_gather32(x->dev, x->rid[t], sel, n_new, nr))
				return dev_fail(x, "re-mapping row ids");
			x->rid[t] = nr;
		} else {
			x->rid[t] = (uint32_t *)sel;	/* identity composed with sel */
		}
	}
	x->n = n_new;
	return MIDORIDB_OK;
}

/* keep the rows sel[0..n_new) of the current stream: row-id vectors (or the fused key column) and COUNT(*) */
int stream_apply_sel(struct exec *x, int ntabs_in_stream, const uint32_t *sel, uint64_t n_new)
{
	if (x->d_count) {
		int64_t *nc = dalloc(x, (n_new ? n_new : 1) * 8);
		if (!nc || (n_new && mdb_dev_gather64(x->dev, x->d_count, NULL, sel, n_new, nc, NULL)))
			return dev_fail(x, "re-mapping COUNT(*)");
		x->d_count = nc;
	}
	for (int i = 0; i < x->nagg; i++) {	/* SUM / MIN / MAX / AVG columns of the grouped stream, with their NULL bits */
		void *nv;
		uint64_t *nb;
		if (!x->d_agg[i])
			continue;
		nv = dalloc(x, (n_new ? n_new : 1) * 8);
		nb = dalloc(x, ((n_new + 63) / 64 + 1) * 8);
		if (!nv || !nb || (n_new && mdb_dev_gather64(x->dev, x->d_agg[i], x->d_agg_nulls[i], sel, n_new, nv, nb)))
			return dev_fail(x, "re-mapping an aggregate column");
		x->d_agg[i] = nv;
		x->d_agg_nulls[i] = nb;
	}
	for (int i = 0; i < x->nwin; i++) {	/* the window items' columns, with their NULL bits */
		void *nv;
		uint64_t *nb;
		if (!x->d_win[i])
			continue;
		nv = dalloc(x, (n_new ? n_new : 1) * 8);
		nb = dalloc(x, ((n_new + 63) / 64 + 1) * 8);
		if (!nv || !nb || (n_new && mdb_dev_gather64(x->dev, x->d_win[i], x->d_win_nulls[i], sel, n_new, nv, nb)))
			return dev_fail(x, "re-mapping a window function's column");
		x->d_win[i] = nv;
		x->d_win_nulls[i] = nb;
	}
	if (stream_is_keys(x)) {
		for (int k = 0; k < (x->nfused ? x->nfused : 1); k++) {	/* (a composite key: every key column of the stream) */
			const int64_t *from = x->nfused ? x->d_fused_keys[k] : x->d_fused_key;
			int64_t *nk = dalloc(x, (n_new ? n_new : 1) * 8);
			if (!nk || (n_new && mdb_dev_gather64(x->dev, from, NULL, sel, n_new, nk, NULL)))
				return dev_fail(x, "re-mapping the group key");
			if (x->nfused)
				x->d_fused_keys[k] = nk;
			if (!k)
				x->d_fused_key = nk;
		}
		x->n = n_new;
		return MIDORIDB_OK;
	}
	return stream_select(x, ntabs_in_stream, sel, n_new);
}

/* the key column of the fused stream that holds field (tbl_idx, col_idx): the one there is, or - on a composite key - the column of the
 * ON equality that names the field on either side */
int64_t *fused_key_column(const struct exec *x, int tbl_idx, int col_idx)
{
	for (int i = 0; i < x->nfused_map; i++)
		if (x->fused_tbl[i] == tbl_idx && x->fused_col[i] == col_idx)
			return x->d_fused_keys[x->fused_at[i]];
	return x->d_fused_key;
}

/* device pointer to a column's key/value vector for the current stream (gathered when needed) */
int stream_column(struct exec *x, const struct mdb_expr *f, const int64_t **vals, const uint64_t **nulls)
{
	struct mdb_column *col = &x->s->tabs[f->tbl_idx].t->cols[f->col_idx];
	*vals = col->d_data;
	*nulls = col->d_nullbits;
	if (x->rid[f->tbl_idx] && x->n) {
		int64_t *v = dalloc(x, x->n * 8);
		const bool want_nb = col->d_nullbits || x->may_be_absent[f->tbl_idx];	/* ("no row" cells are NULL cells) */
		uint64_t *nb = want_nb ? dalloc(x, ((x->n + 63) / 64) * 8) : NULL;
		if (!v || (want_nb && !nb))
			return dev_fail(x, "allocating a key column");
		if (mdb_dev_gather64(x->dev, col->d_data, col->d_nullbits, x->rid[f->tbl_idx], x->n, v, nb))
			return dev_fail(x, "gathering a key column");
		*vals = v;
		*nulls = nb;
	}
	return MIDORIDB_OK;
}

/* Key vector of an equi-join over table column `col`, rows rid[0..n) (rid == NULL: rows 0..n-1).  INTEGER keys are the
 * column itself; DOUBLE keys go through mdb_dev_double_join_keys so that the join's word comparison is the reference's
 * IEEE `==` (cmp_double_value_to_value, executor_select.c:440-460): -0.0 joins +0.0, NaN joins nothing. */
int double_join_keys(struct exec *x, const struct mdb_column *col, const uint32_t *rid, uint64_t n, const void **vals,
			    const uint64_t **nulls)
{
	int64_t *v = dalloc(x, (n ? n : 1) * 8);
	uint64_t *nb = dalloc(x, ((n + 63) / 64 + 1) * 8);
	if (!v || !nb)
		return dev_fail(x, "allocating a key column");
	if (mdb_dev_double_join_keys(x->dev, col->d_data, col->d_nullbits, rid, n, v, nb))
		return dev_fail(x, "preparing DOUBLE join keys");
	*vals = v;
	*nulls = nb;
	return MIDORIDB_OK;
}

/* ------------------------------------------------------------------ FROM clause */

/* split an ON expression into conjuncts; pick the first "left-stream field = field of table t" as the hash key */
void collect_conjuncts(struct mdb_expr *e, struct mdb_expr **out, int *n, int cap)
{
	if (e->kind == MDB_EX_LOGOP && e->op == 0) {
		collect_conjuncts(e->kids[0], out, n, cap);
		collect_conjuncts(e->kids[1], out, n, cap);
	} else if (*n < cap) {
		out[(*n)++] = e;
	} else {
		*n = cap + 1;	/* overflow marker */
	}
}

/* which FROM tables an expression reads: bit t set for table t */
uint64_t expr_tables(const struct mdb_expr *e)
{
	uint64_t m = 0;
	if (!e)
		return 0;
	if (e->kind == MDB_EX_FIELD && e->tbl_idx >= 0 && e->tbl_idx < 64)
		m |= 1ull << e->tbl_idx;
	for (int i = 0; i < e->nkids; i++)
		m |= expr_tables(e->kids[i]);
	return m;
}

/* WHERE push-down: the reference filters AFTER the joins (proc_where_clause :1435-1463), which for inner joins gives
 * the same rows as filtering a table first whenever a conjunct reads only that table.  Splits the top-level
 * AND-conjuncts of the WHERE clause: push[t][..] = table t's own conjuncts (constants go with table 0),
 * residual[..] = conjuncts that read several tables and stay above the joins.  false = too many to split.
 * Outer joins: WHERE runs after the join, and a table that some join NULL-supplies (T of S LEFT JOIN T; every table of S in S RIGHT
 * JOIN T; both, T and every table of S, in S FULL JOIN T) has rows in the stream that are not rows of the table - its conjuncts stay above the joins too (they see the NULL cells);
 * a table that every join preserves keeps its push-down (a row the filter drops would be dropped after the joins with all its pairs). */

bool where_split(const struct mdb_select *s, struct where_split *w)
{
	struct mdb_expr *all[64];
	int n = 0;
	memset(w, 0, sizeof(*w));
	if (!s->where)
		return true;
	if (s->ntabs > PUSH_TABS)
		return false;
	collect_conjuncts(s->where, all, &n, 64);
	if (n > 64)
		return false;
	uint64_t null_supplied = 0;
	for (int t = 1; t < s->ntabs; t++) {
		if (mdb_join_is_left(s->join_type[t]))
			null_supplied |= 1ull << t;
		else if (mdb_join_is_right(s->join_type[t]))
			null_supplied |= (1ull << t) - 1;
		else if (mdb_join_is_full(s->join_type[t]))
			null_supplied |= (2ull << t) - 1;
	}
	for (int i = 0; i < n; i++) {
		const uint64_t m = expr_tables(all[i]);
		int t = 0;
		if ((m & (m - 1)) || ((m ? m : 1ull) & null_supplied)) {	/* (a constant goes with table 0) */
			w->residual[w->nresidual++] = all[i];
			continue;
		}
		while (m && !((m >> t) & 1))
			t++;
		if (w->npush[t] == PUSH_MAX)
			return false;
		w->push[t][w->npush[t]++] = all[i];
	}
	return true;
}

/* rows of base table t that pass its pushed-down conjuncts: *sel = ascending row ids (NULL = every row), *m = how many */
int table_filter(struct exec *x, int t, const struct mdb_expr *const *conj, int nconj, const uint32_t **sel, uint64_t *m)
{
	struct mdb_table *tb = x->s->tabs[t].t;
	struct pred_prog p;
	uint32_t *v;
	*sel = NULL;
	*m = tb->nrows;
	if (!nconj || !tb->nrows)
		return MIDORIDB_OK;
	memset(&p, 0, sizeof(p));
	{
		uint32_t *saved = x->rid[t];	/* the program reads the BASE table, whatever the stream holds for t */
		x->rid[t] = NULL;
		for (int i = 0; i < nconj; i++)
			if (pred_compile(x, &p, conj[i]) || (i && pred_emit(&p, MDB_P_AND, 0, 0, 0, 0, 0))) {
				x->rid[t] = saved;
				pred_compile_failed(x);
				return -MIDORIDB_ERROR;
			}
		x->rid[t] = saved;
	}
	v = dalloc(x, tb->nrows * 4);
	if (!v)
		return dev_fail(x, "allocating the selection vector");
	if (mdb_dev_filter(x->dev, p.insn, p.n, p.cols, p.ncols, tb->nrows, v, m))
		return dev_fail(x, "filter");
	*sel = v;
	return MIDORIDB_OK;
}

/* column `key` of base table t restricted to the rows in sel (NULL = all): device pointers for an operator */
int table_column(struct exec *x, int t, const struct mdb_expr *key, const uint32_t *sel, uint64_t m, const void **vals,
			const uint64_t **nulls)
{
	struct mdb_column *col = &x->s->tabs[t].t->cols[key->col_idx];
	*vals = col->d_data;
	*nulls = col->d_nullbits;
	if (sel) {
		int64_t *v = dalloc(x, (m ? m : 1) * 8);
		uint64_t *nb = col->d_nullbits ? dalloc(x, ((m + 63) / 64 + 1) * 8) : NULL;
		if (!v || (col->d_nullbits && !nb))
			return dev_fail(x, "allocating a key column");
		if (m && mdb_dev_gather64(x->dev, col->d_data, col->d_nullbits, sel, m, v, nb))
			return dev_fail(x, "gathering a key column");
		*vals = v;
		*nulls = nb;
	}
	return MIDORIDB_OK;
}

/* key column of table t for the fused plan: the base column, or the keys of the rows that pass the pushed conjuncts */
int fused_operand(struct exec *x, int t, const struct mdb_expr *key, const struct mdb_expr *const *conj, int nconj,
			 const void **vals, const uint64_t **nulls, uint64_t *n)
{
	const uint32_t *sel;
	int rc = table_filter(x, t, conj, nconj, &sel, n);
	if (rc)
		return rc;
	return table_column(x, t, key, sel, *n, vals, nulls);
}

/* The catalog's statistics of the key columns of the operator call that follows (mdb_dev_call_stats, include/mdb_dev.h): fl / fr = the
 * fields the key columns pl / pr come from - the columns themselves or filtered streams of them (a superset range is fine).  Nothing is
 * handed over for column types without a range (DOUBLE, VARCHAR), for shadow tables of the sharded mode, or when a range cannot be had:
 * the operator then looks at the data itself.  op_stats_end() after the call. */
void op_stats_begin(struct exec *x, const struct mdb_expr *fl, const void *pl, const struct mdb_expr *fr, const void *pr)
{
	struct mdb_dev_col_stats st[2];
	const struct mdb_expr *f[2] = { fl, fr };
	memset(st, 0, sizeof(st));
	if (x->cat->dist || !fl || !pl || (fr && !pr))
		return;
	if (x->has_outer)	/* (a stream that repeats or NULL-extends rows: the columns' statistics promise nothing about it) */
		return;
	for (int i = 0; i < (fr ? 2 : 1); i++) {
		if (f[i]->kind != MDB_EX_FIELD || f[i]->tbl_idx < 0 || x->orig_tab[f[i]->tbl_idx])
			return;
		struct mdb_table *tb = x->s->tabs[f[i]->tbl_idx].t;
		struct mdb_column *col = &tb->cols[f[i]->col_idx];
		if (mdb_col_range(x->cat, tb, col, &st[i].min, &st[i].max) != MIDORIDB_OK)
			return;
		st[i].rows = tb->device_only ? tb->dev_rows : tb->nrows;
		st[i].nulls = col->null_count;
		/* (measured at ingest, followed through appended rows; a filtered stream of a column without a value twice has none either) */
		if (mdb_col_distinct(x->cat, tb, col))
			st[i].flags |= MDB_COL_DISTINCT;
	}
	(void)mdb_dev_call_stats(x->dev, pl, &st[0], fr ? pr : NULL, fr ? &st[1] : NULL);
}

/* Most groups a GROUP BY over the key field f can have, by the catalog: a group needs a key value, and the column holds at most
 * max - min + 1 of them (a filtered stream of the column: fewer).  `rows` when nothing is known. */
uint64_t op_groups_bound(struct exec *x, const struct mdb_expr *f, uint64_t rows)
{
	int64_t lo, hi;
	if (x->cat->dist || !f || f->kind != MDB_EX_FIELD || f->tbl_idx < 0 || x->orig_tab[f->tbl_idx])
		return rows;
	struct mdb_table *tb = x->s->tabs[f->tbl_idx].t;
	if (mdb_col_range(x->cat, tb, &tb->cols[f->col_idx], &lo, &hi) != MIDORIDB_OK || lo > hi)
		return rows;
	const uint64_t span = (uint64_t)hi - (uint64_t)lo;	/* (max - min: + 1 below, unless that is 2^64) */
	return span + 1 && span + 1 < rows ? span + 1 : rows;
}

void op_stats_end(struct exec *x)
{
	(void)mdb_dev_call_stats(x->dev, NULL, NULL, NULL, NULL);
}


double now_ms(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

/* is the plan the fused north-star shape?  returns the group field's side (0 = left key, 1 = right key) or -1 */
/* SUM / MIN / MAX / AVG: one mdb_dev_group_aggregate call for all aggregates of the statement, over the stream as it is BEFORE its rows are
 * reduced to the groups' first rows (first[G] of the GROUP BY operator over gk[0 .. nk); nk == 0: one group, nk == MDB_AGG_IDENTITY: group i is
 * row i).  The result columns d_agg[] have G rows and belong to the grouped stream. */
static int stream_aggregate(struct exec *x, const struct mdb_sort_key *gk, int nk, const uint32_t *first, uint64_t G)
{
	struct mdb_agg ag[MDB_AGG_MAX_AGGS];
	struct mdb_count_distinct cd[MDB_AGG_MAX_AGGS];
	uint32_t form = 0, cd_forms[MDB_AGG_MAX_AGGS];
	int na = 0, ncd = 0;

	for (int i = 0; i < x->nagg; i++) {
		const int t = x->agg_tbl[i];
		struct mdb_table *tb = x->s->tabs[t].t;
		struct mdb_column *col = &tb->cols[x->agg_col[i]];
		const void *values = col->d_data;
		if (!values && !(values = dalloc(x, 8)))	/* (an empty table under an outer join: every tuple is at "no row", no cell is read) */
			return dev_fail(x, "aggregates");
		const size_t nbytes = ((G + 63) / 64 + 1) * 8;
		x->d_agg[i] = dalloc(x, G * 8);
		x->d_agg_nulls[i] = dalloc(x, nbytes);
		if (!x->d_agg[i] || !x->d_agg_nulls[i])
			return dev_fail(x, "allocating aggregate columns");
		if (x->agg_op[i] == MDB_AGG_COUNT_DISTINCT) {
			/* COUNT(DISTINCT col): the other operator; a count is never NULL.  The catalog's value range - for VARCHAR the ids the
			 * dictionary has given out - lets the operator take its bitmap form; it is a promise the operator checks */
			struct mdb_count_distinct *c = &cd[ncd++];
			int64_t lo = 0, hi = -1;
			memset(c, 0, sizeof(*c));
			c->type = col->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
			c->values = values;
			c->nullbits = col->d_nullbits;
			c->rid = x->rid[t];
			if (col->type == MDB_CT_VARCHAR) {
				lo = 1;
				hi = (int64_t)x->cat->dict.n;
			} else if (x->orig_tab[t] || mdb_col_range(x->cat, tb, col, &lo, &hi) != MIDORIDB_OK) {
				lo = 0;
				hi = -1;
			}
			c->has_range = lo <= hi;
			c->min = lo;
			c->max = hi;
			c->out = x->d_agg[i];
			if (mdb_dev_memset(x->dev, x->d_agg_nulls[i], 0, nbytes))
				return dev_fail(x, "clearing the NULL bits of COUNT(DISTINCT)");
			continue;
		}
		ag[na].op = x->agg_op[i];
		ag[na].type = col->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
		ag[na].values = values;
		ag[na].nullbits = col->d_nullbits;
		ag[na].rid = x->rid[t];
		ag[na].out = x->d_agg[i];
		ag[na].out_nullbits = x->d_agg_nulls[i];
		na++;
	}
	if (na) {
		if (mdb_dev_group_aggregate(x->dev, gk, nk, x->n, first, G, ag, na, &form))
			return dev_fail(x, "SUM / MIN / MAX / AVG");
		if (form == 1 || form == 2)
			x->agg_calls[form - 1]++;
	}
	if (ncd) {
		if (mdb_dev_group_count_distinct(x->dev, gk, nk, x->n, first, G, cd, ncd, cd_forms))
			return dev_fail(x, "COUNT(DISTINCT)");
		for (int c = 0; c < ncd; c++)
			if (cd_forms[c] == 1 || cd_forms[c] == 2)
				x->cd_calls[cd_forms[c] - 1]++;
	}
	return MIDORIDB_OK;
}

/* Window functions: the plan stage between FROM / WHERE and the tail clauses.  The statement's items whose OVER clauses are equal field for
 * field share one mdb_dev_window call - one sort, one pair of head bitmaps, one set of scan passes.  Keys and arguments are read through the
 * stream's row ids, as ORDER BY and DISTINCT read theirs: a tuple without a row of the table (MDB_NO_ROW under an outer join) is a NULL cell
 * to the operator.  The result columns d_win[] have one row per row of the stream. */
static void window_key(struct exec *x, const struct mdb_expr *f, int desc, struct mdb_sort_key *k)
{
	bind_operand(x, f, &k->values, &k->nullbits, &k->rid);
	k->type = f->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
	k->desc = desc;
}

int stream_windows(struct exec *x)
{
	bool done[MDB_WIN_MAX_FNS] = { false };
	const uint64_t n = x->n;
	void *no_cells = NULL;

	for (int i = 0; i < x->nwin; i++) {
		x->d_win[i] = dalloc(x, (n ? n : 1) * 8);
		x->d_win_nulls[i] = dalloc(x, ((n + 63) / 64 + 1) * 8);
		if (!x->d_win[i] || !x->d_win_nulls[i])
			return dev_fail(x, "allocating window function columns");
	}
	if (!n)
		return MIDORIDB_OK;
	for (int i = 0; i < x->nwin; i++) {
		const struct mdb_expr *lead = x->win_item[i];
		const int narg0 = mdb_win_narg(lead->op);
		struct mdb_sort_key part[MDB_SORT_MAX_KEYS], order[MDB_SORT_MAX_KEYS];
		struct mdb_window_fn fn[MDB_WIN_MAX_FNS];
		uint32_t form = 0;
		int nfn = 0;
		if (done[i])
			continue;
		for (int k = 0; k < lead->win_npart; k++)
			window_key(x, lead->kids[narg0 + k], 0, &part[k]);
		for (int k = 0; k < lead->win_norder; k++)
			window_key(x, lead->kids[narg0 + lead->win_npart + k], (lead->win_desc >> k) & 1u, &order[k]);
		for (int k = 0; k < lead->win_npart + lead->win_norder; k++) {
			struct mdb_sort_key *key = k < lead->win_npart ? &part[k] : &order[k - lead->win_npart];
			if (!key->values && !(key->values = no_cells ? no_cells : (no_cells = dalloc(x, 8))))	/* (an empty table under an outer join: every tuple is at "no row") */
				return dev_fail(x, "window functions");
		}
		for (int j = i; j < x->nwin; j++) {
			const struct mdb_expr *e = x->win_item[j];
			if (done[j] || !window_same_over(lead, e))
				continue;
			done[j] = true;
			memset(&fn[nfn], 0, sizeof(fn[nfn]));
			fn[nfn].op = e->op;
			fn[nfn].arg = e->win_arg;	/* LAG / LEAD / NTILE; a default is an INTEGER's int64, a TINYINT's 0 / 1 or a DOUBLE's bits (resolve_window) */
			fn[nfn].dflt_null = e->win_dflt == MDB_EX_NULL;
			if (e->win_dflt == MDB_EX_FLOAT)
				memcpy(&fn[nfn].dflt, &e->dval, 8);
			else
				fn[nfn].dflt = (uint64_t)e->ival;
			if (mdb_win_narg(e->op)) {
				struct mdb_sort_key arg;
				window_key(x, e->kids[0], 0, &arg);
				if (!arg.values && !(arg.values = no_cells ? no_cells : (no_cells = dalloc(x, 8))))
					return dev_fail(x, "window functions");
				fn[nfn].type = arg.type;
				fn[nfn].values = arg.values;
				fn[nfn].nullbits = arg.nullbits;
				fn[nfn].rid = arg.rid;
			}
			fn[nfn].out = x->d_win[j];
			fn[nfn].out_nullbits = x->d_win_nulls[j];
			nfn++;
		}
		if (mdb_dev_window(x->dev, part, lead->win_npart, order, lead->win_norder, n, fn, nfn, &form))
			return dev_fail(x, "window functions");
		x->win_calls++;
	}
	return MIDORIDB_OK;
}

/* The fused plan applies to  T0 JOIN T1 ON k0 = k1 [JOIN T2 ON (k0 | k1) = k2 ...] GROUP BY one of those keys, COUNT(*):
 * every join is an equi-join on the SAME key (each ON clause ties the new table's column to a key column already
 * in the chain); a WHERE clause must be pushable below the joins (where_pushable).  keys[t] = the key field of
 * table t.  count_only: the query is SELECT COUNT(*) over the join without GROUP BY - the same operator, of which only
 * the joined-row total is used.  Returns 0 when it applies, -1 otherwise. */
int fused_chain(struct mdb_select *s, const struct mdb_expr **keys, bool count_only)
{
	if (s->ntabs < 2 || (count_only ? s->ngroup != 0 : s->ngroup != 1))
		return -1;
	for (int t = 0; t < s->ntabs; t++)
		keys[t] = NULL;
	for (int t = 1; t < s->ntabs; t++) {
		const struct mdb_expr *on = s->on[t], *mine, *other;
		if (!on || on->kind != MDB_EX_CMP || on->op != MDB_CMP_EQ || on->kids[0]->kind != MDB_EX_FIELD || on->kids[1]->kind != MDB_EX_FIELD)
			return -1;
		if (on->kids[0]->tbl_idx == t && on->kids[1]->tbl_idx < t) {
			mine = on->kids[0];
			other = on->kids[1];
		} else if (on->kids[1]->tbl_idx == t && on->kids[0]->tbl_idx < t) {
			mine = on->kids[1];
			other = on->kids[0];
		} else {
			return -1;
		}
		if (t == 1)
			keys[0] = other;
		else if (!keys[other->tbl_idx] || !field_eq(other, keys[other->tbl_idx]))
			return -1;
		if (mine->type != other->type)
			return -1;
		if (mine->type == MDB_CT_DOUBLE)
			return -1;	/* DOUBLE keys join through their IEEE-canonical words (join_next_table), whose values are not
					 * the column's: the general plan gathers the group keys from the table itself */
		keys[t] = mine;
	}
	if (count_only)
		return 0;	/* SELECT COUNT(*) FROM the join: only the number of joined rows is wanted */
	for (int t = 0; t < s->ntabs; t++)
		if (field_eq(s->group[0], keys[t]))
			return 0;
	return -1;
}

/* a two-table INNER JOIN ON l = r whose result columns are all one of the two key columns, nothing else asked of it: kj[0..1] = the key
 * fields (left table's first).  With the order left open by the host (mdb_database_groups_any_order) mdb_dev_join_keys answers; in the
 * reference's order mdb_dev_join_keys_ordered, when the join turns out to be a primary-key join */
bool keys_only_join(const struct mdb_select *s, const struct mdb_catalog *cat, const struct result_cols *rc, bool has_agg, const struct mdb_expr **kj)
{
	if (cat->dist || s->ntabs != 2 || s->where || s->ngroup || rc->has_count || has_agg || s->distinct || s->norder || s->having || s->has_limit || !rc->ncols)
		return false;
	const struct mdb_expr *on = s->on[1];
	if (!on || on->kind != MDB_EX_CMP || on->op != MDB_CMP_EQ || on->kids[0]->kind != MDB_EX_FIELD || on->kids[1]->kind != MDB_EX_FIELD)
		return false;
	const struct mdb_expr *a = on->kids[0], *b = on->kids[1];
	if (a->tbl_idx == b->tbl_idx || a->type != b->type || a->type == MDB_CT_DOUBLE)
		return false;	/* (DOUBLE keys join through their IEEE-canonical words, whose values are not the column's) */
	kj[0] = a->tbl_idx == 0 ? a : b;
	kj[1] = a->tbl_idx == 0 ? b : a;
	if (!s->tabs[0].t->nrows || !s->tabs[1].t->nrows)
		return false;	/* (an empty side: the general plan answers "no rows") */
	for (int c = 0; c < rc->ncols; c++) {
		const int t = rc->tbl[rc->src[c]], col = rc->col[rc->src[c]];
		if (t < 0 || !((t == kj[0]->tbl_idx && col == kj[0]->col_idx) || (t == kj[1]->tbl_idx && col == kj[1]->col_idx)))
			return false;
	}
	return true;
}

/* ------------------------------------------------------------------ x [NOT] IN (SELECT ...)
 * Every subquery node under e is evaluated once, inner subqueries first (the nested statement evaluates its own on its way), before the
 * outer statement's plan is chosen: the nested SELECT runs with its result kept on the device - whatever the database's setting is -,
 * its one column goes to mdb_dev_set_from_column, the result is freed at once.  The set lives in the node until the outer statement
 * ends (subqueries_release, on every path out of the statement). */
int subqueries_eval(struct mdb_catalog *cat, struct mdb_expr *e, char *err, size_t errlen)
{
	int rc;

	if (!e)
		return MIDORIDB_OK;
	for (int i = 0; i < e->nkids; i++)
		if ((rc = subqueries_eval(cat, e->kids[i], err, errlen)))
			return rc;
	if (e->kind != MDB_EX_ISIN || !e->sub)
		return MIDORIDB_OK;

	if (e->sub_set) {	/* (a statement that is run again builds its sets again) */
		mdb_dev_set_free(cat->dev, e->sub_set);
		e->sub_set = NULL;
	}
	struct mdb_result *r = NULL;
	const bool on_device = cat->results_on_device;
	cat->results_on_device = true;
	rc = mdb_exec_select(cat, e->sub, &r, err, errlen);
	cat->results_on_device = on_device;
	if (rc)
		return rc;
	const void *vals = NULL;
	const uint64_t *nulls = NULL;
	void *one = NULL;	/* a result of one row stays on the host (a lone COUNT(*) or MAX(v)): its cell and NULL word, uploaded */
	struct mdb_dev_set_info info = { 0 };
	if (r->ncols != 1) {
		ERR("a subquery must select one column\n");
		rc = -MIDORIDB_ERROR;
	} else if (r->nrows && r->d_data && r->d_data[0]) {
		vals = r->d_data[0];
		nulls = r->d_nullbits ? r->d_nullbits[0] : NULL;
	} else if (r->nrows == 1 && r->data && r->data[0]) {
		const uint64_t cell[2] = { (uint64_t)r->data[0][0], r->nullbits && r->nullbits[0] ? r->nullbits[0][0] & 1u : 0u };
		if (mdb_dev_alloc(cat->dev, sizeof(cell), &one) || mdb_dev_h2d(cat->dev, one, cell, sizeof(cell))) {
			ERR("execution phase: IN (SELECT ...): %s\n", mdb_dev_last_error(cat->dev));
			rc = -MIDORIDB_INTERNAL;
		}
		vals = one;
		nulls = cell[1] ? (const uint64_t *)one + 1 : NULL;
	} else if (r->nrows) {
		ERR("execution phase: internal error (IN (SELECT ...): the subquery's column is nowhere)\n");
		rc = -MIDORIDB_INTERNAL;
	}
	if (!rc) {
		rc = mdb_dev_set_from_column(cat->dev, vals, nulls, NULL, r->nrows, e->kids[0]->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64, 0,
					     &e->sub_set, &info);
		if (rc && info.members > MDB_SET_MAX_VALUES)
			ERR("IN (SELECT ...): %llu distinct values, a set takes at most %llu\n", (unsigned long long)info.members,
			    (unsigned long long)MDB_SET_MAX_VALUES);
		else if (rc)
			ERR("execution phase: IN (SELECT ...): %s\n", mdb_dev_last_error(cat->dev));
	}
	if (!rc) {
		e->sub_rows = r->nrows;
		e->sub_nulls = info.cells_null;
		e->sub_members = info.members;
		cat->subquery_sets++;
	}
	if (one)
		mdb_dev_free(cat->dev, one);
	mdb_result_free(r);
	stmt_dict = &cat->dict;
	return rc;
}

void subqueries_release(struct mdb_catalog *cat, struct mdb_expr *e)
{
	if (!e)
		return;
	for (int i = 0; i < e->nkids; i++)
		subqueries_release(cat, e->kids[i]);
	if (e->sub_set) {
		mdb_dev_set_free(cat->dev, e->sub_set);
		e->sub_set = NULL;
	}
}

/* ------------------------------------------------------------------ the statement: result column plan and shape */

static void result_cols_free(struct result_cols *rc)
{
	free(rc->keys);
	free(rc->order);
	free(rc->tbl);
	free(rc->col);
	free(rc->src);
}

/* The result column set in the reference's order (R3): COUNT(*) first if selected, then every column of every FROM table left to right;
 * projected afterwards to the select list.  Collects the select list's SUM / MIN / MAX / AVG into x on its way, each (function, column)
 * once: result column "SUM(<table>.<column>)", ordered with all the others.  result_cols_free() whatever is returned. */
static int result_cols_build(struct exec *x, struct result_cols *rc)
{
	struct mdb_select *s = x->s;
	int total, r;

	for (int i = 0; i < s->nsel; i++)
		rc->has_count |= s->sel[i]->kind == MDB_EX_COUNT;
	for (int i = 0; i < s->nsel; i++)
		if (s->sel[i]->kind == MDB_EX_AGG && agg_index(x, s->sel[i]) < 0 && x->nagg < MDB_AGG_MAX_AGGS) {
			x->agg_op[x->nagg] = s->sel[i]->op;
			x->agg_tbl[x->nagg] = s->sel[i]->tbl_idx;
			x->agg_col[x->nagg] = s->sel[i]->col_idx;
			x->agg_type[x->nagg] = s->sel[i]->type;
			x->nagg++;
		}
	for (int i = 0; i < s->nsel; i++)
		if (s->sel[i]->kind == MDB_EX_WINDOW && s->sel[i]->win_idx >= 0 && s->sel[i]->win_idx < MDB_WIN_MAX_FNS) {
			x->win_item[s->sel[i]->win_idx] = s->sel[i];
			x->nwin = s->sel[i]->win_idx + 1 > x->nwin ? s->sel[i]->win_idx + 1 : x->nwin;
		}
	total = rc->has_count + x->nagg + x->nwin;
	for (int t = 0; t < s->ntabs; t++)
		total += s->tabs[t].t->ncols;
	rc->keys = calloc((size_t)total, sizeof(*rc->keys));
	rc->order = calloc((size_t)total, sizeof(int));
	rc->tbl = calloc((size_t)total, sizeof(int));
	rc->col = calloc((size_t)total, sizeof(int));
	if (!rc->keys || !rc->order || !rc->tbl || !rc->col)
		return -MIDORIDB_NOMEM;
	if (rc->has_count) {
		strcpy(rc->keys[rc->nkeys], "COUNT(*)");
		rc->tbl[rc->nkeys++] = COLSRC_COUNT;
	}
	for (int a = 0; a < x->nagg; a++) {
		snprintf(rc->keys[rc->nkeys], MDB_NAME_LEN, "%s%.*s.%.*s)", mdb_agg_open(x->agg_op[a]), x->agg_op[a] == MDB_AGG_COUNT_DISTINCT ? 50 : 56,
			 s->tabs[x->agg_tbl[a]].t->name, x->agg_op[a] == MDB_AGG_COUNT_DISTINCT ? 50 : 56, s->tabs[x->agg_tbl[a]].t->cols[x->agg_col[a]].name);
		rc->tbl[rc->nkeys++] = COLSRC_AGG(a);
	}
	for (int w = 0; w < x->nwin; w++) {	/* a window item: named by its alias, or by its function's text ("SUM(A.v) OVER") */
		mdb_win_result_name(x->win_item[w], rc->keys[rc->nkeys]);
		for (int i = 0; s->sel_alias && i < s->nsel; i++)
			if (s->sel[i] == x->win_item[w] && s->sel_alias[i][0])
				mdb_copy_name(rc->keys[rc->nkeys], s->sel_alias[i]);
		rc->tbl[rc->nkeys++] = COLSRC_WIN(w);
	}
	for (int t = 0; t < s->ntabs; t++)
		for (int c = 0; c < s->tabs[t].t->ncols; c++) {
			snprintf(rc->keys[rc->nkeys], MDB_NAME_LEN, "%.60s.%.60s", s->tabs[t].t->name, s->tabs[t].t->cols[c].name);
			rc->tbl[rc->nkeys] = t;
			rc->col[rc->nkeys++] = c;
		}
	if ((r = mdb_reference_column_order((const char (*)[MDB_NAME_LEN])rc->keys, rc->nkeys, rc->order)))
		return r;

	/* the result columns that are wanted, in the reference's order */
	rc->src = calloc((size_t)(rc->nkeys ? rc->nkeys : 1), sizeof(int));
	if (!rc->src)
		return -MIDORIDB_NOMEM;
	for (int k = 0; k < rc->nkeys; k++) {
		const int key = rc->order[k];
		bool want = rc->tbl[key] < 0 || s->select_all;
		for (int i = 0; i < s->nsel && !want; i++)
			want = s->sel[i]->kind == MDB_EX_FIELD && s->sel[i]->tbl_idx == rc->tbl[key] && s->sel[i]->col_idx == rc->col[key];
		if (want)
			rc->src[rc->ncols++] = key;
	}
	return MIDORIDB_OK;
}

/* The statement's shape, computed once: how the WHERE clause splits, whether the statement is a bare COUNT(*), and which of the plans
 * that apply to a whole statement does - the single-key fused chain (st->fkeys) or the join of two key columns (st->kj). */
static void select_shape(struct exec *x, struct select_stmt *st)
{
	struct mdb_select *s = x->s;
	struct mdb_catalog *cat = x->cat;

	st->split_ok = where_split(s, &st->ws);
	st->only_count = st->rc.has_count && !s->ngroup && !s->select_all;
	for (int i = 0; i < s->nsel; i++)
		st->only_count = st->only_count && s->sel[i]->kind == MDB_EX_COUNT;
	/* (the fused operator is an inner join and knows COUNT(*) only: a statement with SUM / MIN / MAX / AVG materialises its join) */
	/* (nor a window function: it asks for a value per row of the joined stream) */
	st->fused_chain = s->ntabs <= PUSH_TABS && !x->has_outer && !st->has_agg && !st->has_win && fused_chain(s, st->fkeys, st->only_count) >= 0;
	if (st->fused_chain && !cat->dist && st->split_ok) {
		/* join elimination: when the catalog says every right table of the chain is a complete primary key over the first table's key range,
		 * the fused join + GROUP BY operator has nothing to find out - the general plan drops those joins (join_next_table) and groups the
		 * first table's key column alone (the identity when that column holds no value twice) */
		bool all = s->ntabs > 1;
		for (int t = 1; t < s->ntabs && all; t++)
			all = !st->ws.npush[t] && only_key_needed(x, t, st->fkeys[t]->col_idx) && join_is_total_by_catalog(x, st->fkeys[0], st->fkeys[t]);
		if (all)
			st->fused_chain = false;
	}
	if (st->fused_chain && (!st->split_ok || st->ws.nresidual))
		st->fused_chain = false;	/* a conjunct reads several tables: it has to see the joined rows */
	if (st->fused_chain && cat->dist && s->ntabs > 2 && st->fkeys[0]->type == MDB_CT_VARCHAR)
		st->fused_chain = false;	/* (sharded chains over VARCHAR keys: the general plan exchanges the rows by their strings' common ids) */
	st->keys_only = !x->has_outer && !st->has_win && keys_only_join(s, cat, &st->rc, st->has_agg, st->kj);
}

/* ------------------------------------------------------------------ plan stages */

/* The join of two key columns, nothing else selected, in the reference's order: tried as a primary-key join first (the keys with
 * partners in the left table's row order; large tables only: the attempt runs the ordered join + GROUP BY operator), and left to the
 * materialising join of the general plan when a key has several rows on a side (st->keys_only becomes false).  Runs before any plan. */
static int keys_only_ordered(struct exec *x, struct select_stmt *st)
{
	struct mdb_select *s = x->s;
	const struct mdb_expr *const *kj = st->kj;
	if (!st->keys_only || x->cat->groups_any_order)
		return MIDORIDB_OK;
	const struct mdb_table *tl = s->tabs[kj[0]->tbl_idx].t, *tr = s->tabs[kj[1]->tbl_idx].t;
	int served = 0;
	int krc = 0;
	if (tl->nrows && !tl->cols[kj[0]->col_idx].d_nullbits && tl->cols[kj[0]->col_idx].d_data && join_is_total_by_catalog(x, kj[0], kj[1])) {
		/* join elimination: every row of the left table has exactly one partner (the catalog's statistics) - the joined rows' key column
		 * IS the left table's key column, in its order, without a kernel */
		st->keys_ordered = (int64_t *)tl->cols[kj[0]->col_idx].d_data;
		st->keys_ordered_rows = tl->nrows;
		served = 2;
		x->joins_eliminated++;
	} else if (tl->nrows + tr->nrows >= (1u << 21)) {
		op_stats_begin(x, kj[0], tl->cols[kj[0]->col_idx].d_data, kj[1], tr->cols[kj[1]->col_idx].d_data);
		krc = mdb_dev_join_keys_ordered(x->dev, tl->cols[kj[0]->col_idx].d_data, tl->cols[kj[0]->col_idx].d_nullbits, tl->nrows,
						 tr->cols[kj[1]->col_idx].d_data, tr->cols[kj[1]->col_idx].d_nullbits, tr->nrows, &st->keys_ordered,
						 &st->keys_ordered_rows, &served);
		op_stats_end(x);
	}
	if (krc)
		return dev_fail(x, "join of two key columns");
	st->keys_only = served != 0;
	/* (served == 2: the joined rows' key column IS the left table's key column - held by the result, never freed here) */
	if (st->keys_ordered && served != 2 && track(x, st->keys_ordered))
		return -MIDORIDB_NOMEM;
	return MIDORIDB_OK;
}

/* the single-key fused plan's operands and what its operator calls found so far */
struct fused_ops {
	const void *lv, *rv;		/* the first two tables' key columns (their rows that pass their pushed conjuncts) */
	const uint64_t *ln, *rn;
	uint64_t nl_rows, nr_rows;
	uint64_t G, J;			/* groups and joined rows so far */
	bool multi_done;		/* one call took every table of the chain: nothing is left to chain */
};

/* the right-hand operands of a call that takes every table of the chain at once: the second table's key column, then the further tables' */
static int fused_right_tables(struct exec *x, const struct select_stmt *st, const struct fused_ops *o, const int64_t **rk, const uint64_t **rnb,
			      uint64_t *rrows)
{
	int rc;
	rk[0] = o->rv;
	rnb[0] = o->rn;
	rrows[0] = o->nr_rows;
	for (int t = 2; t < x->s->ntabs; t++) {
		const void *cv;
		if ((rc = fused_operand(x, t, st->fkeys[t], st->ws.push[t], st->ws.npush[t], &cv, &rnb[t - 1], &rrows[t - 1])))
			return rc;
		rk[t - 1] = cv;
	}
	return MIDORIDB_OK;
}

/* Sharded mode: the tables hold this rank's rows; both key columns are exchanged (RCCL all-to-all per table, include/mdb_dist.h) and this
 * rank keeps the groups whose key hashes to it.  Collective: every rank runs the same statement. */
static int fused_chain_sharded(struct exec *x, const struct select_stmt *st, struct fused_ops *o)
{
	struct mdb_select *s = x->s;
	struct mdb_dist *dist = x->cat->dist;
	int rc;
	if (s->ntabs > 2 && s->ntabs <= 4) {
		/* three or four tables on one key: ONE exchange - every table partitioned once with the same hash, the right tables' counts
		 * multiplied where the regions meet (mdb_dist_join_group_count_multi_alloc); when that form is not served (every rank learns
		 * so together) the chain of two-table calls runs */
		const int64_t *rk[3];
		const uint64_t *rnb[3];
		uint64_t rrows[3];
		if ((rc = fused_right_tables(x, st, o, rk, rnb, rrows)))
			return rc;
		const int mrc = mdb_dist_join_group_count_multi_alloc(dist, o->lv, o->ln, o->nl_rows, s->ntabs - 1, rk, rnb, rrows, &x->d_fused_key, &x->d_count,
								      &o->G, &o->J);
		if (mrc < 0)
			return dist_fail(x, "sharded join + group count");
		if (mrc == 0) {
			o->multi_done = true;
			return track(x, x->d_fused_key) || track(x, x->d_count) ? -MIDORIDB_NOMEM : MIDORIDB_OK;
		}
	}
	/* (more tables follow on the same key: the groups must lie where their key hashes to, for the tables sent after them) */
	if (mdb_dist_join_group_count_alloc(dist, o->lv, o->ln, o->nl_rows, o->rv, o->rn, o->nr_rows, s->ntabs > 2 ? MDB_DIST_PLACE_BY_KEY_HASH : 0u,
					    &x->d_fused_key, &x->d_count, NULL, &o->G, &o->J))
		return dist_fail(x, "sharded join + group count");
	return track(x, x->d_fused_key) || track(x, x->d_count) ? -MIDORIDB_NOMEM : MIDORIDB_OK;
}

/* One GPU: the output columns sized by `cap`, one operator call over the first two tables - or, three or four tables, over all of them */
static int fused_chain_single(struct exec *x, const struct select_stmt *st, struct fused_ops *o, uint64_t cap)
{
	struct mdb_select *s = x->s;
	/* (a bare COUNT(*) has no group order to keep; nor has a GROUP BY when the database says so) */
	const uint32_t flags = ((st->only_count || x->cat->groups_any_order) ? 0u : MDB_ORDER_FIRST) | MDB_KEYS_MAY_ALIAS;
	int rc;
	x->d_fused_key = dalloc(x, cap * 8);
	x->d_count = dalloc(x, cap * 8);
	if (!x->d_fused_key || !x->d_count)
		return dev_fail(x, "allocating group outputs");
	if (s->ntabs > 2 && s->ntabs <= 4) {
		/* A JOIN B ON a = b JOIN C ON a = c [JOIN D ...]: every table partitioned once, the right tables' counts multiplied
		 * in the leaf kernel, the groups ordered once (mdb_dev_join_group_count_multi; it chains by itself when the keys
		 * do not take the compact form) */
		const int64_t *rk[3];
		const uint64_t *rnb[3];
		uint64_t rrows[3];
		if ((rc = fused_right_tables(x, st, o, rk, rnb, rrows)))
			return rc;
		if (mdb_dev_join_group_count_multi(x->dev, o->lv, o->ln, o->nl_rows, s->ntabs - 1, rk, rnb, rrows, flags, x->d_fused_key, x->d_count, NULL, cap,
						   &o->G, &o->J))
			return dev_fail(x, "join + group count over several tables");
		o->multi_done = true;
	} else {
		if (st->fkeys[0]->type != MDB_CT_DOUBLE)
			op_stats_begin(x, st->fkeys[0], o->lv, st->fkeys[1], o->rv);
		const int frc = mdb_dev_join_group_count(x->dev, o->lv, o->ln, o->nl_rows, o->rv, o->rn, o->nr_rows, flags, x->d_fused_key, x->d_count, NULL, cap,
							  &o->G, &o->J);
		op_stats_end(x);
		if (frc)
			return dev_fail(x, "join + group count");
	}
	/* every left row turned out to be a group: the group keys ARE the left key column, in its order - the operator wrote none
	 * (MDB_KEYS_MAY_ALIAS) and the stream reads the column itself; a result kept on the device becomes one more holder of the
	 * table's buffer (0.8 GB less read and written at 10^8 rows) */
	struct mdb_dev_plan_info pi;
	if (mdb_dev_last_plan(x->dev, &pi) == 0 && pi.keys_are_left_column && o->G == o->nl_rows)
		x->d_fused_key = (int64_t *)(uintptr_t)o->lv;
	return MIDORIDB_OK;
}

/* one more table t on the same key: the group keys so far are joined with it, a group's COUNT(*) multiplied by its rows there */
static int fused_chain_step(struct exec *x, const struct select_stmt *st, int t, struct fused_ops *o)
{
	struct mdb_dist *dist = x->cat->dist;
	const uint64_t G = o->G;
	const void *cv;
	const uint64_t *cn;
	uint64_t nc_rows;
	int rc;
	if ((rc = fused_operand(x, t, st->fkeys[t], st->ws.push[t], st->ws.npush[t], &cv, &cn, &nc_rows)))
		return rc;
	int64_t *key2 = NULL, *cnt2 = NULL, *cnt3 = dalloc(x, (G ? G : 1) * 8);
	uint32_t *first2 = NULL;
	uint64_t G2 = 0, J2 = 0;
	if (dist) {
		/* the groups so far already live on the rank their key hashes to: only the new table travels */
		if (mdb_dist_join_group_count_alloc(dist, x->d_fused_key, NULL, G, cv, cn, nc_rows, MDB_DIST_LEFT_IN_PLACE, &key2, &cnt2, &first2, &G2, &J2))
			return dist_fail(x, "sharded join + group count");
		if (track(x, key2) || track(x, cnt2) || track(x, first2))
			return -MIDORIDB_NOMEM;
	} else {
		key2 = dalloc(x, G * 8);
		cnt2 = dalloc(x, G * 8);
		first2 = dalloc(x, G * 4);
	}
	if (!key2 || !cnt2 || !cnt3 || !first2)
		return dev_fail(x, "allocating group outputs");
	if ((!dist && mdb_dev_join_group_count(x->dev, x->d_fused_key, NULL, G, cv, cn, nc_rows, MDB_ORDER_FIRST, key2, cnt2, first2, G, &G2, &J2)) ||
	    mdb_dev_combine_counts(x->dev, x->d_count, NULL, first2, cnt2, G2, cnt3, NULL, &o->J))
		return dev_fail(x, "chained join + group count");
	x->d_fused_key = key2;
	x->d_count = cnt3;
	o->G = G2;
	return MIDORIDB_OK;
}

/* The north-star plan: join + GROUP BY key + COUNT(*) without materialising the join.  More than two tables on the same key chain the
 * operator: the group keys of (T0, T1) are joined with T2, and so on; a group's COUNT(*) is the product of the per-table multiplicities
 * (mdb_dev_combine_counts).  WHERE conjuncts that read one table filter that table before it enters the join. */
static int plan_fused_chain(struct exec *x, const struct select_stmt *st)
{
	struct mdb_select *s = x->s;
	struct mdb_catalog *cat = x->cat;
	const struct mdb_expr *const *fkeys = st->fkeys;
	struct fused_ops o;
	int rc;
	memset(&o, 0, sizeof(o));
	if ((rc = fused_operand(x, 0, fkeys[0], st->ws.push[0], st->ws.npush[0], &o.lv, &o.ln, &o.nl_rows)) ||
	    (rc = fused_operand(x, 1, fkeys[1], st->ws.push[1], st->ws.npush[1], &o.rv, &o.rn, &o.nr_rows)))
		return rc;
	uint64_t cap = o.nl_rows ? o.nl_rows : 1;
	/* a group of the join needs a key that both sides hold: no more groups than rows or key values of either column (catalog
	 * statistics) - the output columns are sized for that, and become the result's own without a copy when the bound is close */
	if (!cat->dist && fkeys[0]->type != MDB_CT_DOUBLE) {
		cap = op_groups_bound(x, fkeys[0], cap);
		cap = op_groups_bound(x, fkeys[1], cap < o.nr_rows ? cap : (o.nr_rows ? o.nr_rows : 1));
	}
	const bool text_keys = cat->dist && fkeys[0]->type == MDB_CT_VARCHAR;
	if (text_keys) {
		/* sharded mode, VARCHAR join keys: the ids of this process's dictionary mean nothing to the other ranks - the operator
		 * runs on the ranks' common ids (shard_ids) and its group keys are translated back where they arrive */
		const int64_t *cl = NULL, *cr = NULL;
		if ((rc = shard_ids(x, (const int64_t *)o.lv, o.nl_rows, true, false, &cl)) || (rc = shard_ids(x, (const int64_t *)o.rv, o.nr_rows, true, false, &cr)))
			return rc;
		o.lv = cl;
		o.rv = cr;
	}
	if (cat->dist && fkeys[0]->type != MDB_CT_DOUBLE && !text_keys && (rc = shard_promise_ranges(x, fkeys[0], fkeys[1])))
		return rc;
	if ((rc = cat->dist ? fused_chain_sharded(x, st, &o) : fused_chain_single(x, st, &o, cap)))
		return rc;
	for (int t = 2; t < s->ntabs && (o.G || cat->dist) && !o.multi_done; t++)
		if ((rc = fused_chain_step(x, st, t, &o)))
			return rc;
	if (!o.G)
		o.J = 0;
	if (cat->dist && st->only_count) {
		/* SELECT COUNT(*) over the sharded join: every rank reports the global number of joined rows */
		if (mdb_dist_allreduce_sum_u64(cat->dist, &o.J, 1))
			return dist_fail(x, NULL);
	}
	if (text_keys && o.G && !st->only_count) {	/* the group keys that arrived: common ids -> ids of this rank's dictionary */
		const int64_t *same = NULL;
		if ((rc = shard_ids(x, x->d_fused_key, o.G, false, true, &same)))
			return rc;
	}
	x->plan = STREAM_FUSED_CHAIN;
	x->n = st->only_count ? o.J : o.G;	/* COUNT(*) without GROUP BY = the stream length = the joined rows */
	x->joined_rows = o.J;
	return MIDORIDB_OK;
}

/* A two-table equi-join whose select list names nothing but the two key columns (BASELINE configs[3]: SELECT * over two key columns):
 * both sides hold the same value in every joined row, so no row has to be identified.  In the reference's order keys_only_ordered() has
 * answered already; with any order allowed (mdb_database_groups_any_order) the any-order join + GROUP BY pipeline counts every key's
 * partners and the key is written COUNT times (mdb_dev_join_keys).  The stream is the fused plan's: one key column, no row ids */
static int plan_keys_only(struct exec *x, const struct select_stmt *st)
{
	struct mdb_select *s = x->s;
	const struct mdb_expr *const *kj = st->kj;
	const struct mdb_column *cl = &s->tabs[kj[0]->tbl_idx].t->cols[kj[0]->col_idx], *cr = &s->tabs[kj[1]->tbl_idx].t->cols[kj[1]->col_idx];
	int64_t *jk = st->keys_ordered;
	uint64_t J = st->keys_ordered_rows;
	if (x->cat->groups_any_order) {
		op_stats_begin(x, kj[0], cl->d_data, kj[1], cr->d_data);
		const int krc = mdb_dev_join_keys(x->dev, cl->d_data, cl->d_nullbits, s->tabs[kj[0]->tbl_idx].t->nrows, cr->d_data, cr->d_nullbits,
						  s->tabs[kj[1]->tbl_idx].t->nrows, &jk, &J);
		op_stats_end(x);
		if (krc)
			return dev_fail(x, "join of two key columns");
	}
	if (jk && jk != st->keys_ordered && track(x, jk))
		return -MIDORIDB_NOMEM;
	x->d_fused_key = jk;
	x->plan = STREAM_JOIN_KEYS;
	x->n = J;
	x->joined_rows = J;
	return MIDORIDB_OK;
}

static bool filter_project_applies(const struct select_stmt *st, const struct mdb_select *s)
{
	return s->ntabs == 1 && s->where && st->split_ok && !st->ws.nresidual && st->ws.npush[0] && !s->ngroup && !st->rc.has_count && !st->has_agg && !st->has_win &&
	       !s->distinct && !s->norder && !s->having && !s->has_limit && s->tabs[0].t->nrows && st->rc.ncols && st->rc.ncols <= MDB_GATHER_MAX_COLS;
}

/* Scan + WHERE + projection of one table (BASELINE configs[0] shape): the predicate bitmap is turned straight into the compacted
 * result columns (mdb_dev_filter_project) - no selection vector, no gathers.  st->direct_vals / direct_nulls: the result columns, final */
static int plan_filter_project(struct exec *x, struct select_stmt *st)
{
	struct mdb_table *tb = x->s->tabs[0].t;
	const int ncols = st->rc.ncols;
	struct pred_prog p;
	struct mdb_project_col pc[MDB_GATHER_MAX_COLS];
	uint64_t m = 0;
	memset(&p, 0, sizeof(p));
	for (int i = 0; i < st->ws.npush[0]; i++)
		if (pred_compile(x, &p, st->ws.push[0][i]) || (i && pred_emit(&p, MDB_P_AND, 0, 0, 0, 0, 0))) {
			pred_compile_failed(x);
			return -MIDORIDB_ERROR;
		}
	st->direct_vals = calloc((size_t)ncols, sizeof(void *));
	st->direct_nulls = calloc((size_t)ncols, sizeof(uint64_t *));
	if (!st->direct_vals || !st->direct_nulls)
		return -MIDORIDB_NOMEM;
	for (int c = 0; c < ncols; c++) {
		struct mdb_column *col = &tb->cols[st->rc.col[st->rc.src[c]]];
		pc[c].values = col->d_data;
		pc[c].nullbits = col->d_nullbits;
		pc[c].out_values = &st->direct_vals[c];
		pc[c].out_nullbits = &st->direct_nulls[c];
	}
	if (mdb_dev_filter_project(x->dev, p.insn, p.n, p.cols, p.ncols, tb->nrows, pc, ncols, &m))
		return dev_fail(x, "scan + filter + projection");
	for (int c = 0; c < ncols; c++)
		if ((st->direct_vals[c] && track(x, st->direct_vals[c])) || (st->direct_nulls[c] && track(x, st->direct_nulls[c])))
			return -MIDORIDB_NOMEM;
	x->n = m;
	return MIDORIDB_OK;
}

/* ---- the general plan: scan, joins, WHERE, then GROUP BY in one of its forms */

static int general_scan_and_joins(struct exec *x, const struct select_stmt *st)
{
	struct mdb_select *s = x->s;
	const struct where_split *ws = &st->ws;
	int rc;
	x->n = s->tabs[0].t->nrows;	/* scan: identity stream over the first table */
	if (!st->split_ok) {
		for (int t = 1; t < s->ntabs; t++)
			if ((rc = join_next_table(x, t, NULL, 0)))
				return rc;
		return s->where ? stream_filter(x, s->ntabs, s->where) : MIDORIDB_OK;
	}
	/* WHERE conjuncts that read one table filter that table before it is joined; the others after the joins */
	const uint32_t *sel0;
	uint64_t m0;
	if ((rc = table_filter(x, 0, ws->push[0], ws->npush[0], &sel0, &m0)))
		return rc;
	if (sel0) {
		x->rid[0] = (uint32_t *)sel0;
		x->n = m0;
	}
	x->ws = ws;
	for (int t = 1; t < s->ntabs; t++)
		if ((rc = join_next_table(x, t, ws->push[t], ws->npush[t])))
			return rc;
	for (int i = 0; i < ws->nresidual; i++)
		if ((rc = stream_filter(x, s->ntabs, ws->residual[i])))
			return rc;
	return MIDORIDB_OK;
}

/* Sharded GROUP BY on one field, any order allowed and only the group key and COUNT(*) can be named (S4): no rows need to travel - every
 * rank's ONE partition pass over its key column, the first-level regions exchanged, counted where they land
 * (mdb_dist_group_count_keys_alloc).  Every rank must take the same way: they agree on "no NULL keys anywhere" first.  The decision is
 * taken from the STREAM's key column (its NULL bitmap as it is after joins and exchanges: a shadow table that arrived over the wire carries
 * bitmaps but no NULL counts), never from catalog counters.  0: grouped, 1: not this way (the row exchange answers), < 0: error */
static int sharded_group_keys(struct exec *x)
{
	struct mdb_select *s = x->s;
	struct mdb_dist *dist = x->cat->dist;
	const int64_t *kv;
	const uint64_t *kn;
	int64_t *gk = NULL, *gc = NULL;
	uint64_t Gk = 0;
	int rc;
	if ((rc = stream_column(x, s->group[0], &kv, &kn)))
		return rc;
	uint64_t ok = kn == NULL ? 1u : 0u;
	if (mdb_dist_allreduce_sum_u64(dist, &ok, 1))
		return dist_fail(x, NULL);
	if (ok != (uint64_t)mdb_dist_world(dist))
		return 1;
	if ((rc = shard_promise_ranges(x, s->group[0], s->group[0])))
		return rc;
	if (!x->promised)
		return 1;	/* (no range to promise - an empty column somewhere) */
	const int krc = mdb_dist_group_count_keys_alloc(dist, kv, NULL, x->n, &gk, &gc, &Gk);
	if (krc < 0)
		return dist_fail(x, "sharded group count");
	if (krc)
		return 1;
	if (track(x, gk) || track(x, gc))
		return -MIDORIDB_NOMEM;
	x->d_fused_key = gk;
	x->d_count = gc;
	x->plan = STREAM_GROUP_KEYS;
	x->n = Gk;
	return 0;
}

/* Sharded mode: a group's rows must meet on one rank - they do when the stream is partitioned by one of the group fields (a join key);
 * otherwise it is exchanged by the first one, NULL keys included (one group, :1477-1482) - unless the groups can be counted without
 * moving rows (*grouped: the stream is the groups already) */
static int general_place_groups(struct exec *x, const struct select_stmt *st, bool *grouped)
{
	struct mdb_select *s = x->s;
	bool placed = false;
	int rc;
	for (int g = 0; g < s->ngroup; g++)
		placed = placed || in_part(x, s->group[g]);
	if (!placed && x->cat->groups_any_order && s->ngroup == 1 && !stream_is_keys(x) && !s->select_all && !s->distinct && !st->has_agg &&
	    s->group[0]->kind == MDB_EX_FIELD && s->group[0]->type != MDB_CT_DOUBLE && s->group[0]->type != MDB_CT_VARCHAR) {
		if ((rc = sharded_group_keys(x)) < 0)
			return rc;
		*grouped = rc == 0;
		if (*grouped)
			return MIDORIDB_OK;
	}
	return placed ? MIDORIDB_OK : shard_stream(x, s->ntabs, s->group[0], MDB_DIST_KEEP_NULL_KEYS);
}

/* ... and so must equal rows under DISTINCT */
static int general_place_distinct(struct exec *x)
{
	struct mdb_select *s = x->s;
	bool placed = false;
	const struct mdb_expr *by = NULL;
	static __thread struct mdb_expr first_col;	/* (its address is kept in x->part[] beyond this call) */
	for (int i = 0; i < s->nsel; i++)
		if (s->sel[i]->kind == MDB_EX_FIELD) {
			placed = placed || in_part(x, s->sel[i]);
			by = by ? by : s->sel[i];
		}
	if (s->select_all) {
		placed = placed || x->npart > 0;
		if (!by && s->tabs[0].t->ncols) {
			memset(&first_col, 0, sizeof(first_col));
			first_col.kind = MDB_EX_FIELD;
			first_col.type = s->tabs[0].t->cols[0].type;
			by = &first_col;
		}
	}
	if (!placed && (s->ngroup || !by)) {
		snprintf(x->err, x->errlen, "execution phase: sharded mode: DISTINCT over an aggregate alone cannot be answered from one rank's groups\n");
		return -MIDORIDB_ERROR;
	}
	return placed ? MIDORIDB_OK : shard_stream(x, s->ntabs, by, MDB_DIST_KEEP_NULL_KEYS);
}

/* GROUP BY one field in any order (mdb_database_groups_any_order), an INTEGER-like key without NULLs: (key, COUNT) pairs without row ids
 * or an ordering sort - the stream becomes what the fused plan's is (S4: only the group key and COUNT(*) can be named from here on).
 * 0: grouped, 1: the operator does not serve these keys (nothing changed), < 0: error */
static int group_keys_any_order(struct exec *x, const int64_t *kv)
{
	int64_t *gk = dalloc(x, x->n * 8), *gc = dalloc(x, x->n * 8);
	uint64_t Gk = 0;
	if (!gk || !gc)
		return dev_fail(x, "allocating group outputs");
	op_stats_begin(x, x->s->group[0], kv, NULL, NULL);
	const int krc = mdb_dev_group_count_keys(x->dev, kv, NULL, x->n, gk, gc, x->n, &Gk);
	op_stats_end(x);
	if (krc < 0)
		return dev_fail(x, "group count (any order)");
	if (krc)
		return 1;
	x->d_fused_key = gk;
	x->d_count = gc;
	x->plan = STREAM_GROUP_KEYS;
	x->n = Gk;
	return 0;
}

static int general_group_one(struct exec *x, const struct select_stmt *st)
{
	struct mdb_select *s = x->s;
	const struct mdb_expr *f = s->group[0];
	const bool ranged = f->kind == MDB_EX_FIELD && f->type != MDB_CT_DOUBLE;	/* the catalog may know the key column's range */
	const int64_t *kv;
	const uint64_t *kn;
	uint32_t *first;
	uint64_t G = 0;
	int rc;
	if ((rc = stream_column(x, f, &kv, &kn)))
		return rc;
	if (x->cat->groups_any_order && !x->cat->dist && !stream_is_keys(x) && x->n && ranged && !s->select_all && !s->distinct &&
	    !st->has_agg /* (the (key, COUNT) pairs carry no rows to aggregate) */ && !x->may_be_absent[f->tbl_idx] &&
	    s->tabs[f->tbl_idx].t->cols[f->col_idx].null_count == 0 && (rc = group_keys_any_order(x, kv)) <= 0)
		return rc;
	/* (no more groups than key values in the column's range - catalog statistics -, plus the NULL group) */
	uint64_t gcap = x->n ? x->n : 1;
	if (ranged) {
		const uint64_t b = op_groups_bound(x, f, gcap);
		gcap = b + 1 < gcap ? b + 1 : gcap;
	}
	first = dalloc(x, gcap * 4);
	x->d_count = dalloc(x, gcap * 8);
	if (!first || !x->d_count)
		return dev_fail(x, "allocating group outputs");
	if (ranged)
		op_stats_begin(x, f, kv, NULL, NULL);
	const int grc = x->n ? mdb_dev_group_count(x->dev, kv, kn, x->n, MDB_ORDER_FIRST, first, x->d_count, gcap, &G) : 0;
	op_stats_end(x);
	if (grc)
		return dev_fail(x, "group count");
	/* the catalog knew that the column holds no value twice and the operator answered with the identity (group i = row i of the
	 * stream, COUNT 1): the stream stays what it is - no row-id vector to compose, no gather through one in the projection; a
	 * result kept on the device holds the table's columns */
	struct mdb_dev_plan_info pi;
	const bool identity = x->n && G == x->n && mdb_dev_last_plan(x->dev, &pi) == 0 && pi.group_form == 3;
	if (st->has_agg && G) {
		struct mdb_sort_key gk1;	/* (the key column as the GROUP BY operator read it: gathered already where the stream has row ids) */
		gk1.values = kv;
		gk1.nullbits = kn;
		gk1.rid = NULL;
		gk1.type = f->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
		gk1.desc = 0;
		if ((rc = stream_aggregate(x, &gk1, identity ? MDB_AGG_IDENTITY : 1, first, G)))
			return rc;
	}
	return identity ? MIDORIDB_OK : stream_select(x, s->ntabs, first, G);
}

/* several fields: groups = distinct combinations (the reference applies its single-field loop once per field,
 * executor_select.c:1537-1541, which is not a grouping by the combination: DESIGN.md 2) */
static int general_group_several(struct exec *x, const struct select_stmt *st)
{
	struct mdb_select *s = x->s;
	struct mdb_sort_key gk[MDB_SORT_MAX_KEYS];
	uint32_t *first;
	uint64_t G = 0;
	int rc;
	for (int g = 0; g < s->ngroup; g++) {
		bind_operand(x, s->group[g], &gk[g].values, &gk[g].nullbits, &gk[g].rid);
		gk[g].type = s->group[g]->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
		gk[g].desc = 0;
	}
	first = dalloc(x, (x->n ? x->n : 1) * 4);
	x->d_count = dalloc(x, (x->n ? x->n : 1) * 8);
	if (!first || !x->d_count)
		return dev_fail(x, "allocating group outputs");
	if (x->n && mdb_dev_group_count_multi(x->dev, gk, s->ngroup, x->n, first, x->d_count, x->n, &G))
		return dev_fail(x, "group count");
	if (st->has_agg && G && (rc = stream_aggregate(x, gk, s->ngroup, first, G)))
		return rc;
	int64_t *cnt = x->d_count;	/* stream_select must not re-map the fresh counts */
	x->d_count = NULL;
	rc = stream_select(x, s->ntabs, first, G);
	x->d_count = cnt;
	return rc;
}

static int plan_general(struct exec *x, const struct select_stmt *st)
{
	struct mdb_select *s = x->s;
	struct mdb_catalog *cat = x->cat;
	bool grouped = false;
	int rc;
	if (cat->dist && s->has_limit && s->limit_off > 0) {
		snprintf(x->err, x->errlen, "execution phase: sharded mode: LIMIT with an offset cannot be answered from one rank's rows\n");
		return -MIDORIDB_ERROR;
	}
	if ((rc = general_scan_and_joins(x, st)))
		return rc;
	if (cat->dist && s->ngroup && ((rc = general_place_groups(x, st, &grouped)) || grouped))
		return rc;
	if (cat->dist && s->distinct && (rc = general_place_distinct(x)))
		return rc;
	if (s->ngroup == 1)
		return general_group_one(x, st);
	if (s->ngroup > 1)
		return general_group_several(x, st);
	if (st->has_win)	/* (never beside GROUP BY or an aggregate: resolve_select) */
		return stream_windows(x);
	/* SUM / MIN / MAX / AVG without GROUP BY: the whole stream is one group (an empty stream: no row, as SELECT COUNT(*) answers it) */
	return st->has_agg && x->n ? stream_aggregate(x, NULL, 0, NULL, 1) : MIDORIDB_OK;
}

/* sharded mode, after the plan: what one rank's stream cannot answer alone */
static int sharded_finish(struct exec *x, const struct select_stmt *st)
{
	struct mdb_select *s = x->s;
	if (!x->cat->dist)
		return MIDORIDB_OK;
	if (x->plan != STREAM_FUSED_CHAIN && st->rc.has_count && !s->ngroup) {
		/* SELECT COUNT(*) [WHERE ...]: every rank reports the global count (the fused chain has summed its joined rows already) */
		uint64_t tot = x->n;
		if (mdb_dist_allreduce_sum_u64(x->cat->dist, &tot, 1))
			return dist_fail(x, NULL);
		x->n = tot;
	}
	if (x->plan == STREAM_FUSED_CHAIN && s->distinct) {
		bool key_selected = false;
		for (int i = 0; i < s->nsel; i++)
			key_selected = key_selected || s->sel[i]->kind == MDB_EX_FIELD;
		if (!key_selected) {
			snprintf(x->err, x->errlen, "execution phase: sharded mode: DISTINCT over an aggregate alone cannot be answered from one rank's groups\n");
			return -MIDORIDB_ERROR;
		}
	}
	return MIDORIDB_OK;
}

/* The result columns a RESOLVED statement will deliver, without running it and without a device: their number, and result column c's name
 * and column type - what a compound checks its arms by before any of them runs.  select_signature_free() whatever is returned. */
int select_signature(struct mdb_select *s, struct select_signature *sig, char *err, size_t errlen)
{
	struct exec x;
	struct result_cols rc;
	int r;

	memset(&x, 0, sizeof(x));
	memset(&rc, 0, sizeof(rc));
	memset(sig, 0, sizeof(*sig));
	x.s = s;
	x.err = err;
	x.errlen = errlen;
	if (!(r = result_cols_build(&x, &rc))) {
		sig->ncols = rc.ncols;
		sig->name = calloc((size_t)(rc.ncols ? rc.ncols : 1), sizeof(*sig->name));
		sig->type = calloc((size_t)(rc.ncols ? rc.ncols : 1), sizeof(int));
		sig->at = calloc((size_t)(rc.ncols ? rc.ncols : 1), sizeof(int));
		if (!sig->name || !sig->type || !sig->at)
			r = -MIDORIDB_NOMEM;
		for (int c = 0; !r && c < rc.ncols; c++) {
			int before = 0;		/* (the columns whose items stand in front of this one's: no two share a place) */
			result_column_name(&x, &rc, c, sig->name[c]);
			sig->type[c] = result_column_type(&x, &rc, c);
			for (int d = 0; d < rc.ncols; d++)
				before += result_column_list_place(&x, &rc, d) < result_column_list_place(&x, &rc, c);
			sig->at[before] = c;
		}
	}
	if (r == -MIDORIDB_NOMEM)
		ERR("out of memory\n");
	result_cols_free(&rc);
	return r;
}

void select_signature_free(struct select_signature *sig)
{
	free(sig->name);
	free(sig->type);
	free(sig->at);
	memset(sig, 0, sizeof(*sig));
}

int mdb_exec_select(struct mdb_catalog *cat, struct mdb_select *s, struct mdb_result **out, char *err, size_t errlen)
{
	return s->nset ? exec_setop(cat, s, out, err, errlen) : exec_select_one(cat, s, out, err, errlen);
}

/* one SELECT: a whole statement, a subquery, or an arm of a compound */
int exec_select_one(struct mdb_catalog *cat, struct mdb_select *s, struct mdb_result **out, char *err, size_t errlen)
{
	stmt_dict = &cat->dict;
	struct exec x;
	struct select_stmt st;
	struct mdb_result *res = NULL;
	int rc;

	*out = NULL;
	memset(&x, 0, sizeof(x));
	memset(&st, 0, sizeof(st));
	for (int t = 0; t < MDB_MAX_TABS; t++)
		x.same_col[t] = -1;
	if (!s->resolved && (rc = resolve_select(cat, s, err, errlen)))
		return rc;
	if ((rc = mdb_catalog_device(cat, err, errlen)))
		return rc;
	for (int t = 0; t < s->ntabs; t++)
		if ((rc = mdb_table_sync_device(cat, s->tabs[t].t, err, errlen)))
			return rc;
	x.cat = cat;
	x.dev = cat->dev;
	x.s = s;
	x.err = err;
	x.errlen = errlen;
	for (int t = 1; t < s->ntabs; t++)
		x.has_outer = x.has_outer || s->join_type[t] != 1;
	mark_needed_all(&x);	/* (which columns the statement reads: the sharded exchange and the join that carries payload cells ask) */
	/* (the subqueries are part of what the statement costs: their time counts in exec_ms, beside the pipeline's own from t0 on) */
	const double sub_t0 = now_ms();
	double sub_ms = 0.0, t0 = 0.0;
	if ((rc = subqueries_eval(cat, s->where, err, errlen)) || (rc = subqueries_eval(cat, s->having, err, errlen)))
		goto out;
	if ((s->where && expr_has_subquery(s->where)) || (s->having && expr_has_subquery(s->having)))
		sub_ms = now_ms() - sub_t0;
	if ((rc = result_cols_build(&x, &st.rc)))
		goto out;
	st.has_agg = x.nagg > 0;
	st.has_win = x.nwin > 0;

	t0 = now_ms();
	select_shape(&x, &st);
	if ((rc = keys_only_ordered(&x, &st)))
		goto out;
	/* the plan that produces the stream: the first that applies (composite_fused_plan: 1 = it does not) */
	if (st.fused_chain)
		rc = plan_fused_chain(&x, &st);
	else if (!st.keys_only && st.split_ok && !st.has_agg && !st.has_win && (rc = composite_fused_plan(&x, &st.ws, st.only_count)) <= 0)
		;
	else if (st.keys_only)
		rc = plan_keys_only(&x, &st);
	else if (filter_project_applies(&st, s))
		rc = plan_filter_project(&x, &st);
	else
		rc = plan_general(&x, &st);
	if (rc)
		goto out;
	if ((rc = sharded_finish(&x, &st)))
		goto out;
	/* ---- HAVING -> DISTINCT -> ORDER BY -> LIMIT (SQL order of evaluation; extension) */
	if ((rc = select_tail(&x, st.rc.has_count || st.has_agg)))
		goto out;
	/* ---- projection + COUNT-only handling */
	res = calloc(1, sizeof(*res));
	if (!res) {
		rc = -MIDORIDB_NOMEM;
		goto out;
	}
	if ((rc = project_result(&x, &st, res)))
		goto out;
	res->dict = &cat->dict;
	mdb_result_legacy_header(res);		/* the reference's struct table in front of the columnar result (include/mdb_legacy.h) ... */
	mdb_result_legacy_rows(res);		/* ... and, for a small result whose columns are on the host, its rows as datablocks */
	res->exec_ms = now_ms() - t0 + sub_ms;
	res->joined_rows = x.joined_rows;
	*out = res;
	res = NULL;
	rc = MIDORIDB_OK;
out:
	/* (the statement's counters reach the catalog on error paths too) */
	cat->joins_eliminated += (uint64_t)x.joins_eliminated;
	cat->composite_joins += (uint64_t)x.composite_joins;
	cat->composite_fused += (uint64_t)x.composite_fused;
	cat->aggregate_calls[0] += (uint64_t)x.agg_calls[0];
	cat->aggregate_calls[1] += (uint64_t)x.agg_calls[1];
	cat->count_distinct_calls[0] += (uint64_t)x.cd_calls[0];
	cat->count_distinct_calls[1] += (uint64_t)x.cd_calls[1];
	cat->window_calls += (uint64_t)x.win_calls;
	shard_cleanup(&x);
	subqueries_release(cat, s->where);
	subqueries_release(cat, s->having);
	free_all(&x);
	mdb_result_free(res);
	result_cols_free(&st.rc);
	free(st.direct_vals);
	free(st.direct_nulls);
	return rc;
}

