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
 * LIMIT (select_tail) - and, at the end of the file, DELETE and UPDATE on the device mirror.
 *
 * Early materialisation is replaced by late materialisation: a tuple stream is a set of uint32
 * row-id vectors (one per FROM table; NULL = identity), so joins / filters / grouping move 4-byte
 * ids and only the selected columns are gathered once at the end.
 *
 * The plan normalisation the reference does in its optimiser (optimiser_select.c:114-238: NAME ->
 * fully qualified FIELDNAME, alias -> table name, SELECT * expansion) and the checks of its
 * semantic phase that guard the executor (semantic_select.c: unknown table/column, duplicate
 * column names across FROM tables S1, operand types S2, GROUP BY rule S4) happen in
 * resolve_select() below.
 */
#include "mdb_exec_internal.h"

/* ------------------------------------------------------------------ device-side execution state */



int dev_fail(struct exec *x, const char *what)
{
	snprintf(x->err, x->errlen, "execution phase: %s: %s\n", what, mdb_dev_last_error(x->dev));
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
	if (x->fused) {
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

/* The join of table t when EVERY row of the stream finds exactly one partner in it (a foreign key to a primary key) and the statement
 * reads at most two other columns of t, neither with NULLs: mdb_dev_join_payload carries those cells through t's one partition level
 * and delivers them in stream order - no partner row ids, no compaction, no random gather in the projection (BASELINE configs[1]).
 * Table t is then read through a SHADOW (like a table that arrived over the wire in sharded mode): its key column is the stream's own
 * key column, its payload columns are the carried cells, its row-id vector the identity.  0 = done, 1 = not such a join (nothing
 * changed: the pairs path answers), < 0 = error. */
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

/* Table t after a join that carried its payload cells to the stream's rows: read through a SHADOW whose key column is the stream's own key
 * column, whose payload columns pc[0 .. np) are the carried cells out[], whose row-id vector is the identity */
static int payload_shadow(struct exec *x, int t, int key_col, const int64_t *vl, const int *pc, int np, void *const *out)
{
	struct mdb_select *s = x->s;
	const struct mdb_table *rt = s->tabs[t].t;
	struct mdb_table *sh = calloc(1, sizeof(*sh));
	if (!sh)
		return -MIDORIDB_NOMEM;
	memcpy(sh->name, rt->name, sizeof(sh->name));
	sh->ncols = rt->ncols;
	for (int c = 0; c < rt->ncols; c++) {
		memcpy(sh->cols[c].name, rt->cols[c].name, sizeof(sh->cols[c].name));
		sh->cols[c].type = rt->cols[c].type;
		sh->cols[c].precision = rt->cols[c].precision;
		sh->cols[c].not_null = rt->cols[c].not_null;
	}
	sh->cols[key_col].d_data = (void *)vl;	/* (in every joined tuple the key of t IS the stream's key; a NULL key joined nothing) */
	for (int i = 0; i < np; i++)
		sh->cols[pc[i]].d_data = out[i];
	sh->nrows = sh->dev_rows = x->n;
	sh->dev_cap = x->n;
	sh->device_only = true;
	x->orig_tab[t] = s->tabs[t].t;
	x->shadow[t] = sh;
	s->tabs[t].t = sh;
	x->rid[t] = NULL;
	x->joined_rows = x->n;
	return 0;
}

/* the payload columns of table t a join would have to carry: the columns the statement reads, the key column apart - at most two, none
 * with NULLs, all on the device; -1 when the table does not qualify */
static int payload_columns(struct exec *x, int t, int key_col, int *pc)
{
	const struct mdb_table *rt = x->s->tabs[t].t;
	int np = 0;
	for (int c = 0; c < rt->ncols; c++) {
		if (!x->need[t][c] || c == key_col)
			continue;
		if (np == 2 || rt->cols[c].d_nullbits || !rt->cols[c].d_data)
			return -1;
		pc[np++] = c;
	}
	return np;
}

/* Join elimination (round 6): table t joined on `stream key = its own column kr`, when the CATALOG says that every row of the
 * stream finds exactly one partner in it - kr holds no value twice (MDB_COL_DISTINCT: measured at ingest, followed through appends, looked
 * at again after UPDATE / DELETE), no NULL, and as many rows as its range has values: EVERY value of [min, max]; the stream's key column
 * has no NULL and its range lies inside - and the statement reads nothing of t but that key: the joined rows ARE the stream's rows, t's key
 * column in them IS the stream's key column.  The reference runs its nested loop over B for every row of A
 * (/root/reference/src/engine/executor_select.c:1076-1149) to find the same; here the table is not touched at all.  The statistics are the
 * store's own invariants (ranges are never narrower than the data, the distinct flag is never set on a column that holds a value twice):
 * a range that went stale wider only makes the rule not apply.  MDB_JOIN_ELIMINATION=0: never. */
static bool join_is_total_by_catalog(struct exec *x, const struct mdb_expr *kl, const struct mdb_expr *kr)
{
	if (x->cat->dist || mdb_knob_off("MDB_JOIN_ELIMINATION") || !kl || !kr || kl->kind != MDB_EX_FIELD || kr->kind != MDB_EX_FIELD || kl->tbl_idx < 0 || kr->tbl_idx < 0 ||
	    kl->type == MDB_CT_DOUBLE || kr->type == MDB_CT_DOUBLE || kl->type != kr->type || x->orig_tab[kr->tbl_idx])
		return false;
	/* (the stream's key may be named through a table that was itself joined this way: its key column is an earlier table's) */
	int lt = kl->tbl_idx, lc = kl->col_idx;
	for (int hops = 0; x->orig_tab[lt] && hops < MDB_MAX_TABS; hops++) {
		if (x->same_col[lt] != lc)
			return false;
		const int nt = x->same_as_tbl[lt];
		lc = x->same_as_col[lt];
		lt = nt;
	}
	if (x->orig_tab[lt])
		return false;
	struct mdb_table *tl = x->s->tabs[lt].t, *tr = x->s->tabs[kr->tbl_idx].t;
	struct mdb_column *cl = &tl->cols[lc], *cr = &tr->cols[kr->col_idx];
	const uint64_t r_rows = tr->device_only ? tr->dev_rows : tr->nrows;
	int64_t llo, lhi, rlo, rhi;
	if (!r_rows || cl->null_count || cr->null_count || mdb_col_range(x->cat, tl, cl, &llo, &lhi) != MIDORIDB_OK ||
	    mdb_col_range(x->cat, tr, cr, &rlo, &rhi) != MIDORIDB_OK || rlo > rhi)
		return false;
	if ((uint64_t)rhi - (uint64_t)rlo + 1 != r_rows || (llo <= lhi && (llo < rlo || lhi > rhi)))
		return false;
	return mdb_col_distinct(x->cat, tr, cr);	/* (last: it may scan the column) */
}

/* ... and nothing but the key column of table t is read by the statement */
static bool only_key_needed(const struct exec *x, int t, int key_col)
{
	const struct mdb_table *rt = x->s->tabs[t].t;
	for (int c = 0; c < rt->ncols; c++)
		if (x->need[t][c] && c != key_col)
			return false;
	return true;
}

/* SEVERAL tables joined to the stream on ONE key, each a primary-key table that every row of the stream finds exactly one partner in
 * (SELECT * FROM A JOIN B ON A.k = B.k JOIN C ON A.k = C.k - BASELINE configs[4]'s join-only form; the reference joins B, then C against the
 * materialised A x B: executor_select.c:1076-1232): table t and the tables behind it whose whole ON clause is `earlier key = own column`,
 * that have no WHERE conjunct of their own and qualify like table t does, are handed to mdb_dev_join_payload_multi in one call - the
 * stream's key column is sorted once for all of them - with the catalog's key ranges as the window.  0 = done for table t and
 * x->joined_ahead[] tables (join_next_table returns at once for those), 1 = not such a statement or not such a join (nothing changed:
 * table t is joined on its own), < 0 = error. */
static int join_with_payload_multi(struct exec *x, int t, const struct mdb_expr *kl, const struct mdb_expr *kr, const int64_t *vl, const uint64_t *nl,
				   const void *vr, const uint64_t *nr, uint64_t r_rows)
{
	struct mdb_select *s = x->s;
	struct mdb_dev_payload_right right[4];
	const struct mdb_expr *keys[4];
	int tabs[4], pcs[4][2], nt = 0, streams = 0;
	int64_t lo, hi;
	char rowjoin[2];	/* ("2": the row-order form for tables of any size - tests) */
	mdb_knob_str("MDB_ROWJOIN", rowjoin, sizeof(rowjoin));
	if ((x->n < ((uint64_t)1 << 24) && rowjoin[0] != '2') || nl || nr || x->orig_tab[t] || kl->kind != MDB_EX_FIELD || kl->tbl_idx < 0 || x->orig_tab[kl->tbl_idx])
		return 1;
	{
		struct mdb_table *lt = s->tabs[kl->tbl_idx].t;
		if (mdb_col_range(x->cat, lt, &lt->cols[kl->col_idx], &lo, &hi) != MIDORIDB_OK || lo > hi)
			return 1;
	}
	memset(right, 0, sizeof(right));
	for (int t2 = t; t2 < s->ntabs && nt < 4; t2++) {
		const struct mdb_expr *k2 = kr;
		if (t2 > t) {
			const struct mdb_expr *on = s->on[t2], *mine = NULL, *other = NULL;
			if (s->join_type[t2] != 1)
				break;
			if (!on || on->kind != MDB_EX_CMP || on->op != MDB_CMP_EQ || on->kids[0]->kind != MDB_EX_FIELD || on->kids[1]->kind != MDB_EX_FIELD)
				break;
			if (on->kids[0]->tbl_idx == t2 && on->kids[1]->tbl_idx < t2) {
				mine = on->kids[0];
				other = on->kids[1];
			} else if (on->kids[1]->tbl_idx == t2 && on->kids[0]->tbl_idx < t2) {
				mine = on->kids[1];
				other = on->kids[0];
			} else {
				break;
			}
			bool same_key = field_eq(other, kl);	/* (the stream's key, or the key column of a table this call joins on it) */
			for (int i = 0; i < nt && !same_key; i++)
				same_key = field_eq(other, keys[i]);
			if (!same_key || mine->type == MDB_CT_DOUBLE || x->orig_tab[t2] || (x->ws ? x->ws->npush[t2] != 0 : 0))
				break;
			k2 = mine;
		}
		struct mdb_table *rt = s->tabs[t2].t;
		const int np = payload_columns(x, t2, k2->col_idx, pcs[nt]);
		int64_t rlo, rhi;
		if (np < 1 || streams + np > 4 || !rt->nrows || mdb_col_range(x->cat, rt, &rt->cols[k2->col_idx], &rlo, &rhi) != MIDORIDB_OK || rlo > rhi)
			break;
		const void *kv = vr;
		const uint64_t *kn = nr;
		if (t2 > t && table_column(x, t2, k2, NULL, rt->nrows, &kv, &kn))
			break;
		if (kn)
			break;
		lo = rlo < lo ? rlo : lo;
		hi = rhi > hi ? rhi : hi;
		right[nt].keys = (const int64_t *)kv;
		right[nt].rows = t2 > t ? rt->nrows : r_rows;
		right[nt].npay = np;
		for (int i = 0; i < np; i++)
			right[nt].pay_in[i] = rt->cols[pcs[nt][i]].d_data;
		keys[nt] = k2;
		tabs[nt] = t2;
		streams += np;
		nt++;
	}
	if (nt < 2 || (uint64_t)hi - (uint64_t)lo >= ((uint64_t)1 << 27))
		return 1;
	for (int i = 0; i < nt; i++)
		for (int c = 0; c < right[i].npay; c++)
			if (!(right[i].out[c] = dalloc(x, x->n * 8)))
				return dev_fail(x, "allocating carried columns");
	const int rc = mdb_dev_join_payload_multi(x->dev, vl, NULL, x->n, right, nt, lo, hi);
	if (rc == 1)
		return 1;
	if (rc)
		return dev_fail(x, "join with payload (several tables on one key)");
	for (int i = 0; i < nt; i++) {
		const int prc = payload_shadow(x, tabs[i], keys[i]->col_idx, vl, pcs[i], right[i].npay, right[i].out);
		if (prc)
			return prc;
		if (i) {
			x->joined_ahead[tabs[i]] = true;
			x->same_col[tabs[i]] = keys[i]->col_idx;
			x->same_as_tbl[tabs[i]] = kl->tbl_idx;
			x->same_as_col[tabs[i]] = kl->col_idx;
		}
	}
	return 0;
}

int join_with_payload(struct exec *x, int t, const struct mdb_expr *kr, const int64_t *vl, const uint64_t *nl, const void *vr,
			     const uint64_t *nr, uint64_t r_rows)
{
	struct mdb_select *s = x->s;
	const struct mdb_table *rt = s->tabs[t].t;
	int pc[2], np = 0;
	for (int c = 0; c < rt->ncols; c++) {
		if (!x->need[t][c] || c == kr->col_idx)
			continue;
		if (np == 2 || rt->cols[c].d_nullbits || !rt->cols[c].d_data)
			return 1;
		pc[np++] = c;
	}
	if (!np || !x->n || x->orig_tab[t])
		return 1;
	const void *pin[2] = { NULL, NULL };
	void *out[2] = { NULL, NULL };
	for (int i = 0; i < np; i++) {
		pin[i] = rt->cols[pc[i]].d_data;
		out[i] = dalloc(x, x->n * 8);
		if (!out[i])
			return dev_fail(x, "allocating carried columns");
	}
	const int rc = mdb_dev_join_payload(x->dev, vl, nl, x->n, (const int64_t *)vr, nr, r_rows, pin, np, out);
	if (rc == 1)
		return 1;
	if (rc)
		return dev_fail(x, "join with payload");
	return payload_shadow(x, t, kr->col_idx, vl, pc, np, out);
}

/* ------------------------------------------------------------------ composite join keys
 *
 * ON A.x = B.x AND A.y = B.y [AND ...]: the reference evaluates the whole ON expression per pair (executor_select.c:1128).  Joining on the
 * first equality and filtering the pairs by the others materialises every pair of the FIRST column - 8 values in x and 5000 in y over two
 * tables of 40 000 rows are 2 x 10^8 pairs where the conjunction has 4 x 10^4 - so the equalities whose columns' value ranges fit 63 bits
 * together are packed into one key per row (mdb_dev_join_key_layout / mdb_dev_join_key_pack, mdb_dev.h) and the pair operator joins on all
 * of them at once.  composite_join_plan() decides, composite_join_pack() packs both sides; join_next_table and outer_join_next_table use
 * both.  The rule:
 *   - the conjuncts `earlier-table column = table-t column`, both sides non-DOUBLE (DOUBLE keeps its IEEE `==`: double_join_keys, or a
 *     residual), at least two of them;
 *   - not in sharded mode (the shuffle places rows by the first key), not with MDB_COMPOSITE_JOIN=0;
 *   - not when table t's column of the first such conjunct is measured distinct: no row of the stream then has more than one partner on
 *     that column alone, nothing can explode, and the one-key plans (with their unique-key forms) are kept;
 *   - at least two columns fit (a column that does not fit stays a residual, later ones may still be taken).
 * Ranges are the catalog's (a base column's range is a superset for a stream or a filtered table: the pack tests every row against its
 * field, nothing is assumed), measured with mdb_dev_key_range for column types the catalog keeps none for (VARCHAR ids).
 * Rows and their order are the same as without: the pairs come out (left position, right position)-ordered either way, and a residual
 * filter keeps that order. */
struct composite_key {
	struct mdb_join_key_layout lay;
	const struct mdb_expr *kl[MDB_JOIN_KEY_MAX_COLS], *kr[MDB_JOIN_KEY_MAX_COLS];	/* the taken conjuncts' sides, layout order */
	uint32_t mask;			/* bit i: conjunct i of the ON clause is answered by the packed key */
	bool empty;			/* the layout says that nothing can match: nothing was packed, there are no pairs */
	const int64_t *vl, *vr;		/* the packed key columns: the stream's, table t's (its rows rsel) */
	const uint64_t *nl, *nr;	/* their NULL bits; NULL: every row has a key */
	struct mdb_dev_col_stats st[2];	/* their own statistics for mdb_dev_call_stats: the operator takes no key sample */
};

static int composite_key_range(struct exec *x, struct mdb_table *tb, struct mdb_column *col, struct mdb_dev_col_stats *st)
{
	int rc = mdb_col_range(x->cat, tb, col, &st->min, &st->max);
	if (rc == 1) {	/* (no catalog range for this type) */
		const uint64_t rows = tb->device_only ? tb->dev_rows : tb->nrows;
		st->min = 0;
		st->max = -1;
		if (rows && mdb_dev_key_range(x->dev, col->d_data, col->d_nullbits, rows, &st->min, &st->max))
			return dev_fail(x, "measuring a key column's range");
		rc = MIDORIDB_OK;
	}
	return rc ? dev_fail(x, "reading a key column's range") : MIDORIDB_OK;
}

/* 0: the join of table t runs on a composite key (ck->lay, ck->mask, ck->kl / kr filled), 1: it does not, < 0: error */
static int composite_join_plan(struct exec *x, int t, struct mdb_expr *const *conj, int nconj, struct composite_key *ck)
{
	struct mdb_select *s = x->s;
	struct mdb_table *rt = s->tabs[t].t;
	const struct mdb_expr *ql[32], *qr[32];
	struct mdb_dev_col_stats sl[32], sr[32];
	int qi[32], q = 0;
	memset(ck, 0, sizeof(*ck));
	if (nconj < 2 || nconj > 32 || x->cat->dist || !x->n || !rt->nrows || x->orig_tab[t] || mdb_knob_off("MDB_COMPOSITE_JOIN"))
		return 1;
	for (int i = 0; i < nconj; i++) {
		const struct mdb_expr *c = conj[i];
		if (c->kind != MDB_EX_CMP || c->op != MDB_CMP_EQ || c->kids[0]->kind != MDB_EX_FIELD || c->kids[1]->kind != MDB_EX_FIELD)
			continue;
		const struct mdb_expr *a = c->kids[0], *b = c->kids[1];
		if (!(a->tbl_idx >= 0 && a->tbl_idx < t && b->tbl_idx == t)) {
			const struct mdb_expr *sw = a;
			a = b;
			b = sw;
		}
		if (!(a->tbl_idx >= 0 && a->tbl_idx < t && b->tbl_idx == t) || a->type == MDB_CT_DOUBLE || b->type == MDB_CT_DOUBLE)
			continue;
		if (!s->tabs[a->tbl_idx].t->cols[a->col_idx].d_data || !rt->cols[b->col_idx].d_data)
			return 1;
		ql[q] = a;
		qr[q] = b;
		qi[q++] = i;
	}
	if (q < 2 || mdb_col_distinct(x->cat, rt, &rt->cols[qr[0]->col_idx]))
		return 1;
	memset(sl, 0, sizeof(sl));
	memset(sr, 0, sizeof(sr));
	for (int i = 0; i < q; i++) {
		struct mdb_table *lt = s->tabs[ql[i]->tbl_idx].t;
		int rc;
		if ((rc = composite_key_range(x, lt, &lt->cols[ql[i]->col_idx], &sl[i])) || (rc = composite_key_range(x, rt, &rt->cols[qr[i]->col_idx], &sr[i])))
			return rc;
	}
	if (mdb_dev_join_key_layout(sl, sr, q, &ck->lay))
		return 1;
	if (!ck->lay.empty && ck->lay.ntaken < 2)
		return 1;
	ck->empty = ck->lay.empty != 0;
	for (uint32_t c = 0; c < ck->lay.ntaken; c++) {
		ck->kl[c] = ql[ck->lay.taken[c]];
		ck->kr[c] = qr[ck->lay.taken[c]];
		ck->mask |= 1u << qi[ck->lay.taken[c]];
	}
	return 0;
}

/* ... and the two packed key columns: the stream's rows through their row-id vectors (no gather per key column; a tuple without a row of
 * the table - MDB_NO_ROW - gets no key), table t's rows rsel[0 .. r_rows) (NULL: all).  An empty layout packs nothing.
 * left_table (the fused plan, whose left side is no stream yet): the left side is the left table's rows lsel[0 .. l_rows) (NULL: all),
 * read through that selection vector the same way. */
static int composite_pack_sides(struct exec *x, struct composite_key *ck, bool left_table, const uint32_t *lsel, uint64_t l_rows, const uint32_t *rsel,
				uint64_t r_rows)
{
	struct mdb_select *s = x->s;
	const uint64_t rows[2] = { left_table ? l_rows : x->n, r_rows };
	if (ck->empty)
		return MIDORIDB_OK;
	for (int side = 0; side < 2; side++) {
		struct mdb_join_key_col cols[MDB_JOIN_KEY_MAX_COLS];
		const uint64_t n = rows[side];
		uint64_t nulls = 0, top = 0;
		for (uint32_t c = 0; c < ck->lay.ntaken; c++) {
			const struct mdb_expr *f = side ? ck->kr[c] : ck->kl[c];
			const struct mdb_column *col = &s->tabs[f->tbl_idx].t->cols[f->col_idx];
			cols[c].values = col->d_data;
			cols[c].nullbits = col->d_nullbits;
			cols[c].rid = side ? rsel : left_table ? lsel : x->rid[f->tbl_idx];
			top |= ck->lay.span[c] << ck->lay.shift[c];
		}
		int64_t *key = dalloc(x, (n ? n : 1) * 8);
		uint64_t *nb = dalloc(x, ((n + 63) / 64 + 1) * 8);
		if (!key || !nb)
			return dev_fail(x, "allocating a composite key column");
		if (mdb_dev_join_key_pack(x->dev, &ck->lay, cols, n, key, nb, &nulls))
			return dev_fail(x, "packing a composite join key");
		ck->st[side].min = 0;
		ck->st[side].max = (int64_t)top;	/* (below 2^63: the fields do not overlap) */
		ck->st[side].rows = n;
		ck->st[side].nulls = nulls;
		if (side) {
			ck->vr = key;
			ck->nr = nulls ? nb : NULL;
		} else {
			ck->vl = key;
			ck->nl = nulls ? nb : NULL;
		}
	}
	return MIDORIDB_OK;
}

static int composite_join_pack(struct exec *x, int t, struct composite_key *ck, const uint32_t *rsel, uint64_t r_rows)
{
	(void)t;
	x->composite_joins++;
	return composite_pack_sides(x, ck, false, NULL, 0, rsel, r_rows);
}

/* The fused join + GROUP BY + COUNT(*) operator on a packed composite key:
 *     SELECT A.x, A.y, COUNT(*) FROM A JOIN B ON A.x = B.x AND A.y = B.y GROUP BY A.x, A.y      and      SELECT COUNT(*) FROM the same join
 * without a pair, a gathered key column or a multi-field GROUP BY: both tables (their rows that pass the pushed WHERE conjuncts) are
 * packed, mdb_dev_join_group_count joins and groups the packed keys as it does one key column, mdb_dev_join_key_unpack turns the packed
 * group keys back into the key columns.  It applies to exactly two tables of an inner join, one GPU, when EVERY conjunct of the ON clause
 * is an equality the composite key takes (composite_join_plan's rule and layout, nothing left as a residual; the two sides of an equality of
 * one type), no WHERE conjunct reads both tables, and the statement groups by one side of every equality (any order, sides may mix) or is
 * count-only.  MDB_COMPOSITE_JOIN=0 switches it off with the other composite-key plans, MDB_COMPOSITE_FUSED=0 alone.
 * The groups come in the order of each key tuple's first left row that has a partner (MDB_ORDER_FIRST on the packed key: equal tuples are
 * equal keys) - what the pair join + multi-field GROUP BY returns.
 * 0: answered - the stream is (d_fused_keys[0 .. nfused), d_count), x->n set; 1: not such a statement, nothing changed; < 0: error. */
static int composite_fused_plan(struct exec *x, const struct where_split *ws, bool only_count)
{
	struct mdb_select *s = x->s;
	struct mdb_catalog *cat = x->cat;
	struct mdb_expr *conj[32];
	struct composite_key ck;
	int nconj = 0, rc;

	if (s->ntabs != 2 || x->has_outer || s->join_type[1] != 1 || cat->dist || !s->on[1] || ws->nresidual || s->select_all || mdb_knob_off("MDB_COMPOSITE_FUSED"))
		return 1;
	if (only_count ? s->ngroup != 0 : (s->ngroup < 2 || s->ngroup > MDB_JOIN_KEY_MAX_COLS))
		return 1;
	collect_conjuncts(s->on[1], conj, &nconj, 32);
	if (nconj < 2 || nconj > MDB_JOIN_KEY_MAX_COLS || (!only_count && s->ngroup != nconj))
		return 1;
	for (int i = 0; i < nconj; i++) {
		const struct mdb_expr *c = conj[i];
		if (c->kind != MDB_EX_CMP || c->op != MDB_CMP_EQ || c->kids[0]->kind != MDB_EX_FIELD || c->kids[1]->kind != MDB_EX_FIELD ||
		    c->kids[0]->tbl_idx == c->kids[1]->tbl_idx || c->kids[0]->type != c->kids[1]->type || c->kids[0]->type == MDB_CT_DOUBLE)
			return 1;
	}
	for (int g = 0; g < s->ngroup; g++)
		if (s->group[g]->kind != MDB_EX_FIELD)
			return 1;
	x->n = s->tabs[0].t->nrows;	/* (the plan asks whether there is a left stream at all; none is made here) */
	rc = composite_join_plan(x, 1, conj, nconj, &ck);
	x->n = 0;
	if (rc)
		return rc;
	if (ck.lay.ntaken != (uint32_t)nconj)
		return 1;
	/* GROUP BY one side of every taken equality: each group field finds an equality of its own */
	bool used[MDB_JOIN_KEY_MAX_COLS] = { false };
	for (int g = 0; g < s->ngroup; g++) {
		int c = 0;
		while (c < nconj && (used[c] || !(field_eq(s->group[g], ck.kl[c]) || field_eq(s->group[g], ck.kr[c]))))
			c++;
		if (c == nconj)
			return 1;
		used[c] = true;
	}

	x->composite_fused++;
	x->nfused = nconj;
	x->nfused_map = 0;
	for (int c = 0; c < nconj; c++)
		for (int side = 0; side < 2; side++) {
			const struct mdb_expr *f = side ? ck.kr[c] : ck.kl[c];
			x->fused_tbl[x->nfused_map] = f->tbl_idx;
			x->fused_col[x->nfused_map] = f->col_idx;
			x->fused_at[x->nfused_map++] = c;
		}
	uint64_t G = 0, J = 0;
	if (!ck.empty) {
		const uint32_t *lsel, *rsel;
		uint64_t l_rows, r_rows;
		if ((rc = table_filter(x, 0, ws->push[0], ws->npush[0], &lsel, &l_rows)) || (rc = table_filter(x, 1, ws->push[1], ws->npush[1], &rsel, &r_rows)))
			return rc;
		if (l_rows && r_rows) {
			if ((rc = composite_pack_sides(x, &ck, true, lsel, l_rows, rsel, r_rows)))
				return rc;
			/* a group needs a packed key that both sides hold: no more groups than rows of either side or values of the packed field */
			uint64_t cap = l_rows < r_rows ? l_rows : r_rows;
			const uint64_t top = (uint64_t)ck.st[0].max;	/* (below 2^63) */
			cap = top + 1 < cap ? top + 1 : cap;
			int64_t *pk = dalloc(x, cap * 8);
			x->d_count = dalloc(x, cap * 8);
			if (!pk || !x->d_count)
				return dev_fail(x, "allocating group outputs");
			/* the packed columns' own statistics, as the pair path hands them over: temporaries, nothing measured distinct */
			(void)mdb_dev_call_stats(x->dev, ck.vl, &ck.st[0], ck.vr, &ck.st[1]);
			const int frc = mdb_dev_join_group_count(x->dev, ck.vl, ck.nl, l_rows, ck.vr, ck.nr, r_rows,
								  ((only_count || cat->groups_any_order) ? 0u : MDB_ORDER_FIRST) | MDB_KEYS_MAY_ALIAS, pk, x->d_count, NULL, cap,
								  &G, &J);
			op_stats_end(x);
			if (frc)
				return dev_fail(x, "join + group count on a composite key");
			struct mdb_dev_plan_info pi;
			const int64_t *gk = pk;
			if (mdb_dev_last_plan(x->dev, &pi) == 0 && pi.keys_are_left_column && G == l_rows)
				gk = ck.vl;	/* (every left row a group: the packed left column holds the group keys, none were written) */
			if (G && !only_count) {
				for (int c = 0; c < nconj; c++)
					if (!(x->d_fused_keys[c] = dalloc(x, G * 8)))
						return dev_fail(x, "allocating group outputs");
				if (mdb_dev_join_key_unpack(x->dev, &ck.lay, gk, G, x->d_fused_keys))
					return dev_fail(x, "unpacking the group keys");
			}
		}
	}
	if (!G)
		J = 0;
	for (int c = 0; c < nconj; c++)	/* (no group, or count-only: columns that are never read, but there) */
		if (!x->d_fused_keys[c] && !(x->d_fused_keys[c] = dalloc(x, 8)))
			return dev_fail(x, "allocating group outputs");
	if (!x->d_count && !(x->d_count = dalloc(x, 8)))
		return dev_fail(x, "allocating group outputs");
	x->d_fused_key = x->d_fused_keys[0];
	x->fused = true;
	x->n = only_count ? J : G;
	x->joined_rows = J;
	return 0;
}

/* S LEFT / RIGHT / FULL [OUTER] JOIN T ON c (S = the stream of the tables joined so far, T = table t).  SQL's meaning, in the emission order of
 * the inner join: the pairs for which the WHOLE ON expression is true, and every row of the PRESERVED side (LEFT: S, RIGHT: T) without
 * such a pair once, the other side's tables at MDB_NO_ROW (their cells read as NULL); rows come preserved-side-major.
 * FULL preserves both sides and runs in the LEFT orientation: the LEFT JOIN's rows in their order, then T's rows without a pair in T's row
 * order, S's tables at MDB_NO_ROW (mdb_dev_outer_complete_full).  Neither side may be thinned in front of the pair operator: where_split pushes
 * no WHERE conjunct below a FULL join, and an ON conjunct over T alone stays a residual on the pairs (it makes rows unmatched, on both sides).  None of the inner
 * join's shortcuts apply (join elimination, carried payload cells, "the right key IS the left key": it is NULL where there is no row).
 * Order of work: T filtered by its pushed WHERE conjuncts (where_split pushes them only when every join preserves T) and, for LEFT, by
 * the ON conjuncts that read T alone (they decide matching, and T is not preserved: a T row that fails them matches nothing) ->
 * the pair operator, preserved side on the left -> the other ON conjuncts on the pairs, seen as a stream for the length of one filter
 * (a conjunct over the preserved side alone makes rows unmatched, it drops none) -> mdb_dev_outer_complete -> the stream composed. */
static int outer_join_next_table(struct exec *x, int t, const struct mdb_expr *const *pconj, int npconj)
{
	struct mdb_select *s = x->s;
	struct mdb_table *rt = s->tabs[t].t;
	const bool full = mdb_join_is_full(s->join_type[t]);
	const bool left = full || mdb_join_is_left(s->join_type[t]);	/* the orientation: S on the left of the pair operator, S-major pairs */
	struct mdb_expr *conj[32];
	const struct mdb_expr *tconj[PUSH_MAX + 32], *resid[32];
	int nconj = 0, key = -1, ntconj = 0, nresid = 0;
	const struct mdb_expr *kl = NULL, *kr = NULL;
	uint32_t *ps = NULL, *pt = NULL;	/* the pairs: positions in S, positions in (filtered) T */
	uint64_t J = 0;
	int rc;

	if (rt->nrows >= MDB_NO_ROW || x->n >= MDB_NO_ROW) {
		snprintf(x->err, x->errlen, "execution phase: an outer join over 2^32 - 1 rows or more cannot be addressed\n");
		return -MIDORIDB_ERROR;
	}
	if (s->on[t]) {
		collect_conjuncts(s->on[t], conj, &nconj, 32);
		if (nconj > 32) {	/* too many conjuncts: the whole ON is one residual predicate */
			nconj = 0;
			resid[nresid++] = s->on[t];
		}
	}
	for (int i = 0; i < npconj; i++)
		tconj[ntconj++] = pconj[i];
	struct composite_key ck;
	const int crc = composite_join_plan(x, t, conj, nconj, &ck);
	if (crc < 0)
		return crc;
	const bool comp = crc == 0;	/* the equalities of ck.mask are one packed key: none of them is a residual, no other conjunct is the key */
	for (int i = 0; i < nconj; i++) {
		struct mdb_expr *c = conj[i];
		if (comp && ((ck.mask >> i) & 1u)) {
			key = i;
			continue;
		}
		if (!comp && key < 0 && c->kind == MDB_EX_CMP && c->op == MDB_CMP_EQ && c->kids[0]->kind == MDB_EX_FIELD && c->kids[1]->kind == MDB_EX_FIELD) {
			struct mdb_expr *a = c->kids[0], *b = c->kids[1];
			if (a->tbl_idx < t && b->tbl_idx == t) {
				kl = a;
				kr = b;
				key = i;
				continue;
			} else if (b->tbl_idx < t && a->tbl_idx == t) {
				kl = b;
				kr = a;
				key = i;
				continue;
			}
		}
		if (left && !full && expr_tables(c) == 1ull << t)
			tconj[ntconj++] = c;
		else
			resid[nresid++] = c;
	}
	const uint32_t *rsel = NULL;
	uint64_t r_rows = rt->nrows;
	if ((rc = table_filter(x, t, tconj, ntconj, &rsel, &r_rows)))
		return rc;
	const uint64_t n_s = x->n, n_p = left ? n_s : r_rows;
	if (key >= 0 && n_s && r_rows) {
		const int64_t *vl;
		const uint64_t *nl, *nr;
		const void *vr;
		if (comp) {
			if ((rc = composite_join_pack(x, t, &ck, rsel, r_rows)))
				return rc;
			vl = ck.vl;
			nl = ck.nl;
			vr = ck.vr;
			nr = ck.nr;
			if (!ck.empty)
				(void)(left ? mdb_dev_call_stats(x->dev, vl, &ck.st[0], vr, &ck.st[1]) : mdb_dev_call_stats(x->dev, vr, &ck.st[1], vl, &ck.st[0]));
		} else if (kl->type == MDB_CT_DOUBLE) {
			const void *dl;
			if ((rc = double_join_keys(x, &s->tabs[kl->tbl_idx].t->cols[kl->col_idx], x->rid[kl->tbl_idx], n_s, &dl, &nl)) ||
			    (rc = double_join_keys(x, &rt->cols[kr->col_idx], rsel, r_rows, &vr, &nr)))
				return rc;
			vl = dl;
		} else if ((rc = stream_column(x, kl, &vl, &nl)) || (rc = table_column(x, t, kr, rsel, r_rows, &vr, &nr))) {
			return rc;
		}
		if (comp && ck.empty) {
			J = 0;		/* (no pair: every preserved row is unmatched) */
		} else {
			const int jrc = left ? mdb_dev_join_pairs(x->dev, vl, nl, n_s, vr, nr, r_rows, &ps, &pt, &J)
					     : mdb_dev_join_pairs(x->dev, vr, nr, r_rows, vl, nl, n_s, &pt, &ps, &J);
			if (comp)
				op_stats_end(x);
			if (jrc)
				return dev_fail(x, "hash join");
		}
		if ((ps && track(x, ps)) || (pt && track(x, pt)))
			return -MIDORIDB_NOMEM;
	} else if (key < 0) {
		/* no equi-join key (ON 1=1, ON a < b): all pairs, preserved side major, then the ON predicate */
		if (n_s * r_rows > (1ull << 28)) {
			snprintf(x->err, x->errlen, "execution phase: cross join of %llu x %llu rows is too large (no equi-join key in the ON clause)\n",
				 (unsigned long long)n_s, (unsigned long long)r_rows);
			return -MIDORIDB_ERROR;
		}
		J = n_s * r_rows;
		if (J) {
			ps = dalloc(x, J * 4);
			pt = dalloc(x, J * 4);
			if (!ps || !pt)
				return dev_fail(x, "allocating join pairs");
			if (left ? mdb_dev_cross_pairs(x->dev, n_s, r_rows, ps, pt) : mdb_dev_cross_pairs(x->dev, r_rows, n_s, pt, ps))
				return dev_fail(x, "cross join");
		}
	}
	if (J && nresid) {
		/* the pairs as a stream, for the length of the filter: the earlier tables through ps, T through pt */
		uint32_t *saved[MDB_MAX_TABS];
		struct pred_prog p;
		uint32_t *sel, *ps2, *pt2;
		uint64_t m = 0;
		memcpy(saved, x->rid, sizeof(saved));
		rc = stream_select(x, t, ps, J);
		if (!rc && rsel) {
			uint32_t *mapped = dalloc(x, J * 4);
			if (!mapped || mdb_dev_gather32(x->dev, rsel, pt, J, mapped))
				rc = dev_fail(x, "re-mapping row ids");
			x->rid[t] = mapped;
		} else {
			x->rid[t] = pt;
		}
		memset(&p, 0, sizeof(p));
		for (int i = 0; i < nresid && !rc; i++)
			if (pred_compile(x, &p, resid[i]) || (i && pred_emit(&p, MDB_P_AND, 0, 0, 0, 0, 0))) {
				pred_compile_failed(x);
				rc = -MIDORIDB_ERROR;
			}
		sel = rc ? NULL : dalloc(x, J * 4);
		if (!rc && (!sel || mdb_dev_filter(x->dev, p.insn, p.n, p.cols, p.ncols, J, sel, &m)))
			rc = dev_fail(x, "filter");
		memcpy(x->rid, saved, sizeof(saved));
		x->n = n_s;
		if (rc)
			return rc;
		if (m < J) {
			ps2 = dalloc(x, (m ? m : 1) * 4);
			pt2 = dalloc(x, (m ? m : 1) * 4);
			if (!ps2 || !pt2 || (m && (mdb_dev_gather32(x->dev, ps, sel, m, ps2) || mdb_dev_gather32(x->dev, pt, sel, m, pt2))))
				return dev_fail(x, "thinning the join pairs");
			ps = ps2;
			pt = pt2;
			J = m;
		}
	}
	/* the preserved side's rows without partner, at their places */
	uint32_t *cp = NULL, *co = NULL;
	uint64_t total = 0, u_o = 0;	/* u_o: FULL, T's rows without a pair (they follow the LEFT JOIN's rows) */
	if (full ? mdb_dev_outer_complete_full(x->dev, J ? ps : NULL, J ? pt : NULL, J, n_p, r_rows, &cp, &co, &total, &u_o)
		 : mdb_dev_outer_complete(x->dev, J ? (left ? ps : pt) : NULL, J ? (left ? pt : ps) : NULL, J, n_p, &cp, &co, &total))
		return dev_fail(x, "outer completion");
	if ((cp && track(x, cp)) || (co && track(x, co)))
		return -MIDORIDB_NOMEM;
	const bool identity = total == J && J == n_p;	/* every preserved row exactly one pair: cp is 0, 1, 2 ... */
	uint32_t *cs = left ? cp : co, *ct = left ? co : cp;
	if (left && identity)
		x->n = total;	/* (the earlier tables' row ids stand as they are) */
	else if ((rc = stream_select(x, t, cs, total)))
		return rc;
	if (rsel && total) {
		uint32_t *mapped = dalloc(x, total * 4);
		if (!mapped || mdb_dev_gather32(x->dev, rsel, ct, total, mapped))
			return dev_fail(x, "re-mapping row ids");
		ct = mapped;
	} else if (!left && identity) {
		ct = NULL;
	}
	x->rid[t] = ct;
	if (total > J + u_o)	/* rows of the preserved side without a pair: the other side's tables are absent there */
		for (int u = left ? t : 0; u < (left ? t + 1 : t); u++)
			x->may_be_absent[u] = true;
	if (u_o)
		for (int u = 0; u < t; u++)
			x->may_be_absent[u] = true;
	x->joined_rows = total;
	return MIDORIDB_OK;
}

int join_next_table(struct exec *x, int t, const struct mdb_expr *const *pconj, int npconj)
{
	struct mdb_select *s = x->s;
	struct mdb_table *rt = s->tabs[t].t;
	struct mdb_expr *conj[32];
	int nconj = 0, key = -1;
	const struct mdb_expr *kl = NULL, *kr = NULL;
	uint32_t *pl = NULL, *pr = NULL;
	uint32_t answered = 0;	/* the ON conjuncts the join operator itself answers: the key, or the equalities of a composite key */
	uint64_t J = 0;
	int rc;

	if (x->joined_ahead[t])		/* (joined together with an earlier table on the same key: join_with_payload_multi) */
		return MIDORIDB_OK;
	if (s->join_type[t] != 1)
		return outer_join_next_table(x, t, pconj, npconj);
	if (s->on[t]) {
		collect_conjuncts(s->on[t], conj, &nconj, 32);
		if (nconj > 32)
			nconj = 0;	/* too many conjuncts: treat the whole ON as a residual predicate */
		for (int i = 0; i < nconj && key < 0; i++) {
			struct mdb_expr *c = conj[i];
			if (c->kind == MDB_EX_CMP && c->op == MDB_CMP_EQ && c->kids[0]->kind == MDB_EX_FIELD && c->kids[1]->kind == MDB_EX_FIELD) {
				struct mdb_expr *a = c->kids[0], *b = c->kids[1];
				if (a->tbl_idx < t && b->tbl_idx == t) {
					kl = a;
					kr = b;
					key = i;
				} else if (b->tbl_idx < t && a->tbl_idx == t) {
					kl = b;
					kr = a;
					key = i;
				}
			}
		}
	}
	if (key >= 0 && nconj == 1 && !npconj && !x->cat->dist && x->n && !x->nagg /* (SUM / MIN / MAX / AVG: the materialising join, always) */ &&
	    only_key_needed(x, t, kr->col_idx) && join_is_total_by_catalog(x, kl, kr)) {
		/* join elimination: the catalog says every row of the stream has exactly one partner, and only t's key is read */
		const int64_t *vl;
		const uint64_t *nl;
		if ((rc = stream_column(x, kl, &vl, &nl)))
			return rc;
		if (!nl) {
			x->same_col[t] = kr->col_idx;
			x->same_as_tbl[t] = kl->tbl_idx;
			x->same_as_col[t] = kl->col_idx;
			x->joins_eliminated++;
			return payload_shadow(x, t, kr->col_idx, vl, NULL, 0, NULL);
		}
	}
	/* the new table's own WHERE conjuncts filter it before it is joined */
	const uint32_t *rsel = NULL;
	uint64_t r_rows = rt->nrows;
	if ((rc = table_filter(x, t, pconj, npconj, &rsel, &r_rows)))
		return rc;
	if (x->cat->dist) {
		/* sharded mode: both sides go where their join key hashes to - the left stream unless it already is there (joined on
		 * this key before), the new table always (its rows that passed its own WHERE conjuncts at home) */
		if (key < 0) {
			/* no equi-join key (FROM A, B; a general ON expression: reference executor_select.c:1096-1141): nothing says which rank a
			 * row's partners live on - the new table (its rows that passed its own WHERE conjuncts) is replicated on every rank
			 * and each rank pairs ITS stream with all of it: every (l, r) pair is produced exactly once, where l lives */
			const int tabs1[1] = { t };
			uint32_t *rids1[1] = { (uint32_t *)rsel };
			if ((rc = shard_rows(x, tabs1, 1, rids1, r_rows, NULL, NULL, SHARD_BROADCAST, &r_rows)))
				return rc;
			rsel = NULL;
			rt = s->tabs[t].t;
		} else {
		if (!in_part(x, kl) && (rc = shard_stream(x, t, kl, 0)))
			return rc;
		{
			const void *kv;
			const uint64_t *kn;
			const int tabs1[1] = { t };
			uint32_t *rids1[1] = { (uint32_t *)rsel };
			if (kr->type == MDB_CT_DOUBLE)
				rc = double_join_keys(x, &rt->cols[kr->col_idx], rsel, r_rows, &kv, &kn);
			else
				rc = table_column(x, t, kr, rsel, r_rows, &kv, &kn);
			if (!rc && kr->type == MDB_CT_VARCHAR) {	/* (rows go where their STRING hashes to: the ranks' common id of it) */
				const int64_t *common = NULL;
				rc = shard_ids(x, kv, r_rows, true, false, &common);
				kv = common;
			}
			if (rc || (rc = shard_rows(x, tabs1, 1, rids1, r_rows, kv, kn, 0, &r_rows)))
				return rc;
			rsel = NULL;
			rt = s->tabs[t].t;
		}
		if (x->npart < 2 * MDB_MAX_TABS)
			x->part[x->npart++] = kr;
		}
	}
	if (key >= 0) {
		const int64_t *vl;
		const uint64_t *nl;
		const void *vr;
		const uint64_t *nr;
		if (kl->type == MDB_CT_DOUBLE) {
			const void *dl;
			if ((rc = double_join_keys(x, &s->tabs[kl->tbl_idx].t->cols[kl->col_idx], x->rid[kl->tbl_idx], x->n, &dl, &nl)) ||
			    (rc = double_join_keys(x, &rt->cols[kr->col_idx], rsel, r_rows, &vr, &nr)))
				return rc;
			vl = dl;
		} else if ((rc = stream_column(x, kl, &vl, &nl)) || (rc = table_column(x, t, kr, rsel, r_rows, &vr, &nr))) {
			return rc;
		}
		if (kl->type != MDB_CT_DOUBLE && kr->type != MDB_CT_DOUBLE) {
			x->same_col[t] = kr->col_idx;
			x->same_as_tbl[t] = kl->tbl_idx;
			x->same_as_col[t] = kl->col_idx;
		}
		if (kl->type != MDB_CT_DOUBLE && kr->type != MDB_CT_DOUBLE)
			op_stats_begin(x, kl, vl, kr, vr);	/* (until the join is done: op_stats_end below / at the early returns) */
		if (x->n && r_rows && !x->cat->dist && !rsel && kl->type != MDB_CT_DOUBLE && kr->type != MDB_CT_DOUBLE) {
			int prc = nconj == 1 ? join_with_payload_multi(x, t, kl, kr, vl, nl, vr, nr, r_rows) : 1;
			if (prc == 1)
				prc = join_with_payload(x, t, kr, vl, nl, vr, nr, r_rows);
			if (prc <= 0)
				op_stats_end(x);
			if (prc < 0)
				return prc;
			if (prc == 0) {
				for (int i = 0; i < nconj; i++)		/* residual ON conjuncts, on the merged tuples */
					if (i != key && (rc = stream_filter(x, t + 1, conj[i])))
						return rc;
				if (nconj > 1)
					x->joined_rows = x->n;
				return MIDORIDB_OK;
			}
		}
		answered = 1u << key;
		struct composite_key ck;
		ck.empty = false;
		if (x->n && r_rows) {
			/* none of the one-key shortcuts served: several equalities as ONE packed key, when the rule above says so */
			const int crc = composite_join_plan(x, t, conj, nconj, &ck);
			if (crc <= 0)
				op_stats_end(x);
			if (crc < 0 || (crc == 0 && (rc = composite_join_pack(x, t, &ck, rsel, r_rows))))
				return crc < 0 ? crc : rc;
			if (crc == 0) {
				answered = ck.mask;
				vl = ck.vl;
				nl = ck.nl;
				vr = ck.vr;
				nr = ck.nr;
				if (!ck.empty)
					(void)mdb_dev_call_stats(x->dev, vl, &ck.st[0], vr, &ck.st[1]);
			}
		}
		if (x->n && r_rows && !ck.empty) {
			const int jrc = mdb_dev_join_pairs(x->dev, vl, nl, x->n, vr, nr, r_rows, &pl, &pr, &J);
			op_stats_end(x);
			if (jrc)
				return dev_fail(x, "hash join");
			if (pl && track(x, pl))
				return -MIDORIDB_NOMEM;
			if (pr && track(x, pr))
				return -MIDORIDB_NOMEM;
		}
		op_stats_end(x);
	} else {
		/* no equi-join key: FROM A, B (ON 1=1) or a general ON -> all pairs, then the ON predicate */
		const uint64_t total = x->n * r_rows;
		uint64_t too_large = total > (1ull << 28) ? 1u : 0u;
		if (x->cat->dist && mdb_dist_allreduce_sum_u64(x->cat->dist, &too_large, 1)) {	/* (every rank must leave the statement together) */
			snprintf(x->err, x->errlen, "execution phase: %s\n", mdb_dist_last_error(x->cat->dist));
			return -MIDORIDB_INTERNAL;
		}
		if (too_large) {
			snprintf(x->err, x->errlen, "execution phase: cross join of %llu x %llu rows is too large (no equi-join key in the ON clause)\n",
				 (unsigned long long)x->n, (unsigned long long)r_rows);
			return -MIDORIDB_ERROR;
		}
		J = total;
		if (J) {
			pl = dalloc(x, J * 4);
			pr = dalloc(x, J * 4);
			if (!pl || !pr)
				return dev_fail(x, "allocating join pairs");
			if (mdb_dev_cross_pairs(x->dev, x->n, r_rows, pl, pr))
				return dev_fail(x, "cross join");
		}
	}
	if (rsel && J) {	/* pairs index the filtered right rows: back to row ids of the base table */
		uint32_t *mapped = dalloc(x, J * 4);
		if (!mapped || mdb_dev_gather32(x->dev, rsel, pr, J, mapped))
			return dev_fail(x, "re-mapping row ids");
		pr = mapped;
	}
	/* compose the stream: earlier tables through pl, the new table = pr - unless pl is 0, 1, 2 ... (every row of the stream joined
	 * exactly one right row: a primary-key join): the earlier tables' row ids then stand as they are, nothing is gathered */
	struct mdb_dev_plan_info pi;
	if (key >= 0 && J == x->n && pl && mdb_dev_last_plan(x->dev, &pi) == 0 && pi.pairs_identity)
		x->n = J;
	else if ((rc = stream_select(x, t, pl, J)))
		return rc;
	x->rid[t] = pr;
	x->joined_rows = J;
	/* residual ON conjuncts (everything except the hash key), evaluated on the merged tuples */
	if (s->on[t]) {
		if (key < 0) {
			if ((rc = stream_filter(x, t + 1, s->on[t])))
				return rc;
		} else {
			for (int i = 0; i < nconj; i++)
				if (!((answered >> i) & 1u) && (rc = stream_filter(x, t + 1, conj[i])))
					return rc;
		}
		x->joined_rows = x->n;
	}
	return MIDORIDB_OK;
}

/* ------------------------------------------------------------------ result assembly */

void mdb_result_free(struct mdb_result *r)
{
	if (!r)
		return;
	for (int c = 0; c < r->ncols; c++) {
		if (r->data)
			mdb_dev_host_free(r->data[c]);
		if (r->nullbits)
			free(r->nullbits[c]);
		/* (two result columns may be ONE device buffer - both key columns of SELECT * over an equi-join: freed with the first) */
		bool dup_d = false, dup_n = false;
		for (int k = 0; k < c; k++) {
			dup_d = dup_d || (r->d_data && r->d_data[c] && r->d_data[k] == r->d_data[c]);
			dup_n = dup_n || (r->d_nullbits && r->d_nullbits[c] && r->d_nullbits[k] == r->d_nullbits[c]);
		}
		if (r->d_data && r->d_data[c] && !dup_d)
			mdb_dev_free(r->dev, r->d_data[c]);
		if (r->d_nullbits && r->d_nullbits[c] && !dup_n)
			mdb_dev_free(r->dev, r->d_nullbits[c]);
	}
	mdb_result_legacy_free(r);
	pthread_mutex_destroy(&r->legacy.mutex);
	free(r->data);
	free(r->nullbits);
	free(r->d_data);
	free(r->d_nullbits);
	free(r->colname);
	free(r->coltype);
	free(r->colprec);
	free(r);
}

/* one result column device -> host; a NULL cell reads as 0 through query_column_int64(), like the reference
 * (cpy_cols skips the copy into the zeroed row, executor_select.c:384-387) */
int result_column_to_host(mdb_dev_ctx *dev, struct mdb_result *res, int c, const void *d_vals, const uint64_t *d_nulls)
{
	const uint64_t rows = res->nrows;
	if (!d_vals || !rows)
		return MIDORIDB_OK;
	if (mdb_dev_d2h(dev, res->data[c], d_vals, rows * 8))
		return -MIDORIDB_INTERNAL;
	if (d_nulls) {
		const uint64_t words = (rows + 63) / 64;
		if (!res->nullbits[c])		/* (a fetch that is tried again after a failure finds the bitmap of its first attempt) */
			res->nullbits[c] = calloc((size_t)words, 8);
		if (!res->nullbits[c] || mdb_dev_d2h(dev, res->nullbits[c], d_nulls, words * 8))
			return -MIDORIDB_INTERNAL;
		for (uint64_t i = 0; i < rows; i++)
			if ((res->nullbits[c][i >> 6] >> (i & 63)) & 1)
				res->data[c][i] = 0;
	}
	return MIDORIDB_OK;
}

int mdb_result_fetch(struct mdb_result *r)
{
	if (!r || r->fetched)
		return MIDORIDB_OK;
	for (int c = 0; c < r->ncols; c++) {
		if (!r->d_data || !r->d_data[c])
			continue;
		if (!r->data[c]) {
			r->data[c] = mdb_dev_host_alloc((size_t)(r->nrows ? r->nrows : 1) * 8);
			if (!r->data[c])
				return -MIDORIDB_NOMEM;
		}
		if (result_column_to_host(r->dev, r, c, r->d_data[c], r->d_nullbits ? r->d_nullbits[c] : NULL))
			return -MIDORIDB_INTERNAL;
	}
	r->fetched = true;
	mdb_result_legacy_rows(r);
	return MIDORIDB_OK;
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
	uint32_t form = 0;

	for (int i = 0; i < x->nagg; i++) {
		const int t = x->agg_tbl[i];
		const struct mdb_column *col = &x->s->tabs[t].t->cols[x->agg_col[i]];
		ag[i].op = x->agg_op[i];
		ag[i].type = col->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
		ag[i].values = col->d_data;
		ag[i].nullbits = col->d_nullbits;
		ag[i].rid = x->rid[t];
		if (!ag[i].values && !(ag[i].values = dalloc(x, 8)))	/* (an empty table under an outer join: every tuple is at "no row", no cell is read) */
			return dev_fail(x, "aggregates");
		x->d_agg[i] = dalloc(x, G * 8);
		x->d_agg_nulls[i] = dalloc(x, ((G + 63) / 64 + 1) * 8);
		ag[i].out = x->d_agg[i];
		ag[i].out_nullbits = x->d_agg_nulls[i];
		if (!x->d_agg[i] || !x->d_agg_nulls[i])
			return dev_fail(x, "allocating aggregate columns");
	}
	if (mdb_dev_group_aggregate(x->dev, gk, nk, x->n, first, G, ag, x->nagg, &form))
		return dev_fail(x, "SUM / MIN / MAX / AVG");
	if (form == 1 || form == 2)
		x->agg_calls[form - 1]++;
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
bool keys_only_join(const struct mdb_select *s, const struct mdb_catalog *cat, int has_count, const int *key_tbl, const int *key_col,
			   const int *src, int ncols, const struct mdb_expr **kj)
{
	if (cat->dist || s->ntabs != 2 || s->where || s->ngroup || has_count || s->distinct || s->norder || s->having || s->has_limit || !ncols)
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
	for (int c = 0; c < ncols; c++) {
		const int t = key_tbl[src[c]], col = key_col[src[c]];
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

int mdb_exec_select(struct mdb_catalog *cat, struct mdb_select *s, struct mdb_result **out, char *err, size_t errlen)
{
	stmt_dict = &cat->dict;
	struct exec x;
	struct mdb_result *res = NULL;
	char (*keys)[MDB_NAME_LEN] = NULL;
	int *order = NULL, *key_tbl = NULL, *key_col = NULL, *src = NULL;
	int nkeys = 0, ncols = 0, rc, has_count = 0;
	void **direct_vals = NULL;		/* scan + WHERE + projection plan: the result columns on the device, final */
	uint64_t **direct_nulls = NULL;
	double t0;
	const struct mdb_expr *fkeys[MDB_MAX_TABS];
	const struct mdb_expr *kj[2] = { NULL, NULL };
	int fused, cfrc = 1;

	*out = NULL;
	memset(&x, 0, sizeof(x));
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
	if ((rc = subqueries_eval(cat, s->where, err, errlen)) || (rc = subqueries_eval(cat, s->having, err, errlen)))
		goto out;
	const double sub_ms = (s->where && expr_has_subquery(s->where)) || (s->having && expr_has_subquery(s->having)) ? now_ms() - sub_t0 : 0.0;

	/* ---- result column set in the reference's order (R3): COUNT(*) first if selected, then every column
	 *      of every FROM table left to right; projected afterwards to the select list */
	for (int i = 0; i < s->nsel; i++)
		has_count |= s->sel[i]->kind == MDB_EX_COUNT;
	/* SUM / MIN / MAX / AVG of the select list, each (function, column) once: result column "SUM(<table>.<column>)", ordered with all the others */
	for (int i = 0; i < s->nsel; i++)
		if (s->sel[i]->kind == MDB_EX_AGG && agg_index(&x, s->sel[i]) < 0 && x.nagg < MDB_AGG_MAX_AGGS) {
			x.agg_op[x.nagg] = s->sel[i]->op;
			x.agg_tbl[x.nagg] = s->sel[i]->tbl_idx;
			x.agg_col[x.nagg] = s->sel[i]->col_idx;
			x.agg_type[x.nagg] = s->sel[i]->type;
			x.nagg++;
		}
	const bool has_agg = x.nagg > 0;
	{
		int total = has_count + x.nagg;
		for (int t = 0; t < s->ntabs; t++)
			total += s->tabs[t].t->ncols;
		keys = calloc((size_t)total, sizeof(*keys));
		order = calloc((size_t)total, sizeof(int));
		key_tbl = calloc((size_t)total, sizeof(int));
		key_col = calloc((size_t)total, sizeof(int));
		if (!keys || !order || !key_tbl || !key_col) {
			rc = -MIDORIDB_NOMEM;
			goto out;
		}
		if (has_count) {
			strcpy(keys[nkeys], "COUNT(*)");
			key_tbl[nkeys] = -1;
			nkeys++;
		}
		for (int a = 0; a < x.nagg; a++) {	/* key_tbl = -2 - a: the statement's a-th aggregate */
			snprintf(keys[nkeys], MDB_NAME_LEN, "%s(%.56s.%.56s)", mdb_agg_name(x.agg_op[a]), s->tabs[x.agg_tbl[a]].t->name,
				 s->tabs[x.agg_tbl[a]].t->cols[x.agg_col[a]].name);
			key_tbl[nkeys] = -2 - a;
			nkeys++;
		}
		for (int t = 0; t < s->ntabs; t++)
			for (int c = 0; c < s->tabs[t].t->ncols; c++) {
				snprintf(keys[nkeys], MDB_NAME_LEN, "%.60s.%.60s", s->tabs[t].t->name, s->tabs[t].t->cols[c].name);
				key_tbl[nkeys] = t;
				key_col[nkeys] = c;
				nkeys++;
			}
		if ((rc = mdb_reference_column_order((const char (*)[MDB_NAME_LEN])keys, nkeys, order)))
			goto out;
	}

	/* the result columns that are wanted, in the reference's order */
	src = calloc((size_t)(nkeys ? nkeys : 1), sizeof(int));
	if (!src) {
		rc = -MIDORIDB_NOMEM;
		goto out;
	}
	for (int k = 0; k < nkeys; k++) {
		int key = order[k];
		bool want = false;
		if (key_tbl[key] < 0) {
			want = true;
		} else if (s->select_all) {
			want = true;
		} else {
			for (int i = 0; i < s->nsel; i++)
				if (s->sel[i]->kind == MDB_EX_FIELD && s->sel[i]->tbl_idx == key_tbl[key] && s->sel[i]->col_idx == key_col[key])
					want = true;
		}
		if (want)
			src[ncols++] = key;
	}

	t0 = now_ms();
	struct where_split ws;
	const bool split_ok = where_split(s, &ws);
	bool only_count = has_count && !s->ngroup && !s->select_all;
	for (int i = 0; i < s->nsel; i++)
		only_count = only_count && s->sel[i]->kind == MDB_EX_COUNT;
	/* (the fused operator is an inner join and knows COUNT(*) only: a statement with SUM / MIN / MAX / AVG materialises its join) */
	fused = s->ntabs <= PUSH_TABS && !x.has_outer && !has_agg ? fused_chain(s, fkeys, only_count) : -1;
	if (fused >= 0 && !cat->dist && split_ok) {
		/* join elimination: when the catalog says every right table of the chain is a complete primary key over the first table's key range,
		 * the fused join + GROUP BY operator has nothing to find out - the general plan drops those joins (join_next_table) and groups the
		 * first table's key column alone (the identity when that column holds no value twice) */
		bool all = s->ntabs > 1;
		for (int t = 1; t < s->ntabs && all; t++)
			all = !ws.npush[t] && only_key_needed(&x, t, fkeys[t]->col_idx) && join_is_total_by_catalog(&x, fkeys[0], fkeys[t]);
		if (all)
			fused = -1;
	}
	/* the join of two key columns, nothing else selected: in the reference's order it is tried as a primary-key join first (the keys with
	 * partners in the left table's row order; large tables only: the attempt runs the ordered join + GROUP BY operator), and left to the
	 * materialising join below when a key has several rows on a side */
	bool keys_only = !x.has_outer && keys_only_join(s, cat, has_count || has_agg, key_tbl, key_col, src, ncols, kj);
	int64_t *keys_ordered = NULL;
	uint64_t keys_ordered_rows = 0;
	if (keys_only && !cat->groups_any_order) {
		const struct mdb_table *tl = s->tabs[kj[0]->tbl_idx].t, *tr = s->tabs[kj[1]->tbl_idx].t;
		int served = 0;
		int krc = 0;
		if (tl->nrows && !tl->cols[kj[0]->col_idx].d_nullbits && tl->cols[kj[0]->col_idx].d_data && join_is_total_by_catalog(&x, kj[0], kj[1])) {
			/* join elimination: every row of the left table has exactly one partner (the catalog's statistics) - the joined rows' key column
			 * IS the left table's key column, in its order, without a kernel */
			keys_ordered = (int64_t *)tl->cols[kj[0]->col_idx].d_data;
			keys_ordered_rows = tl->nrows;
			served = 2;
			x.joins_eliminated++;
		} else if (tl->nrows + tr->nrows >= (1u << 21)) {
			op_stats_begin(&x, kj[0], tl->cols[kj[0]->col_idx].d_data, kj[1], tr->cols[kj[1]->col_idx].d_data);
			krc = mdb_dev_join_keys_ordered(x.dev, tl->cols[kj[0]->col_idx].d_data, tl->cols[kj[0]->col_idx].d_nullbits, tl->nrows,
							 tr->cols[kj[1]->col_idx].d_data, tr->cols[kj[1]->col_idx].d_nullbits, tr->nrows, &keys_ordered,
							 &keys_ordered_rows, &served);
			op_stats_end(&x);
		}
		if (krc) {
			rc = dev_fail(&x, "join of two key columns");
			goto out;
		}
		keys_only = served != 0;
		/* (served == 2: the joined rows' key column IS the left table's key column - held by the result, never freed here) */
		if (keys_ordered && served != 2 && track(&x, keys_ordered)) {
			rc = -MIDORIDB_NOMEM;
			goto out;
		}
	}
	if (fused >= 0 && (!split_ok || ws.nresidual))
		fused = -1;	/* a conjunct reads several tables: it has to see the joined rows */
	if (fused >= 0 && cat->dist && s->ntabs > 2 && fkeys[0]->type == MDB_CT_VARCHAR)
		fused = -1;	/* (sharded chains over VARCHAR keys: the general plan exchanges the rows by their strings' common ids) */
	if (fused >= 0) {
		/* ---- north-star plan: join + GROUP BY key + COUNT(*) without materialising the join.  More than two tables
		 *      on the same key chain the operator: the group keys of (T0, T1) are joined with T2, and so on; a group's
		 *      COUNT(*) is the product of the per-table multiplicities (mdb_dev_combine_counts).  WHERE conjuncts that
		 *      read one table filter that table before it enters the join. */
		const void *lv, *rv;
		const uint64_t *ln, *rn;
		uint64_t nl_rows, nr_rows;
		if ((rc = fused_operand(&x, 0, fkeys[0], ws.push[0], ws.npush[0], &lv, &ln, &nl_rows)) ||
		    (rc = fused_operand(&x, 1, fkeys[1], ws.push[1], ws.npush[1], &rv, &rn, &nr_rows)))
			goto out;
		uint64_t cap = nl_rows ? nl_rows : 1, G = 0, J = 0;
		/* a group of the join needs a key that both sides hold: no more groups than rows or key values of either column (catalog
		 * statistics) - the output columns are sized for that, and become the result's own without a copy when the bound is close */
		if (!cat->dist && fkeys[0]->type != MDB_CT_DOUBLE) {
			cap = op_groups_bound(&x, fkeys[0], cap);
			cap = op_groups_bound(&x, fkeys[1], cap < nr_rows ? cap : (nr_rows ? nr_rows : 1));
		}
		bool multi_done = false, alias_checked = false;
		const bool text_keys = cat->dist && fkeys[0]->type == MDB_CT_VARCHAR;
		if (text_keys) {
			/* sharded mode, VARCHAR join keys: the ids of this process's dictionary mean nothing to the other ranks - the operator
			 * runs on the ranks' common ids (shard_ids) and its group keys are translated back where they arrive */
			const int64_t *cl = NULL, *cr = NULL;
			if ((rc = shard_ids(&x, (const int64_t *)lv, nl_rows, true, false, &cl)) || (rc = shard_ids(&x, (const int64_t *)rv, nr_rows, true, false, &cr)))
				goto out;
			lv = cl;
			rv = cr;
		}
		if (cat->dist && fkeys[0]->type != MDB_CT_DOUBLE && !text_keys && (rc = shard_promise_ranges(&x, fkeys[0], fkeys[1])))
			goto out;
		if (cat->dist && s->ntabs > 2 && s->ntabs <= 4) {
			/* sharded mode, three or four tables on one key: ONE exchange - every table partitioned once with the same hash, the
			 * right tables' counts multiplied where the regions meet (mdb_dist_join_group_count_multi_alloc); when that form is
			 * not served (every rank learns so together) the chain of two-table calls below runs */
			const int64_t *rk[3];
			const uint64_t *rnb[3];
			uint64_t rrows[3];
			rk[0] = rv;
			rnb[0] = rn;
			rrows[0] = nr_rows;
			for (int t = 2; t < s->ntabs; t++) {
				const void *cv;
				if ((rc = fused_operand(&x, t, fkeys[t], ws.push[t], ws.npush[t], &cv, &rnb[t - 1], &rrows[t - 1])))
					goto out;
				rk[t - 1] = cv;
			}
			const int mrc = mdb_dist_join_group_count_multi_alloc(cat->dist, lv, ln, nl_rows, s->ntabs - 1, rk, rnb, rrows, &x.d_fused_key, &x.d_count,
									      &G, &J);
			if (mrc < 0) {
				snprintf(err, errlen, "execution phase: sharded join + group count: %s\n", mdb_dist_last_error(cat->dist));
				rc = -MIDORIDB_INTERNAL;
				goto out;
			}
			if (mrc == 0) {
				if (track(&x, x.d_fused_key) || track(&x, x.d_count)) {
					rc = -MIDORIDB_NOMEM;
					goto out;
				}
				multi_done = true;
			}
		}
		if (cat->dist && !multi_done) {
			/* sharded mode: the tables hold this rank's rows; both key columns are exchanged (RCCL all-to-all per table,
			 * include/mdb_dist.h) and this rank keeps the groups whose key hashes to it.  Collective: every rank runs the
			 * same statement. */
			/* (more tables follow on the same key: the groups must lie where their key hashes to, for the tables sent after them) */
			if (mdb_dist_join_group_count_alloc(cat->dist, lv, ln, nl_rows, rv, rn, nr_rows, s->ntabs > 2 ? MDB_DIST_PLACE_BY_KEY_HASH : 0u,
							    &x.d_fused_key, &x.d_count, NULL, &G, &J)) {
				snprintf(err, errlen, "execution phase: sharded join + group count: %s\n", mdb_dist_last_error(cat->dist));
				rc = -MIDORIDB_INTERNAL;
				goto out;
			}
			if (track(&x, x.d_fused_key) || track(&x, x.d_count)) {
				rc = -MIDORIDB_NOMEM;
				goto out;
			}
		} else if (!cat->dist) {
			x.d_fused_key = dalloc(&x, cap * 8);
			x.d_count = dalloc(&x, cap * 8);
			if (!x.d_fused_key || !x.d_count) {
				rc = dev_fail(&x, "allocating group outputs");
				goto out;
			}
			if (s->ntabs > 2 && s->ntabs <= 4) {
				/* A JOIN B ON a = b JOIN C ON a = c [JOIN D ...]: every table partitioned once, the right tables' counts multiplied
				 * in the leaf kernel, the groups ordered once (mdb_dev_join_group_count_multi; it chains by itself when the keys
				 * do not take the compact form) */
				const int64_t *rk[3];
				const uint64_t *rnb[3];
				uint64_t rrows[3];
				rk[0] = rv;
				rnb[0] = rn;
				rrows[0] = nr_rows;
				for (int t = 2; t < s->ntabs; t++) {
					const void *cv;
					if ((rc = fused_operand(&x, t, fkeys[t], ws.push[t], ws.npush[t], &cv, &rnb[t - 1], &rrows[t - 1])))
						goto out;
					rk[t - 1] = cv;
				}
				if (mdb_dev_join_group_count_multi(x.dev, lv, ln, nl_rows, s->ntabs - 1, rk, rnb, rrows,
								   ((only_count || cat->groups_any_order) ? 0u : MDB_ORDER_FIRST) | MDB_KEYS_MAY_ALIAS, x.d_fused_key,
								   x.d_count, NULL, cap, &G, &J)) {
					rc = dev_fail(&x, "join + group count over several tables");
					goto out;
				}
				multi_done = true;
				alias_checked = true;
			} else {
				if (fkeys[0]->type != MDB_CT_DOUBLE && !text_keys)
					op_stats_begin(&x, fkeys[0], lv, fkeys[1], rv);
				const int frc = mdb_dev_join_group_count(x.dev, lv, ln, nl_rows, rv, rn, nr_rows,
									  /* (a bare COUNT(*) has no group order to keep; nor has a GROUP BY when the database says so) */
									  ((only_count || cat->groups_any_order) ? 0u : MDB_ORDER_FIRST) | MDB_KEYS_MAY_ALIAS,
									  x.d_fused_key, x.d_count, NULL, cap, &G, &J);
				op_stats_end(&x);
				if (frc) {
					rc = dev_fail(&x, "join + group count");
					goto out;
				}
				alias_checked = true;
			}
		}
		if (alias_checked) {
			/* every left row turned out to be a group: the group keys ARE the left key column, in its order - the operator wrote none
			 * (MDB_KEYS_MAY_ALIAS) and the stream reads the column itself; a result kept on the device becomes one more holder of the
			 * table's buffer (0.8 GB less read and written at 10^8 rows) */
			struct mdb_dev_plan_info pi;
			if (mdb_dev_last_plan(x.dev, &pi) == 0 && pi.keys_are_left_column && G == nl_rows)
				x.d_fused_key = (int64_t *)(uintptr_t)lv;
		}
		for (int t = 2; t < s->ntabs && (G || cat->dist) && !multi_done; t++) {
			const void *cv;
			const uint64_t *cn;
			uint64_t nc_rows;
			if ((rc = fused_operand(&x, t, fkeys[t], ws.push[t], ws.npush[t], &cv, &cn, &nc_rows)))
				goto out;
			int64_t *key2 = NULL, *cnt2 = NULL, *cnt3 = dalloc(&x, (G ? G : 1) * 8);
			uint32_t *first2 = NULL;
			uint64_t G2 = 0, J2 = 0;
			if (cat->dist) {
				/* the groups so far already live on the rank their key hashes to: only the new table travels */
				if (mdb_dist_join_group_count_alloc(cat->dist, x.d_fused_key, NULL, G, cv, cn, nc_rows, MDB_DIST_LEFT_IN_PLACE, &key2, &cnt2,
								    &first2, &G2, &J2)) {
					snprintf(err, errlen, "execution phase: sharded join + group count: %s\n", mdb_dist_last_error(cat->dist));
					rc = -MIDORIDB_INTERNAL;
					goto out;
				}
				if (track(&x, key2) || track(&x, cnt2) || track(&x, first2)) {
					rc = -MIDORIDB_NOMEM;
					goto out;
				}
			} else {
				key2 = dalloc(&x, G * 8);
				cnt2 = dalloc(&x, G * 8);
				first2 = dalloc(&x, G * 4);
			}
			if (!key2 || !cnt2 || !cnt3 || !first2) {
				rc = dev_fail(&x, "allocating group outputs");
				goto out;
			}
			if ((!cat->dist && mdb_dev_join_group_count(x.dev, x.d_fused_key, NULL, G, cv, cn, nc_rows, MDB_ORDER_FIRST, key2, cnt2, first2, G,
								    &G2, &J2)) ||
			    mdb_dev_combine_counts(x.dev, x.d_count, NULL, first2, cnt2, G2, cnt3, NULL, &J)) {
				rc = dev_fail(&x, "chained join + group count");
				goto out;
			}
			x.d_fused_key = key2;
			x.d_count = cnt3;
			G = G2;
		}
		if (!G)
			J = 0;
		if (cat->dist && only_count) {
			/* SELECT COUNT(*) over the sharded join: every rank reports the global number of joined rows */
			uint64_t tot = J;
			if (mdb_dist_allreduce_sum_u64(cat->dist, &tot, 1)) {
				snprintf(err, errlen, "execution phase: %s\n", mdb_dist_last_error(cat->dist));
				rc = -MIDORIDB_INTERNAL;
				goto out;
			}
			J = tot;
		}
		if (text_keys && G && !only_count) {	/* the group keys that arrived: common ids -> ids of this rank's dictionary */
			const int64_t *same = NULL;
			if ((rc = shard_ids(&x, x.d_fused_key, G, false, true, &same)))
				goto out;
		}
		x.fused = true;
		x.n = only_count ? J : G;	/* COUNT(*) without GROUP BY = the stream length = the joined rows */
		x.joined_rows = J;
	} else if (!keys_only && split_ok && !has_agg && (cfrc = composite_fused_plan(&x, &ws, only_count)) <= 0) {
		/* ---- the fused plan on a packed composite key (several ON equalities): answered, or an error */
		if (cfrc < 0) {
			rc = cfrc;
			goto out;
		}
	} else if (keys_only) {
		/* ---- a two-table equi-join whose select list names nothing but the two key columns (BASELINE configs[3]: SELECT * over
		 *      two key columns), any order allowed (mdb_database_groups_any_order): both sides hold the same value in every
		 *      joined row, so no row has to be identified - the any-order join + GROUP BY pipeline counts every key's partners and
		 *      the key is written COUNT times (mdb_dev_join_keys); the stream is the fused plan's: one key column, no row ids */
		const struct mdb_column *cl = &s->tabs[kj[0]->tbl_idx].t->cols[kj[0]->col_idx], *cr = &s->tabs[kj[1]->tbl_idx].t->cols[kj[1]->col_idx];
		int64_t *jk = keys_ordered;	/* (the reference's order: answered above) */
		uint64_t J = keys_ordered_rows;
		if (cat->groups_any_order) {
			op_stats_begin(&x, kj[0], cl->d_data, kj[1], cr->d_data);
			const int krc2 = mdb_dev_join_keys(x.dev, cl->d_data, cl->d_nullbits, s->tabs[kj[0]->tbl_idx].t->nrows, cr->d_data, cr->d_nullbits,
							   s->tabs[kj[1]->tbl_idx].t->nrows, &jk, &J);
			op_stats_end(&x);
			if (krc2) {
				rc = dev_fail(&x, "join of two key columns");
				goto out;
			}
		}
		if (jk && jk != keys_ordered && track(&x, jk)) {
			rc = -MIDORIDB_NOMEM;
			goto out;
		}
		x.d_fused_key = jk;
		x.fused = true;
		x.n = J;
		x.joined_rows = J;
	} else if (s->ntabs == 1 && s->where && split_ok && !ws.nresidual && ws.npush[0] && !s->ngroup && !has_count && !has_agg && !s->distinct &&
		   !s->norder && !s->having && !s->has_limit && s->tabs[0].t->nrows && ncols && ncols <= MDB_GATHER_MAX_COLS) {
		/* ---- scan + WHERE + projection of one table (BASELINE configs[0] shape): the predicate bitmap is turned
		 *      straight into the compacted result columns (mdb_dev_filter_project) - no selection vector, no gathers */
		struct mdb_table *tb = s->tabs[0].t;
		struct pred_prog p;
		struct mdb_project_col pc[MDB_GATHER_MAX_COLS];
		uint64_t m = 0;
		memset(&p, 0, sizeof(p));
		for (int i = 0; i < ws.npush[0]; i++)
			if (pred_compile(&x, &p, ws.push[0][i]) || (i && pred_emit(&p, MDB_P_AND, 0, 0, 0, 0, 0))) {
				pred_compile_failed(&x);
				rc = -MIDORIDB_ERROR;
				goto out;
			}
		direct_vals = calloc((size_t)ncols, sizeof(void *));
		direct_nulls = calloc((size_t)ncols, sizeof(uint64_t *));
		if (!direct_vals || !direct_nulls) {
			rc = -MIDORIDB_NOMEM;
			goto out;
		}
		for (int c = 0; c < ncols; c++) {
			struct mdb_column *col = &tb->cols[key_col[src[c]]];
			pc[c].values = col->d_data;
			pc[c].nullbits = col->d_nullbits;
			pc[c].out_values = &direct_vals[c];
			pc[c].out_nullbits = &direct_nulls[c];
		}
		if (mdb_dev_filter_project(x.dev, p.insn, p.n, p.cols, p.ncols, tb->nrows, pc, ncols, &m)) {
			rc = dev_fail(&x, "scan + filter + projection");
			goto out;
		}
		for (int c = 0; c < ncols; c++)
			if ((direct_vals[c] && track(&x, direct_vals[c])) || (direct_nulls[c] && track(&x, direct_nulls[c]))) {
				rc = -MIDORIDB_NOMEM;
				goto out;
			}
		x.n = m;
	} else {
		/* ---- general plan */
		if (cat->dist && s->has_limit && s->limit_off > 0) {
			ERR("execution phase: sharded mode: LIMIT with an offset cannot be answered from one rank's rows\n");
			rc = -MIDORIDB_ERROR;
			goto out;
		}
		x.n = s->tabs[0].t->nrows;	/* scan: identity stream over the first table */
		if (split_ok) {
			/* WHERE conjuncts that read one table filter that table before it is joined; the others after the joins */
			const uint32_t *sel0;
			uint64_t m0;
			if ((rc = table_filter(&x, 0, ws.push[0], ws.npush[0], &sel0, &m0)))
				goto out;
			if (sel0) {
				x.rid[0] = (uint32_t *)sel0;
				x.n = m0;
			}
			x.ws = &ws;
			for (int t = 1; t < s->ntabs; t++)
				if ((rc = join_next_table(&x, t, ws.push[t], ws.npush[t])))
					goto out;
			for (int i = 0; i < ws.nresidual; i++)
				if ((rc = stream_filter(&x, s->ntabs, ws.residual[i])))
					goto out;
		} else {
			for (int t = 1; t < s->ntabs; t++)
				if ((rc = join_next_table(&x, t, NULL, 0)))
					goto out;
			if (s->where && (rc = stream_filter(&x, s->ntabs, s->where)))
				goto out;
		}
		if (cat->dist && s->ngroup) {
			/* sharded mode: a group's rows must meet on one rank - they do when the stream is partitioned by one of the group
			 * fields (a join key); otherwise it is exchanged by the first one, NULL keys included (one group, :1477-1482) */
			bool placed = false;
			for (int g = 0; g < s->ngroup; g++)
				placed = placed || in_part(&x, s->group[g]);
			if (!placed && cat->groups_any_order && s->ngroup == 1 && !x.fused && !s->select_all && !s->distinct && !has_agg &&
			    s->group[0]->kind == MDB_EX_FIELD && s->group[0]->type != MDB_CT_DOUBLE && s->group[0]->type != MDB_CT_VARCHAR) {
				/* any order allowed and only the group key and COUNT(*) can be named (S4): no rows need to travel - every rank's ONE
				 * partition pass over its key column, the first-level regions exchanged, counted where they land
				 * (mdb_dist_group_count_keys_alloc).  Every rank must take the same way: they agree on "no NULL keys anywhere" first.
				 * The decision is taken from the STREAM's key column (its NULL bitmap as it is after joins and exchanges: a shadow table
				 * that arrived over the wire carries bitmaps but no NULL counts), never from catalog counters. */
				const int64_t *kv;
				const uint64_t *kn;
				if ((rc = stream_column(&x, s->group[0], &kv, &kn)))
					goto out;
				uint64_t ok = kn == NULL ? 1u : 0u;
				if (mdb_dist_allreduce_sum_u64(cat->dist, &ok, 1)) {
					snprintf(err, errlen, "execution phase: %s\n", mdb_dist_last_error(cat->dist));
					rc = -MIDORIDB_INTERNAL;
					goto out;
				}
				if (ok == (uint64_t)mdb_dist_world(cat->dist)) {
					int64_t *gk = NULL, *gc = NULL;
					uint64_t Gk = 0;
					if ((rc = shard_promise_ranges(&x, s->group[0], s->group[0])))
						goto out;
					if (!x.promised)
						goto exchange_rows;	/* (no range to promise - an empty column somewhere: the row exchange answers) */
					const int krc = mdb_dist_group_count_keys_alloc(cat->dist, kv, NULL, x.n, &gk, &gc, &Gk);
					if (krc < 0) {
						snprintf(err, errlen, "execution phase: sharded group count: %s\n", mdb_dist_last_error(cat->dist));
						rc = -MIDORIDB_INTERNAL;
						goto out;
					}
					if (krc == 0) {
						if (track(&x, gk) || track(&x, gc)) {
							rc = -MIDORIDB_NOMEM;
							goto out;
						}
						x.d_fused_key = gk;
						x.d_count = gc;
						x.fused = true;
						x.n = Gk;
						goto grouped;
					}
				}
			}
exchange_rows:
			if (!placed && (rc = shard_stream(&x, s->ntabs, s->group[0], MDB_DIST_KEEP_NULL_KEYS)))
				goto out;
		}
		if (cat->dist && s->distinct) {
			/* ... and so must equal rows under DISTINCT */
			bool placed = false;
			const struct mdb_expr *by = NULL;
			static __thread struct mdb_expr first_col;
			for (int i = 0; i < s->nsel; i++)
				if (s->sel[i]->kind == MDB_EX_FIELD) {
					placed = placed || in_part(&x, s->sel[i]);
					by = by ? by : s->sel[i];
				}
			if (s->select_all) {
				placed = placed || x.npart > 0;
				if (!by && s->tabs[0].t->ncols) {
					memset(&first_col, 0, sizeof(first_col));
					first_col.kind = MDB_EX_FIELD;
					first_col.type = s->tabs[0].t->cols[0].type;
					by = &first_col;
				}
			}
			if (!placed && (s->ngroup || !by)) {
				ERR("execution phase: sharded mode: DISTINCT over an aggregate alone cannot be answered from one rank's groups\n");
				rc = -MIDORIDB_ERROR;
				goto out;
			}
			if (!placed && (rc = shard_stream(&x, s->ntabs, by, MDB_DIST_KEEP_NULL_KEYS)))
				goto out;
		}
		if (s->ngroup == 1) {
			const int64_t *kv;
			const uint64_t *kn;
			uint32_t *first;
			uint64_t G = 0;
			if ((rc = stream_column(&x, s->group[0], &kv, &kn)))
				goto out;
			/* any order allowed (mdb_database_groups_any_order), an INTEGER-like key without NULLs: (key, COUNT) pairs without row
			 * ids or an ordering sort - the stream becomes what the fused plan's is (S4: only the group key and COUNT(*) can be
			 * named from here on) */
			if (cat->groups_any_order && !cat->dist && !x.fused && x.n && s->group[0]->kind == MDB_EX_FIELD && s->group[0]->type != MDB_CT_DOUBLE &&
			    !s->select_all && !s->distinct && !has_agg /* (the (key, COUNT) pairs carry no rows to aggregate) */ && !x.may_be_absent[s->group[0]->tbl_idx] &&
			    s->tabs[s->group[0]->tbl_idx].t->cols[s->group[0]->col_idx].null_count == 0) {
				int64_t *gk = dalloc(&x, x.n * 8), *gc = dalloc(&x, x.n * 8);
				uint64_t Gk = 0;
				if (!gk || !gc) {
					rc = dev_fail(&x, "allocating group outputs");
					goto out;
				}
				op_stats_begin(&x, s->group[0], kv, NULL, NULL);
				const int krc = mdb_dev_group_count_keys(x.dev, kv, NULL, x.n, gk, gc, x.n, &Gk);
				op_stats_end(&x);
				if (krc < 0) {
					rc = dev_fail(&x, "group count (any order)");
					goto out;
				}
				if (krc == 0) {
					x.d_fused_key = gk;
					x.d_count = gc;
					x.fused = true;
					x.n = Gk;
					goto grouped;
				}
			}
			/* (no more groups than key values in the column's range - catalog statistics -, plus the NULL group) */
			uint64_t gcap = x.n ? x.n : 1;
			if (s->group[0]->kind == MDB_EX_FIELD && s->group[0]->type != MDB_CT_DOUBLE) {
				const uint64_t b = op_groups_bound(&x, s->group[0], gcap);
				gcap = b + 1 < gcap ? b + 1 : gcap;
			}
			first = dalloc(&x, gcap * 4);
			x.d_count = dalloc(&x, gcap * 8);
			if (!first || !x.d_count) {
				rc = dev_fail(&x, "allocating group outputs");
				goto out;
			}
			if (s->group[0]->kind == MDB_EX_FIELD && s->group[0]->type != MDB_CT_DOUBLE)
				op_stats_begin(&x, s->group[0], kv, NULL, NULL);
			const int grc = x.n ? mdb_dev_group_count(x.dev, kv, kn, x.n, MDB_ORDER_FIRST, first, x.d_count, gcap, &G) : 0;
			op_stats_end(&x);
			if (grc) {
				rc = dev_fail(&x, "group count");
				goto out;
			}
			{
				/* the catalog knew that the column holds no value twice and the operator answered with the identity (group i = row i of the
				 * stream, COUNT 1): the stream stays what it is - no row-id vector to compose, no gather through one in the projection; a
				 * result kept on the device holds the table's columns */
				struct mdb_dev_plan_info pi;
				const bool identity = x.n && G == x.n && mdb_dev_last_plan(x.dev, &pi) == 0 && pi.group_form == 3;
				if (has_agg && G) {
					struct mdb_sort_key gk1;	/* (the key column as the GROUP BY operator read it: gathered already where the stream has row ids) */
					gk1.values = kv;
					gk1.nullbits = kn;
					gk1.rid = NULL;
					gk1.type = s->group[0]->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
					gk1.desc = 0;
					if ((rc = stream_aggregate(&x, &gk1, identity ? MDB_AGG_IDENTITY : 1, first, G)))
						goto out;
				}
				if (!identity && (rc = stream_select(&x, s->ntabs, first, G)))
					goto out;
			}
		} else if (s->ngroup > 1) {
			/* several fields: groups = distinct combinations (the reference applies its single-field loop once
			 * per field, executor_select.c:1537-1541, which is not a grouping by the combination: DESIGN.md 2) */
			struct mdb_sort_key gk[MDB_SORT_MAX_KEYS];
			uint32_t *first;
			uint64_t G = 0;
			for (int g = 0; g < s->ngroup; g++) {
				bind_operand(&x, s->group[g], &gk[g].values, &gk[g].nullbits, &gk[g].rid);
				gk[g].type = s->group[g]->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
				gk[g].desc = 0;
			}
			first = dalloc(&x, (x.n ? x.n : 1) * 4);
			x.d_count = dalloc(&x, (x.n ? x.n : 1) * 8);
			if (!first || !x.d_count) {
				rc = dev_fail(&x, "allocating group outputs");
				goto out;
			}
			if (x.n && mdb_dev_group_count_multi(x.dev, gk, s->ngroup, x.n, first, x.d_count, x.n, &G)) {
				rc = dev_fail(&x, "group count");
				goto out;
			}
			if (has_agg && G && (rc = stream_aggregate(&x, gk, s->ngroup, first, G)))
				goto out;
			{
				int64_t *cnt = x.d_count;	/* stream_select must not re-map the fresh counts */
				x.d_count = NULL;
				rc = stream_select(&x, s->ntabs, first, G);
				x.d_count = cnt;
				if (rc)
					goto out;
			}
		}
		/* SUM / MIN / MAX / AVG without GROUP BY: the whole stream is one group (an empty stream: no row, as SELECT COUNT(*) answers it) */
		if (has_agg && !s->ngroup && x.n && (rc = stream_aggregate(&x, NULL, 0, NULL, 1)))
			goto out;
	}

grouped:
	if (cat->dist && fused < 0 && has_count && !s->ngroup) {
		/* SELECT COUNT(*) [WHERE ...] in sharded mode: every rank reports the global count */
		uint64_t tot = x.n;
		if (mdb_dist_allreduce_sum_u64(cat->dist, &tot, 1)) {
			snprintf(err, errlen, "execution phase: %s\n", mdb_dist_last_error(cat->dist));
			rc = -MIDORIDB_INTERNAL;
			goto out;
		}
		x.n = tot;
	}
	if (cat->dist && fused >= 0 && s->distinct) {
		bool key_selected = false;
		for (int i = 0; i < s->nsel; i++)
			key_selected = key_selected || s->sel[i]->kind == MDB_EX_FIELD;
		if (!key_selected) {
			ERR("execution phase: sharded mode: DISTINCT over an aggregate alone cannot be answered from one rank's groups\n");
			rc = -MIDORIDB_ERROR;
			goto out;
		}
	}
	/* ---- HAVING -> DISTINCT -> ORDER BY -> LIMIT (SQL order of evaluation; extension) */
	if ((rc = select_tail(&x, has_count || has_agg)))
		goto out;

	/* ---- projection + COUNT-only handling */
	res = calloc(1, sizeof(*res));
	if (!res) {
		rc = -MIDORIDB_NOMEM;
		goto out;
	}
	{
		bool count_only = (has_count || has_agg) && !s->ngroup;	/* SELECT COUNT(*) [, SUM(v) ...] FROM ... [WHERE ...]: one row */
		uint64_t out_rows = count_only ? (x.n ? 1 : 0) : x.n;	/* the reference returns no row for an empty input */
		if (count_only && s->has_limit && (s->limit_off > 0 || s->limit_cnt == 0))
			out_rows = 0;
		const void **d_vals = calloc((size_t)(ncols ? ncols : 1), sizeof(void *));
		const uint64_t **d_nulls = calloc((size_t)(ncols ? ncols : 1), sizeof(uint64_t *));
		res->ncols = ncols;
		res->nrows = out_rows;
		res->colname = calloc((size_t)(ncols ? ncols : 1), sizeof(*res->colname));
		res->coltype = calloc((size_t)(ncols ? ncols : 1), sizeof(int));
		res->colprec = calloc((size_t)(ncols ? ncols : 1), sizeof(int));
		res->data = calloc((size_t)(ncols ? ncols : 1), sizeof(int64_t *));
		res->nullbits = calloc((size_t)(ncols ? ncols : 1), sizeof(uint64_t *));
		if (!d_vals || !d_nulls || !res->colname || !res->coltype || !res->colprec || !res->data || !res->nullbits) {
			free(d_vals);
			free(d_nulls);
			rc = -MIDORIDB_NOMEM;
			goto out;
		}
		const bool keep = cat->results_on_device && out_rows > 1;
		/* pass 1: where every result column lives on the device.  Columns read through a row-id vector are gathered -
		 * all of them in one launch per MDB_GATHER_MAX_COLS columns (mdb_dev_gather_cols), not one launch each */
		struct mdb_gather_col gl[MDB_GATHER_MAX_COLS];
		int ngl = 0, nrid = 0;
		const uint32_t *seen_rid[MDB_GATHER_MAX_RIDS];
		for (int c = 0; c < ncols && rc == MIDORIDB_OK; c++) {
			int key = src[c];
			memcpy(res->colname[c], keys[key], MDB_NAME_LEN);
			for (int i = 0; s->sel_alias && !s->select_all && i < s->nsel; i++)	/* `item AS name` names the column (the first alias of an item wins) */
				if (s->sel_alias[i][0] && (key_tbl[key] <= -2 ? s->sel[i]->kind == MDB_EX_AGG && agg_index(&x, s->sel[i]) == -2 - key_tbl[key]
							   : key_tbl[key] < 0 ? s->sel[i]->kind == MDB_EX_COUNT
									      : s->sel[i]->kind == MDB_EX_FIELD && s->sel[i]->tbl_idx == key_tbl[key] && s->sel[i]->col_idx == key_col[key])) {
					mdb_copy_name(res->colname[c], s->sel_alias[i]);
					break;
				}
			if (!keep) {	/* (a result kept on the device gets its host columns on first use, mdb_result_fetch) */
				res->data[c] = mdb_dev_host_alloc((size_t)(out_rows ? out_rows : 1) * 8);	/* pinned when large */
				if (!res->data[c]) {
					rc = -MIDORIDB_NOMEM;
					break;
				}
				if (out_rows <= 1)
					res->data[c][0] = 0;
			}
			if (key_tbl[key] <= -2) {	/* SUM / MIN / MAX / AVG: an ordinary typed column with its NULL bitmap - one row without GROUP BY */
				const int a = -2 - key_tbl[key];
				res->coltype[c] = x.agg_type[a];
				if (out_rows) {
					if (!x.d_agg[a]) {
						ERR("execution phase: internal error (aggregate not computed)\n");
						rc = -MIDORIDB_INTERNAL;
						break;
					}
					d_vals[c] = x.d_agg[a];
					d_nulls[c] = x.d_agg_nulls[a];
				}
				continue;
			}
			if (key_tbl[key] < 0) {
				res->coltype[c] = MDB_CT_INTEGER;
				if (count_only) {
					if (out_rows)
						res->data[c][0] = (int64_t)x.n;
				} else if (out_rows) {
					if (!x.d_count) {	/* COUNT without aggregation cannot reach here (S4) */
						ERR("execution phase: internal error\n");
						rc = -MIDORIDB_INTERNAL;
						break;
					}
					d_vals[c] = x.d_count;
				}
				continue;
			}
			struct mdb_column *col = &s->tabs[key_tbl[key]].t->cols[key_col[key]];
			res->coltype[c] = col->type;
			res->colprec[c] = col->type == MDB_CT_VARCHAR ? col->precision : 0;
			if (!out_rows || count_only)
				continue;
			if (fused >= 0 || x.fused) {
				/* only the group key can be selected (S4); both sides hold the same value.  A composite key: the field's key column */
				d_vals[c] = fused_key_column(&x, key_tbl[key], key_col[key]);
				continue;
			}
			if (direct_vals) {			/* scan + WHERE + projection plan: the columns are final already */
				d_vals[c] = direct_vals[c];
				d_nulls[c] = direct_nulls[c];
				continue;
			}
			int from_tbl = key_tbl[key];
			const struct mdb_column *from = col;
			while (x.same_col[from_tbl] == (int)(from - s->tabs[from_tbl].t->cols)) {	/* the join key of a joined table: read the earlier table's column */
				const int t2 = x.same_as_tbl[from_tbl];
				from = &s->tabs[t2].t->cols[x.same_as_col[from_tbl]];
				from_tbl = t2;
			}
			const bool aliased = from != col;
			const uint64_t *src_nb = aliased ? NULL : from->d_nullbits;
			const uint32_t *rid = x.rid[from_tbl];
			if (!rid) {
				d_vals[c] = from->d_data;
				d_nulls[c] = aliased ? NULL : from->d_nullbits;
				continue;
			}
			const void *src_vals = from->d_data;
			if (!src_vals && !(src_vals = dalloc(&x, 8))) {	/* (an empty table under an outer join: every tuple is at "no row", no cell is read) */
				rc = dev_fail(&x, "projection gather");
				break;
			}
			{
				/* the same column through the same row ids twice (SELECT * after an equi-join: both key columns): gathered once */
				int g = 0;
				while (g < ngl && !(gl[g].src == src_vals && gl[g].rid == rid && gl[g].src_nullbits == src_nb))
					g++;
				if (g < ngl) {
					d_vals[c] = gl[g].dst;
					d_nulls[c] = gl[g].dst_nullbits;
					continue;
				}
			}
			{
				int t = 0;
				while (t < nrid && seen_rid[t] != rid)
					t++;
				if (ngl == MDB_GATHER_MAX_COLS || (t == nrid && nrid == MDB_GATHER_MAX_RIDS)) {
					if (mdb_dev_gather_cols(x.dev, gl, ngl, out_rows)) {
						rc = dev_fail(&x, "projection gather");
						break;
					}
					ngl = nrid = 0;
					t = 0;
				}
				if (t == nrid)
					seen_rid[nrid++] = rid;
			}
			int64_t *v = dalloc(&x, out_rows * 8);
			const bool want_nb = src_nb || x.may_be_absent[from_tbl];	/* (a tuple without a row of the table: its cells are NULL) */
			uint64_t *nb = want_nb ? dalloc(&x, ((out_rows + 63) / 64) * 8) : NULL;
			if (!v || (want_nb && !nb)) {
				rc = dev_fail(&x, "projection gather");
				break;
			}
			gl[ngl].src = src_vals;
			gl[ngl].src_nullbits = src_nb;
			gl[ngl].rid = rid;
			gl[ngl].dst = v;
			gl[ngl].dst_nullbits = nb;
			ngl++;
			d_vals[c] = v;
			d_nulls[c] = nb;
		}
		if (rc == MIDORIDB_OK && ngl && mdb_dev_gather_cols(x.dev, gl, ngl, out_rows))
			rc = dev_fail(&x, "projection gather");
		/* pass 2: device -> host - or, with results kept on the device (mdb_database_results_on_device), the device columns
		 * become the result's own: a buffer of this statement changes hands, a base-table column is copied on the device */
		res->fetched = !keep;
		if (keep) {
			res->dev = x.dev;
			res->d_data = calloc((size_t)(ncols ? ncols : 1), sizeof(void *));
			res->d_nullbits = calloc((size_t)(ncols ? ncols : 1), sizeof(uint64_t *));
			if (!res->d_data || !res->d_nullbits)
				rc = -MIDORIDB_NOMEM;
		}
		for (int c = 0; c < ncols && rc == MIDORIDB_OK; c++) {
			if (!d_vals[c] || !out_rows)
				continue;
			if (!keep) {
				if (result_column_to_host(x.dev, res, c, d_vals[c], d_nulls[c]))
					rc = dev_fail(&x, "reading a result column");
				continue;
			}
			for (int pass = 0; pass < 2 && rc == MIDORIDB_OK; pass++) {
				const void *src = pass ? (const void *)d_nulls[c] : d_vals[c];
				const size_t bytes = pass ? (size_t)((out_rows + 63) / 64) * 8 : (size_t)out_rows * 8;
				void *own = NULL;
				bool shared = false;
				if (!src)
					continue;
				/* the same device column under two result columns (both key columns of SELECT * over an equi-join): ONE buffer of the
				 * result serves both - query_column_data_device() hands out read-only columns - instead of a copy each (0.3 ms per
				 * 10^8-row column) */
				for (int k = 0; k < c && !own; k++) {
					if (d_vals[k] == src && res->d_data[k])
						own = res->d_data[k];
					else if ((const void *)d_nulls[k] == src && res->d_nullbits[k])
						own = res->d_nullbits[k];
				}
				if (own) {
					if (pass)
						res->d_nullbits[c] = own;
					else
						res->d_data[c] = own;
					continue;
				}
				/* (a statement buffer sized for the worst case - every left row a group - must not pin hundreds of megabytes
				 * behind a small result until query_free: such a column is copied into a buffer of its own size instead) */
				for (int i = 0; i < x.bufs.n && !shared; i++)
					if (x.bufs.p[i] == src) {
						if (mdb_dev_alloc_size(x.dev, src) > 4 * bytes + ((size_t)1 << 20))
							break;
						own = x.bufs.p[i];
						x.bufs.p[i] = x.bufs.p[--x.bufs.n];
						break;
					}
				/* a base table's own device column, all of its rows in order (no row ids between): the result becomes one more holder
				 * of the buffer instead of copying it (0.04 ms per 10^7-row column, 0.3 per 10^8) - result columns are read-only, rows
				 * appended later lie behind the result's, and an UPDATE copies a column that has other holders before it writes */
				if (!own && !shared && mdb_dev_alloc_size(x.dev, src) >= bytes &&
				    !mdb_knob_off("MDB_RESULT_ALIAS")) {
					bool stmt_buf = false;
					for (int i = 0; i < x.bufs.n; i++)
						stmt_buf = stmt_buf || x.bufs.p[i] == src;
					if (!stmt_buf && mdb_dev_retain(x.dev, src) == 0)
						own = (void *)src;
				}
				if (!own) {
					if (mdb_dev_alloc(x.dev, bytes, &own) || mdb_dev_gather64(x.dev, src, NULL, NULL, bytes / 8, own, NULL)) {
						rc = dev_fail(&x, "keeping a result column on the device");
						break;
					}
				}
				if (pass)
					res->d_nullbits[c] = own;
				else
					res->d_data[c] = own;
			}
		}
		if (keep && rc == MIDORIDB_OK && mdb_dev_sync(x.dev))
			rc = dev_fail(&x, "result columns");
		free(d_vals);
		free(d_nulls);
		if (rc)
			goto out;
	}
	res->dict = &cat->dict;
	mdb_result_legacy_header(res);		/* the reference's struct table in front of the columnar result (include/mdb_legacy.h) ... */
	mdb_result_legacy_rows(res);		/* ... and, for a small result whose columns are on the host, its rows as datablocks */
	res->exec_ms = now_ms() - t0 + sub_ms;
	res->joined_rows = x.joined_rows;
	*out = res;
	res = NULL;
	rc = MIDORIDB_OK;
out:
	cat->joins_eliminated += (uint64_t)x.joins_eliminated;
	cat->composite_joins += (uint64_t)x.composite_joins;
	cat->composite_fused += (uint64_t)x.composite_fused;
	cat->aggregate_calls[0] += (uint64_t)x.agg_calls[0];
	cat->aggregate_calls[1] += (uint64_t)x.agg_calls[1];
	shard_cleanup(&x);
	subqueries_release(cat, s->where);
	subqueries_release(cat, s->having);
	free_all(&x);
	mdb_result_free(res);
	free(keys);
	free(order);
	free(key_tbl);
	free(key_col);
	free(src);
	free(direct_vals);
	free(direct_nulls);
	return rc;
}
