/*
 * mdb_exec_result.c - result assembly of the SELECT executor: the projection of the final stream onto the result columns, results on
 * the host or kept on the device, and the result's life after the statement.
 */
#include "mdb_exec_internal.h"

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

/* ------------------------------------------------------------------ projection: the final stream onto the result columns
 *
 * Pass 1 finds where every result column lives on the device; columns read through a row-id vector are gathered, all of them in one launch
 * per MDB_GATHER_MAX_COLS columns or MDB_GATHER_MAX_RIDS row-id vectors (mdb_dev_gather_cols), not one launch each.  Pass 2 brings the
 * columns to the host - or, with results kept on the device (mdb_database_results_on_device), makes them the result's own. */
struct projection {
	uint64_t out_rows;
	bool count_only;		/* SELECT COUNT(*) [, SUM(v) ...] FROM ... [WHERE ...]: one row */
	bool keep;			/* the result's columns stay on the device; it gets its host columns on first use (mdb_result_fetch) */
	const void **d_vals;		/* per result column: where it lives on the device; NULL: nowhere - its host cell is final */
	const uint64_t **d_nulls;
	struct mdb_gather_col gl[MDB_GATHER_MAX_COLS];	/* the gather batch, and the row-id vectors it reads through */
	int ngl, nrid;
	const uint32_t *seen_rid[MDB_GATHER_MAX_RIDS];
};

static int result_alloc(struct mdb_result *res, struct projection *pj, int ncols)
{
	const size_t n = (size_t)(ncols ? ncols : 1);
	pj->d_vals = calloc(n, sizeof(void *));
	pj->d_nulls = calloc(n, sizeof(uint64_t *));
	res->ncols = ncols;
	res->nrows = pj->out_rows;
	res->colname = calloc(n, sizeof(*res->colname));
	res->coltype = calloc(n, sizeof(int));
	res->colprec = calloc(n, sizeof(int));
	res->data = calloc(n, sizeof(int64_t *));
	res->nullbits = calloc(n, sizeof(uint64_t *));
	if (!pj->d_vals || !pj->d_nulls || !res->colname || !res->coltype || !res->colprec || !res->data || !res->nullbits)
		return -MIDORIDB_NOMEM;
	return MIDORIDB_OK;
}

/* does select-list item e deliver result column c? */
static bool item_is_column(const struct exec *x, const struct result_cols *rc, int c, const struct mdb_expr *e)
{
	const int key = rc->src[c], tbl = rc->tbl[key];
	return colsrc_win(tbl) >= 0  ? e->kind == MDB_EX_WINDOW && e->win_idx == colsrc_win(tbl)
	       : colsrc_agg(tbl) >= 0  ? e->kind == MDB_EX_AGG && agg_index(x, e) == colsrc_agg(tbl)
	       : tbl == COLSRC_COUNT ? e->kind == MDB_EX_COUNT
				     : e->kind == MDB_EX_FIELD && e->tbl_idx == tbl && e->col_idx == rc->col[key];
}

/* result column c's name: its candidate's, or the alias of its select-list item (`item AS name`; the first alias of an item wins) */
void result_column_name(const struct exec *x, const struct result_cols *rc, int c, char *out)
{
	const struct mdb_select *s = x->s;
	memcpy(out, rc->keys[rc->src[c]], MDB_NAME_LEN);
	for (int i = 0; s->sel_alias && !s->select_all && i < s->nsel; i++)
		if (s->sel_alias[i][0] && item_is_column(x, rc, c, s->sel[i])) {
			mdb_copy_name(out, s->sel_alias[i]);
			break;
		}
}

/* where result column c stands in the statement's select list: the index of the first item that delivers it; for SELECT * its place among
 * the FROM tables' columns, left to right.  (The result's own column order is the reference's, R3 - not the list's.) */
int result_column_list_place(const struct exec *x, const struct result_cols *rc, int c)
{
	const struct mdb_select *s = x->s;
	for (int i = 0; !s->select_all && i < s->nsel; i++)
		if (item_is_column(x, rc, c, s->sel[i]))
			return i;
	return rc->src[c];
}

/* result column c's column type: an aggregate's or a window item's result type, INTEGER for COUNT(*), else its table column's */
int result_column_type(const struct exec *x, const struct result_cols *rc, int c)
{
	const int key = rc->src[c], tbl = rc->tbl[key];
	if (colsrc_agg(tbl) >= 0)
		return x->agg_type[colsrc_agg(tbl)];
	if (colsrc_win(tbl) >= 0)
		return x->win_item[colsrc_win(tbl)]->type;
	if (tbl == COLSRC_COUNT)
		return MDB_CT_INTEGER;
	return x->s->tabs[tbl].t->cols[rc->col[key]].type;
}

/* result column c's name and, for a result that goes to the host, its host column */
static int result_column_open(const struct exec *x, const struct result_cols *rc, struct mdb_result *res, const struct projection *pj, int c)
{
	result_column_name(x, rc, c, res->colname[c]);
	if (!pj->keep) {
		res->data[c] = mdb_dev_host_alloc((size_t)(pj->out_rows ? pj->out_rows : 1) * 8);	/* pinned when large */
		if (!res->data[c])
			return -MIDORIDB_NOMEM;
		if (pj->out_rows <= 1)
			res->data[c][0] = 0;
	}
	return MIDORIDB_OK;
}

static int gather_flush(struct exec *x, struct projection *pj)
{
	if (pj->ngl && mdb_dev_gather_cols(x->dev, pj->gl, pj->ngl, pj->out_rows))
		return dev_fail(x, "projection gather");
	pj->ngl = pj->nrid = 0;
	return MIDORIDB_OK;
}

/* result column c is column (src_vals, src_nb) read through rid: into the gather batch, which is flushed first when it is full */
static int gather_add(struct exec *x, struct projection *pj, int c, const void *src_vals, const uint64_t *src_nb, const uint32_t *rid, bool may_be_absent)
{
	const uint64_t out_rows = pj->out_rows;
	int t = 0, rc;
	/* the same column through the same row ids twice (SELECT * after an equi-join: both key columns): gathered once */
	for (int g = 0; g < pj->ngl; g++)
		if (pj->gl[g].src == src_vals && pj->gl[g].rid == rid && pj->gl[g].src_nullbits == src_nb) {
			pj->d_vals[c] = pj->gl[g].dst;
			pj->d_nulls[c] = pj->gl[g].dst_nullbits;
			return MIDORIDB_OK;
		}
	while (t < pj->nrid && pj->seen_rid[t] != rid)
		t++;
	if (pj->ngl == MDB_GATHER_MAX_COLS || (t == pj->nrid && pj->nrid == MDB_GATHER_MAX_RIDS)) {
		if ((rc = gather_flush(x, pj)))
			return rc;
		t = 0;
	}
	if (t == pj->nrid)
		pj->seen_rid[pj->nrid++] = rid;
	int64_t *v = dalloc(x, out_rows * 8);
	const bool want_nb = src_nb || may_be_absent;	/* (a tuple without a row of the table: its cells are NULL) */
	uint64_t *nb = want_nb ? dalloc(x, ((out_rows + 63) / 64) * 8) : NULL;
	if (!v || (want_nb && !nb))
		return dev_fail(x, "projection gather");
	pj->gl[pj->ngl].src = src_vals;
	pj->gl[pj->ngl].src_nullbits = src_nb;
	pj->gl[pj->ngl].rid = rid;
	pj->gl[pj->ngl].dst = v;
	pj->gl[pj->ngl].dst_nullbits = nb;
	pj->ngl++;
	pj->d_vals[c] = v;
	pj->d_nulls[c] = nb;
	return MIDORIDB_OK;
}

/* pass 1 for result column c: its type, and where it lives on the device */
static int locate_column(struct exec *x, const struct select_stmt *st, struct mdb_result *res, struct projection *pj, int c)
{
	struct mdb_select *s = x->s;
	const int key = st->rc.src[c], tbl = st->rc.tbl[key], a = colsrc_agg(tbl);
	res->coltype[c] = result_column_type(x, &st->rc, c);
	if (a >= 0) {	/* SUM / MIN / MAX / AVG: an ordinary typed column with its NULL bitmap - one row without GROUP BY */
		if (pj->out_rows) {
			if (!x->d_agg[a]) {
				snprintf(x->err, x->errlen, "execution phase: internal error (aggregate not computed)\n");
				return -MIDORIDB_INTERNAL;
			}
			pj->d_vals[c] = x->d_agg[a];
			pj->d_nulls[c] = x->d_agg_nulls[a];
		}
		return MIDORIDB_OK;
	}
	if (colsrc_win(tbl) >= 0) {	/* a window item: a typed column with its NULL bitmap, one row per row of the stream */
		const int w = colsrc_win(tbl);
		const struct mdb_expr *e = x->win_item[w];
		if (e->type == MDB_CT_VARCHAR && e->tbl_idx >= 0 && e->col_idx >= 0)	/* (LAG ... of a VARCHAR column: its cells, its precision) */
			res->colprec[c] = s->tabs[e->tbl_idx].t->cols[e->col_idx].precision;
		if (pj->out_rows) {
			if (!x->d_win[w]) {
				snprintf(x->err, x->errlen, "execution phase: internal error (window function not computed)\n");
				return -MIDORIDB_INTERNAL;
			}
			pj->d_vals[c] = x->d_win[w];
			pj->d_nulls[c] = x->d_win_nulls[w];
		}
		return MIDORIDB_OK;
	}
	if (tbl == COLSRC_COUNT) {
		if (pj->count_only) {
			if (pj->out_rows)
				res->data[c][0] = (int64_t)x->n;
		} else if (pj->out_rows) {
			if (!x->d_count) {	/* COUNT without aggregation cannot reach here (S4) */
				snprintf(x->err, x->errlen, "execution phase: internal error\n");
				return -MIDORIDB_INTERNAL;
			}
			pj->d_vals[c] = x->d_count;
		}
		return MIDORIDB_OK;
	}
	const int col_idx = st->rc.col[key];
	struct mdb_column *col = &s->tabs[tbl].t->cols[col_idx];
	res->colprec[c] = col->type == MDB_CT_VARCHAR ? col->precision : 0;
	if (!pj->out_rows || pj->count_only)
		return MIDORIDB_OK;
	if (stream_is_keys(x)) {
		/* only the group key can be selected (S4); both sides hold the same value.  A composite key: the field's key column */
		pj->d_vals[c] = fused_key_column(x, tbl, col_idx);
		return MIDORIDB_OK;
	}
	if (st->direct_vals) {			/* scan + WHERE + projection plan: the columns are final already */
		pj->d_vals[c] = st->direct_vals[c];
		pj->d_nulls[c] = st->direct_nulls[c];
		return MIDORIDB_OK;
	}
	int from_tbl = tbl;
	const struct mdb_column *from = col;
	while (x->same_col[from_tbl] == (int)(from - s->tabs[from_tbl].t->cols)) {	/* the join key of a joined table: read the earlier table's column */
		const int t2 = x->same_as_tbl[from_tbl];
		from = &s->tabs[t2].t->cols[x->same_as_col[from_tbl]];
		from_tbl = t2;
	}
	const bool aliased = from != col;
	const uint64_t *src_nb = aliased ? NULL : from->d_nullbits;
	const uint32_t *rid = x->rid[from_tbl];
	if (!rid) {
		pj->d_vals[c] = from->d_data;
		pj->d_nulls[c] = src_nb;
		return MIDORIDB_OK;
	}
	const void *src_vals = from->d_data;
	if (!src_vals && !(src_vals = dalloc(x, 8)))	/* (an empty table under an outer join: every tuple is at "no row", no cell is read) */
		return dev_fail(x, "projection gather");
	return gather_add(x, pj, c, src_vals, src_nb, rid, x->may_be_absent[from_tbl]);
}

/* pass 2, a result for the host */
static int result_columns_to_host(struct exec *x, struct mdb_result *res, const struct projection *pj)
{
	for (int c = 0; c < res->ncols; c++)
		if (pj->d_vals[c] && pj->out_rows && result_column_to_host(x->dev, res, c, pj->d_vals[c], pj->d_nulls[c]))
			return dev_fail(x, "reading a result column");
	return MIDORIDB_OK;
}

/* The result's own buffer for the device column src (bytes long; it serves result column c), in this order:
 *  - the same device column under an earlier result column (both key columns of SELECT * over an equi-join): ONE buffer of the result
 *    serves both - query_column_data_device() hands out read-only columns - instead of a copy each (0.3 ms per 10^8-row column);
 *  - a buffer of this statement changes hands - unless it was sized for the worst case (every left row a group) and would pin hundreds
 *    of megabytes behind a small result until query_free: such a column is copied into a buffer of its own size;
 *  - a base table's own device column, all of its rows in order (no row ids between): the result becomes one more holder of the buffer
 *    instead of copying it (0.04 ms per 10^7-row column, 0.3 per 10^8) - result columns are read-only, rows appended later lie behind
 *    the result's, and an UPDATE copies a column that has other holders before it writes;
 *  - a copy on the device. */
static int result_own_buffer(struct exec *x, const struct mdb_result *res, const struct projection *pj, int c, const void *src, size_t bytes, void **out)
{
	void *own = NULL;
	bool stmt_buf = false;
	for (int k = 0; k < c && !own; k++) {
		if (pj->d_vals[k] == src && res->d_data[k])
			own = res->d_data[k];
		else if ((const void *)pj->d_nulls[k] == src && res->d_nullbits[k])
			own = res->d_nullbits[k];
	}
	for (int i = 0; i < x->bufs.n && !own && !stmt_buf; i++)
		if (x->bufs.p[i] == src) {
			stmt_buf = true;
			if (mdb_dev_alloc_size(x->dev, src) > 4 * bytes + ((size_t)1 << 20))
				break;
			own = x->bufs.p[i];
			x->bufs.p[i] = x->bufs.p[--x->bufs.n];
		}
	if (!own && !stmt_buf && mdb_dev_alloc_size(x->dev, src) >= bytes && !mdb_knob_off("MDB_RESULT_ALIAS") && mdb_dev_retain(x->dev, src) == 0)
		own = (void *)src;
	if (!own && (mdb_dev_alloc(x->dev, bytes, &own) || mdb_dev_gather64(x->dev, src, NULL, NULL, bytes / 8, own, NULL)))
		return dev_fail(x, "keeping a result column on the device");
	*out = own;
	return MIDORIDB_OK;
}

/* pass 2, a result kept on the device: the device columns become the result's own */
static int result_take_columns(struct exec *x, struct mdb_result *res, const struct projection *pj)
{
	const size_t n = (size_t)(res->ncols ? res->ncols : 1);
	int rc;
	res->dev = x->dev;
	res->d_data = calloc(n, sizeof(void *));
	res->d_nullbits = calloc(n, sizeof(uint64_t *));
	if (!res->d_data || !res->d_nullbits)
		return -MIDORIDB_NOMEM;
	for (int c = 0; c < res->ncols; c++) {
		void *own;
		if (!pj->d_vals[c] || !pj->out_rows)
			continue;
		if ((rc = result_own_buffer(x, res, pj, c, pj->d_vals[c], (size_t)pj->out_rows * 8, &own)))
			return rc;
		res->d_data[c] = own;
		if (!pj->d_nulls[c])
			continue;
		if ((rc = result_own_buffer(x, res, pj, c, pj->d_nulls[c], (size_t)((pj->out_rows + 63) / 64) * 8, &own)))
			return rc;
		res->d_nullbits[c] = own;
	}
	return mdb_dev_sync(x->dev) ? dev_fail(x, "result columns") : MIDORIDB_OK;
}

/* the statement's final stream -> res: result columns named, typed and filled (or, kept on the device, owned) */
int project_result(struct exec *x, const struct select_stmt *st, struct mdb_result *res)
{
	const struct mdb_select *s = x->s;
	struct projection pj;
	int rc;
	memset(&pj, 0, sizeof(pj));
	pj.count_only = (st->rc.has_count || st->has_agg) && !s->ngroup;
	pj.out_rows = pj.count_only ? (x->n ? 1 : 0) : x->n;	/* the reference returns no row for an empty input */
	if (pj.count_only && s->has_limit && (s->limit_off > 0 || s->limit_cnt == 0))
		pj.out_rows = 0;
	pj.keep = x->cat->results_on_device && pj.out_rows > 1;
	rc = result_alloc(res, &pj, st->rc.ncols);
	for (int c = 0; c < st->rc.ncols && !rc; c++)
		if (!(rc = result_column_open(x, &st->rc, res, &pj, c)))
			rc = locate_column(x, st, res, &pj, c);
	if (!rc)
		rc = gather_flush(x, &pj);
	res->fetched = !pj.keep;
	if (!rc)
		rc = pj.keep ? result_take_columns(x, res, &pj) : result_columns_to_host(x, res, &pj);
	free(pj.d_vals);
	free(pj.d_nulls);
	return rc;
}
