/*
 * mdb_exec_join.c - the join side of the SELECT executor: one more FROM table into the tuple stream (join_next_table and its shortcuts,
 * the outer joins), packed composite join keys, and the fused plan on a composite key.
 */
#include "mdb_exec_internal.h"

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
bool join_is_total_by_catalog(struct exec *x, const struct mdb_expr *kl, const struct mdb_expr *kr)
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
bool only_key_needed(const struct exec *x, int t, int key_col)
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

/* The join of table t when EVERY row of the stream finds exactly one partner in it (a foreign key to a primary key) and the statement
 * reads at most two other columns of t, neither with NULLs: mdb_dev_join_payload carries those cells through t's one partition level
 * and delivers them in stream order - no partner row ids, no compaction, no random gather in the projection (BASELINE configs[1]).
 * Table t is then read through a SHADOW (like a table that arrived over the wire in sharded mode): its key column is the stream's own
 * key column, its payload columns are the carried cells, its row-id vector the identity.  0 = done, 1 = not such a join (nothing
 * changed: the pairs path answers), < 0 = error. */
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
int composite_fused_plan(struct exec *x, const struct where_split *ws, bool only_count)
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
	x->plan = STREAM_FUSED_COMPOSITE;
	x->n = only_count ? J : G;
	x->joined_rows = J;
	return 0;
}

/* ------------------------------------------------------------------ one more table into the stream: what inner and outer joins share */

/* the first ON conjunct `field of an earlier table = field of table t` - the hash key: its index, its sides in *kl (the stream's) and *kr
 * (table t's); -1: there is none */
static int equi_key_conjunct(struct mdb_expr *const *conj, int nconj, int t, const struct mdb_expr **kl, const struct mdb_expr **kr)
{
	for (int i = 0; i < nconj; i++) {
		const struct mdb_expr *c = conj[i];
		if (c->kind != MDB_EX_CMP || c->op != MDB_CMP_EQ || c->kids[0]->kind != MDB_EX_FIELD || c->kids[1]->kind != MDB_EX_FIELD)
			continue;
		const struct mdb_expr *a = c->kids[0], *b = c->kids[1];
		if (a->tbl_idx < t && b->tbl_idx == t) {
			*kl = a;
			*kr = b;
			return i;
		}
		if (b->tbl_idx < t && a->tbl_idx == t) {
			*kl = b;
			*kr = a;
			return i;
		}
	}
	return -1;
}

/* the key columns of both sides of the join on kl = kr: the stream's (vl, nl) and table t's rows rsel[0 .. r_rows) (NULL: all; vr, nr).
 * DOUBLE keys as their IEEE-canonical words (double_join_keys), every other type the column itself, gathered where row ids say so */
static int join_key_columns(struct exec *x, int t, const struct mdb_expr *kl, const struct mdb_expr *kr, const uint32_t *rsel, uint64_t r_rows,
			    const int64_t **vl, const uint64_t **nl, const void **vr, const uint64_t **nr)
{
	struct mdb_select *s = x->s;
	int rc;
	if (kl->type == MDB_CT_DOUBLE) {
		const void *dl;
		if ((rc = double_join_keys(x, &s->tabs[kl->tbl_idx].t->cols[kl->col_idx], x->rid[kl->tbl_idx], x->n, &dl, nl)) ||
		    (rc = double_join_keys(x, &s->tabs[t].t->cols[kr->col_idx], rsel, r_rows, vr, nr)))
			return rc;
		*vl = dl;
		return MIDORIDB_OK;
	}
	if ((rc = stream_column(x, kl, vl, nl)))
		return rc;
	return table_column(x, t, kr, rsel, r_rows, vr, nr);
}

/* positions pos[0 .. n) in the filtered rows rsel of a table -> row ids of the base table */
static int rows_to_base(struct exec *x, const uint32_t *rsel, const uint32_t *pos, uint64_t n, uint32_t **out)
{
	uint32_t *mapped = dalloc(x, n * 4);
	if (!mapped || mdb_dev_gather32(x->dev, rsel, pos, n, mapped))
		return dev_fail(x, "re-mapping row ids");
	*out = mapped;
	return MIDORIDB_OK;
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
	if (!comp)
		key = equi_key_conjunct(conj, nconj, t, &kl, &kr);
	for (int i = 0; i < nconj; i++) {
		struct mdb_expr *c = conj[i];
		if (comp && ((ck.mask >> i) & 1u))
			key = i;
		if (i == key)
			continue;
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
		} else if ((rc = join_key_columns(x, t, kl, kr, rsel, r_rows, &vl, &nl, &vr, &nr))) {
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
		x->rid[t] = pt;
		if (!rc && rsel)
			rc = rows_to_base(x, rsel, pt, J, &x->rid[t]);
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
		if ((rc = rows_to_base(x, rsel, ct, total, &ct)))
			return rc;
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

/* Join elimination for table t joined on kl = kr, the whole ON clause, nothing of t filtered: the catalog says every row of the stream has
 * exactly one partner, and only t's key is read.  0 = the table needs no join, 1 = it does, < 0 = error */
static int join_eliminate(struct exec *x, int t, const struct mdb_expr *kl, const struct mdb_expr *kr, int nconj, int npconj)
{
	const int64_t *vl;
	const uint64_t *nl;
	int rc;
	if (nconj != 1 || npconj || x->cat->dist || !x->n || x->nagg /* (SUM / MIN / MAX / AVG: the materialising join, always) */ ||
	    !only_key_needed(x, t, kr->col_idx) || !join_is_total_by_catalog(x, kl, kr))
		return 1;
	if ((rc = stream_column(x, kl, &vl, &nl)))
		return rc;
	if (nl)
		return 1;
	x->same_col[t] = kr->col_idx;
	x->same_as_tbl[t] = kl->tbl_idx;
	x->same_as_col[t] = kl->col_idx;
	x->joins_eliminated++;
	return payload_shadow(x, t, kr->col_idx, vl, NULL, 0, NULL);
}

/* Sharded mode: both sides of the join of table t go where their join key hashes to - the left stream unless it already is there (joined
 * on this key before), the new table always (its rows *rsel[0 .. *r_rows) that passed its own WHERE conjuncts at home).  No equi-join key
 * (kl == NULL: FROM A, B; a general ON expression: reference executor_select.c:1096-1141): nothing says which rank a row's partners
 * live on - the new table is replicated on every rank and each rank pairs ITS stream with all of it: every (l, r) pair is produced exactly
 * once, where l lives.  Afterwards table t is the shadow of the rows this rank received: all *r_rows of them, *rsel = NULL. */
static int shard_join_sides(struct exec *x, int t, const struct mdb_expr *kl, const struct mdb_expr *kr, const uint32_t **rsel, uint64_t *r_rows)
{
	const int tabs1[1] = { t };
	uint32_t *rids1[1] = { (uint32_t *)*rsel };
	const void *kv;
	const uint64_t *kn;
	int rc;
	if (!kl) {
		if ((rc = shard_rows(x, tabs1, 1, rids1, *r_rows, NULL, NULL, SHARD_BROADCAST, r_rows)))
			return rc;
		*rsel = NULL;
		return MIDORIDB_OK;
	}
	if (!in_part(x, kl) && (rc = shard_stream(x, t, kl, 0)))
		return rc;
	if (kr->type == MDB_CT_DOUBLE)
		rc = double_join_keys(x, &x->s->tabs[t].t->cols[kr->col_idx], *rsel, *r_rows, &kv, &kn);
	else
		rc = table_column(x, t, kr, *rsel, *r_rows, &kv, &kn);
	if (!rc && kr->type == MDB_CT_VARCHAR) {	/* (rows go where their STRING hashes to: the ranks' common id of it) */
		const int64_t *common = NULL;
		rc = shard_ids(x, kv, *r_rows, true, false, &common);
		kv = common;
	}
	if (rc || (rc = shard_rows(x, tabs1, 1, rids1, *r_rows, kv, kn, 0, r_rows)))
		return rc;
	*rsel = NULL;
	if (x->npart < 2 * MDB_MAX_TABS)
		x->part[x->npart++] = kr;
	return MIDORIDB_OK;
}

/* The inner join's carried-payload shortcuts for table t joined on kl = kr (conjunct `key` of the ON clause): several tables on one key in
 * one call, then table t alone; the other ON conjuncts filter the merged tuples.  0 = joined, 1 = neither served (nothing changed), < 0 =
 * error.  The catalog's statistics (op_stats_begin) stay handed over when 1 is returned. */
static int join_carrying_payload(struct exec *x, int t, struct mdb_expr *const *conj, int nconj, int key, const struct mdb_expr *kl, const struct mdb_expr *kr,
				 const int64_t *vl, const uint64_t *nl, const void *vr, const uint64_t *nr, uint64_t r_rows)
{
	int rc, prc = nconj == 1 ? join_with_payload_multi(x, t, kl, kr, vl, nl, vr, nr, r_rows) : 1;
	if (prc == 1)
		prc = join_with_payload(x, t, kr, vl, nl, vr, nr, r_rows);
	if (prc <= 0)
		op_stats_end(x);
	if (prc)
		return prc;
	for (int i = 0; i < nconj; i++)		/* residual ON conjuncts, on the merged tuples */
		if (i != key && (rc = stream_filter(x, t + 1, conj[i])))
			return rc;
	if (nconj > 1)
		x->joined_rows = x->n;
	return 0;
}

/* None of the one-key shortcuts served: several equalities of the ON clause as ONE packed key, when composite_join_plan's rule says so.
 * 0 = the key operands are the packed columns now (*answered = the conjuncts they answer; ck->empty: nothing can match, no operands),
 * 1 = the join stays on its one key, < 0 = error */
static int join_on_composite_key(struct exec *x, int t, struct mdb_expr *const *conj, int nconj, const uint32_t *rsel, uint64_t r_rows, struct composite_key *ck,
				 uint32_t *answered, const int64_t **vl, const uint64_t **nl, const void **vr, const uint64_t **nr)
{
	int rc;
	const int crc = composite_join_plan(x, t, conj, nconj, ck);
	if (crc <= 0)
		op_stats_end(x);
	if (crc)
		return crc;
	if ((rc = composite_join_pack(x, t, ck, rsel, r_rows)))
		return rc;
	*answered = ck->mask;
	*vl = ck->vl;
	*nl = ck->nl;
	*vr = ck->vr;
	*nr = ck->nr;
	if (!ck->empty)
		(void)mdb_dev_call_stats(x->dev, *vl, &ck->st[0], *vr, &ck->st[1]);
	return 0;
}

/* all pairs of the stream's rows and table t's r_rows rows (no equi-join key: FROM A, B (ON 1=1) or a general ON, which filters them afterwards) */
static int join_cross_pairs(struct exec *x, uint64_t r_rows, uint32_t **pl, uint32_t **pr, uint64_t *J)
{
	const uint64_t total = x->n * r_rows;
	uint64_t too_large = total > (1ull << 28) ? 1u : 0u;
	if (x->cat->dist && mdb_dist_allreduce_sum_u64(x->cat->dist, &too_large, 1))	/* (every rank must leave the statement together) */
		return dist_fail(x, NULL);
	if (too_large) {
		snprintf(x->err, x->errlen, "execution phase: cross join of %llu x %llu rows is too large (no equi-join key in the ON clause)\n",
			 (unsigned long long)x->n, (unsigned long long)r_rows);
		return -MIDORIDB_ERROR;
	}
	*J = total;
	if (total) {
		*pl = dalloc(x, total * 4);
		*pr = dalloc(x, total * 4);
		if (!*pl || !*pr)
			return dev_fail(x, "allocating join pairs");
		if (mdb_dev_cross_pairs(x->dev, x->n, r_rows, *pl, *pr))
			return dev_fail(x, "cross join");
	}
	return MIDORIDB_OK;
}

/* S [INNER] JOIN T ON c: the stream of the tables joined so far with table t (its rows that pass its own WHERE conjuncts pconj).  With an
 * equi-join key in the ON clause the shortcuts are tried in this order, each 0 = done / 1 = not this way: join elimination, carried
 * payload (several tables, then one), a packed composite key, and the pair operator, which always answers. */
int join_next_table(struct exec *x, int t, const struct mdb_expr *const *pconj, int npconj)
{
	struct mdb_select *s = x->s;
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
		key = equi_key_conjunct(conj, nconj, t, &kl, &kr);
	}
	if (key >= 0 && (rc = join_eliminate(x, t, kl, kr, nconj, npconj)) <= 0)
		return rc;
	/* the new table's own WHERE conjuncts filter it before it is joined */
	const uint32_t *rsel = NULL;
	uint64_t r_rows = s->tabs[t].t->nrows;
	if ((rc = table_filter(x, t, pconj, npconj, &rsel, &r_rows)))
		return rc;
	if (x->cat->dist && (rc = shard_join_sides(x, t, key >= 0 ? kl : NULL, kr, &rsel, &r_rows)))
		return rc;
	if (key >= 0) {
		const bool words = kl->type != MDB_CT_DOUBLE && kr->type != MDB_CT_DOUBLE;	/* the key columns hold the values themselves */
		const int64_t *vl;
		const uint64_t *nl, *nr;
		const void *vr;
		if ((rc = join_key_columns(x, t, kl, kr, rsel, r_rows, &vl, &nl, &vr, &nr)))
			return rc;
		if (words) {
			x->same_col[t] = kr->col_idx;
			x->same_as_tbl[t] = kl->tbl_idx;
			x->same_as_col[t] = kl->col_idx;
			op_stats_begin(x, kl, vl, kr, vr);	/* (until the join is done: op_stats_end below / in the shortcuts) */
		}
		if (x->n && r_rows && !x->cat->dist && !rsel && words &&
		    (rc = join_carrying_payload(x, t, conj, nconj, key, kl, kr, vl, nl, vr, nr, r_rows)) <= 0)
			return rc;
		answered = 1u << key;
		struct composite_key ck;
		ck.empty = false;
		if (x->n && r_rows && (rc = join_on_composite_key(x, t, conj, nconj, rsel, r_rows, &ck, &answered, &vl, &nl, &vr, &nr)) < 0)
			return rc;
		if (x->n && r_rows && !ck.empty) {
			const int jrc = mdb_dev_join_pairs(x->dev, vl, nl, x->n, vr, nr, r_rows, &pl, &pr, &J);
			op_stats_end(x);
			if (jrc)
				return dev_fail(x, "hash join");
			if ((pl && track(x, pl)) || (pr && track(x, pr)))
				return -MIDORIDB_NOMEM;
		}
		op_stats_end(x);
	} else if ((rc = join_cross_pairs(x, r_rows, &pl, &pr, &J))) {
		return rc;
	}
	if (rsel && J && (rc = rows_to_base(x, rsel, pr, J, &pr)))	/* pairs index the filtered right rows: back to row ids of the base table */
		return rc;
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

