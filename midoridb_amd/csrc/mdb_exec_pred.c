/*
 * mdb_exec_pred.c - WHERE / ON / HAVING expressions compiled into the device's postfix predicate programs (mdb_dev_filter)
 * and run over the tuple stream (reference: eval_row_cond / eval_cmp / eval_isxnull / eval_isxin,
 * src/engine/executor_select.c:865-1074).  Split off mdb_exec.c in round 4.
 */
#include "mdb_exec_internal.h"

/* ------------------------------------------------------------------ predicate compiler */


/* device binding of a column-like operand for the current stream: a table column read through the table's
 * row-id vector, the COUNT(*) column (HAVING), or - in the fused north-star plan, whose stream carries no row
 * ids - the group key column (the only field S4 lets such a query name; on a composite key: the key column of that field) */
void bind_operand(struct exec *x, const struct mdb_expr *f, const void **values, const uint64_t **nullbits, const uint32_t **rid)
{
	if (f->kind == MDB_EX_COUNT) {
		*values = x->d_count;
		*nullbits = NULL;
		*rid = NULL;
	} else if (f->kind == MDB_EX_AGG) {	/* a result column of mdb_dev_group_aggregate over the grouped stream (resolve_agg_refs: it is one of the statement's) */
		const int i = agg_index(x, f);
		*values = i >= 0 ? x->d_agg[i] : NULL;
		*nullbits = i >= 0 ? x->d_agg_nulls[i] : NULL;
		*rid = NULL;
	} else if (f->kind == MDB_EX_WINDOW) {	/* a result column of mdb_dev_window over the stream (stream_windows) */
		const int i = f->win_idx >= 0 && f->win_idx < x->nwin ? f->win_idx : -1;
		*values = i >= 0 ? x->d_win[i] : NULL;
		*nullbits = i >= 0 ? x->d_win_nulls[i] : NULL;
		*rid = NULL;
	} else if (stream_is_keys(x)) {
		*values = fused_key_column(x, f->tbl_idx, f->col_idx);
		*nullbits = NULL;
		*rid = NULL;
	} else {
		struct mdb_column *col = &x->s->tabs[f->tbl_idx].t->cols[f->col_idx];
		*values = col->d_data;
		*nullbits = col->d_nullbits;
		*rid = x->rid[f->tbl_idx];
	}
}

int pred_slot(struct exec *x, struct pred_prog *p, const struct mdb_expr *f)
{
	/* slot keys: (table, column) of a field; -2 COUNT(*); -3 - i the statement's i-th aggregate; -100 - i its i-th window item */
	const int ak = f->kind == MDB_EX_AGG ? -3 - agg_index(x, f) : f->kind == MDB_EX_WINDOW ? -100 - f->win_idx : 0;
	const bool computed = f->kind == MDB_EX_AGG || f->kind == MDB_EX_WINDOW;
	const int st = f->kind == MDB_EX_COUNT ? -2 : computed ? ak : f->tbl_idx, sc = f->kind == MDB_EX_COUNT ? -2 : computed ? ak : f->col_idx;
	if (f->kind == MDB_EX_WINDOW && (f->win_idx < 0 || f->win_idx >= x->nwin))
		return -1;
	if (f->kind == MDB_EX_AGG && agg_index(x, f) < 0)
		return -1;
	for (int i = 0; i < p->ncols; i++)
		if (p->slot_tbl[i] == st && p->slot_col[i] == sc)
			return i;
	if (p->ncols == MDB_PRED_MAX_SLOTS)
		return -1;
	p->slot_tbl[p->ncols] = st;
	p->slot_col[p->ncols] = sc;
	bind_operand(x, f, &p->cols[p->ncols].values, &p->cols[p->ncols].nullbits, &p->cols[p->ncols].rid);
	return p->ncols++;
}

int pred_emit(struct pred_prog *p, int op, int cmp, int type, int a, int b, int64_t imm)
{
	struct mdb_pred_insn *in;
	if (p->n == MDB_PRED_MAX_INSNS)
		return -1;
	in = &p->insn[p->n++];
	memset(in, 0, sizeof(*in));
	in->op = op;
	in->cmp = cmp;
	in->type = type;
	in->a = a;
	in->b = b;
	in->imm = imm;
	return 0;
}

/* the 8 bytes a literal stands for in a column of type coltype (a DATE / DATETIME string: its time_t, validated by
 * check_predicate_x / the UPDATE checks) */
/* the string dictionary of the database the running statement belongs to (set by the statement entry points) */
__thread const struct mdb_strdict *stmt_dict __attribute__((visibility("hidden")));

int64_t lit_bits_for(const struct mdb_expr *v, int coltype)
{
	int64_t bits = 0;
	if (v->kind == MDB_EX_FLOAT) {
		memcpy(&bits, &v->dval, 8);
		return bits;
	}
	if (v->kind == MDB_EX_STRING && coltype == MDB_CT_VARCHAR)	/* a string no cell holds has id -1: equal to nothing */
		return stmt_dict ? mdb_dict_find(stmt_dict, v->sval + 1, strlen(v->sval) - 2) : -1;
	if (v->kind == MDB_EX_STRING) {
		(void)mdb_parse_time(v->sval, coltype, &bits);
		return bits;
	}
	return v->ival;
}

bool const_cmp(int op, const struct mdb_expr *l, const struct mdb_expr *r)
{
	if (l->kind == MDB_EX_NULL || r->kind == MDB_EX_NULL)
		return false;			/* executor_select.c:660-662 */
	if (l->kind == MDB_EX_STRING || r->kind == MDB_EX_STRING)
		return false;			/* (rejected by the type check; never evaluated) */
	if (l->kind == MDB_EX_FLOAT) {
		double a = l->dval, b = r->dval;
		return op == 1 ? a < b : op == 2 ? a > b : op == 3 ? a != b : op == 4 ? a == b : op == 5 ? a <= b : a >= b;
	} else {
		int64_t a = l->ival, b = r->ival;
		return op == 1 ? a < b : op == 2 ? a > b : op == 3 ? a != b : op == 4 ? a == b : op == 5 ? a <= b : a >= b;
	}
}

/* SQL LIKE: '%' any run of characters (none included), '_' exactly one; everything else itself, case-sensitive */
static bool like_match(const char *s, size_t n, const char *pat, size_t m)
{
	size_t i = 0, j = 0, star = (size_t)-1, mark = 0;
	while (i < n) {
		if (j < m && pat[j] == '%') {
			star = j++;
			mark = i;
		} else if (j < m && (pat[j] == '_' || pat[j] == s[i])) {
			i++;
			j++;
		} else if (star != (size_t)-1) {
			j = star + 1;
			i = ++mark;
		} else {
			return false;
		}
	}
	while (j < m && pat[j] == '%')
		j++;
	return j == m;
}

/* An IN / NOT IN list of more values than the term kernels take (MDB_FILTER_MAX_TERMS, mdb_dev.h) compiles to ONE lookup
 * instead of one comparison and one OR / AND per value, which MDB_PRED_MAX_INSNS ends at 32 values:
 *   VARCHAR columns    MDB_P_IN_BITS over a bit per dictionary id, as LIKE builds it (a string no cell holds has id -1: no bit)
 *   every other type   MDB_P_IN_SET over a hash table of the non-NULL literals (mdb_set.c), uploaded into a statement buffer
 * A NULL literal keeps its meaning: in IN it adds nothing, in NOT IN it makes the test false for every row (x <> NULL is never true).
 * A list without effective members: IN is false, NOT IN is `x IS NOT NULL`.  Shorter lists compile exactly as before.
 * MDB_IN_SET=0 expands every list as before. */

/* a lookup table could not be built or uploaded: the statement's error says so (pred_compile_failed leaves it standing) */
static int lookup_failed(struct exec *x, const char *what, size_t bytes)
{
	snprintf(x->err, x->errlen, "execution phase: IN list: %s (%zu bytes): %s\n", what, bytes, x->dev ? mdb_dev_last_error(x->dev) : "");
	x->pred_err_said = true;
	return -1;
}

/* what a failed pred_compile() leaves in the statement's error: the program's limits, unless the compiler has named another cause */
void pred_compile_failed(struct exec *x)
{
	if (!x->pred_err_said)
		snprintf(x->err, x->errlen, "execution phase: predicate too large for the device program (max %d steps, %d columns)\n",
			 MDB_PRED_MAX_INSNS, MDB_PRED_MAX_SLOTS);
	x->pred_err_said = false;
}

static int pred_compile_in_lookup(struct exec *x, struct pred_prog *p, const struct mdb_expr *e, int a)
{
	const struct mdb_expr *f = e->kids[0];
	const int neg = e->op ? 1 : 0, k = e->nkids - 1;
	int rc = -1;

	for (int i = 1; neg && i <= k; i++)
		if (e->kids[i]->kind == MDB_EX_NULL)
			return pred_emit(p, MDB_P_CONST, 0, 0, 0, 0, 0);
	if (f->type == MDB_CT_VARCHAR) {
		const struct mdb_strdict *d = stmt_dict;
		const uint64_t words = ((d ? d->n : 0) + 1 + 63) / 64;
		uint64_t *bits = calloc((size_t)words, 8);
		void *dbits;
		if (!bits)
			return lookup_failed(x, "no host memory for the dictionary bits", (size_t)words * 8);
		for (int i = 1; i <= k; i++) {
			const int64_t id = e->kids[i]->kind == MDB_EX_NULL ? -1 : lit_bits_for(e->kids[i], f->type);
			if (id >= 0 && (uint64_t)id < words * 64)
				bits[id >> 6] |= 1ull << (id & 63);
		}
		dbits = dalloc(x, (size_t)words * 8);
		if (dbits && !mdb_dev_h2d(x->dev, dbits, bits, (size_t)words * 8))
			rc = pred_emit(p, MDB_P_IN_BITS, neg, MDB_T_INT64, a, (int)(words > 0x7FFFFFFF ? 0x7FFFFFFF : words), (int64_t)(uintptr_t)dbits);
		else
			(void)lookup_failed(x, "the dictionary bits could not be placed on the device", (size_t)words * 8);
		free(bits);
	} else {
		const int type = f->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64;
		int64_t *vals = malloc(sizeof(int64_t) * (size_t)k);
		struct mdb_set_image img;
		uint64_t n = 0;
		if (!vals)
			return lookup_failed(x, "no host memory for the values", sizeof(int64_t) * (size_t)k);
		for (int i = 1; i <= k; i++)
			if (e->kids[i]->kind != MDB_EX_NULL)
				vals[n++] = lit_bits_for(e->kids[i], f->type);
		if (mdb_set_build(vals, n, type, &img)) {
			free(vals);
			return lookup_failed(x, n > MDB_SET_MAX_VALUES ? "more values than a set takes" : "no host memory for the set", (size_t)n * 8);
		}
		free(vals);
		if (!img.members) {	/* (NaN literals only) */
			mdb_set_image_free(&img);
			return neg ? pred_emit(p, MDB_P_ISNULL, 1, 0, a, 0, 0) : pred_emit(p, MDB_P_CONST, 0, 0, 0, 0, 0);
		} else {
			const size_t bytes = (size_t)(2 + img.slots) * 8;
			void *dtab = dalloc(x, bytes);
			if (dtab && !mdb_dev_h2d(x->dev, dtab, img.words, bytes))
				rc = pred_emit(p, MDB_P_IN_SET, neg, type, a, (int)img.log2_slots, (int64_t)(uintptr_t)dtab);
			else
				(void)lookup_failed(x, "the set could not be placed on the device", bytes);
		}
		mdb_set_image_free(&img);
	}
	if (!rc && x->cat)
		x->cat->in_set_lookups++;
	return rc;
}

/* x [NOT] IN (SELECT ...): the subquery has run (subqueries_eval) - e->sub_set is the device set of its column's non-NULL cells,
 * sub_rows / sub_nulls / sub_members its rows, the NULL cells among them and the distinct values.  SQL's three-valued rules, which are
 * the list's where they overlap:
 *   no rows at all            IN false;  NOT IN true for every row, a NULL x included
 *   rows, some cell NULL      IN the lookup (false without a member);  NOT IN never true
 *   rows, no NULL             the lookup, negated for NOT IN (a NULL x fails both); without a member (NaN cells only) IN is false and
 *                             NOT IN is `x IS NOT NULL`
 * The instruction is the one a long list compiles to: every plan that takes such a list takes this. */
static int pred_compile_in_subquery(struct pred_prog *p, const struct mdb_expr *e, int a)
{
	const int neg = e->op ? 1 : 0;
	struct mdb_pred_insn in;

	if (!e->sub_rows)
		return pred_emit(p, MDB_P_CONST, 0, 0, 0, 0, neg);
	if (neg && e->sub_nulls)
		return pred_emit(p, MDB_P_CONST, 0, 0, 0, 0, 0);
	if (!e->sub_members || !e->sub_set)
		return neg ? pred_emit(p, MDB_P_ISNULL, 1, 0, a, 0, 0) : pred_emit(p, MDB_P_CONST, 0, 0, 0, 0, 0);
	if (mdb_dev_set_insn(e->sub_set, a, neg, &in))
		return -1;
	return pred_emit(p, in.op, in.cmp, in.type, in.a, in.b, in.imm);
}

/* a TINYINT column's cells: the column itself, or a window item that copies them (LAG / LEAD / FIRST_VALUE / LAST_VALUE of it) */
static bool is_bool_column(const struct mdb_expr *f)
{
	if (f->type != MDB_CT_TINYINT)
		return false;
	return f->kind == MDB_EX_FIELD || (f->kind == MDB_EX_WINDOW && f->op >= MDB_WIN_LAG && f->op <= MDB_WIN_LAST_VALUE);
}

int pred_compile(struct exec *x, struct pred_prog *p, const struct mdb_expr *e)
{
	int rc = 0, a, b;

	switch (e->kind) {
	case MDB_EX_LOGOP:
		if ((rc = pred_compile(x, p, e->kids[0])) || (rc = pred_compile(x, p, e->kids[1])))
			return rc;
		return pred_emit(p, e->op == 0 ? MDB_P_AND : (e->op == 1 ? MDB_P_OR : MDB_P_XOR), 0, 0, 0, 0, 0);
	case MDB_EX_CMP: {
		const struct mdb_expr *l = e->kids[0], *r = e->kids[1];
		const bool lcol = l->kind == MDB_EX_FIELD || l->kind == MDB_EX_COUNT || l->kind == MDB_EX_AGG || l->kind == MDB_EX_WINDOW;
		const bool rcol = r->kind == MDB_EX_FIELD || r->kind == MDB_EX_COUNT || r->kind == MDB_EX_AGG || r->kind == MDB_EX_WINDOW;
		if (lcol && rcol) {
			if (is_bool_column(l) && e->op != MDB_CMP_EQ && e->op != MDB_CMP_NE)
				return pred_emit(p, MDB_P_CONST, 0, 0, 0, 0, 0);
			a = pred_slot(x, p, l);
			b = pred_slot(x, p, r);
			if (a < 0 || b < 0)
				return -1;
			return pred_emit(p, MDB_P_CMP_COL_COL, e->op, (l->kind != MDB_EX_COUNT && l->type == MDB_CT_DOUBLE) ? MDB_T_DOUBLE : MDB_T_INT64,
					 a, b, 0);
		}
		if (lcol || rcol) {
			const struct mdb_expr *f = lcol ? l : r, *v = lcol ? r : l;
			if (v->kind == MDB_EX_NULL)	/* NULL operand: never true (executor_select.c:793-795) */
				return pred_emit(p, MDB_P_CONST, 0, 0, 0, 0, 0);
			/* TINYINT (bool) operands only know = and <> upstream (cmp_bool_value_to_value, executor_select.c:484-494): false */
			if (is_bool_column(f) && e->op != MDB_CMP_EQ && e->op != MDB_CMP_NE)
				return pred_emit(p, MDB_P_CONST, 0, 0, 0, 0, 0);
			a = pred_slot(x, p, f);
			if (a < 0)
				return -1;
			return pred_emit(p, lcol ? MDB_P_CMP_COL_CONST : MDB_P_CMP_CONST_COL, e->op,
					 (f->kind != MDB_EX_COUNT && f->type == MDB_CT_DOUBLE) ? MDB_T_DOUBLE : MDB_T_INT64, a, 0,
					 lit_bits_for(v, f->kind != MDB_EX_COUNT ? f->type : MDB_CT_INTEGER));	/* (an aggregate: its result's type) */
		}
		return pred_emit(p, MDB_P_CONST, 0, 0, 0, 0, const_cmp(e->op, l, r));
	}
	case MDB_EX_ISNULL:
		a = pred_slot(x, p, e->kids[0]);
		if (a < 0)
			return -1;
		return pred_emit(p, MDB_P_ISNULL, e->op ? 1 : 0, 0, a, 0, 0);
	case MDB_EX_ISIN: {
		/* x IN (v1..vk)  = (x = v1) OR ... OR (x = vk)   - SQL semantics; the reference's
		 *                  conjunction (eval_isxin :1013-1021) is defect D3, identical for k = 1
		 * x NOT IN (...) = (x <> v1) AND ... AND (x <> vk) - same as the reference */
		const struct mdb_expr *f = e->kids[0];
		a = pred_slot(x, p, f);
		if (a < 0)
			return -1;
		if (e->sub)
			return pred_compile_in_subquery(p, e, a);
		if (e->nkids - 1 > MDB_FILTER_MAX_TERMS && !mdb_knob_off("MDB_IN_SET"))
			return pred_compile_in_lookup(x, p, e, a);
		for (int i = 1; i < e->nkids; i++) {
			const struct mdb_expr *v = e->kids[i];
			if (v->kind == MDB_EX_NULL)
				rc = pred_emit(p, MDB_P_CONST, 0, 0, 0, 0, 0);
			else
				rc = pred_emit(p, MDB_P_CMP_COL_CONST, e->op ? MDB_CMP_NE : MDB_CMP_EQ,
					       f->type == MDB_CT_DOUBLE ? MDB_T_DOUBLE : MDB_T_INT64, a, 0, lit_bits_for(v, f->type));
			if (rc)
				return rc;
			if (i > 1 && (rc = pred_emit(p, e->op ? MDB_P_AND : MDB_P_OR, 0, 0, 0, 0, 0)))
				return rc;
		}
		return 0;
	}
	case MDB_EX_LIKE: {
		/* the pattern is matched ONCE per distinct string, on the host, against the database's dictionary; the device sees a bit per
		 * dictionary id and tests the cell's (MDB_P_IN_BITS): 10^8 cells over 10^4 distinct strings are 10^4 matches */
		const struct mdb_expr *f = e->kids[0], *v = e->kids[1];
		const struct mdb_strdict *d = stmt_dict;
		const size_t plen = strlen(v->sval) >= 2 ? strlen(v->sval) - 2 : 0;
		const uint64_t words = ((d ? d->n : 0) + 1 + 63) / 64;
		uint64_t *bits = calloc((size_t)words, 8);
		if (!bits)
			return -1;
		for (uint64_t id = 1; d && id <= d->n; id++)
			if (like_match(d->str[id - 1], d->len[id - 1], v->sval + 1, plen))
				bits[id >> 6] |= 1ull << (id & 63);
		void *dbits = dalloc(x, (size_t)words * 8);
		if (!dbits || mdb_dev_h2d(x->dev, dbits, bits, (size_t)words * 8)) {
			free(bits);
			return -1;
		}
		free(bits);
		a = pred_slot(x, p, f);
		if (a < 0)
			return -1;
		return pred_emit(p, MDB_P_IN_BITS, e->op ? 1 : 0, MDB_T_INT64, a, (int)(words > 0x7FFFFFFF ? 0x7FFFFFFF : words), (int64_t)(uintptr_t)dbits);
	}
	default:
		return -1;
	}
}

/* filter the current stream (tables 0..ntabs-1) by predicate e */
int stream_filter(struct exec *x, int ntabs_in_stream, const struct mdb_expr *e)
{
	struct pred_prog p;
	uint32_t *sel;
	uint64_t m = 0;

	if (x->n == 0)
		return MIDORIDB_OK;
	memset(&p, 0, sizeof(p));
	if (pred_compile(x, &p, e)) {
		pred_compile_failed(x);
		return -MIDORIDB_ERROR;
	}
	sel = dalloc(x, x->n * 4);
	if (!sel)
		return dev_fail(x, "allocating the selection vector");
	if (mdb_dev_filter(x->dev, p.insn, p.n, p.cols, p.ncols, x->n, sel, &m))
		return dev_fail(x, "filter");
	return stream_apply_sel(x, ntabs_in_stream, sel, m);
}
