/*
 * mdb_exec_resolve.c - plan normalisation and the semantic checks that guard the executor: what the reference does in
 * its optimiser (src/engine/optimiser_select.c:114-238: NAME -> fully qualified FIELDNAME, alias -> table name, SELECT * expansion)
 * and in its semantic phase (src/parser/semantic_select.c:1575-1718, 2135-2186, 2470-2478: unknown table / column, duplicate column
 * names across FROM tables, operand types, the GROUP BY rule), with the reference's error texts.  Split off mdb_exec.c in round 4.
 */
#include "mdb_exec_internal.h"

/* ------------------------------------------------------------------ plan resolution */

bool field_eq(const struct mdb_expr *a, const struct mdb_expr *b)
{
	return a->kind == MDB_EX_FIELD && b->kind == MDB_EX_FIELD && a->tbl_idx == b->tbl_idx && a->col_idx == b->col_idx;
}

/* SUM / MIN / MAX / AVG / COUNT(DISTINCT): the function's name, how its result column's name begins in front of "<table>.<column>)", and the
 * column type of its result over a column of type coltype */
const char *mdb_agg_name(int op)
{
	return op == MDB_AGG_SUM ? "SUM" : op == MDB_AGG_MIN ? "MIN" : op == MDB_AGG_MAX ? "MAX" : op == MDB_AGG_AVG ? "AVG" : "COUNT(DISTINCT)";
}

const char *mdb_agg_open(int op)
{
	return op == MDB_AGG_SUM ? "SUM(" : op == MDB_AGG_MIN ? "MIN(" : op == MDB_AGG_MAX ? "MAX(" : op == MDB_AGG_AVG ? "AVG(" : "COUNT(DISTINCT ";
}

int mdb_agg_result_type(int op, int coltype)
{
	if (op == MDB_AGG_COUNT_DISTINCT)
		return MDB_CT_INTEGER;
	if (op == MDB_AGG_AVG)
		return MDB_CT_DOUBLE;
	if (op == MDB_AGG_SUM)
		return coltype == MDB_CT_DOUBLE ? MDB_CT_DOUBLE : MDB_CT_INTEGER;
	return coltype;
}

bool agg_eq(const struct mdb_expr *a, const struct mdb_expr *b)
{
	return a->kind == MDB_EX_AGG && b->kind == MDB_EX_AGG && a->op == b->op && a->tbl_idx == b->tbl_idx && a->col_idx == b->col_idx;
}

/* an aggregate as the parser left it (kid[0] = its column): the column is resolved and the type rules are applied - no function over VARCHAR
 * (the cells are dictionary ids, which are not in string order) but COUNT(DISTINCT), which only asks whether two cells are equal; no SUM / AVG
 * over DATE / DATETIME */
static int resolve_agg(struct mdb_select *s, struct mdb_expr *e, char *err, size_t errlen)
{
	int rc;
	struct mdb_expr *c;

	if (e->nkids != 1 || (e->kids[0]->kind != MDB_EX_NAME && e->kids[0]->kind != MDB_EX_FIELD)) {
		ERR("%s takes one column\n", mdb_agg_name(e->op));
		return -MIDORIDB_ERROR;
	}
	c = e->kids[0];
	if ((rc = resolve_expr(s, c, err, errlen)))
		return rc;
	if (c->type == MDB_CT_VARCHAR && e->op != MDB_AGG_COUNT_DISTINCT) {
		ERR("%s over the VARCHAR column '%.100s.%.100s' is not supported: its cells are dictionary ids, which are not in string order\n",
		    mdb_agg_name(e->op), c->tbl, c->col);
		return -MIDORIDB_ERROR;
	}
	if ((e->op == MDB_AGG_SUM || e->op == MDB_AGG_AVG) && (c->type == MDB_CT_DATE || c->type == MDB_CT_DATETIME)) {
		ERR("%s over the %s column '%.100s.%.100s' is not supported: only MIN and MAX of a point in time mean something\n", mdb_agg_name(e->op),
		    c->type == MDB_CT_DATE ? "DATE" : "DATETIME", c->tbl, c->col);
		return -MIDORIDB_ERROR;
	}
	mdb_copy_name(e->tbl, c->tbl);
	mdb_copy_name(e->col, c->col);
	e->tbl_idx = c->tbl_idx;
	e->col_idx = c->col_idx;
	e->type = mdb_agg_result_type(e->op, c->type);
	return MIDORIDB_OK;
}

/* ------------------------------------------------------------------ window functions: fn(...) OVER (PARTITION BY ... ORDER BY ...)
 * An extension.  The function's text as its result column is named without an alias: "ROW_NUMBER() OVER", "SUM(A.v) OVER" */
const char *mdb_win_name(int op)
{
	static const char *const names[] = { "?", "ROW_NUMBER", "RANK", "DENSE_RANK", "COUNT", "SUM", "MIN", "MAX", "AVG" };
	static const char *const nav[] = { "LAG", "LEAD", "FIRST_VALUE", "LAST_VALUE", "NTILE" };
	if (op >= MDB_WIN_LAG && op <= MDB_WIN_NTILE)
		return nav[op - MDB_WIN_LAG];
	return op >= MDB_WIN_ROW_NUMBER && op <= MDB_WIN_AVG ? names[op] : names[0];
}

/* how many columns a window function takes as its argument: one for the aggregates and for LAG / LEAD / FIRST_VALUE / LAST_VALUE */
int mdb_win_narg(int op)
{
	return (op >= MDB_WIN_SUM && op <= MDB_WIN_AVG) || (op >= MDB_WIN_LAG && op <= MDB_WIN_LAST_VALUE) ? 1 : 0;
}

static bool win_is_nav_col(int op)
{
	return op >= MDB_WIN_LAG && op <= MDB_WIN_LAST_VALUE;
}

/* the aggregate function a window function folds with (enum mdb_agg_op), 0: a ranking function or COUNT(*) */
static int win_agg_op(int op)
{
	return op == MDB_WIN_SUM ? MDB_AGG_SUM : op == MDB_WIN_MIN ? MDB_AGG_MIN : op == MDB_WIN_MAX ? MDB_AGG_MAX : op == MDB_WIN_AVG ? MDB_AGG_AVG : 0;
}

/* the result column's name of a resolved window item without an alias: the function's text as aggregates are named, then " OVER" */
void mdb_win_result_name(const struct mdb_expr *e, char *out /* [MDB_NAME_LEN] */)
{
	if (e->op == MDB_WIN_NTILE)
		snprintf(out, MDB_NAME_LEN, "NTILE(%llu) OVER", (unsigned long long)e->win_arg);
	else if ((e->op == MDB_WIN_LAG || e->op == MDB_WIN_LEAD) && e->win_arg != 1)	/* (the offset where it is not 1; the default is not named) */
		snprintf(out, MDB_NAME_LEN, "%s(%.50s.%.50s, %llu) OVER", mdb_win_name(e->op), e->tbl, e->col, (unsigned long long)e->win_arg);
	else if (mdb_win_narg(e->op))
		snprintf(out, MDB_NAME_LEN, "%s(%.56s.%.56s) OVER", mdb_win_name(e->op), e->tbl, e->col);
	else
		snprintf(out, MDB_NAME_LEN, "%s OVER", e->op == MDB_WIN_COUNT ? "COUNT(*)" : e->op == MDB_WIN_ROW_NUMBER ? "ROW_NUMBER()" :
						       e->op == MDB_WIN_RANK ? "RANK()" : "DENSE_RANK()");
}

bool expr_has_window(const struct mdb_expr *e)
{
	if (!e)
		return false;
	if (e->kind == MDB_EX_WINDOW)
		return true;
	for (int i = 0; i < e->nkids; i++)
		if (expr_has_window(e->kids[i]))
			return true;
	return false;
}

/* two resolved window items share one operator call when their OVER clauses are equal field for field */
bool window_same_over(const struct mdb_expr *a, const struct mdb_expr *b)
{
	const int na = mdb_win_narg(a->op), nb = mdb_win_narg(b->op);
	if (a->win_npart != b->win_npart || a->win_norder != b->win_norder || a->win_desc != b->win_desc)
		return false;
	for (int k = 0; k < a->win_npart + a->win_norder; k++)
		if (!field_eq(a->kids[na + k], b->kids[nb + k]))
			return false;
	return true;
}

/* a window item as the parser left it: its fields are resolved and the type rules of resolve_agg are applied to its argument - no function
 * over VARCHAR, no SUM / AVG over DATE / DATETIME, and no SUM / AVG over DOUBLE (a scan sums in another order than any sequential reference
 * would) -; PARTITION BY takes a column of any type (cells compare as in GROUP BY), ORDER BY what the statement's ORDER BY takes */
static int resolve_window(struct mdb_select *s, struct mdb_expr *e, char *err, size_t errlen)
{
	const int narg = mdb_win_narg(e->op);
	int rc;

	if (!strcmp(mdb_win_name(e->op), "?") || e->win_npart < 0 || e->win_norder < 0 || e->nkids != narg + e->win_npart + e->win_norder) {
		ERR("error while running syntax analysis on query\n");
		return -MIDORIDB_ERROR;
	}
	for (int k = 0; k < e->nkids; k++) {
		if (e->kids[k]->kind != MDB_EX_NAME && e->kids[k]->kind != MDB_EX_FIELD) {
			ERR("%s ... OVER takes columns: col or tbl.col\n", mdb_win_name(e->op));
			return -MIDORIDB_ERROR;
		}
		if ((rc = resolve_expr(s, e->kids[k], err, errlen)))
			return rc;
	}
	if (e->win_npart + e->win_norder > MDB_SORT_MAX_KEYS) {
		ERR("%s ... OVER: more than %d PARTITION BY and ORDER BY fields together are not supported\n", mdb_win_name(e->op), MDB_SORT_MAX_KEYS);
		return -MIDORIDB_ERROR;
	}
	for (int k = 0; k < e->win_norder; k++) {
		const struct mdb_expr *o = e->kids[narg + e->win_npart + k];
		if (o->type == MDB_CT_VARCHAR) {	/* cells are dictionary ids: equality only, no collation order */
			ERR("ORDER BY over the VARCHAR column '%s.%s' inside OVER is not supported on the MI355X path\n", o->tbl, o->col);
			return -MIDORIDB_ERROR;
		}
	}
	e->type = MDB_CT_INTEGER;
	if (e->op == MDB_WIN_NTILE && !e->win_arg) {
		ERR("NTILE(0) ... OVER: the number of buckets must be at least 1\n");
		return -MIDORIDB_ERROR;
	}
	if (win_is_nav_col(e->op)) {	/* a cell of the column is copied: every type is served, the result has the column's type */
		const struct mdb_expr *c = e->kids[0];
		const char *want = c->type == MDB_CT_INTEGER ? "an integer" : c->type == MDB_CT_TINYINT ? "TRUE or FALSE" : "a number with a decimal point";
		if (e->win_dflt != MDB_EX_NULL && (c->type == MDB_CT_VARCHAR || c->type == MDB_CT_DATE || c->type == MDB_CT_DATETIME)) {
			ERR("%s ... OVER: a default for the %s column '%.100s.%.100s' is not supported: write NULL, or leave the default out\n", mdb_win_name(e->op),
			    c->type == MDB_CT_VARCHAR ? "VARCHAR" : c->type == MDB_CT_DATE ? "DATE" : "DATETIME", c->tbl, c->col);
			return -MIDORIDB_ERROR;
		}
		if (e->win_dflt == MDB_EX_BOOL && e->ival != 0 && e->ival != 1) {
			ERR("%s ... OVER: UNKNOWN as a default is not supported: write NULL\n", mdb_win_name(e->op));
			return -MIDORIDB_ERROR;
		}
		if (e->win_dflt != MDB_EX_NULL && e->win_dflt != (c->type == MDB_CT_INTEGER ? MDB_EX_INT : c->type == MDB_CT_TINYINT ? MDB_EX_BOOL : MDB_EX_FLOAT)) {
			ERR("%s ... OVER: the default does not match the type of column '%.100s.%.100s': it takes %s, or NULL\n", mdb_win_name(e->op), c->tbl, c->col, want);
			return -MIDORIDB_ERROR;
		}
		mdb_copy_name(e->tbl, c->tbl);
		mdb_copy_name(e->col, c->col);
		e->tbl_idx = c->tbl_idx;
		e->col_idx = c->col_idx;
		e->type = c->type;
	} else if (narg) {
		const struct mdb_expr *c = e->kids[0];
		if (c->type == MDB_CT_VARCHAR) {
			ERR("%s ... OVER over the VARCHAR column '%.100s.%.100s' is not supported: its cells are dictionary ids, which are not in string order\n",
			    mdb_win_name(e->op), c->tbl, c->col);
			return -MIDORIDB_ERROR;
		}
		if ((e->op == MDB_WIN_SUM || e->op == MDB_WIN_AVG) && (c->type == MDB_CT_DATE || c->type == MDB_CT_DATETIME)) {
			ERR("%s ... OVER over the %s column '%.100s.%.100s' is not supported: only MIN and MAX of a point in time mean something\n",
			    mdb_win_name(e->op), c->type == MDB_CT_DATE ? "DATE" : "DATETIME", c->tbl, c->col);
			return -MIDORIDB_ERROR;
		}
		if ((e->op == MDB_WIN_SUM || e->op == MDB_WIN_AVG) && c->type == MDB_CT_DOUBLE) {
			ERR("%s ... OVER over the DOUBLE column '%.100s.%.100s' is not supported: a scan would sum in another order than a sequential reference does\n",
			    mdb_win_name(e->op), c->tbl, c->col);
			return -MIDORIDB_ERROR;
		}
		mdb_copy_name(e->tbl, c->tbl);
		mdb_copy_name(e->col, c->col);
		e->tbl_idx = c->tbl_idx;
		e->col_idx = c->col_idx;
		e->type = mdb_agg_result_type(win_agg_op(e->op), c->type);
	}
	return MIDORIDB_OK;
}

/* the aggregates under a HAVING / ORDER BY expression that repeat their function and column (an alias has been replaced by its item already):
 * each must be one of the select list's - the executor computes those and nothing else */
static int resolve_agg_refs(struct mdb_select *s, struct mdb_expr *e, const char *clause, char *err, size_t errlen)
{
	int rc;

	if (!e)
		return MIDORIDB_OK;
	if (e->kind == MDB_EX_AGG) {
		bool found = false;
		if (e->nkids && (rc = resolve_agg(s, e, err, errlen)))
			return rc;
		for (int i = 0; i < s->nsel && !found; i++)
			found = agg_eq(s->sel[i], e);
		if (!found) {
			ERR("%s%.100s.%.100s) in the %s clause must also stand in the select list\n", mdb_agg_open(e->op), e->tbl, e->col, clause);
			return -MIDORIDB_ERROR;
		}
		return MIDORIDB_OK;
	}
	for (int i = 0; i < e->nkids; i++)
		if ((rc = resolve_agg_refs(s, e->kids[i], clause, err, errlen)))
			return rc;
	return MIDORIDB_OK;
}

/* a bare name that is a select-list alias stands for the aliased item: a column (any clause), COUNT(*) (HAVING: count_ok) or an aggregate (HAVING,
 * ORDER BY: agg_ok); names of real columns win */
static void subst_alias(const struct mdb_select *s, struct mdb_expr *e, bool count_ok, bool agg_ok)
{
	if (!e)
		return;
	if (e->kind == MDB_EX_NAME && s->sel_alias) {
		for (int t = 0; t < s->ntabs; t++)
			for (int c = 0; c < s->tabs[t].t->ncols; c++)
				if (strcmp(s->tabs[t].t->cols[c].name, e->col) == 0)
					return;
		for (int i = 0; i < s->nsel; i++) {
			if (!s->sel_alias[i][0] || strcmp(s->sel_alias[i], e->col) != 0)
				continue;
			const struct mdb_expr *to = s->sel[i];
			if (to->kind == MDB_EX_FIELD) {		/* (resolved: the select list is resolved first) */
				e->kind = MDB_EX_FIELD;
				mdb_copy_name(e->tbl, to->tbl);
				mdb_copy_name(e->col, to->col);
				e->tbl_idx = to->tbl_idx;
				e->col_idx = to->col_idx;
				e->type = to->type;
			} else if (to->kind == MDB_EX_COUNT && count_ok && to->nkids == 0) {
				e->kind = MDB_EX_COUNT;
				e->op = to->op;
				e->ival = to->ival;
			} else if (to->kind == MDB_EX_WINDOW && agg_ok) {	/* (resolved; the copy has no kid and stands for the item's result column) */
				e->kind = MDB_EX_WINDOW;
				e->op = to->op;
				e->win_idx = to->win_idx;
				e->type = to->type;
			} else if (to->kind == MDB_EX_AGG && agg_ok) {	/* (resolved; the copy has no kid) */
				e->kind = MDB_EX_AGG;
				e->op = to->op;
				mdb_copy_name(e->tbl, to->tbl);
				mdb_copy_name(e->col, to->col);
				e->tbl_idx = to->tbl_idx;
				e->col_idx = to->col_idx;
				e->type = to->type;
			}
			return;
		}
	}
	if (e->kind == MDB_EX_AGG || e->kind == MDB_EX_WINDOW)
		return;		/* (the argument of an aggregate is a column, never an alias) */
	for (int i = 0; i < e->nkids; i++)
		subst_alias(s, e->kids[i], count_ok, agg_ok);
}

int resolve_expr(struct mdb_select *s, struct mdb_expr *e, char *err, size_t errlen)
{
	int rc;

	if (!e)
		return MIDORIDB_OK;
	if (e->kind == MDB_EX_NAME) {
		int ft = -1, fc = -1, hits = 0;
		for (int t = 0; t < s->ntabs; t++)
			for (int c = 0; c < s->tabs[t].t->ncols; c++)
				if (strcmp(s->tabs[t].t->cols[c].name, e->col) == 0) {
					ft = t;
					fc = c;
					hits++;
				}
		if (hits == 0) {
			ERR("no such column: '%.128s'\n", e->col);
			return -MIDORIDB_ERROR;
		}
		if (hits > 1) {
			ERR("ambiguous column name: '%.128s'\n", e->col);
			return -MIDORIDB_ERROR;
		}
		e->kind = MDB_EX_FIELD;
		e->tbl_idx = ft;
		e->col_idx = fc;
		mdb_copy_name(e->tbl, s->tabs[ft].t->name);
	} else if (e->kind == MDB_EX_FIELD) {
		int ft = -1;
		for (int t = 0; t < s->ntabs; t++)
			if (strcmp(s->tabs[t].alias, e->tbl) == 0 || (!s->tabs[t].alias[0] && strcmp(s->tabs[t].name, e->tbl) == 0) ||
			    strcmp(s->tabs[t].name, e->tbl) == 0)
				ft = t;
		if (ft < 0) {
			ERR("table is not part of from clause: '%.128s'\n", e->tbl);
			return -MIDORIDB_ERROR;
		}
		e->tbl_idx = ft;
		e->col_idx = -1;
		for (int c = 0; c < s->tabs[ft].t->ncols; c++)
			if (strcmp(s->tabs[ft].t->cols[c].name, e->col) == 0)
				e->col_idx = c;
		if (e->col_idx < 0) {
			ERR("no such column: '%.128s'.'%.128s'\n", e->tbl, e->col);
			return -MIDORIDB_ERROR;
		}
		mdb_copy_name(e->tbl, s->tabs[ft].t->name);	/* alias -> real table name */
	}
	if (e->kind == MDB_EX_FIELD) {
		e->type = s->tabs[e->tbl_idx].t->cols[e->col_idx].type;
	}
	for (int i = 0; i < e->nkids; i++)
		if ((rc = resolve_expr(s, e->kids[i], err, errlen)))
			return rc;
	return MIDORIDB_OK;
}

/* predicate shape check (what the device predicate compiler accepts); in the HAVING clause COUNT(*) is an
 * INTEGER operand of comparisons (semantic_select.c:1983-1985 lets it through) */
bool is_having_clause(const char *clause)
{
	return strcmp(clause, "having") == 0;
}

/* type of a comparison operand as the reference's semantic phase sees it (check_value_types_cmp, semantic_select.c:2135-2186):
 * a raw string is a VARCHAR - SELECT does not box it into a DATE ("raw values are not auto-boxed", executor_select.c:193) -
 * while DELETE / UPDATE parse it against a DATE / DATETIME column (semantic_delete.c:160-200): `dml` */
int operand_type(const struct mdb_expr *o, const struct mdb_expr *other, bool dml)
{
	switch (o->kind) {
	case MDB_EX_FIELD: case MDB_EX_AGG: case MDB_EX_WINDOW: return o->type;	/* (an aggregate, a window item: its result's type) */
	case MDB_EX_INT: case MDB_EX_COUNT: return MDB_CT_INTEGER;
	case MDB_EX_FLOAT: return MDB_CT_DOUBLE;
	case MDB_EX_BOOL: return MDB_CT_TINYINT;
	case MDB_EX_STRING:
		if (dml && other->kind == MDB_EX_FIELD && (other->type == MDB_CT_DATE || other->type == MDB_CT_DATETIME))
			return other->type;
		return MDB_CT_VARCHAR;
	default: return -1;
	}
}

int check_predicate_x(const struct mdb_expr *e, const char *clause, bool dml, char *err, size_t errlen)
{
	int rc;
	switch (e->kind) {
	case MDB_EX_LOGOP:
		if ((rc = check_predicate_x(e->kids[0], clause, dml, err, errlen)) || (rc = check_predicate_x(e->kids[1], clause, dml, err, errlen)))
			return rc;
		return MIDORIDB_OK;
	case MDB_EX_CMP: {
		const struct mdb_expr *l = e->kids[0], *r = e->kids[1];
		for (int i = 0; i < 2; i++) {
			const struct mdb_expr *o = e->kids[i];
			if ((o->kind == MDB_EX_COUNT || o->kind == MDB_EX_AGG || o->kind == MDB_EX_WINDOW) && is_having_clause(clause))
				continue;
			if (o->kind == MDB_EX_WINDOW) {
				ERR("a window function can't be used in the %s-clause: name its alias in HAVING or ORDER BY\n", clause);
				return -MIDORIDB_ERROR;
			}
			if (o->kind != MDB_EX_FIELD && o->kind != MDB_EX_INT && o->kind != MDB_EX_FLOAT && o->kind != MDB_EX_NULL &&
			    o->kind != MDB_EX_BOOL && o->kind != MDB_EX_STRING) {
				ERR("expressions in %s clause must compare columns with literal values\n", clause);
				return -MIDORIDB_ERROR;
			}
		}
		/* operand types must match exactly (reference check_value_types_cmp, semantic_select.c:2135-2186) */
		{
			const int tl = operand_type(l, r, dml), tr = operand_type(r, l, dml);
			int64_t tv;
			if (tl >= 0 && tr >= 0 && tl != tr) {
				ERR("comparison operands must have the same type\n");
				return -MIDORIDB_ERROR;
			}
			/* VARCHAR cells are dictionary ids: equal strings, equal ids - and nothing else (semantic_select.c:2171-2176,
			 * semantic_delete.c:211-216) */
			if ((tl == MDB_CT_VARCHAR || tr == MDB_CT_VARCHAR) && e->op != MDB_CMP_EQ && e->op != MDB_CMP_NE) {
				if (dml)
					ERR("VARCHAR fields can only use '=' or '<>' ops\n");
				else
					ERR("VARCHAR values can only use '=' or '<>' ops\n");
				return -MIDORIDB_ERROR;
			}
			for (int i = 0; i < 2; i++)
				if (e->kids[i]->kind == MDB_EX_STRING && (i ? tl : tr) != MDB_CT_VARCHAR &&
				    !mdb_parse_time(e->kids[i]->sval, i ? tl : tr, &tv)) {
					ERR("val: '%.256s' can't be parsed for DATE | DATETIME column\n", e->kids[i]->sval);
					return -MIDORIDB_ERROR;
				}
			if ((l->kind == MDB_EX_NULL || r->kind == MDB_EX_NULL) && e->op != MDB_CMP_EQ && e->op != MDB_CMP_NE) {
				ERR("NULL values can only use '=' or '<>' ops\n");
				return -MIDORIDB_ERROR;
			}
		}
		return MIDORIDB_OK;
	}
	case MDB_EX_ISNULL:
		/* (... and, in HAVING, a window item by its alias: LAG(v) OVER (...) AS prev ... HAVING prev IS NULL) */
		if (e->kids[0]->kind != MDB_EX_FIELD && !(e->kids[0]->kind == MDB_EX_WINDOW && is_having_clause(clause))) {
			ERR("only fields are allowed in IS NULL|IS NOT NULL\n");
			return -MIDORIDB_ERROR;
		}
		return MIDORIDB_OK;
	case MDB_EX_ISIN:
		if (e->kids[0]->kind != MDB_EX_FIELD) {
			ERR("Fields aren't allowed on IN-clauses\n");
			return -MIDORIDB_ERROR;
		}
		for (int i = 1; i < e->nkids; i++) {
			const struct mdb_expr *v = e->kids[i];
			if (v->kind != MDB_EX_INT && v->kind != MDB_EX_FLOAT && v->kind != MDB_EX_NULL && v->kind != MDB_EX_BOOL &&
			    v->kind != MDB_EX_STRING) {
				ERR("IN-clause can only contain raw values\n");
				return -MIDORIDB_ERROR;
			}
			if (v->kind == MDB_EX_STRING && e->kids[0]->type != MDB_CT_VARCHAR) {	/* (semantic_select.c:2308-2326) */
				ERR("val: '%.256s' requires an VARCHAR() column\n", v->sval);
				return -MIDORIDB_ERROR;
			}
			if ((v->kind == MDB_EX_INT && e->kids[0]->type != MDB_CT_INTEGER) ||
			    (v->kind == MDB_EX_BOOL && e->kids[0]->type != MDB_CT_TINYINT) ||
			    (v->kind == MDB_EX_FLOAT && e->kids[0]->type != MDB_CT_DOUBLE)) {
				ERR("comparison operands must have the same type\n");
				return -MIDORIDB_ERROR;
			}
		}
		return MIDORIDB_OK;
	case MDB_EX_COUNT:
		ERR("COUNT function can't be used in the %s-clause\n", clause);
		return -MIDORIDB_ERROR;
	case MDB_EX_AGG:
		ERR("%s function can't be used in the %s-clause\n", mdb_agg_name(e->op), clause);
		return -MIDORIDB_ERROR;
	case MDB_EX_LIKE:
		/* upstream parses LIKE, checks its operands (semantic_select.c) and then evaluates it - and NOT LIKE - to TRUE for every
		 * row, NULL cells included (executor_select.c:1027-1074: no case for it): a defect, not a semantics to keep.  Here it
		 * has SQL's meaning over a VARCHAR column and a string pattern ('%' any run of characters, '_' any one character; a
		 * NULL cell matches nothing, neither does it under NOT LIKE), SELECT only */
		if (dml || e->nkids != 2 || e->kids[0]->kind != MDB_EX_FIELD || e->kids[0]->type != MDB_CT_VARCHAR || e->kids[1]->kind != MDB_EX_STRING) {
			ERR("expressions in %s clause must be a type of comparison (LIKE takes a VARCHAR column and a string pattern)\n", clause);
			return -MIDORIDB_ERROR;
		}
		return MIDORIDB_OK;
	default:
		ERR("expressions in %s clause must be a type of comparison\n", clause);
		return -MIDORIDB_ERROR;
	}
}

int check_predicate(const struct mdb_expr *e, const char *clause, char *err, size_t errlen)
{
	return check_predicate_x(e, clause, false, err, errlen);
}

bool expr_has_count(const struct mdb_expr *e)
{
	if (e->kind == MDB_EX_COUNT)
		return true;
	for (int i = 0; i < e->nkids; i++)
		if (expr_has_count(e->kids[i]))
			return true;
	return false;
}

bool expr_has_agg(const struct mdb_expr *e)
{
	if (e->kind == MDB_EX_AGG)
		return true;
	for (int i = 0; i < e->nkids; i++)
		if (expr_has_agg(e->kids[i]))
			return true;
	return false;
}

/* every field under e appears in the select list ("SELECT list is not in <clause> clause", the reference's
 * wording, semantic_select.c:1836-1852, 1965-1985) */
int fields_in_select_list(const struct mdb_select *s, const struct mdb_expr *e, const char *clause, char *err, size_t errlen)
{
	int rc;
	if (e->kind == MDB_EX_FIELD && !s->select_all) {
		bool ok = false;
		for (int i = 0; i < s->nsel; i++)
			ok |= field_eq(s->sel[i], e);
		if (!ok) {
			ERR("SELECT list is not in %s clause: '%.128s'.'%.128s'\n", clause, e->tbl, e->col);
			return -MIDORIDB_ERROR;
		}
	}
	if (e->kind == MDB_EX_COUNT || e->kind == MDB_EX_AGG || e->kind == MDB_EX_WINDOW)
		return MIDORIDB_OK;	/* (an aggregate's column need not be selected: the aggregate itself must be, resolve_agg_refs) */
	for (int i = 0; i < e->nkids; i++)
		if ((rc = fields_in_select_list(s, e->kids[i], clause, err, errlen)))
			return rc;
	return MIDORIDB_OK;
}

/* ------------------------------------------------------------------ x [NOT] IN (SELECT ...)
 * An extension (the reference's grammar has value lists only).  The nested statement hangs beside the node's one kid (mdb_expr.sub), not
 * among its kids: it is resolved here on its own, against its own FROM tables alone - a correlated reference fails with the inner
 * statement's ordinary unknown-table / unknown-column error - and must deliver one column of the left operand's type. */
bool expr_has_subquery(const struct mdb_expr *e)
{
	if (!e)
		return false;
	if (e->sub)
		return true;
	for (int i = 0; i < e->nkids; i++)
		if (expr_has_subquery(e->kids[i]))
			return true;
	return false;
}

const char *coltype_name(int type)
{
	switch (type) {
	case MDB_CT_VARCHAR: return "VARCHAR";
	case MDB_CT_INTEGER: return "INTEGER";
	case MDB_CT_TINYINT: return "TINYINT";
	case MDB_CT_DOUBLE: return "DOUBLE";
	case MDB_CT_DATE: return "DATE";
	case MDB_CT_DATETIME: return "DATETIME";
	default: return "?";
	}
}

/* every subquery under e (resolved and checked already: the left operands are fields) */
int resolve_subqueries(struct mdb_catalog *cat, struct mdb_expr *e, char *err, size_t errlen)
{
	int rc;

	if (!e)
		return MIDORIDB_OK;
	for (int i = 0; i < e->nkids; i++)
		if ((rc = resolve_subqueries(cat, e->kids[i], err, errlen)))
			return rc;
	if (e->kind != MDB_EX_ISIN || !e->sub)
		return MIDORIDB_OK;
	if (cat->dist) {
		/* (known from the statement alone: every rank leaves here together, before anything is exchanged) */
		ERR("sharded mode: IN (SELECT ...) is not executed (subqueries run on one GPU)\n");
		return -MIDORIDB_ERROR;
	}
	struct mdb_select *q = e->sub;
	if (q->select_all || q->nsel != 1) {
		ERR("a subquery must select one column\n");
		return -MIDORIDB_ERROR;
	}
	if (!q->resolved && (rc = resolve_select(cat, q, err, errlen)))
		return rc;
	q->resolved = true;
	const struct mdb_expr *it = q->sel[0];
	const int have = it->kind == MDB_EX_COUNT ? MDB_CT_INTEGER : it->type, want = e->kids[0]->type;	/* (an aggregate: its result's type) */
	if (have != want) {
		ERR("IN (SELECT ...): the column '%.100s.%.100s' is %s, the subquery's column is %s: both sides must have the same type\n",
		    e->kids[0]->tbl, e->kids[0]->col, coltype_name(want), coltype_name(have));
		return -MIDORIDB_ERROR;
	}
	return MIDORIDB_OK;
}

int resolve_select(struct mdb_catalog *cat, struct mdb_select *s, char *err, size_t errlen)
{
	int rc;

	if (s->ntabs == 0) {
		ERR("SELECT without FROM is not supported by the MI355X path\n");
		return -MIDORIDB_ERROR;
	}
	if (s->ntabs > MDB_MAX_TABS) {
		ERR("more than %d tables in the FROM clause are not supported\n", MDB_MAX_TABS);
		return -MIDORIDB_ERROR;
	}
	for (int t = 0; t < s->ntabs; t++) {
		s->tabs[t].t = mdb_catalog_find(cat, s->tabs[t].name);
		if (!s->tabs[t].t) {
			ERR("table doesn't exist: '%.128s'\n", s->tabs[t].name);
			return -MIDORIDB_ERROR;
		}
		for (int u = 0; u < t; u++) {
			const char *a = s->tabs[t].alias[0] ? s->tabs[t].alias : s->tabs[t].name;
			const char *b = s->tabs[u].alias[0] ? s->tabs[u].alias : s->tabs[u].name;
			if (strcmp(a, b) == 0) {
				ERR("Not unique table/alias: '%.128s'\n", a);
				return -MIDORIDB_ERROR;
			}
			/* S1: bare column names must be unique across all FROM tables (semantic_select.c:2470-2478) */
			for (int c = 0; c < s->tabs[t].t->ncols; c++)
				for (int d = 0; d < s->tabs[u].t->ncols; d++)
					if (strcmp(s->tabs[t].t->cols[c].name, s->tabs[u].t->cols[d].name) == 0) {
						ERR("duplicate column name: '%s'\n", s->tabs[t].t->cols[c].name);
						return -MIDORIDB_ERROR;
					}
		}
		/* 1 INNER; 2 / 8 LEFT [OUTER], 4 / 10 RIGHT [OUTER], 6 / 12 FULL [OUTER] (the reference aborts on them, executor_select.c:1094: here SQL's meaning) */
		if (s->join_type[t] != 1 && !mdb_join_is_left(s->join_type[t]) && !mdb_join_is_right(s->join_type[t]) && !mdb_join_is_full(s->join_type[t])) {
			ERR("join type %d is not executed: INNER, LEFT [OUTER], RIGHT [OUTER] and FULL [OUTER] JOIN are\n", s->join_type[t]);
			return -MIDORIDB_ERROR;
		}
		if (s->join_type[t] != 1 && cat->dist) {
			/* (known from the statement alone: every rank leaves here together, before anything is exchanged) */
			ERR("sharded mode: LEFT / RIGHT OUTER JOIN is not executed (outer joins run on one GPU)\n");
			return -MIDORIDB_ERROR;
		}
	}
	/* `column AS name` / `COUNT(*) AS name` (upstream parses and checks aliases, then fails at execution: "cannot build columns hashtable" -
	 * SURVEY.md 8a D7; here the alias names the result column and may stand for its item in GROUP BY, HAVING and ORDER BY) */
	for (int i = 0; i < s->nsel; i++) {
		struct mdb_expr *e = s->sel[i];
		if (e->kind != MDB_EX_ALIAS || e->nkids != 1)
			continue;
		struct mdb_expr *kid = e->kids[0];
		if (kid->kind != MDB_EX_NAME && kid->kind != MDB_EX_FIELD && kid->kind != MDB_EX_COUNT && kid->kind != MDB_EX_AGG && kid->kind != MDB_EX_WINDOW)
			continue;	/* (an aliased expression: rejected below like the expression itself) */
		if (!s->sel_alias && !(s->sel_alias = calloc((size_t)s->nsel, sizeof(*s->sel_alias)))) {
			ERR("out of memory\n");
			return -MIDORIDB_NOMEM;
		}
		for (int k = 0; k < i; k++)
			if (s->sel_alias[k][0] && strcmp(s->sel_alias[k], e->col) == 0) {
				ERR("duplicate alias: '%.128s'\n", e->col);
				return -MIDORIDB_ERROR;
			}
		mdb_copy_name(s->sel_alias[i], e->col);
		e->nkids = 0;
		mdb_expr_free(e);
		s->sel[i] = kid;
	}
	int nagg = 0, nwin = 0;
	for (int i = 0; i < s->nsel; i++) {
		struct mdb_expr *e = s->sel[i];
		if (e->kind == MDB_EX_WINDOW) {
			/* fn(...) OVER (...): an extension (upstream has no OVER clause) */
			if (nwin == MDB_WIN_MAX_FNS) {
				ERR("more than %d window functions in one select list are not supported\n", MDB_WIN_MAX_FNS);
				return -MIDORIDB_ERROR;
			}
			if (cat->dist) {
				/* (known from the statement alone: every rank leaves here together, before anything is exchanged) */
				ERR("sharded mode: %s ... OVER is not executed (window functions run on one GPU)\n", mdb_win_name(e->op));
				return -MIDORIDB_ERROR;
			}
			if ((rc = resolve_window(s, e, err, errlen)))
				return rc;
			e->win_idx = nwin++;
			continue;
		}
		if (e->kind == MDB_EX_COUNT) {
			for (int k = 0; k < e->nkids; k++)
				if ((rc = resolve_expr(s, e->kids[k], err, errlen)))
					return rc;
			continue;
		}
		if (e->kind == MDB_EX_AGG) {
			/* SUM / MIN / MAX / AVG / COUNT(DISTINCT) over one column: an extension (upstream knows COUNT only) */
			if (++nagg > MDB_AGG_MAX_AGGS) {
				ERR("more than %d SUM / MIN / MAX / AVG aggregates in one select list are not supported\n", MDB_AGG_MAX_AGGS);
				return -MIDORIDB_ERROR;
			}
			if (cat->dist) {
				/* (known from the statement alone: every rank leaves here together, before anything is exchanged) */
				if (e->op == MDB_AGG_COUNT_DISTINCT)
					ERR("sharded mode: COUNT(DISTINCT) is not executed (COUNT(DISTINCT col) runs on one GPU)\n");
				else
					ERR("sharded mode: %s is not executed (SUM / MIN / MAX / AVG run on one GPU)\n", mdb_agg_name(e->op));
				return -MIDORIDB_ERROR;
			}
			if ((rc = resolve_agg(s, e, err, errlen)))
				return rc;
			continue;
		}
		if (expr_has_window(e)) {
			ERR("a window function inside an expression is not supported: fn(...) OVER (...) stands alone in the select list, with or without an alias\n");
			return -MIDORIDB_ERROR;
		}
		if (e->kind != MDB_EX_NAME && e->kind != MDB_EX_FIELD) {
			ERR("only columns, COUNT(*) and SUM / MIN / MAX / AVG of a column - with or without an alias - are supported in the select list (expressions are not executed by the reference)\n");
			return -MIDORIDB_ERROR;
		}
		if ((rc = resolve_expr(s, e, err, errlen)))
			return rc;
	}
	/* two window items without an alias that would name their result columns alike (their windows may differ: the name does not say) */
	for (int i = 0; nwin > 1 && i < s->nsel; i++)
		for (int k = 0; k < i; k++) {
			char a[MDB_NAME_LEN], b[MDB_NAME_LEN];
			if (s->sel[i]->kind != MDB_EX_WINDOW || s->sel[k]->kind != MDB_EX_WINDOW || (s->sel_alias && (s->sel_alias[i][0] || s->sel_alias[k][0])))
				continue;
			mdb_win_result_name(s->sel[i], a);
			mdb_win_result_name(s->sel[k], b);
			if (strcmp(a, b) == 0) {
				ERR("duplicate column name: '%s'\n", a);
				return -MIDORIDB_ERROR;
			}
		}
	for (int t = 1; t < s->ntabs; t++)
		if (s->on[t]) {
			if (expr_has_subquery(s->on[t])) {
				ERR("IN (SELECT ...) in JOIN ... ON is not supported: a subquery stands in WHERE or HAVING\n");
				return -MIDORIDB_ERROR;
			}
			if ((rc = resolve_expr(s, s->on[t], err, errlen)) || (rc = check_predicate(s->on[t], "JOIN ON", err, errlen)))
				return rc;
		}
	if (s->where && ((rc = resolve_expr(s, s->where, err, errlen)) || (rc = check_predicate(s->where, "where", err, errlen)) ||
			 (rc = resolve_subqueries(cat, s->where, err, errlen))))
		return rc;
	if (s->ngroup > MDB_SORT_MAX_KEYS) {
		ERR("GROUP BY over more than %d fields is not supported\n", MDB_SORT_MAX_KEYS);
		return -MIDORIDB_ERROR;
	}
	for (int i = 0; i < s->ngroup; i++) {
		subst_alias(s, s->group[i], false, false);
		if (s->group[i]->kind != MDB_EX_NAME && s->group[i]->kind != MDB_EX_FIELD) {
			ERR("group-by clauses support only fields and aliases\n");
			return -MIDORIDB_ERROR;
		}
		if ((rc = resolve_expr(s, s->group[i], err, errlen)))
			return rc;
	}
	/* S4: with GROUP BY or COUNT, every plain select field must be a GROUP BY field */
	{
		int ncount = 0, nfield = 0;
		if (nwin && s->ngroup) {
			ERR("a window function beside GROUP BY is not supported on the MI355X path\n");
			return -MIDORIDB_ERROR;
		}
		for (int i = 0; nwin && i < s->nsel; i++)
			if (s->sel[i]->kind == MDB_EX_COUNT || s->sel[i]->kind == MDB_EX_AGG) {
				ERR("a window function beside COUNT(*) or an aggregate without OVER is not supported on the MI355X path\n");
				return -MIDORIDB_ERROR;
			}
		for (int i = 0; i < s->nsel; i++) {
			if (s->sel[i]->kind == MDB_EX_WINDOW)
				continue;	/* (a value per row, like a field; no field of the statement has to be selected for it) */
			if (s->sel[i]->kind == MDB_EX_COUNT || s->sel[i]->kind == MDB_EX_AGG) {	/* (an aggregate stands where COUNT(*) may) */
				ncount++;
				continue;
			}
			nfield++;
			if (s->ngroup) {
				bool ok = false;
				for (int g = 0; g < s->ngroup; g++)
					ok |= field_eq(s->sel[i], s->group[g]);
				if (!ok) {
					ERR("SELECT list is not in GROUP BY clause: '%.128s'.'%.128s'\n", s->sel[i]->tbl, s->sel[i]->col);
					return -MIDORIDB_ERROR;
				}
			}
		}
		if (s->select_all && (s->ngroup || ncount)) {
			ERR("SELECT * can't be combined with GROUP BY / COUNT\n");
			return -MIDORIDB_ERROR;
		}
		if (ncount && nfield && !s->ngroup) {
			ERR("mixing fields and COUNT in the select list requires a GROUP BY clause\n");
			return -MIDORIDB_ERROR;
		}
		/* ---- DISTINCT / HAVING / ORDER BY / LIMIT: parsed and checked but never executed upstream (SURVEY 8a
		 *      D7); executed here with SQL semantics (8f row 4), under the reference's own semantic rules */
		if (s->distinct && (s->ngroup || ncount) && !nagg) {	/* (with an aggregate DISTINCT runs over the grouped stream, select_tail) */
			ERR("DISTINCT can't be combined with GROUP BY / COUNT on the MI355X path\n");
			return -MIDORIDB_ERROR;
		}
		if (s->having) {
			subst_alias(s, s->having, true, true);
			if ((rc = resolve_agg_refs(s, s->having, "HAVING", err, errlen)))
				return rc;
			if ((rc = resolve_expr(s, s->having, err, errlen)) || (rc = check_predicate(s->having, "having", err, errlen)))
				return rc;
			/* fields must come from the SELECT list (check_having_clause_inselect, semantic_select.c:1953-2001) */
			if ((rc = fields_in_select_list(s, s->having, "HAVING", err, errlen)))
				return rc;
			if ((rc = resolve_subqueries(cat, s->having, err, errlen)))
				return rc;
			if (expr_has_count(s->having) && !s->ngroup) {
				ERR("COUNT in the having-clause requires a GROUP BY clause on the MI355X path\n");
				return -MIDORIDB_ERROR;
			}
			if (nagg && !s->ngroup) {
				ERR("HAVING over an ungrouped aggregate is not supported on the MI355X path\n");
				return -MIDORIDB_ERROR;
			}
			if (ncount && !s->ngroup) {
				ERR("HAVING over an ungrouped COUNT is not supported on the MI355X path\n");
				return -MIDORIDB_ERROR;
			}
		}
		for (int i = 0; i < s->norder; i++) {
			struct mdb_expr *o = s->order[i];
			subst_alias(s, o, false, true);
			if (o->kind == MDB_EX_WINDOW) {	/* a window item by its alias: ordered by its result column */
				if (o->type == MDB_CT_VARCHAR) {	/* (LAG ... of a VARCHAR column: dictionary ids, as below) */
					ERR("ORDER BY over the VARCHAR column '%s' is not supported on the MI355X path\n", o->col);
					return -MIDORIDB_ERROR;
				}
				continue;
			}
			if (o->kind == MDB_EX_AGG) {	/* an aggregate of the select list, repeated or by its alias: ordered by its result column */
				if ((rc = resolve_agg_refs(s, o, "ORDER BY", err, errlen)))
					return rc;
				continue;
			}
			if (o->kind == MDB_EX_COUNT) {		/* check_orderby_clause_count, semantic_select.c:1755-1795 */
				ERR("COUNT function can't be used in the orderby-clause\n");
				return -MIDORIDB_ERROR;
			}
			if (o->kind != MDB_EX_NAME && o->kind != MDB_EX_FIELD) {	/* check_orderby_clause_expr :1718-1753 */
				ERR("order-by clauses support only fields and aliases\n");
				return -MIDORIDB_ERROR;
			}
			if ((rc = resolve_expr(s, o, err, errlen)) || (rc = fields_in_select_list(s, o, "ORDER BY", err, errlen)))
				return rc;
			if (o->type == MDB_CT_VARCHAR) {	/* cells are dictionary ids: equality only, no collation order */
				ERR("ORDER BY over the VARCHAR column '%s.%s' is not supported on the MI355X path\n", o->tbl, o->col);
				return -MIDORIDB_ERROR;
			}
		}
		if (s->norder > MDB_SORT_MAX_KEYS) {
			ERR("too many ORDER BY items (max %d)\n", MDB_SORT_MAX_KEYS);
			return -MIDORIDB_ERROR;
		}
	}
	return MIDORIDB_OK;
}
