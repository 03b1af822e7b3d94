/*
 * mdb_exec_internal.h - what the files of the executor share (mdb_exec.c: SELECT lowering - the driver, its plan stages, the stream
 * helpers; mdb_exec_join.c: one more FROM table into the stream, composite join keys; mdb_exec_result.c: projection and result assembly;
 * mdb_exec_resolve.c: plan normalisation and the semantic checks; mdb_exec_pred.c: predicate programs; mdb_exec_shard.c: sharded mode;
 * mdb_exec_tail.c: HAVING / DISTINCT / ORDER BY / LIMIT; mdb_exec_setop.c: UNION [ALL] / INTERSECT / EXCEPT over the results of several SELECTs;
 * mdb_exec_dml.c: CREATE / INSERT / DELETE / UPDATE).  Nothing here is part of the
 * library's interface.
 */
#ifndef MDB_EXEC_INTERNAL_H
#define MDB_EXEC_INTERNAL_H

#include "mdb_host.h"
#include <time.h>

#define ERR(...) snprintf(err, errlen, __VA_ARGS__)

#pragma GCC visibility push(hidden)

/* ------------------------------------------------------------------ device-side execution state */

struct dbuf_list {
	void **p;
	int n, cap;
};

struct where_split;

/* Which plan produced the tuple stream.  STREAM_ROWS: row-id vectors per FROM table (the general plan before it groups in any order, scan +
 * WHERE + projection).  Every other: the stream is the key column(s) d_fused_key[s] and, but for STREAM_JOIN_KEYS, d_count - no row ids. */
enum stream_plan {
	STREAM_ROWS = 0,
	STREAM_FUSED_CHAIN,	/* the single-key fused join + GROUP BY + COUNT(*) plan, chained over every FROM table (plan_fused_chain) */
	STREAM_FUSED_COMPOSITE,	/* the same operator on a packed composite key (composite_fused_plan) */
	STREAM_JOIN_KEYS,	/* the join of two key columns, nothing else selected (plan_keys_only) */
	STREAM_GROUP_KEYS,	/* the general plan's GROUP BY on one field in its any-order keys form, sharded or not */
};

struct exec {
	struct mdb_catalog *cat;
	mdb_dev_ctx *dev;
	struct mdb_select *s;
	char *err;
	size_t errlen;
	struct dbuf_list bufs;
	uint32_t *rid[MDB_MAX_TABS];	/* per FROM table: row-id vector of the current stream or NULL = identity */
	bool have_stream;		/* false until the first table is in the stream */
	uint64_t n;			/* stream length */
	int64_t *d_count;		/* COUNT(*) column of the stream (after GROUP BY), device */
	enum stream_plan plan;		/* which plan produced the stream (stream_is_keys: it is (d_fused_key, d_count), no row ids) */
	int64_t *d_fused_key;
	/* the fused plan on a packed composite key (composite_fused_plan): the stream carries nfused >= 2 key columns d_fused_keys[0 .. nfused)
	 * (d_fused_key is the first of them) and a map from the fields of the ON equalities to them - both sides of an equality name the
	 * same column.  nfused == 0: the stream has the one key column d_fused_key, whatever field is asked for (fused_key_column) */
	int nfused;
	int64_t *d_fused_keys[MDB_JOIN_KEY_MAX_COLS];
	int fused_tbl[2 * MDB_JOIN_KEY_MAX_COLS], fused_col[2 * MDB_JOIN_KEY_MAX_COLS], fused_at[2 * MDB_JOIN_KEY_MAX_COLS];
	int nfused_map;
	uint64_t joined_rows;
	/* per joined table: its equi-join key column holds, in every tuple of the stream, the value of an earlier table's column
	 * (INT64-represented types: the join compared all 64 bits; never NULL - a NULL key joins nothing): the projection reads
	 * that column, through the earlier table's row ids (ascending after a join: near-sequential reads instead of a random gather) */
	int same_col[MDB_MAX_TABS], same_as_tbl[MDB_MAX_TABS], same_as_col[MDB_MAX_TABS];
	/* sharded mode (cat->dist): a FROM table whose rows were exchanged is read through a SHADOW table - the same schema over the
	 * columns this rank received - that stands in s->tabs[t].t for the rest of the statement (orig_tab[] puts the catalog's
	 * tables back at the end).  part[]: the fields whose value the current stream is hash-partitioned by (all equal in every
	 * tuple: the equi-join keys tied together so far); need[t][c]: the statement reads column c of table t */
	struct mdb_table *shadow[MDB_MAX_TABS], *orig_tab[MDB_MAX_TABS];
	const struct mdb_expr *part[2 * MDB_MAX_TABS];
	int npart;
	bool promised;		/* the exchange handle holds this statement's key ranges (shard_promise_ranges) */
	bool dict_synced;	/* the ranks' string dictionaries were made known to each other for this statement (shard_dict_sync) */
	bool need[MDB_MAX_TABS][MDB_MAX_COLS];
	const struct where_split *ws;		/* the WHERE conjuncts pushed down to single tables (general plan; NULL: none are) */
	int joins_eliminated;			/* tables that were not joined at all: the catalog said every row of the stream has exactly one partner (join_next_table) */
	int composite_joins;			/* joins that ran on a packed composite key (composite_join_keys) */
	int composite_fused;			/* the statement ran the fused join + GROUP BY operator on a packed composite key (composite_fused_plan) */
	bool joined_ahead[MDB_MAX_TABS];	/* table t was joined together with an earlier table on the same key (join_with_payload_multi) */
	/* LEFT / RIGHT OUTER JOIN: rid[t] may hold MDB_NO_ROW (table t is the NULL-supplied side of a join that left rows without partner) -
	 * every column of t read through rid[t] needs a NULL bitmap of its own, whether or not the column has one */
	bool may_be_absent[MDB_MAX_TABS];
	bool pred_err_said;			/* pred_compile() failed for a cause it has written into err itself (pred_compile_failed keeps it) */
	bool has_outer;				/* some join of the statement is an outer join: no plan that assumes inner semantics */
	/* SUM / MIN / MAX / AVG: the select list's aggregates, each (function, column) once.  After GROUP BY (or over the whole stream, without one)
	 * d_agg[i] / d_agg_nulls[i] are their result columns over the grouped stream: row k belongs to row k of the stream, as d_count[k] does, and
	 * follows it through HAVING, DISTINCT, ORDER BY and LIMIT (stream_apply_sel).  A statement with one of them takes the general plan only */
	int nagg;
	int agg_op[MDB_AGG_MAX_AGGS], agg_tbl[MDB_AGG_MAX_AGGS], agg_col[MDB_AGG_MAX_AGGS], agg_type[MDB_AGG_MAX_AGGS];	/* agg_type: the result's column type */
	void *d_agg[MDB_AGG_MAX_AGGS];
	uint64_t *d_agg_nulls[MDB_AGG_MAX_AGGS];
	int agg_calls[2];			/* mdb_dev_group_aggregate calls by form: [0] groups in LDS, [1] sorted segments */
	/* window functions: the select list's fn(...) OVER (...) items, win_item[i] the item with win_idx i.  After FROM / WHERE d_win[i] /
	 * d_win_nulls[i] are their result columns over the stream (stream_windows): row k belongs to row k of the stream and follows it
	 * through HAVING, DISTINCT, ORDER BY and LIMIT as d_agg[] does.  A statement with one of them takes the general plan only */
	int nwin;
	const struct mdb_expr *win_item[MDB_WIN_MAX_FNS];
	void *d_win[MDB_WIN_MAX_FNS];
	uint64_t *d_win_nulls[MDB_WIN_MAX_FNS];
	int win_calls;				/* mdb_dev_window calls: one per distinct OVER clause */
	int cd_calls[2];			/* COUNT(DISTINCT) items answered by mdb_dev_group_count_distinct, by form: [0] bitmap, [1] sorted */
};

static inline bool stream_is_keys(const struct exec *x) { return x->plan != STREAM_ROWS; }

/* which of the statement's aggregates e (MDB_EX_AGG, resolved) is; -1: none */
static inline int agg_index(const struct exec *x, const struct mdb_expr *e)
{
	for (int i = 0; i < x->nagg; i++)
		if (x->agg_op[i] == e->op && x->agg_tbl[i] == e->tbl_idx && x->agg_col[i] == e->col_idx)
			return i;
	return -1;
}

struct pred_prog {
	struct mdb_pred_insn insn[MDB_PRED_MAX_INSNS];
	int n;
	struct mdb_col_binding cols[MDB_PRED_MAX_SLOTS];
	int slot_tbl[MDB_PRED_MAX_SLOTS], slot_col[MDB_PRED_MAX_SLOTS];
	int ncols;
};

#define PUSH_MAX 16
#define PUSH_TABS MDB_MAX_TABS
struct where_split {
	const struct mdb_expr *push[PUSH_TABS][PUSH_MAX];
	int npush[PUSH_TABS];
	const struct mdb_expr *residual[64];
	int nresidual;
};

/* The result column plan: every column the statement could return - COUNT(*) if selected, the aggregates, then every column of every FROM
 * table left to right - named, put into the reference's order (R3), and of those the ones that are wanted (result_cols_build / _free) */
struct result_cols {
	char (*keys)[MDB_NAME_LEN];	/* candidate k's result column name */
	int *order;			/* the candidates in the reference's order */
	int *tbl, *col;			/* candidate k's source: tbl = FROM table and col = its column, or COLSRC_COUNT / COLSRC_AGG(a) */
	int *src;			/* result column c is candidate src[c] */
	int nkeys, ncols;
	int has_count;			/* the select list names COUNT(*) */
};
#define COLSRC_COUNT (-1)
#define COLSRC_AGG(a) (-2 - (a))
#define COLSRC_WIN(w) (-100 - (w))
/* which of the statement's aggregates a candidate's source is; -1: none (COUNT(*), a window item or a table column) */
static inline int colsrc_agg(int tbl) { return tbl <= -2 && tbl > -100 ? -2 - tbl : -1; }
/* ... which of its window items; -1: none */
static inline int colsrc_win(int tbl) { return tbl <= -100 ? -100 - tbl : -1; }

/* What one SELECT statement's stages share beside the stream (struct exec): the result column plan and the statement's shape, computed
 * once (select_shape) */
struct select_stmt {
	struct result_cols rc;
	struct where_split ws;
	bool split_ok;			/* ws holds the WHERE clause's conjuncts (where_split) */
	bool only_count;		/* SELECT COUNT(*) alone, no GROUP BY */
	bool has_agg;			/* SUM / MIN / MAX / AVG in the select list */
	bool has_win;			/* a window function in the select list: the general plan only */
	bool fused_chain;		/* the single-key fused plan applies; fkeys[t] = table t's key field of the chain */
	const struct mdb_expr *fkeys[MDB_MAX_TABS];
	bool keys_only;			/* the keys-only plan applies; kj[0..1] = the two key fields */
	const struct mdb_expr *kj[2];
	int64_t *keys_ordered;		/* ... answered in the reference's order already (keys_only_ordered) */
	uint64_t keys_ordered_rows;
	void **direct_vals;		/* scan + WHERE + projection plan: the result columns on the device, final */
	uint64_t **direct_nulls;
};

/* join types as the parser numbers them (mdb_sql.c: LEFT 2, RIGHT 4, FULL 6, + 6 with OUTER; the reference's grammar, midorisql.y:229-233) */
static inline bool mdb_join_is_left(int jt) { return jt == 2 || jt == 8; }
static inline bool mdb_join_is_right(int jt) { return jt == 4 || jt == 10; }
/* FULL [OUTER]: this grammar's own, numbered like the others - LEFT 2 + RIGHT 4, + 6 with OUTER */
static inline bool mdb_join_is_full(int jt) { return jt == 6 || jt == 12; }

extern __thread const struct mdb_strdict *stmt_dict;	/* the statement's string dictionary (VARCHAR literals) */

bool field_eq(const struct mdb_expr *a, const struct mdb_expr *b);
int resolve_expr(struct mdb_select *s, struct mdb_expr *e, char *err, size_t errlen);
bool is_having_clause(const char *clause);
int operand_type(const struct mdb_expr *o, const struct mdb_expr *other, bool dml);
int check_predicate_x(const struct mdb_expr *e, const char *clause, bool dml, char *err, size_t errlen);
int check_predicate(const struct mdb_expr *e, const char *clause, char *err, size_t errlen);
bool expr_has_count(const struct mdb_expr *e);
bool expr_has_agg(const struct mdb_expr *e);
bool expr_has_window(const struct mdb_expr *e);
bool window_same_over(const struct mdb_expr *a, const struct mdb_expr *b);
const char *mdb_win_name(int op);
void mdb_win_result_name(const struct mdb_expr *e, char *out);
int stream_windows(struct exec *x);
bool agg_eq(const struct mdb_expr *a, const struct mdb_expr *b);
const char *mdb_agg_name(int op);
const char *mdb_agg_open(int op);
int mdb_agg_result_type(int op, int coltype);
int fields_in_select_list(const struct mdb_select *s, const struct mdb_expr *e, const char *clause, char *err, size_t errlen);
int resolve_select(struct mdb_catalog *cat, struct mdb_select *s, char *err, size_t errlen);
bool expr_has_subquery(const struct mdb_expr *e);
int resolve_subqueries(struct mdb_catalog *cat, struct mdb_expr *e, char *err, size_t errlen);
int subqueries_eval(struct mdb_catalog *cat, struct mdb_expr *e, char *err, size_t errlen);
void subqueries_release(struct mdb_catalog *cat, struct mdb_expr *e);
int dev_fail(struct exec *x, const char *what);
int dist_fail(struct exec *x, const char *what);
int track(struct exec *x, void *p);
void *dalloc(struct exec *x, size_t bytes);
void free_all(struct exec *x);
int stream_select(struct exec *x, int ntabs_in_stream, const uint32_t *sel, uint64_t n_new);
int stream_apply_sel(struct exec *x, int ntabs_in_stream, const uint32_t *sel, uint64_t n_new);
int64_t *fused_key_column(const struct exec *x, int tbl_idx, int col_idx);
int stream_column(struct exec *x, const struct mdb_expr *f, const int64_t **vals, const uint64_t **nulls);
int double_join_keys(struct exec *x, const struct mdb_column *col, const uint32_t *rid, uint64_t n, const void **vals, const uint64_t **nulls);
void mark_needed(struct exec *x, const struct mdb_expr *e);
void mark_needed_all(struct exec *x);
bool in_part(const struct exec *x, const struct mdb_expr *f);
int shard_dict_sync(struct exec *x);
int shard_ids(struct exec *x, const int64_t *cells, uint64_t n, bool to_common, bool in_place, const int64_t **out);
#define SHARD_BROADCAST (1u << 30)	/* shard_rows flag: every rank's rows to every rank (mdb_dist_broadcast_rows) instead of rows by key */
int shard_rows(struct exec *x, const int *tabs, int nt, uint32_t *const *rid_of, uint64_t n, const int64_t *kv, const uint64_t *kn, uint32_t flags, uint64_t *n_out);
int shard_stream(struct exec *x, int nt, const struct mdb_expr *f, uint32_t flags);
int shard_promise_ranges(struct exec *x, const struct mdb_expr *fl, const struct mdb_expr *fr);
void shard_cleanup(struct exec *x);
void bind_operand(struct exec *x, const struct mdb_expr *f, const void **values, const uint64_t **nullbits, const uint32_t **rid);
int pred_slot(struct exec *x, struct pred_prog *p, const struct mdb_expr *f);
int pred_emit(struct pred_prog *p, int op, int cmp, int type, int a, int b, int64_t imm);
int64_t lit_bits_for(const struct mdb_expr *v, int coltype);
bool const_cmp(int op, const struct mdb_expr *l, const struct mdb_expr *r);
int pred_compile(struct exec *x, struct pred_prog *p, const struct mdb_expr *e);
void pred_compile_failed(struct exec *x);
int stream_filter(struct exec *x, int ntabs_in_stream, const struct mdb_expr *e);
void collect_conjuncts(struct mdb_expr *e, struct mdb_expr **out, int *n, int cap);
uint64_t expr_tables(const struct mdb_expr *e);
bool where_split(const struct mdb_select *s, struct where_split *w);
int table_filter(struct exec *x, int t, const struct mdb_expr *const *conj, int nconj, const uint32_t **sel, uint64_t *m);
int table_column(struct exec *x, int t, const struct mdb_expr *key, const uint32_t *sel, uint64_t m, const void **vals, const uint64_t **nulls);
int fused_operand(struct exec *x, int t, const struct mdb_expr *key, const struct mdb_expr *const *conj, int nconj, const void **vals, const uint64_t **nulls, uint64_t *n);
int join_with_payload(struct exec *x, int t, const struct mdb_expr *kr, const int64_t *vl, const uint64_t *nl, const void *vr, const uint64_t *nr, uint64_t r_rows);
int join_next_table(struct exec *x, int t, const struct mdb_expr *const *pconj, int npconj);
bool join_is_total_by_catalog(struct exec *x, const struct mdb_expr *kl, const struct mdb_expr *kr);
bool only_key_needed(const struct exec *x, int t, int key_col);
int composite_fused_plan(struct exec *x, const struct where_split *ws, bool only_count);
int result_column_to_host(mdb_dev_ctx *dev, struct mdb_result *res, int c, const void *d_vals, const uint64_t *d_nulls);
int project_result(struct exec *x, const struct select_stmt *st, struct mdb_result *res);
double now_ms(void);
int fused_chain(struct mdb_select *s, const struct mdb_expr **keys, bool count_only);
bool keys_only_join(const struct mdb_select *s, const struct mdb_catalog *cat, const struct result_cols *rc, bool has_agg, const struct mdb_expr **kj);
int select_tail(struct exec *x, int has_count);
uint64_t order_rows_wanted(uint64_t n, bool has_limit, int64_t limit_off, int64_t limit_cnt);
int order_perm(mdb_dev_ctx *dev, const struct mdb_sort_key *keys, int nkeys, uint64_t n, uint64_t want, uint32_t *perm);
void limit_window(uint64_t n, int64_t limit_off, int64_t limit_cnt, uint64_t *off, uint64_t *cnt);
const char *coltype_name(int type);
void result_column_name(const struct exec *x, const struct result_cols *rc, int c, char *out);
int result_column_type(const struct exec *x, const struct result_cols *rc, int c);
/* a compound statement (UNION [ALL] / INTERSECT / EXCEPT; mdb_exec_setop.c) and what it asks of the executor of one SELECT */
int result_column_list_place(const struct exec *x, const struct result_cols *rc, int c);
struct select_signature {
	int ncols;
	char (*name)[MDB_NAME_LEN];	/* result column c's name and column type */
	int *type;
	int *at;			/* at[i] = the result column that the i-th (different) item of the select list delivers: a result's columns stand
					 * in the reference's order (R3), the arms of a compound correspond by their lists */
};
int select_signature(struct mdb_select *s, struct select_signature *sig, char *err, size_t errlen);
void select_signature_free(struct select_signature *sig);
int exec_select_one(struct mdb_catalog *cat, struct mdb_select *s, struct mdb_result **out, char *err, size_t errlen);
int exec_setop(struct mdb_catalog *cat, struct mdb_select *s, struct mdb_result **out, char *err, size_t errlen);
int dml_value_on_left(const struct mdb_expr *e);
int dml_check_values(const struct mdb_expr *e, char *err, size_t errlen);
int dml_select_rows(struct mdb_catalog *cat, struct mdb_dml *d, struct exec *x, struct mdb_select *s, struct mdb_from_tab *tab, bool complement, struct mdb_table **out_t, const uint32_t **sel, uint64_t *m, char *err, size_t errlen);

#pragma GCC visibility pop
/* the catalog's statistics of an operator call's key columns (mdb_exec.c) */
void op_stats_begin(struct exec *x, const struct mdb_expr *fl, const void *pl, const struct mdb_expr *fr, const void *pr);
void op_stats_end(struct exec *x);
uint64_t op_groups_bound(struct exec *x, const struct mdb_expr *f, uint64_t rows);

#endif
