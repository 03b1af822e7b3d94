/*
 * mdb_sql.c - hand-written SQL-subset front end.
 *
 * The reference front end is a flex lexer + bison grammar (reference
 * src/parser/midorisql.l, src/parser/midorisql.y) whose only product is a FIFO of
 * RPN token strings (emit(), midorisql.y:517-528) consumed by the AST builder.
 * Neither tool exists in this image or on the GPU box, and the front end is out of
 * scope for this build - a MidoriDB maintainer keeps the
 * bison/flex parser and hands its queue to mdb_query_execute_rpn().
 * This file exists so that SQL text works without bison: a small precedence-climbing
 * parser that emits the SAME token vocabulary in the SAME order as the grammar's
 * reductions, for the statements the SELECT path and its tests need:
 *
 *   SELECT [DISTINCT] exprs FROM refs [WHERE] [GROUP BY] [HAVING] [ORDER BY] [LIMIT] ;
 *       (in its expressions, and in those of DELETE / UPDATE:  x [NOT] IN ( SELECT ... ), nested up to 8 deep)
 *   CREATE TABLE [IF NOT EXISTS] t (col type [attrs], ...) ;
 *   INSERT [INTO] t [(cols)] VALUES (...), (...) ;
 *
 * Window functions - an extension, in a SELECT list only (the reference's grammar has no OVER clause):
 *
 *   ROW_NUMBER() | RANK() | DENSE_RANK() | COUNT(*) | SUM(col) | MIN(col) | MAX(col) | AVG(col)
 *       OVER ( [PARTITION BY f, ...] [ORDER BY f [ASC|DESC], ...] )          f: col | tbl.col
 *
 * emit this project's own tokens, in the style of "AGG SUM":
 *
 *   [NAME col | FIELDNAME tbl.col]          the argument of SUM / MIN / MAX / AVG (nothing for the other four)
 *   NAME | FIELDNAME ...                    the PARTITION BY fields, in order
 *   NAME | FIELDNAME, WINORDER d ...        every ORDER BY field, wrapped: d = 0 ASC, 1 DESC
 *   WINDOW fn npart norder                  closes the item: fn = ROW_NUMBER | RANK | DENSE_RANK | COUNT | SUM | MIN | MAX | AVG
 *
 * and the navigation functions
 *
 *   LAG(col [, k [, default]]) | LEAD(col [, k [, default]]) | FIRST_VALUE(col) | LAST_VALUE(col) | NTILE(n)     OVER ( ... )
 *       col: col | tbl.col; k: a non-negative integer literal (default 1); n: a positive integer literal; default: a literal or NULL
 *
 * emit the column as SUM's argument is emitted, then the literals as their own tokens and one word that closes them:
 *
 *   NAME col | FIELDNAME tbl.col            (not NTILE)
 *   [NUMBER k [NUMBER | FLOAT | BOOL | STRING | NULL]], WINARG count      LAG / LEAD: count = 0 ... 2;  NTILE: NUMBER n, WINARG 1;
 *                                           FIRST_VALUE / LAST_VALUE: nothing
 *   ... the PARTITION BY fields, the ORDER BY items, WINDOW LAG | LEAD | FIRST_VALUE | LAST_VALUE | NTILE npart norder
 *
 * IGNORE NULLS / RESPECT NULLS, FROM FIRST / FROM LAST, an offset or default that is no literal, a negative offset, NTILE(0), NTILE of a
 * column, LAG() without a column and DISTINCT inside are refused, each with a text of its own.  LAG / LEAD / FIRST_VALUE / LAST_VALUE /
 * NTILE are functions only with the parenthesis right behind the name, as ROW_NUMBER is.
 *
 * No word becomes reserved for it: ROW_NUMBER / RANK / DENSE_RANK are functions only with the parenthesis right behind the name (as
 * SUM( is), OVER is a window only behind the `)` of one of the eight functions and in front of `(`, PARTITION only inside that
 * parenthesis.  `SELECT SUM(v) over FROM A` still aliases the aggregate as `over`.
 *
 * Set operations - an extension too (the reference's grammar has one SELECT per statement):
 *
 *   SELECT ... { (UNION [ALL | DISTINCT] | INTERSECT [DISTINCT] | EXCEPT [DISTINCT]) SELECT ... }
 *       [ORDER BY name [ASC|DESC], ...] [LIMIT [off,] cnt] ;                 at most 8 arms, evaluated left to right
 *
 * Every arm emits what it emits as a statement of its own, "SELECT d n" included; then, in the style of "WINDOW fn npart norder":
 *
 *   SETOP UNION | UNIONALL | INTERSECT | EXCEPT     behind every arm but the first: combines the two plans on top of the stack
 *   NAME col, SETORDER d ...                        every ORDER BY item behind the last arm: a bare result column name, d = 0 ASC, 1 DESC
 *   NUMBER ..., SETLIMIT n                          LIMIT cnt (n = 1) | LIMIT off, cnt (n = 2)
 *   COMPOUND narms norder nlimit                    closes the compound: nlimit = 0 | 1 (a SETLIMIT item precedes)
 *
 * The RPN of a statement without a set operator is what it was.  No word becomes reserved: union, intersect, except and all are
 * operators only when the token behind them is SELECT, or ALL / DISTINCT followed by SELECT (setop_follows); everywhere else they stay
 * names and implicit aliases.  A chain in which INTERSECT stands behind UNION or EXCEPT is refused: the standard binds INTERSECT
 * tighter, SQLite reads left to right, and there are no parentheses to say which.
 *
 * Operator precedence follows midorisql.y:48-63; literal lexing follows
 * midorisql.l:83-92 (a '-' directly in front of digits belongs to the number).
 * The emitted queue is accepted unchanged by the reference's ast_build_tree()
 * (checked in tests/test_cpu_frontend_abi.py against oracle/_ref).
 */
#include "mdb_host.h"
#include <ctype.h>
#include <limits.h>
#include <strings.h>

enum tk {
	T_EOF, T_NAME, T_STRING, T_INT, T_FLOAT, T_BOOL, T_CMP, T_PUNCT, T_KW, T_FCOUNT, T_FAGG, T_FWIN, T_FNAV, T_ANDOP, T_OROP, T_ERR
};

static const char *const KEYWORDS[] = {
	"AND", "AS", "ASC", "AUTO_INCREMENT", "BY", "CREATE", "DATE", "DATETIME", "DELETE", "DESC", "DISTINCT",
	"DOUBLE", "EXISTS", "FROM", "FULL", "GROUP", "HAVING", "IF", "IN", "INDEX", "INNER", "INSERT", "INT",
	"INT4", "INTEGER", "INTO", "IS", "JOIN", "KEY", "LEFT", "LIKE", "LIMIT", "MOD", "NOT", "NULL",
	"ON", "OR", "ORDER", "OUTER", "PRIMARY", "RIGHT", "SELECT", "SET", "TABLE", "TINYINT", "UNIQUE", "UPDATE",
	"VALUE", "VALUES", "VARCHAR", "VARCHARACTER", "WHERE", "XOR", NULL
};

struct lexer {
	const char *s;
	size_t pos;
	enum tk type;
	char text[256];		/* NAME / STRING (with quotes) / keyword upper-cased / punct */
	long ival;
	long long wval;		/* T_INT: the literal at full width (ival is what the reference's 32-bit lexer makes of it) */
	double fval;
	int sub;		/* comparison code */
};

struct parser {
	struct lexer lx;
	struct mdb_rpn *out;
	char *err;
	size_t errlen;
	bool failed;
	bool dml;		/* inside delete_expr / update_expr: names, literals, logic, comparisons, IS NULL, IN only */
	int depth;		/* nested SELECTs open: IN (SELECT ...) */
	bool sel_list;		/* inside the select list of a SELECT: the one place where fn(...) OVER (...) is a window function */
	bool arm;		/* parsing an arm of a compound behind the first: ORDER BY / LIMIT are not the arm's, they close the compound */
	bool had_tail;		/* the SELECT parsed last had an ORDER BY or LIMIT of its own */
};

#define MAX_SUBQUERY_DEPTH 8
#define MAX_SETOP_ARMS 8

static void fail(struct parser *p, const char *fmt, ...)
{
	va_list ap;
	if (p->failed)
		return;
	p->failed = true;
	va_start(ap, fmt);
	if (p->err && p->errlen)
		vsnprintf(p->err, p->errlen, fmt, ap);
	va_end(ap);
}

static void emit(struct parser *p, const char *fmt, ...)
{
	char buf[256];
	va_list ap;
	if (p->failed)
		return;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	if (mdb_rpn_push(p->out, buf))
		fail(p, "out of memory");
}

static bool is_keyword(const char *up)
{
	for (int i = 0; KEYWORDS[i]; i++)
		if (strcmp(KEYWORDS[i], up) == 0)
			return true;
	return false;
}

static void next(struct parser *p)
{
	struct lexer *l = &p->lx;
	const char *s = l->s;
	size_t i = l->pos;

	for (;;) {
		while (s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r')
			i++;
		if (s[i] == '#' || (s[i] == '-' && s[i + 1] == '-' && (s[i + 2] == ' ' || s[i + 2] == '\t'))) {
			while (s[i] && s[i] != '\n')
				i++;
			continue;
		}
		if (s[i] == '/' && s[i + 1] == '*') {
			i += 2;
			while (s[i] && !(s[i] == '*' && s[i + 1] == '/'))
				i++;
			if (s[i])
				i += 2;
			continue;
		}
		break;
	}
	l->text[0] = 0;
	if (!s[i]) {
		l->type = T_EOF;
		l->pos = i;
		return;
	}
	/* numbers: -?[0-9]+ | -?[0-9]+"."[0-9]* | -?"."[0-9]+ | exponent forms (midorisql.l:85-92) */
	{
		size_t j = i;
		bool isnum = false, isfloat = false;
		if (s[j] == '-')
			j++;
		if (isdigit((unsigned char)s[j])) {
			isnum = true;
			while (isdigit((unsigned char)s[j]))
				j++;
			if (s[j] == '.') {
				isfloat = true;
				j++;
				while (isdigit((unsigned char)s[j]))
					j++;
			}
		} else if (s[j] == '.' && isdigit((unsigned char)s[j + 1])) {
			isnum = isfloat = true;
			j++;
			while (isdigit((unsigned char)s[j]))
				j++;
		}
		if (isnum && (s[j] == 'E' || s[j] == 'e')) {
			size_t k = j + 1;
			if (s[k] == '+' || s[k] == '-')
				k++;
			if (isdigit((unsigned char)s[k])) {
				while (isdigit((unsigned char)s[k]))
					k++;
				j = k;
				isfloat = true;
			}
		}
		if (isnum) {
			char tmp[128];
			size_t len = j - i < sizeof(tmp) - 1 ? j - i : sizeof(tmp) - 1;
			memcpy(tmp, s + i, len);
			tmp[len] = 0;
			if (isfloat) {
				l->type = T_FLOAT;
				l->fval = atof(tmp);
			} else {
				l->type = T_INT;
				l->ival = atoi(tmp);	/* 32-bit, as the reference lexer (midorisql.l:85) */
				l->wval = strtoll(tmp, NULL, 10);
			}
			l->pos = j;
			return;
		}
	}
	if (s[i] == '\'' || s[i] == '"') {
		char q = s[i];
		size_t j = i + 1;
		while (s[j] && s[j] != '\n') {
			if (s[j] == '\\' && s[j + 1]) {
				j += 2;
				continue;
			}
			if (s[j] == q) {
				if (s[j + 1] == q) {
					j += 2;
					continue;
				}
				break;
			}
			j++;
		}
		if (s[j] != q) {
			l->type = T_ERR;
			fail(p, "Unterminated string");
			return;
		}
		j++;
		{
			size_t len = j - i < sizeof(l->text) - 1 ? j - i : sizeof(l->text) - 1;
			memcpy(l->text, s + i, len);
			l->text[len] = 0;
		}
		l->type = T_STRING;
		l->pos = j;
		return;
	}
	if (s[i] == '`') {
		size_t j = i + 1, len;
		while (s[j] && s[j] != '`' && s[j] != '\n')
			j++;
		if (s[j] != '`') {
			l->type = T_ERR;
			fail(p, "unterminated quoted name");
			return;
		}
		len = j - i - 1 < sizeof(l->text) - 1 ? j - i - 1 : sizeof(l->text) - 1;
		memcpy(l->text, s + i + 1, len);
		l->text[len] = 0;
		l->type = T_NAME;
		l->pos = j + 1;
		return;
	}
	if (isalpha((unsigned char)s[i])) {
		size_t j = i, len;
		char up[256];
		while (isalnum((unsigned char)s[j]) || s[j] == '_')
			j++;
		len = j - i < sizeof(l->text) - 1 ? j - i : sizeof(l->text) - 1;
		memcpy(l->text, s + i, len);
		l->text[len] = 0;
		for (size_t k = 0; k <= len; k++)
			up[k] = (char)toupper((unsigned char)l->text[k]);
		l->pos = j;
		if (strcmp(up, "COUNT") == 0 && s[j] == '(') {	/* midorisql.l:139-142 */
			l->type = T_FCOUNT;
			return;
		}
		/* SUM( MIN( MAX( AVG( - an extension (upstream lexes COUNT( only): a function only with the parenthesis right behind the name,
		 * as COUNT; a column called `sum` stays a name */
		if (s[j] == '(' && (strcmp(up, "SUM") == 0 || strcmp(up, "MIN") == 0 || strcmp(up, "MAX") == 0 || strcmp(up, "AVG") == 0)) {
			l->type = T_FAGG;
			strcpy(l->text, up);
			return;
		}
		/* ROW_NUMBER( RANK( DENSE_RANK( - the ranking window functions, functions only with the parenthesis right behind the name: a
		 * column, table or alias called `rank` stays a name (text keeps the spelling: CREATE TABLE rank(...) names a table) */
		if (s[j] == '(' && (strcmp(up, "ROW_NUMBER") == 0 || strcmp(up, "RANK") == 0 || strcmp(up, "DENSE_RANK") == 0)) {
			l->type = T_FWIN;
			return;
		}
		/* LAG( LEAD( FIRST_VALUE( LAST_VALUE( NTILE( - the navigation window functions, by the same rule */
		if (s[j] == '(' && (strcmp(up, "LAG") == 0 || strcmp(up, "LEAD") == 0 || strcmp(up, "FIRST_VALUE") == 0 || strcmp(up, "LAST_VALUE") == 0 ||
				    strcmp(up, "NTILE") == 0)) {
			l->type = T_FNAV;
			return;
		}
		if (strcmp(up, "TRUE") == 0 || strcmp(up, "FALSE") == 0 || strcmp(up, "UNKNOWN") == 0) {
			l->type = T_BOOL;
			l->ival = up[0] == 'T' ? 1 : (up[0] == 'F' ? 0 : -1);
			return;
		}
		if (is_keyword(up)) {
			l->type = T_KW;
			strcpy(l->text, up);
			return;
		}
		l->type = T_NAME;
		return;
	}
	/* operators */
	l->pos = i + 1;
	l->type = T_PUNCT;
	l->text[0] = s[i];
	l->text[1] = 0;
	switch (s[i]) {
	case '&':
		if (s[i + 1] == '&') {
			l->pos = i + 2;
			l->type = T_ANDOP;
		}
		return;
	case '|':
		if (s[i + 1] == '|') {
			l->pos = i + 2;
			l->type = T_OROP;
		}
		return;
	case '=':
		l->type = T_CMP;
		l->sub = 4;
		return;
	case '>':
		l->type = T_CMP;
		if (s[i + 1] == '=') {
			l->sub = 6;
			l->pos = i + 2;
		} else {
			l->sub = 2;
		}
		return;
	case '<':
		l->type = T_CMP;
		if (s[i + 1] == '=') {
			l->sub = 5;
			l->pos = i + 2;
		} else if (s[i + 1] == '>') {
			l->sub = 3;
			l->pos = i + 2;
		} else {
			l->sub = 1;
		}
		return;
	case '!':
		if (s[i + 1] == '=') {
			l->type = T_CMP;
			l->sub = 3;
			l->pos = i + 2;
		}
		return;
	case '-': case '+': case '*': case '/': case '%': case '(': case ')': case ',': case '.': case ';':
		return;
	default:
		l->type = T_ERR;
		fail(p, "mystery character '%c'", s[i]);
		return;
	}
}

static bool is_kw(struct parser *p, const char *kw)
{
	return p->lx.type == T_KW && strcmp(p->lx.text, kw) == 0;
}

static bool is_punct(struct parser *p, char c)
{
	return p->lx.type == T_PUNCT && p->lx.text[0] == c;
}

static bool accept_kw(struct parser *p, const char *kw)
{
	if (is_kw(p, kw)) {
		next(p);
		return true;
	}
	return false;
}

static void expect_punct(struct parser *p, char c)
{
	if (!is_punct(p, c)) {
		fail(p, "syntax error, unexpected '%s', expecting '%c'", p->lx.type == T_EOF ? "end of input" : p->lx.text, c);
		return;
	}
	next(p);
}

static void expect_kw(struct parser *p, const char *kw)
{
	if (!accept_kw(p, kw))
		fail(p, "syntax error, unexpected '%s', expecting %s", p->lx.type == T_EOF ? "end of input" : p->lx.text, kw);
}

/* precedence levels (midorisql.y:48-63), low to high */
enum { P_OR = 1, P_XOR = 2, P_AND = 3, P_ISIN = 4, P_NOT = 5, P_CMP = 7, P_ADD = 11, P_MUL = 12, P_NEG = 14 };

static void parse_expr(struct parser *p, int min_prec);
static void parse_select(struct parser *p);
static int setop_follows(struct parser *p);
static const char *word_at(const char *q, char *up, size_t cap);

/* IN ( SELECT ... ) - an extension (the reference's grammar knows value lists only, midorisql.y:283-284): the lexer stands on SELECT.
 * The inner statement's tokens are emitted in place and end in its own "SELECT d n"; "SUBQUERY" wraps it into one stack entry.  Inside
 * the parentheses the grammar is SELECT's, whatever the outer statement is. */
static void parse_subquery(struct parser *p)
{
	const bool dml = p->dml, sel_list = p->sel_list, arm = p->arm;

	if (p->depth >= MAX_SUBQUERY_DEPTH) {
		fail(p, "syntax error, subqueries nested deeper than %d", MAX_SUBQUERY_DEPTH);
		return;
	}
	next(p);
	p->dml = false;
	p->arm = false;
	p->depth++;
	parse_select(p);
	p->depth--;
	p->dml = dml;
	p->sel_list = sel_list;
	p->arm = arm;
	if (!p->failed && setop_follows(p) > 0)
		fail(p, "syntax error, a set operation (UNION / INTERSECT / EXCEPT) inside IN (SELECT ...) is not supported: a subquery is one SELECT");
	emit(p, "SUBQUERY");
}

/* ------------------------------------------------------------------ window functions: fn(...) OVER ( ... )
 * No word is reserved for them.  The lexer stands behind the `)` of one of the eight functions: OVER opens a window only as the name
 * `over` with `(` as the next token; with another name behind it, it is a named window, which gets its own error. */
static const char *skip_blank(const char *q)
{
	while (*q == ' ' || *q == '\t' || *q == '\n' || *q == '\r')
		q++;
	return q;
}

static bool name_is(const struct lexer *l, const char *word)
{
	return l->type == T_NAME && strcasecmp(l->text, word) == 0;
}

/* 0: no window behind the function (what follows is an alias or the next clause), 1: OVER ( follows, -1: failed (a named window) */
static int over_follows(struct parser *p)
{
	const char *q;

	if (p->failed || !name_is(&p->lx, "over"))
		return 0;
	q = skip_blank(p->lx.s + p->lx.pos);
	if (*q == '(')
		return 1;
	if (isalpha((unsigned char)*q) || *q == '`') {
		char up[16];
		size_t k = 0;
		while (k < sizeof(up) - 1 && (isalnum((unsigned char)q[k]) || q[k] == '_')) {
			up[k] = (char)toupper((unsigned char)q[k]);
			k++;
		}
		up[k] = 0;
		if (*q == '`' || (!is_keyword(up) && !isalnum((unsigned char)q[k]) && q[k] != '_') || k == sizeof(up) - 1) {
			fail(p, "syntax error, named windows (OVER name, WINDOW name AS ...) are not supported: write the window out, OVER ( ... )");
			return -1;
		}
	}
	return 0;
}

/* the text from q (behind an opening parenthesis) up to its closing one, then OVER ( : does a window clause follow this function call?
 * A scan of the raw text that knows nothing of string literals or back-quoted names: a parenthesis inside one - COUNT(s = ')') - is
 * counted like any other.  It only chooses between two error texts for statements that are refused either way (COUNT(col) OVER, DISTINCT
 * inside a window function) or falls through to the path these forms took before: the worst a mis-scan gives is the other message. */
static bool over_behind_call(const char *q)
{
	int depth = 1;
	while (*q && depth) {
		if (*q == '(')
			depth++;
		else if (*q == ')')
			depth--;
		q++;
	}
	if (depth)
		return false;
	q = skip_blank(q);
	if (strncasecmp(q, "over", 4) != 0 || isalnum((unsigned char)q[4]) || q[4] == '_')
		return false;
	return *skip_blank(q + 4) == '(';
}

static bool window_field(struct parser *p)
{
	char first[256];

	if (p->lx.type != T_NAME) {
		fail(p, "syntax error, PARTITION BY and ORDER BY inside OVER take columns: col or tbl.col");
		return false;
	}
	strcpy(first, p->lx.text);
	next(p);
	if (is_punct(p, '.')) {
		next(p);
		if (p->lx.type != T_NAME) {
			fail(p, "syntax error, expecting column name after '.'");
			return false;
		}
		emit(p, "FIELDNAME %s.%s", first, p->lx.text);
		next(p);
	} else {
		emit(p, "NAME %s", first);
	}
	return !p->failed;
}

/* the lexer stands on OVER (over_follows() == 1); the function's argument, if it has one, is emitted already */
static void parse_over(struct parser *p, const char *fn)
{
	int npart = 0, norder = 0;

	if (p->dml) {
		fail(p, "window function %s ... OVER can't be used in DELETE / UPDATE", fn);
		return;
	}
	if (!p->sel_list) {
		fail(p, "window function %s ... OVER is allowed in the select list only (not in WHERE, ON, GROUP BY, HAVING, ORDER BY or LIMIT)", fn);
		return;
	}
	next(p);
	expect_punct(p, '(');
	if (p->failed)
		return;
	if (name_is(&p->lx, "partition")) {
		next(p);
		expect_kw(p, "BY");
		do {
			if (p->failed || !window_field(p))
				return;
			npart++;
		} while (is_punct(p, ',') && (next(p), true));
	}
	if (accept_kw(p, "ORDER")) {
		expect_kw(p, "BY");
		do {
			int desc = 0;
			if (p->failed || !window_field(p))
				return;
			if (accept_kw(p, "DESC"))
				desc = 1;
			else
				accept_kw(p, "ASC");
			emit(p, "WINORDER %d", desc);
			norder++;
		} while (is_punct(p, ',') && (next(p), true));
	}
	if (name_is(&p->lx, "rows") || name_is(&p->lx, "range") || name_is(&p->lx, "groups")) {
		fail(p, "syntax error, window frame clauses (ROWS / RANGE / GROUPS) are not supported: the frame is SQL's default, up to the row's peers");
		return;
	}
	if (p->lx.type == T_NAME && !is_punct(p, ')')) {
		fail(p, "syntax error, unexpected '%s' in OVER ( [PARTITION BY f, ...] [ORDER BY f [ASC|DESC], ...] ): named windows are not supported", p->lx.text);
		return;
	}
	expect_punct(p, ')');
	emit(p, "WINDOW %s %d %d", fn, npart, norder);
}

/* LAG(col [, k [, default]]) | LEAD(...) | FIRST_VALUE(col) | LAST_VALUE(col) | NTILE(n): the lexer stands on the function's name.  The
 * column is emitted as the argument of SUM is; k, the default and n travel as the literals' own tokens and "WINARG count" closes them
 * (LAG / LEAD / NTILE; FIRST_VALUE / LAST_VALUE have none), then the OVER clause as for every window function. */
static bool nav_literal(struct parser *p)
{
	struct lexer *l = &p->lx;

	if (l->type == T_INT)
		emit(p, "NUMBER %d", (int)l->ival);	/* (the caller has refused what does not fit: "NUMBER" is 32-bit, as the reference's) */
	else if (l->type == T_FLOAT)
		emit(p, "FLOAT %g", l->fval);
	else if (l->type == T_BOOL)
		emit(p, "BOOL %d", (int)l->ival);
	else if (l->type == T_STRING)
		emit(p, "STRING %s", l->text);
	else if (is_kw(p, "NULL"))
		emit(p, "NULL");
	else
		return false;
	next(p);
	return true;
}

/* do the words w1 (one of two spellings) and then w2 (one of three, NULL: any text) stand in the raw text behind the current token? */
static bool words_behind(const struct lexer *l, const char *w1a, const char *w1b, const char *w2a, const char *w2b, const char *w2c)
{
	char up[16];
	const char *q = skip_blank(word_at(skip_blank(l->s + l->pos), up, sizeof(up)));

	if (strcmp(up, w1a) != 0 && (!w1b || strcmp(up, w1b) != 0))
		return false;
	if (!w2a)
		return true;
	(void)word_at(q, up, sizeof(up));
	return !strcmp(up, w2a) || (w2b && !strcmp(up, w2b)) || (w2c && !strcmp(up, w2c));
}

static void parse_nav(struct parser *p)
{
	struct lexer *l = &p->lx;
	char fn[16];
	size_t k = 0;
	int nextra = 0;
	bool offs, ntile;

	for (; l->text[k] && k < sizeof(fn) - 1; k++)
		fn[k] = (char)toupper((unsigned char)l->text[k]);
	fn[k] = 0;
	offs = !strcmp(fn, "LAG") || !strcmp(fn, "LEAD");
	ntile = !strcmp(fn, "NTILE");
	if (p->dml) {
		fail(p, "window function %s ... OVER can't be used in DELETE / UPDATE", fn);
		return;
	}
	next(p);
	expect_punct(p, '(');
	if (p->failed)
		return;
	if (is_kw(p, "DISTINCT")) {
		fail(p, "syntax error, DISTINCT inside a window function is not supported: %s(DISTINCT ...) OVER", fn);
		return;
	}
	if (ntile) {
		if (l->type == T_NAME) {
			fail(p, "syntax error, NTILE takes the number of buckets as a positive integer literal, not a column: NTILE(n)");
			return;
		}
		if (l->type != T_INT) {
			fail(p, "syntax error, NTILE takes the number of buckets as a positive integer literal: NTILE(n)");
			return;
		}
		if (l->wval < 1) {
			fail(p, "syntax error, NTILE(%lld): the number of buckets must be at least 1", l->wval);
			return;
		}
		if (l->wval > INT_MAX) {
			fail(p, "syntax error, NTILE(%lld): more than %d buckets are not supported in a statement", l->wval, INT_MAX);
			return;
		}
		nav_literal(p);
		nextra = 1;
	} else {
		if (is_punct(p, ')')) {
			fail(p, "syntax error, %s() needs a column: %s(col) or %s(tbl.col)", fn, fn, fn);
			return;
		}
		if (l->type != T_NAME) {
			fail(p, "syntax error, %s takes a column as its first argument: %s(col) or %s(tbl.col)", fn, fn, fn);
			return;
		}
		if (!window_field(p))
			return;
		if (!offs && !is_punct(p, ')')) {
			fail(p, "syntax error, %s takes one column: %s(col) or %s(tbl.col)", fn, fn, fn);
			return;
		}
		if (offs && is_punct(p, ',')) {
			next(p);
			if (l->type == T_INT && l->wval < 0) {
				fail(p, "syntax error, a negative offset in %s is not supported: %s(col, %lld) is %s(col, %lld)", fn, fn, l->wval,
				     !strcmp(fn, "LAG") ? "LEAD" : "LAG", -l->wval);
				return;
			}
			if (l->type == T_INT && l->wval > INT_MAX) {
				fail(p, "syntax error, the offset %lld of %s is not supported in a statement: integer literals are 32-bit, at most %d", l->wval, fn, INT_MAX);
				return;
			}
			if (l->type != T_INT || (nav_literal(p), !is_punct(p, ',') && !is_punct(p, ')'))) {
				fail(p, "syntax error, the offset of %s must be a non-negative integer literal: %s(col, k [, default])", fn, fn);
				return;
			}
			nextra = 1;
			if (is_punct(p, ',')) {
				next(p);
				if (l->type == T_INT && (l->wval > INT_MAX || l->wval < INT_MIN)) {
					fail(p, "syntax error, the default %lld of %s is not supported: integer literals are 32-bit, %d ... %d", l->wval, fn, INT_MIN, INT_MAX);
					return;
				}
				if (!nav_literal(p) || !is_punct(p, ')')) {
					fail(p, "syntax error, the default of %s must be a literal or NULL: %s(col, k, default)", fn, fn);
					return;
				}
				nextra = 2;
			}
		}
	}
	if (offs || ntile)
		emit(p, "WINARG %d", nextra);
	expect_punct(p, ')');
	if (p->failed)
		return;
	/* (the current token is what stands behind the call; the words behind IT are looked at in the raw text, as over_follows() does) */
	if (is_kw(p, "FROM") && words_behind(l, "FIRST", "LAST", "OVER", "IGNORE", "RESPECT")) {
		fail(p, "syntax error, FROM FIRST / FROM LAST behind %s is not supported: rows are counted from the partition's first row", fn);
		return;
	}
	if ((name_is(l, "ignore") || name_is(l, "respect")) && words_behind(l, "NULLS", NULL, NULL, NULL, NULL)) {
		fail(p, "syntax error, IGNORE NULLS / RESPECT NULLS behind %s is not supported: NULL cells are respected", fn);
		return;
	}
	{
		const int ov = over_follows(p);
		if (ov < 0)
			return;
		if (!ov) {
			fail(p, "syntax error, %s(...) needs its window: %s(...) OVER ( [PARTITION BY f, ...] [ORDER BY f [ASC|DESC], ...] )", fn, fn);
			return;
		}
	}
	parse_over(p, fn);
}

/* ------------------------------------------------------------------ set operations: UNION [ALL] / INTERSECT / EXCEPT
 * No word is reserved for them either.  The lexer stands on a name: it is a set operator only when SELECT, or ALL / DISTINCT and then
 * SELECT, stands behind it in the text.  A scan of the raw text, as over_follows(). */
enum { SETOP_UNION = 1, SETOP_UNIONALL, SETOP_INTERSECT, SETOP_EXCEPT };

/* the word at q, upper-cased, into up; returns the text behind it (q itself when no word stands there) */
static const char *word_at(const char *q, char *up, size_t cap)
{
	size_t k = 0;
	if (isalpha((unsigned char)*q))
		while (isalnum((unsigned char)q[k]) || q[k] == '_') {
			if (k < cap - 1)
				up[k] = (char)toupper((unsigned char)q[k]);
			k++;
		}
	up[k < cap - 1 ? k : cap - 1] = 0;
	return q + k;
}

static bool paren_select_at(const char *q)
{
	char up[16];
	if (*q != '(')
		return false;
	word_at(skip_blank(q + 1), up, sizeof(up));
	return strcmp(up, "SELECT") == 0;
}

/* 0: the token is no set operator (a name, an alias, or something else altogether), SETOP_*: it is one, -1: failed (a form that is refused) */
static int setop_follows(struct parser *p)
{
	const char *q;
	char w1[16], w2[16];
	int op;

	if (p->failed || p->lx.type != T_NAME)
		return 0;
	op = name_is(&p->lx, "union") ? SETOP_UNION : name_is(&p->lx, "intersect") ? SETOP_INTERSECT : name_is(&p->lx, "except") ? SETOP_EXCEPT : 0;
	if (!op)
		return 0;
	q = skip_blank(p->lx.s + p->lx.pos);
	if (paren_select_at(q))
		goto paren;
	q = skip_blank(word_at(q, w1, sizeof(w1)));
	if (strcmp(w1, "SELECT") == 0)
		return op;
	if (strcmp(w1, "ALL") != 0 && strcmp(w1, "DISTINCT") != 0)
		return 0;
	if (paren_select_at(q))
		goto paren;
	word_at(q, w2, sizeof(w2));
	if (strcmp(w2, "SELECT") != 0)
		return 0;
	if (w1[0] == 'D')
		return op;
	if (op == SETOP_UNION)
		return SETOP_UNIONALL;
	fail(p, "syntax error, %s ALL is not supported: multiset semantics are not built, %s [DISTINCT] is", op == SETOP_INTERSECT ? "INTERSECT" : "EXCEPT",
	     op == SETOP_INTERSECT ? "INTERSECT" : "EXCEPT");
	return -1;
paren:
	fail(p, "syntax error, a parenthesised SELECT as an arm of a set operation is not supported: write the arms without parentheses, they are evaluated left to right");
	return -1;
}

static int parse_val_list(struct parser *p)
{
	int n = 0;
	do {
		parse_expr(p, P_OR);
		n++;
	} while (!p->failed && is_punct(p, ',') && (next(p), true));
	return n;
}

static void parse_primary(struct parser *p)
{
	struct lexer *l = &p->lx;
	const char *behind_paren;

	if (p->failed)
		return;
	switch (l->type) {
	case T_NAME: {
		char first[256];
		strcpy(first, l->text);
		next(p);
		if (is_punct(p, '.') && !p->dml) {
			next(p);
			if (p->lx.type != T_NAME) {
				fail(p, "syntax error, expecting column name after '.'");
				return;
			}
			emit(p, "FIELDNAME %s.%s", first, p->lx.text);
			next(p);
		} else {
			emit(p, "NAME %s", first);
		}
		return;
	}
	case T_STRING:
		emit(p, "STRING %s", l->text);
		next(p);
		return;
	case T_INT:
		emit(p, "NUMBER %d", (int)l->ival);
		next(p);
		return;
	case T_FLOAT:
		emit(p, "FLOAT %g", l->fval);
		next(p);
		return;
	case T_BOOL:
		emit(p, "BOOL %d", (int)l->ival);
		next(p);
		return;
	case T_FCOUNT:
		if (p->dml) {
			/* (COUNT( stays the syntax error it is in DML; the DISTINCT form gets a text of its own: the lexer stands on the parenthesis) */
			const char *q = l->s + l->pos + 1;
			while (*q == ' ' || *q == '\t' || *q == '\n' || *q == '\r')
				q++;
			if (strncasecmp(q, "DISTINCT", 8) == 0 && !isalnum((unsigned char)q[8]) && q[8] != '_') {
				fail(p, "COUNT(DISTINCT) can't be used in DELETE / UPDATE");
				return;
			}
			break;
		}
		behind_paren = l->s + l->pos + 1;	/* (COUNT( is lexed with its parenthesis right behind the name) */
		next(p);
		expect_punct(p, '(');
		if (!p->failed && !is_punct(p, '*') && over_behind_call(behind_paren)) {
			if (p->lx.type == T_KW && !strcmp(p->lx.text, "DISTINCT"))
				fail(p, "syntax error, DISTINCT inside a window function is not supported: COUNT(DISTINCT col) OVER");
			else
				fail(p, "syntax error, COUNT(col) OVER is not supported: COUNT(*) OVER counts the rows of the frame");
			return;
		}
		if (p->lx.type == T_KW && !strcmp(p->lx.text, "DISTINCT")) {
			/* COUNT(DISTINCT col) | COUNT(DISTINCT tbl.col): one column and nothing else, as SUM(col) - no descent into parentheses:
			 * "NAME col" / "FIELDNAME tbl.col", then "AGG COUNTD" */
			char first[256];
			next(p);
			if (p->lx.type != T_NAME) {
				fail(p, "syntax error, COUNT(DISTINCT col) takes one column: COUNT(DISTINCT col) or COUNT(DISTINCT tbl.col)");
				return;
			}
			strcpy(first, p->lx.text);
			next(p);
			if (is_punct(p, '.')) {
				next(p);
				if (p->lx.type != T_NAME) {
					fail(p, "syntax error, expecting column name after '.'");
					return;
				}
				emit(p, "FIELDNAME %s.%s", first, p->lx.text);
				next(p);
			} else {
				emit(p, "NAME %s", first);
			}
			if (!is_punct(p, ')')) {
				fail(p, "syntax error, COUNT(DISTINCT col) takes one column: COUNT(DISTINCT col) or COUNT(DISTINCT tbl.col)");
				return;
			}
			next(p);
			emit(p, "AGG COUNTD");
		} else if (is_punct(p, '*')) {
			next(p);
			expect_punct(p, ')');
			{
				const int ov = over_follows(p);
				if (ov < 0)
					return;
				if (ov) {
					parse_over(p, "COUNT");
					return;
				}
			}
			emit(p, "COUNTALL");
		} else {
			parse_expr(p, P_OR);
			expect_punct(p, ')');
			emit(p, "COUNTFIELD");
		}
		return;
	case T_FAGG: {
		/* SUM(col) | SUM(tbl.col): one column, nothing else (no arithmetic, no DISTINCT) - "NAME col" / "FIELDNAME tbl.col", then "AGG SUM" */
		char fn[8], first[256];
		snprintf(fn, sizeof(fn), "%.3s", l->text);
		if (p->dml) {
			fail(p, "aggregate function %s can't be used in DELETE / UPDATE", fn);
			return;
		}
		next(p);
		expect_punct(p, '(');
		if (p->failed)
			return;
		if (p->lx.type == T_KW && !strcmp(p->lx.text, "DISTINCT") && over_behind_call(l->s + l->pos)) {
			fail(p, "syntax error, DISTINCT inside a window function is not supported: %s(DISTINCT col) OVER", fn);
			return;
		}
		if (p->lx.type != T_NAME) {
			fail(p, "syntax error, %s takes one column: %s(col) or %s(tbl.col)", fn, fn, fn);
			return;
		}
		strcpy(first, p->lx.text);
		next(p);
		if (is_punct(p, '.')) {
			next(p);
			if (p->lx.type != T_NAME) {
				fail(p, "syntax error, expecting column name after '.'");
				return;
			}
			emit(p, "FIELDNAME %s.%s", first, p->lx.text);
			next(p);
		} else {
			emit(p, "NAME %s", first);
		}
		if (!is_punct(p, ')')) {
			fail(p, "syntax error, %s takes one column: %s(col) or %s(tbl.col)", fn, fn, fn);
			return;
		}
		next(p);
		{
			const int ov = over_follows(p);
			if (ov < 0)
				return;
			if (ov) {
				parse_over(p, fn);
				return;
			}
		}
		emit(p, "AGG %s", fn);
		return;
	}
	case T_FWIN: {
		/* ROW_NUMBER() | RANK() | DENSE_RANK(): no argument, and nothing without its OVER clause */
		char fn[16];
		size_t k = 0;
		for (; l->text[k] && k < sizeof(fn) - 1; k++)
			fn[k] = (char)toupper((unsigned char)l->text[k]);
		fn[k] = 0;
		if (p->dml) {
			fail(p, "window function %s ... OVER can't be used in DELETE / UPDATE", fn);
			return;
		}
		next(p);
		expect_punct(p, '(');
		if (p->failed)
			return;
		if (!is_punct(p, ')')) {
			fail(p, "syntax error, %s() takes no argument", fn);
			return;
		}
		next(p);
		{
			const int ov = over_follows(p);
			if (ov < 0)
				return;
			if (!ov) {
				fail(p, "syntax error, %s() needs its window: %s() OVER ( [PARTITION BY f, ...] [ORDER BY f [ASC|DESC], ...] )", fn, fn);
				return;
			}
		}
		parse_over(p, fn);
		return;
	}
	case T_FNAV:
		parse_nav(p);
		return;
	case T_KW:
		if (strcmp(l->text, "NULL") == 0) {
			emit(p, "NULL");
			next(p);
			return;
		}
		break;
	case T_PUNCT:
		if (l->text[0] == '(') {
			next(p);
			parse_expr(p, P_OR);
			expect_punct(p, ')');
			return;
		}
		if (l->text[0] == '-' && !p->dml) {
			next(p);
			parse_expr(p, P_NEG);
			emit(p, "NEG");
			return;
		}
		break;
	default:
		break;
	}
	fail(p, "syntax error, unexpected '%s'", l->type == T_EOF ? "end of input" : l->text);
}

static void parse_expr(struct parser *p, int min_prec)
{
	parse_primary(p);
	while (!p->failed) {
		struct lexer *l = &p->lx;
		int prec;
		char op[16];

		if (l->type == T_OROP || is_kw(p, "OR")) {
			prec = P_OR;
			strcpy(op, "OR");
		} else if (is_kw(p, "XOR")) {
			prec = P_XOR;
			strcpy(op, "XOR");
		} else if (l->type == T_ANDOP || is_kw(p, "AND")) {
			prec = P_AND;
			strcpy(op, "AND");
		} else if (l->type == T_CMP) {
			prec = P_CMP;
			snprintf(op, sizeof(op), "CMP %d", l->sub);
		} else if (!p->dml && (is_punct(p, '+') || is_punct(p, '-'))) {
			prec = P_ADD;
			strcpy(op, l->text[0] == '+' ? "ADD" : "SUB");
		} else if (!p->dml && (is_punct(p, '*') || is_punct(p, '/') || is_punct(p, '%') || is_kw(p, "MOD"))) {
			prec = P_MUL;
			strcpy(op, l->text[0] == '*' ? "MUL" : (l->text[0] == '/' ? "DIV" : "MOD"));
		} else if (is_kw(p, "IS")) {
			bool neg = false;
			if (P_ISIN < min_prec)
				return;
			next(p);
			if (accept_kw(p, "NOT"))
				neg = true;
			expect_kw(p, "NULL");
			emit(p, neg ? "ISNOTNULL" : "ISNULL");
			continue;
		} else if (is_kw(p, "IN") || is_kw(p, "LIKE") || is_kw(p, "NOT")) {
			bool neg = false;
			int n;
			if (P_ISIN < min_prec)
				return;
			if (accept_kw(p, "NOT"))
				neg = true;
			if (accept_kw(p, "IN")) {
				expect_punct(p, '(');
				if (!p->failed && is_kw(p, "SELECT")) {
					parse_subquery(p);
					expect_punct(p, ')');
					emit(p, neg ? "ISNOTINSUB" : "ISINSUB");
					continue;
				}
				n = parse_val_list(p);
				expect_punct(p, ')');
				emit(p, neg ? "ISNOTIN %d" : "ISIN %d", n);
			} else if (!p->dml && accept_kw(p, "LIKE")) {
				parse_expr(p, P_ISIN + 1);
				emit(p, neg ? "NOTLIKE" : "LIKE");
			} else {
				fail(p, "syntax error, unexpected NOT");
			}
			continue;
		} else {
			return;
		}
		if (prec < min_prec)
			return;
		next(p);
		parse_expr(p, prec + 1);	/* all binary operators are left-associative */
		emit(p, "%s", op);
	}
}

/* opt_as_alias: AS NAME | NAME | nil  (midorisql.y:224-227) */
static void parse_opt_alias(struct parser *p)
{
	if (accept_kw(p, "AS")) {
		if (p->lx.type != T_NAME) {
			fail(p, "syntax error, expecting alias name after AS");
			return;
		}
		emit(p, "ALIAS %s", p->lx.text);
		next(p);
	} else if (p->lx.type == T_NAME && !setop_follows(p)) {	/* (union / intersect / except in front of a SELECT: the operator, no alias) */
		emit(p, "ALIAS %s", p->lx.text);
		next(p);
	}
}

static void parse_table_factor(struct parser *p)
{
	if (p->lx.type != T_NAME) {
		fail(p, "syntax error, unexpected '%s', expecting table name", p->lx.type == T_EOF ? "end of input" : p->lx.text);
		return;
	}
	emit(p, "TABLE %s", p->lx.text);
	next(p);
	parse_opt_alias(p);
}

/* table_reference: table_factor | join_table (left-recursive)  (midorisql.y:213-234) */
static void parse_table_reference(struct parser *p)
{
	parse_table_factor(p);
	while (!p->failed) {
		int jt;
		if (is_kw(p, "INNER") || is_kw(p, "JOIN")) {
			accept_kw(p, "INNER");
			jt = 1;
		} else if (is_kw(p, "LEFT") || is_kw(p, "RIGHT") || is_kw(p, "FULL")) {
			jt = is_kw(p, "LEFT") ? 2 : is_kw(p, "RIGHT") ? 4 : 6;	/* (FULL: LEFT + RIGHT; not in the reference's grammar) */
			next(p);
			if (accept_kw(p, "OUTER"))
				jt += 6;
		} else {
			return;
		}
		expect_kw(p, "JOIN");
		parse_table_factor(p);
		expect_kw(p, "ON");
		parse_expr(p, P_OR);
		emit(p, "ONEXPR");
		emit(p, "JOIN %d", jt);
	}
}

static void parse_select(struct parser *p)
{
	int opts = 0, nsel = 0, ntab = 0, extra = 0;

	while (accept_kw(p, "DISTINCT")) {
		if (opts & 2)
			fail(p, "duplicate DISTINCT option");
		opts |= 2;
	}
	if (is_punct(p, '*')) {
		next(p);
		emit(p, "SELECTALL");
		nsel = 1;
	} else {
		do {
			p->sel_list = true;
			parse_expr(p, P_OR);
			p->sel_list = false;
			parse_opt_alias(p);
			nsel++;
		} while (!p->failed && is_punct(p, ',') && (next(p), true));
	}
	if (!accept_kw(p, "FROM")) {
		p->had_tail = false;
		emit(p, "SELECT %d %d", opts, nsel);
		return;
	}
	do {
		parse_table_reference(p);
		ntab++;
	} while (!p->failed && is_punct(p, ',') && (next(p), true));
	if (accept_kw(p, "WHERE")) {
		parse_expr(p, P_OR);
		emit(p, "WHERE");
		extra++;
	}
	if (accept_kw(p, "GROUP")) {
		int n = 0;
		expect_kw(p, "BY");
		do {
			parse_expr(p, P_OR);
			if (!accept_kw(p, "ASC"))
				accept_kw(p, "DESC");
			n++;
		} while (!p->failed && is_punct(p, ',') && (next(p), true));
		emit(p, "GROUPBYLIST %d", n);
		extra++;
	}
	if (accept_kw(p, "HAVING")) {
		parse_expr(p, P_OR);
		emit(p, "HAVING");
		extra++;
	}
	if (name_is(&p->lx, "window")) {
		fail(p, "syntax error, named windows (OVER name, WINDOW name AS ...) are not supported: write the window out, OVER ( ... )");
		return;
	}
	p->had_tail = false;
	if (p->arm) {	/* (an arm behind the first: what follows closes the compound, parse_compound) */
		emit(p, "SELECT %d %d", opts, nsel + ntab + extra);
		return;
	}
	p->had_tail = is_kw(p, "ORDER") || is_kw(p, "LIMIT");
	if (accept_kw(p, "ORDER")) {
		int n = 0;
		expect_kw(p, "BY");
		do {
			int desc = 0;
			parse_expr(p, P_OR);
			if (accept_kw(p, "DESC"))
				desc = 1;
			else
				accept_kw(p, "ASC");
			emit(p, "ORDERBYITEM %d", desc);
			n++;
		} while (!p->failed && is_punct(p, ',') && (next(p), true));
		emit(p, "ORDERBYLIST %d", n);
		extra++;
	}
	if (accept_kw(p, "LIMIT")) {
		parse_expr(p, P_OR);
		if (is_punct(p, ',')) {
			next(p);
			parse_expr(p, P_OR);
			emit(p, "LIMIT 2");
		} else {
			emit(p, "LIMIT 1");
		}
		extra++;
	}
	emit(p, "SELECT %d %d", opts, nsel + ntab + extra);
}

/* The lexer stands behind the first SELECT of a statement: the arms that follow, each behind its operator, and the ORDER BY / LIMIT that
 * close the compound.  Nothing is emitted for a statement without a set operator. */
static void parse_compound(struct parser *p)
{
	static const char *const opname[] = { "", "UNION", "UNIONALL", "INTERSECT", "EXCEPT" };
	int narms = 1, norder = 0, nlimit = 0, op;
	bool loose = false;	/* a UNION or EXCEPT stands in the chain already */

	while ((op = setop_follows(p)) > 0) {
		if (p->had_tail) {
			fail(p, "syntax error, ORDER BY / LIMIT in an arm of a set operation that is not the last: they belong behind the last SELECT and order the whole result");
			return;
		}
		if (op == SETOP_INTERSECT && loose) {
			fail(p, "syntax error, INTERSECT behind UNION or EXCEPT in one chain is not supported: the standard binds INTERSECT tighter, SQLite reads "
				"left to right, and there are no parentheses to say which - put the INTERSECT first or split the statement");
			return;
		}
		loose = loose || op != SETOP_INTERSECT;
		if (narms == MAX_SETOP_ARMS) {
			fail(p, "syntax error, more than %d arms in one set operation", MAX_SETOP_ARMS);
			return;
		}
		next(p);	/* the operator */
		if (name_is(&p->lx, "all") || is_kw(p, "DISTINCT"))
			next(p);
		expect_kw(p, "SELECT");
		p->arm = true;
		parse_select(p);
		p->arm = false;
		if (p->failed)
			return;
		emit(p, "SETOP %s", opname[op]);
		narms++;
		if (is_kw(p, "ORDER") || is_kw(p, "LIMIT")) {
			p->had_tail = true;
			break;
		}
	}
	if (op < 0 || narms == 1)
		return;
	if (accept_kw(p, "ORDER")) {
		expect_kw(p, "BY");
		do {
			int desc = 0;
			if (p->failed)
				return;
			if (p->lx.type != T_NAME || setop_follows(p)) {
				fail(p, "syntax error, ORDER BY behind a set operation takes result columns of the first SELECT by their bare names: a column's name or an alias");
				return;
			}
			emit(p, "NAME %s", p->lx.text);
			next(p);
			if (is_punct(p, '.')) {
				fail(p, "syntax error, ORDER BY behind a set operation takes result columns of the first SELECT by their bare names: a column's name or an alias");
				return;
			}
			if (accept_kw(p, "DESC"))
				desc = 1;
			else
				accept_kw(p, "ASC");
			emit(p, "SETORDER %d", desc);
			norder++;
		} while (is_punct(p, ',') && (next(p), true));
	}
	if (accept_kw(p, "LIMIT")) {
		parse_expr(p, P_OR);
		if (is_punct(p, ',')) {
			next(p);
			parse_expr(p, P_OR);
			emit(p, "SETLIMIT 2");
		} else {
			emit(p, "SETLIMIT 1");
		}
		nlimit = 1;
	}
	if (setop_follows(p) > 0) {
		fail(p, "syntax error, ORDER BY / LIMIT in an arm of a set operation that is not the last: they belong behind the last SELECT and order the whole result");
		return;
	}
	emit(p, "COMPOUND %d %d %d", narms, norder, nlimit);
}

/* CREATE TABLE (midorisql.y:447-483) */
static void parse_create(struct parser *p)
{
	int ifne = 0, ncols = 0;
	char tname[256];

	expect_kw(p, "TABLE");
	if (accept_kw(p, "IF")) {
		expect_kw(p, "NOT");
		expect_kw(p, "EXISTS");
		ifne = 1;
	}
	if (p->lx.type == T_FWIN || p->lx.type == T_FNAV)	/* (a table called `rank` or `lag`, its parenthesis right behind the name) */
		p->lx.type = T_NAME;
	if (p->lx.type != T_NAME) {
		fail(p, "syntax error, expecting table name");
		return;
	}
	strcpy(tname, p->lx.text);
	next(p);
	expect_punct(p, '(');
	do {
		char cname[256];
		int code = 0;
		emit(p, "STARTCOL");
		if (p->lx.type != T_NAME) {
			fail(p, "syntax error, expecting column name");
			return;
		}
		strcpy(cname, p->lx.text);
		next(p);
		if (is_kw(p, "INT") || is_kw(p, "INT4") || is_kw(p, "INTEGER")) {
			code = 50000;	/* the lexer maps INT, INT4 and INTEGER to one token (midorisql.l:45) */
			next(p);
		} else if (accept_kw(p, "TINYINT")) {
			code = 60000;
		} else if (accept_kw(p, "DOUBLE")) {
			code = 80000;
		} else if (accept_kw(p, "DATE")) {
			code = 100000;
		} else if (accept_kw(p, "DATETIME")) {
			code = 110000;
		} else if (is_kw(p, "VARCHAR") || is_kw(p, "VARCHARACTER")) {
			next(p);
			expect_punct(p, '(');
			if (p->lx.type != T_INT) {
				fail(p, "syntax error, expecting VARCHAR length");
				return;
			}
			code = 130000 + (int)p->lx.ival;
			next(p);
			expect_punct(p, ')');
		} else {
			fail(p, "syntax error, unexpected '%s', expecting a data type", p->lx.text);
			return;
		}
		for (;;) {
			if (is_kw(p, "NOT")) {
				next(p);
				expect_kw(p, "NULL");
				emit(p, "ATTR NOTNULL");
			} else if (accept_kw(p, "NULL")) {
				/* no token (midorisql.y:469) */
			} else if (accept_kw(p, "AUTO_INCREMENT")) {
				emit(p, "ATTR AUTOINC");
			} else if (accept_kw(p, "UNIQUE")) {
				emit(p, "ATTR UNIQUEKEY");
			} else if (is_kw(p, "PRIMARY")) {
				next(p);
				expect_kw(p, "KEY");
				emit(p, "ATTR PRIKEY");
			} else {
				break;
			}
			if (p->failed)
				return;
		}
		emit(p, "COLUMNDEF %d %s", code, cname);
		ncols++;
	} while (!p->failed && is_punct(p, ',') && (next(p), true));
	expect_punct(p, ')');
	emit(p, "CREATE %d %d %s", ifne, ncols, tname);
}

/* insert_expr (midorisql.y:377-392): literals with + - * / % and unary minus */
static void parse_insert_expr(struct parser *p, int min_prec)
{
	struct lexer *l = &p->lx;

	if (p->failed)
		return;
	if (l->type == T_STRING) {
		emit(p, "STRING %s", l->text);
		next(p);
	} else if (l->type == T_INT) {
		emit(p, "NUMBER %d", (int)l->ival);
		next(p);
	} else if (l->type == T_FLOAT) {
		emit(p, "FLOAT %g", l->fval);
		next(p);
	} else if (l->type == T_BOOL) {
		emit(p, "BOOL %d", (int)l->ival);
		next(p);
	} else if (is_kw(p, "NULL")) {
		emit(p, "NULL");
		next(p);
	} else if (is_punct(p, '(')) {
		next(p);
		parse_insert_expr(p, P_ADD);
		expect_punct(p, ')');
	} else if (is_punct(p, '-')) {
		next(p);
		parse_insert_expr(p, P_NEG);
		emit(p, "NEG");
	} else {
		fail(p, "syntax error, unexpected '%s' in VALUES", l->type == T_EOF ? "end of input" : l->text);
		return;
	}
	while (!p->failed) {
		int prec;
		const char *op;
		if (is_punct(p, '+') || is_punct(p, '-')) {
			prec = P_ADD;
			op = p->lx.text[0] == '+' ? "ADD" : "SUB";
		} else if (is_punct(p, '*') || is_punct(p, '/') || is_punct(p, '%')) {
			prec = P_MUL;
			op = p->lx.text[0] == '*' ? "MUL" : (p->lx.text[0] == '/' ? "DIV" : "MOD");
		} else {
			return;
		}
		if (prec < min_prec)
			return;
		next(p);
		parse_insert_expr(p, prec + 1);
		emit(p, "%s", op);
	}
}

/* INSERT ... VALUES (midorisql.y:347-375) */
static void parse_insert(struct parser *p)
{
	char tname[256];
	int hascols = 0, ntuples = 0;

	accept_kw(p, "INTO");
	if (p->lx.type == T_FWIN || p->lx.type == T_FNAV)	/* (a table called `rank` or `lag`, its parenthesis right behind the name) */
		p->lx.type = T_NAME;
	if (p->lx.type != T_NAME) {
		fail(p, "syntax error, expecting table name");
		return;
	}
	strcpy(tname, p->lx.text);
	next(p);
	if (is_punct(p, '(')) {
		int n = 0;
		next(p);
		do {
			if (p->lx.type != T_NAME) {
				fail(p, "syntax error, expecting column name");
				return;
			}
			emit(p, "COLUMN %s", p->lx.text);
			next(p);
			n++;
		} while (!p->failed && is_punct(p, ',') && (next(p), true));
		expect_punct(p, ')');
		emit(p, "INSERTCOLS %d", n);
		hascols = 1;
	}
	if (!accept_kw(p, "VALUES") && !accept_kw(p, "VALUE")) {
		fail(p, "syntax error, expecting VALUES");
		return;
	}
	do {
		int n = 0;
		expect_punct(p, '(');
		do {
			parse_insert_expr(p, P_ADD);
			n++;
		} while (!p->failed && is_punct(p, ',') && (next(p), true));
		expect_punct(p, ')');
		emit(p, "VALUES %d", n);
		ntuples++;
	} while (!p->failed && is_punct(p, ',') && (next(p), true));
	emit(p, "INSERTVALS %d %d %s", hascols, ntuples, tname);
}

/* DELETE FROM NAME [WHERE delete_expr]  (midorisql.y:309-343) */
static void parse_delete(struct parser *p)
{
	char tname[256];

	expect_kw(p, "FROM");
	if (p->failed)
		return;
	if (p->lx.type != T_NAME) {
		fail(p, "syntax error, expecting table name");
		return;
	}
	strcpy(tname, p->lx.text);
	next(p);
	if (accept_kw(p, "WHERE")) {
		p->dml = true;
		parse_expr(p, P_OR);
		p->dml = false;
		emit(p, "WHERE");
	}
	emit(p, "DELETEONE %s", tname);
}

/* UPDATE NAME SET NAME = update_expr [, ...] [WHERE update_expr]  (midorisql.y:393-440) */
static void parse_update(struct parser *p)
{
	char tname[256], cname[256];
	int nassign = 0, haswhere = 0;

	if (p->lx.type != T_NAME) {
		fail(p, "syntax error, expecting table name");
		return;
	}
	strcpy(tname, p->lx.text);
	next(p);
	expect_kw(p, "SET");
	do {
		if (p->failed)
			return;
		if (p->lx.type != T_NAME) {
			fail(p, "syntax error, expecting column name");
			return;
		}
		strcpy(cname, p->lx.text);
		next(p);
		if (p->lx.type != T_CMP) {
			fail(p, "syntax error, expecting '='");
			return;
		}
		if (p->lx.sub != 4) {
			fail(p, "bad insert assignment to %s", cname);	/* the reference's own wording, midorisql.y:404 */
			return;
		}
		next(p);
		/* update_expr is left-recursive over COMPARISON too; the right-hand side of an assignment binds
		 * tighter than a following comparison cannot occur before ',' or WHERE, so one full expression */
		p->dml = true;
		parse_expr(p, P_OR);
		p->dml = false;
		emit(p, "ASSIGN %s", cname);
		nassign++;
	} while (!p->failed && is_punct(p, ',') && (next(p), true));
	if (accept_kw(p, "WHERE")) {
		p->dml = true;
		parse_expr(p, P_OR);
		p->dml = false;
		emit(p, "WHERE");
		haswhere = 1;
	}
	emit(p, "UPDATE %s %d %d", tname, nassign, haswhere);
}

int mdb_sql_parse(const char *sql, struct mdb_rpn *out, char *err, size_t errlen)
{
	struct parser p = {0};

	p.lx.s = sql;
	p.out = out;
	p.err = err;
	p.errlen = errlen;
	if (err && errlen)
		err[0] = 0;
	next(&p);
	if (accept_kw(&p, "SELECT")) {
		parse_select(&p);
		parse_compound(&p);
	} else if (is_punct(&p, '(') && paren_select_at(p.lx.s + p.lx.pos - 1))
		fail(&p, "syntax error, a parenthesised SELECT as an arm of a set operation is not supported: write the arms without parentheses, they are evaluated left to right");
	else if (accept_kw(&p, "CREATE"))
		parse_create(&p);
	else if (accept_kw(&p, "INSERT"))
		parse_insert(&p);
	else if (accept_kw(&p, "DELETE"))
		parse_delete(&p);
	else if (accept_kw(&p, "UPDATE"))
		parse_update(&p);
	else
		fail(&p, "syntax error, unexpected '%s'", p.lx.type == T_EOF ? "end of input" : p.lx.text);
	emit(&p, "STMT");
	if (!p.failed) {
		expect_punct(&p, ';');		/* stmt_list: stmt ';'  (midorisql.y:148) */
		if (!p.failed && p.lx.type != T_EOF)
			fail(&p, "syntax error, unexpected '%s' after ';'", p.lx.text);
	}
	if (p.failed) {
		mdb_rpn_free(out);
		return -MIDORIDB_ERROR;
	}
	return MIDORIDB_OK;
}

int mdb_rpn_push(struct mdb_rpn *r, const char *tok)
{
	if (r->n == r->cap) {
		int ncap = r->cap ? r->cap * 2 : 32;
		char **nt = realloc(r->tok, sizeof(char *) * (size_t)ncap);
		if (!nt)
			return -MIDORIDB_NOMEM;
		r->tok = nt;
		r->cap = ncap;
	}
	r->tok[r->n] = strdup(tok);
	if (!r->tok[r->n])
		return -MIDORIDB_NOMEM;
	r->n++;
	return MIDORIDB_OK;
}

void mdb_rpn_free(struct mdb_rpn *r)
{
	for (int i = 0; i < r->n; i++)
		free(r->tok[i]);
	free(r->tok);
	memset(r, 0, sizeof(*r));
}

/* Split '\n'-separated RPN text (what a bison-side integration hands over) into tokens. */
int mdb_rpn_from_text(const char *text, struct mdb_rpn *out)
{
	const char *s = text;
	memset(out, 0, sizeof(*out));
	while (*s) {
		const char *e = strchr(s, '\n');
		size_t len = e ? (size_t)(e - s) : strlen(s);
		if (len) {
			char buf[512];
			if (len >= sizeof(buf))
				len = sizeof(buf) - 1;
			memcpy(buf, s, len);
			buf[len] = 0;
			if (mdb_rpn_push(out, buf)) {
				mdb_rpn_free(out);
				return -MIDORIDB_NOMEM;
			}
		}
		if (!e)
			break;
		s = e + 1;
	}
	return MIDORIDB_OK;
}

/* C-ABI helper: SQL text -> '\n'-joined RPN text (used by tests and by the oracle drivers). */
int mdb_sql_to_rpn(const char *sql, char *buf, size_t buflen, char *err, size_t errlen)
{
	struct mdb_rpn r = {0};
	size_t off = 0;
	int rc = mdb_sql_parse(sql, &r, err, errlen);

	if (rc)
		return rc;
	for (int i = 0; i < r.n; i++) {
		size_t len = strlen(r.tok[i]);
		if (off + len + 2 > buflen) {
			mdb_rpn_free(&r);
			if (err && errlen)
				snprintf(err, errlen, "RPN buffer too small");
			return -MIDORIDB_NOMEM;
		}
		memcpy(buf + off, r.tok[i], len);
		off += len;
		buf[off++] = '\n';
	}
	buf[off] = 0;
	mdb_rpn_free(&r);
	return MIDORIDB_OK;
}
