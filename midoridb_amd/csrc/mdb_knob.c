/*
 * mdb_knob.c - the library's ONE reader of its MDB_* environment knobs (INTEGRATION.md lists them).
 *
 * A knob is looked up in the environment once per process and kept: the operators ask for a handful per call, on the call path.  A
 * process that changes a knob while it runs (tests, same-process A/B scripts) says so: mdb_dev_reload_knobs() (the Python binding
 * does it whenever os.environ changes an MDB_* variable).  The readers hand out values and copies, never a pointer into what is
 * kept: a reload in one thread frees it while an operator call in another may be reading.
 */
#include "mdb_host.h"
#include <pthread.h>

static pthread_mutex_t g_knob_mu = PTHREAD_MUTEX_INITIALIZER;
static struct { char *name; char *value; } g_knobs[192];
static int g_nknobs = 0;

/* the value of `name` (NULL: not set), valid while g_knob_mu is held */
static const char *knob_locked(const char *name)
{
	for (int i = 0; i < g_nknobs; i++)
		if (!strcmp(g_knobs[i].name, name))
			return g_knobs[i].value;
	const char *v = getenv(name);
	if (g_nknobs == (int)(sizeof(g_knobs) / sizeof(g_knobs[0])))
		return v;	/* (more knobs than slots: read through) */
	char *n = strdup(name), *c = v ? strdup(v) : NULL;
	if (!n || (v && !c)) {
		free(n);
		free(c);
		return v;
	}
	g_knobs[g_nknobs].name = n;
	g_knobs[g_nknobs].value = c;
	return g_knobs[g_nknobs++].value;
}

int mdb_knob_set(const char *name)
{
	pthread_mutex_lock(&g_knob_mu);
	const int r = knob_locked(name) != NULL;
	pthread_mutex_unlock(&g_knob_mu);
	return r;
}

int mdb_knob_off(const char *name)
{
	pthread_mutex_lock(&g_knob_mu);
	const char *v = knob_locked(name);
	const int r = v && v[0] == '0';
	pthread_mutex_unlock(&g_knob_mu);
	return r;
}

long long mdb_knob_int(const char *name, long long dflt)
{
	pthread_mutex_lock(&g_knob_mu);
	const char *v = knob_locked(name);
	const long long r = v ? atoll(v) : dflt;
	pthread_mutex_unlock(&g_knob_mu);
	return r;
}

int mdb_knob_str(const char *name, char *buf, size_t cap)
{
	pthread_mutex_lock(&g_knob_mu);
	const char *v = knob_locked(name);
	if (cap) {
		const size_t l = v ? strnlen(v, cap - 1) : 0;
		if (l)
			memcpy(buf, v, l);
		buf[l] = 0;
	}
	pthread_mutex_unlock(&g_knob_mu);
	return v != NULL;
}

void mdb_dev_reload_knobs(void)
{
	pthread_mutex_lock(&g_knob_mu);
	for (int i = 0; i < g_nknobs; i++) {
		free(g_knobs[i].name);
		free(g_knobs[i].value);
	}
	g_nknobs = 0;
	pthread_mutex_unlock(&g_knob_mu);
}
