/*
 * mdb_set.c - host builder of the device sets behind MDB_P_IN_SET (IN / NOT IN lists of any length; layout, hash and
 * semantics: include/mdb_dev.h, "device sets").  Plain C without any device dependency: the executor (mdb_exec_pred.c) and
 * mdb_dev_set_create() upload what this builds, and the whole file runs under the host sanitizers.
 */
#include <stdlib.h>
#include <string.h>
#include "mdb_dev.h"

void mdb_set_image_free(struct mdb_set_image *img)
{
	if (!img)
		return;
	free(img->words);
	memset(img, 0, sizeof(*img));
}

static inline int used_bit(const uint64_t *used, uint64_t i)
{
	return (int)((used[i >> 6] >> (i & 63)) & 1u);
}

/* is v in the table under construction (occupancy from `used`: no marker yet)? */
static int probe_used(const uint64_t *slots, const uint64_t *used, uint64_t nslots, unsigned log2, uint64_t v)
{
	const uint64_t mask = nslots - 1;
	uint64_t i = mdb_set_slot_of(v, log2);
	for (uint64_t step = 0; step < nslots; step++, i = (i + 1) & mask) {
		if (!used_bit(used, i))
			return 0;
		if (slots[i] == v)
			return 1;
	}
	return 0;
}

int mdb_set_build(const int64_t *values, uint64_t n, int type, struct mdb_set_image *out)
{
	uint64_t nslots, *words, *slots, *used, empty, run = 0, longest = 0, members = 0;
	unsigned log2;

	if (!out)
		return -MIDORIDB_ERROR;
	memset(out, 0, sizeof(*out));
	if ((type != 0 && type != 1) || n > MDB_SET_MAX_VALUES || (n && !values))
		return -MIDORIDB_ERROR;
	log2 = mdb_set_slots_log2_for(n);
	nslots = 1ull << log2;
	words = malloc((size_t)(2 + nslots) * 8);
	used = calloc((size_t)((nslots + 63) / 64), 8);
	if (!words || !used) {
		free(words);
		free(used);
		return -MIDORIDB_NOMEM;
	}
	slots = words + 2;
	for (uint64_t k = 0; k < n; k++) {
		uint64_t v = (uint64_t)values[k], i;
		if (!mdb_set_canonical(type, &v))
			continue;	/* a NaN equals nothing */
		i = mdb_set_slot_of(v, log2);
		while (used_bit(used, i) && slots[i] != v)	/* (members <= n <= nslots / 2: a free slot exists) */
			i = (i + 1) & (nslots - 1);
		if (used_bit(used, i))
			continue;	/* a duplicate */
		used[i >> 6] |= 1ull << (i & 63);
		slots[i] = v;
		members++;
	}
	/* The table is sized by the DISTINCT values: a list whose duplicates (or NaNs) made this table larger than its members need is
	 * built again from the members alone - once: they are distinct and canonical, so the second table has the size asked for.  What
	 * mdb_dev_in_set_lds_values() promises holds for the list's distinct values, however often the list repeats them. */
	if (mdb_set_slots_log2_for(members) < log2) {
		int64_t *distinct = malloc((size_t)(members ? members : 1) * 8);
		uint64_t m = 0;
		int rc;
		if (!distinct) {
			free(words);
			free(used);
			return -MIDORIDB_NOMEM;
		}
		for (uint64_t i = 0; i < nslots; i++)
			if (used_bit(used, i))
				distinct[m++] = (int64_t)slots[i];
		free(words);
		free(used);
		rc = mdb_set_build(distinct, m, type, out);
		free(distinct);
		return rc;
	}
	/* the EMPTY marker: the first pattern of a full-period sequence that is not a member */
	empty = MDB_SET_MARKER_FIRST;
	while (probe_used(slots, used, nslots, log2, empty))
		empty = mdb_set_marker_next(empty);
	for (uint64_t i = 0; i < nslots; i++)
		if (!used_bit(used, i))
			slots[i] = empty;
	/* longest cyclic run of occupied slots: two laps, a run that wraps is seen whole in the second */
	for (uint64_t i = 0; i < 2 * nslots; i++) {
		if (used_bit(used, i & (nslots - 1))) {
			if (++run > longest)
				longest = run;
		} else {
			run = 0;
		}
	}
	free(used);
	words[0] = empty;
	words[1] = nslots;
	out->words = words;
	out->slots = nslots;
	out->members = members;
	out->empty = empty;
	out->longest_run = longest > nslots ? nslots : longest;
	out->log2_slots = log2;
	out->type = type;
	return MIDORIDB_OK;
}

int mdb_set_image_contains(const struct mdb_set_image *img, int64_t value)
{
	uint64_t v = (uint64_t)value, i;
	const uint64_t *slots;

	if (!img || !img->words || !mdb_set_canonical(img->type, &v))
		return 0;
	slots = img->words + 2;
	i = mdb_set_slot_of(v, img->log2_slots);
	for (uint64_t step = 0; step < img->slots; step++, i = (i + 1) & (img->slots - 1)) {
		if (slots[i] == img->empty)
			return 0;
		if (slots[i] == v)
			return 1;
	}
	return 0;
}
