/*
 * partition_layout_main.cpp - prints, as JSON, what the radix partition's sizing functions and mdb_partition_w32_applies return over a
 * grid of requests (tests/test_cpu_partition_layout.py compares it with tests/golden/partition_layout.json).  Host C++ only: it is
 * linked against the built library and calls nothing that needs a device.
 */
#include <stdio.h>
#include <set>
#include <utility>
#include <vector>
#include "mdb_dev_internal.h"

#define LEAF_CAP_SORT 4096u	/* SORT_LEAF_CAP of mdb_dev_sort.hip */
static const uint32_t leaf_targets[] = { 1536u /* GC_TARGET */, 640u /* PJ_TARGET */ };	/* mdb_dev_join_internal.h */

int main(void)
{
	const uint64_t ns[] = { 0, 1, 4095, 4096, 4097, 393215, 393217, 1ull << 20, (1ull << 21) + 5, (1ull << 25) - 1, 1ull << 25, 100000000ull,
				(1ull << 32) - 2 };
	const std::pair<int, int> fixed[] = { { 8, 0 }, { 9, 0 }, { 8, 8 }, { 9, 3 }, { 9, 9 } };
	bool first = true;
	printf("{\"rows\": [\n");
#define ROW(fmt, ...) (printf("%s[" fmt "]", first ? "" : ",\n", __VA_ARGS__), first = false)
	for (uint64_t n : ns) {
		/* the fixed pairs, then what mdb_choose_bits gives for n at the callers' leaf targets */
		std::vector<std::pair<int, int>> bits(fixed, fixed + 5);
		for (uint32_t target : leaf_targets) {
			int b1 = 0, b2 = 0;
			mdb_choose_bits(n, target, &b1, &b2);
			ROW("\"choose_bits\", %llu, %u, %d, %d", (unsigned long long)n, target, b1, b2);
			bool seen = false;
			for (const auto &p : bits)
				seen = seen || (p.first == b1 && p.second == b2);
			if (!seen)
				bits.push_back({ b1, b2 });
		}
		ROW("\"sort_pass_hist_words\", %llu, %zu", (unsigned long long)n, mdb_sort_pass_hist_words(n));
		std::set<int> bits1_seen;
		for (const auto &p : bits) {
			const int b1 = p.first, b2 = p.second;
			for (int fast = 0; fast < 2; fast++) {
				ROW("\"w32_applies\", %llu, %d, %d, %d, %d", (unsigned long long)n, b1, b2, fast, (int)mdb_partition_w32_applies(n, b1, b2, fast != 0));
				for (int want_rid = 0; want_rid < 2; want_rid++)
					for (int npay = 0; npay < 3; npay++)
						ROW("\"arena_bytes\", %llu, %d, %d, %d, %d, %d, %zu", (unsigned long long)n, b1, b2, want_rid, fast, npay,
						    mdb_partition_arena_bytes(n, b1, b2, want_rid != 0, fast != 0, npay));
				const uint32_t leaf_caps[] = { 0u, LEAF_CAP_SORT }, digits0[] = { 0u, 1u, (1u << b1) / 2u };
				const uint64_t digit_rows[] = { 0ull, 1ull << (20 - b1) };
				for (uint32_t leaf_cap : leaf_caps)
					for (uint32_t d0 : digits0)
						for (uint64_t dr : digit_rows)
							ROW("\"raw_arena_bytes\", %llu, %d, %d, %u, %d, %u, %llu, %zu", (unsigned long long)n, b1, b2, leaf_cap, fast, d0,
							    (unsigned long long)dr, mdb_partition_raw_arena_bytes(n, b1, b2, leaf_cap, fast != 0, d0, dr));
			}
			if (bits1_seen.insert(b1).second)
				for (int loose = 0; loose < 2; loose++)
					for (int npay = 0; npay < 3; npay++)
						ROW("\"level0_arena_bytes\", %llu, %d, %d, %d, %zu", (unsigned long long)n, b1, loose, npay,
						    mdb_partition_level0_arena_bytes(n, b1, loose != 0, npay));
		}
	}
	printf("\n]}\n");
	return 0;
}
