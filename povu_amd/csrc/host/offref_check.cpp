// offref_check.cpp -- the rules of the off-reference calls (hip/offref_rules.hpp) on the CPU, built with
// -fsanitize=address,undefined (make offref_check; run by tests/test_offref_core.py).  The passes are those of
// offref_kernels.hip with a loop over the sites where the device has a lane each: the climb for subflubbles, the candidates,
// the unparent pass, and the offers of the host traversals by minimum.
// stdin, one problem a block:
//   sites <n>            then n lines `<parent or -1> <family letter> <callable 0|1> <traversals>`
//                        -> n lines `<candidate> <called off-reference>`
//   hosts <f> <l> <k>    then k lines `<first> <last> <site>`, the traversals by the record's path of the sites the references call
//                        -> one line: the host's site and the index of its line, or `-1 -1`
#include "../hip/offref_rules.hpp"

#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

using namespace povu_hip;

#define REQUIRE(cond) \
	do { \
		if (!(cond)) { \
			fprintf(stderr, "offref_check: %s failed (line %d)\n", #cond, __LINE__); \
			return 1; \
		} \
	} while (0)

static int self_check()
{
	REQUIRE(offref_candidate(false, false, 1) && !offref_candidate(true, false, 1) && !offref_candidate(false, true, 1) &&
		!offref_candidate(false, false, 0));
	REQUIRE(offref_clears_parent(true, false) && offref_clears_parent(false, true) && !offref_clears_parent(false, false));
	REQUIRE(offref_encloses(0, 4, 1, 3) && offref_encloses(1, 4, 1, 3) && offref_encloses(0, 3, 1, 3));
	REQUIRE(!offref_encloses(1, 3, 1, 3) && !offref_encloses(2, 5, 1, 3) && !offref_encloses(0, 2, 1, 3));
	REQUIRE(offref_encloses(0, ~0ull - 1, 5, 5)); // (no sum of positions: nothing wraps)
	REQUIRE(offref_host_key(5, 7) < offref_host_key(6, 0) && offref_host_key(5, 7) < offref_host_key(5, 8));
	REQUIRE(offref_host_key(0xFFFFFFFFu, 0xFFFFFFFEu) < OFFREF_NO_HOST && offref_host_site(offref_host_key(9, 1234)) == 1234);
	for (const char *c = "TOCMS"; *c; c++)
		REQUIRE(offref_is_subflubble((uint8_t)*c));
	REQUIRE(!offref_is_subflubble('F') && !offref_is_subflubble('D'));
	return 0;
}

int main()
{
	if (self_check())
		return 1;
	std::string word;
	while (std::cin >> word) {
		if (word == "sites") {
			uint32_t n = 0;
			std::cin >> n;
			std::vector<uint32_t> parent(n), trav(n);
			std::vector<uint8_t> fam(n), callable(n), cand(n), off(n);
			for (uint32_t q = 0; q < n; q++) {
				long p;
				char f;
				int c;
				std::cin >> p >> f >> c >> trav[q];
				parent[q] = p < 0 ? 0xFFFFFFFFu : (uint32_t)p;
				fam[q] = (uint8_t)f;
				callable[q] = (uint8_t)c;
			}
			REQUIRE(std::cin.good());
			for (uint32_t q = 0; q < n; q++) { // k_or_candidate
				bool under = false;
				for (uint32_t v = q, k = 0; v < n && k <= n; v = parent[v], k++)
					under |= offref_is_subflubble(fam[v]);
				cand[q] = off[q] = offref_candidate(under, callable[q] != 0, trav[q]);
			}
			for (uint32_t q = 0; q < n; q++) // k_or_unparent
				if (offref_clears_parent(callable[q] != 0, cand[q] != 0) && parent[q] < n)
					off[parent[q]] = 0;
			for (uint32_t q = 0; q < n; q++)
				printf("%d %d\n", cand[q], off[q]);
		} else if (word == "hosts") {
			uint64_t f, l;
			uint32_t k = 0;
			std::cin >> f >> l >> k;
			std::vector<uint64_t> hf(k), hl(k);
			std::vector<uint32_t> hq(k);
			for (uint32_t x = 0; x < k; x++)
				std::cin >> hf[x] >> hl[x] >> hq[x];
			REQUIRE(std::cin.good());
			uint64_t key = OFFREF_NO_HOST;
			uint32_t line = 0xFFFFFFFFu;
			for (uint32_t x = 0; x < k; x++) // k_or_offer, the keys
				if (offref_encloses(hf[x], hl[x], f, l) && offref_host_key((uint32_t)(hl[x] - hf[x] + 1), hq[x]) < key)
					key = offref_host_key((uint32_t)(hl[x] - hf[x] + 1), hq[x]);
			for (uint32_t x = 0; x < k; x++) // ... the lowest traversal among the offers that won
				if (offref_encloses(hf[x], hl[x], f, l) && offref_host_key((uint32_t)(hl[x] - hf[x] + 1), hq[x]) == key && x < line)
					line = x;
			if (key == OFFREF_NO_HOST)
				printf("-1 -1\n");
			else
				printf("%u %u\n", offref_host_site(key), line);
		} else {
			fprintf(stderr, "offref_check: unknown block %s\n", word.c_str());
			return 1;
		}
	}
	printf("offref_check: ok\n");
	return 0;
}
