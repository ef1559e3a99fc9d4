// vcfcmp_check.cpp -- the rules of the VCF comparison as the device runs them (hip/vcfcmp_rules.hpp) and the CHROM table of
// the VCF reader (host/vcfcheck.cpp), on the CPU.  Built with -fsanitize=address,undefined (`make vcfcmp_check`) and driven by
// tests/test_vcfcmp_ref.py, which compares every line with the restatement.  Blocks on stdin (a text `_` is the empty text):
//   key <pos> <ref> <alt>            -> `skipped`, or `<POS'> <suffix> <prefix> <REF'> <ALT'> <hash>`: the lane's loops, and again as
//                                    a wave runs them -- 64 bytes a ballot backwards, then forwards, the hash as the sum of 64
//                                    partial polynomials; the two must agree or the program fails
//   same <pos> <ref> <alt> <pos> <ref> <alt>  -> 1 when the trimmed keys are equal (and then their hashes are), else 0
//   cell <dose a> <dose b>           -> `<class> <gteq>`, the class none, tp, fp or fn
//   chroms <threads> <bytes>         then the bytes of a VCF  -> `C` and the CHROM strings, `R` and every record's index
//                                    among them, or `error <message>`
#include "../../../include/povu_hip.h"
#include "../hip/vcfcmp_rules.hpp"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace povu_hip;

struct Key {
	bool skipped;
	uint64_t pos, s, p, hash;
	std::string ref, alt; // trimmed and folded
};

// (exact sizes: a read beyond a text is the sanitizer's to report)
static std::vector<char> exact(const std::string &t) { return std::vector<char>(t.begin(), t.end()); }

static Key lane_key(uint64_t pos, const std::vector<char> &ref, const std::vector<char> &alt)
{
	Key k{};
	const uint64_t nr = ref.size(), na = alt.size();
	if ((k.skipped = vm_skipped(ref.data(), nr, alt.data(), na)))
		return k;
	k.s = vm_suffix(ref.data(), nr, alt.data(), na);
	k.p = vm_prefix(ref.data(), nr, alt.data(), na, k.s);
	k.pos = pos + k.p;
	k.hash = vm_key_hash(k.pos, nr - k.s - k.p, na - k.s - k.p, vm_text_hash(ref.data() + k.p, nr - k.s - k.p),
			     vm_text_hash(alt.data() + k.p, na - k.s - k.p));
	for (uint64_t i = k.p; i < nr - k.s; i++)
		k.ref += (char)vm_fold(ref[i]);
	for (uint64_t i = k.p; i < na - k.s; i++)
		k.alt += (char)vm_fold(alt[i]);
	return k;
}

// a ballot: the lanes whose predicate holds
template <class F> static uint64_t ballot(F &&f)
{
	uint64_t m = 0;
	for (uint32_t lane = 0; lane < 64; lane++)
		if (f(lane))
			m |= 1ull << lane;
	return m;
}
static uint64_t wave_text_hash(const char *t, uint64_t n)
{
	uint64_t sum = 0;
	for (uint32_t lane = 0; lane < 64; lane++) {
		uint64_t h = 0, power = vm_pow(lane);
		for (uint64_t x = lane; x < n; x += 64, power *= vm_pow(64))
			h += vm_term(t[x], power);
		sum += h;
	}
	return sum;
}
static Key wave_key(uint64_t pos, const std::vector<char> &ref, const std::vector<char> &alt)
{
	Key k{};
	const uint64_t nr = ref.size(), na = alt.size();
	k.skipped = vm_skip_head(ref.data(), nr, alt.data(), na);
	for (uint64_t c0 = 0; !k.skipped && c0 < na; c0 += 64)
		k.skipped = ballot([&](uint32_t l) { return c0 + l < na && vm_skip_byte(alt[c0 + l]); }) != 0;
	if (k.skipped)
		return k;
	uint64_t limit = vm_trim_limit(nr, na);
	k.s = limit;
	for (uint64_t c0 = 0; c0 < limit; c0 += 64) {
		const uint64_t m = ballot([&](uint32_t l) { return c0 + l < limit && vm_suffix_differs(ref.data(), nr, alt.data(), na, c0 + l); });
		if (m) {
			k.s = c0 + (uint64_t)__builtin_ctzll(m);
			break;
		}
	}
	limit = vm_trim_limit(nr - k.s, na - k.s);
	k.p = limit;
	for (uint64_t c0 = 0; c0 < limit; c0 += 64) {
		const uint64_t m = ballot([&](uint32_t l) { return c0 + l < limit && vm_prefix_differs(ref.data(), alt.data(), c0 + l); });
		if (m) {
			k.p = c0 + (uint64_t)__builtin_ctzll(m);
			break;
		}
	}
	k.pos = pos + k.p;
	k.hash = vm_key_hash(k.pos, nr - k.s - k.p, na - k.s - k.p, wave_text_hash(ref.data() + k.p, nr - k.s - k.p),
			     wave_text_hash(alt.data() + k.p, na - k.s - k.p));
	return k;
}

static std::string text_of(const std::string &token) { return token == "_" ? "" : token; }

static Key both_keys(uint64_t pos, const std::string &ref, const std::string &alt)
{
	const std::vector<char> r = exact(ref), a = exact(alt);
	const Key l = lane_key(pos, r, a), w = wave_key(pos, r, a);
	if (l.skipped != w.skipped || l.pos != w.pos || l.s != w.s || l.p != w.p || l.hash != w.hash) {
		fprintf(stderr, "vcfcmp_check: the lane and the wave disagree on %llu %s %s\n", (unsigned long long)pos, ref.c_str(), alt.c_str());
		exit(1);
	}
	return l;
}

static void do_chroms(const std::string &text, uint32_t threads)
{
	char err[256] = {0};
	povu_hip_vcf_doc *d = povu_hip_vcf_parse(text.data(), text.size(), threads, err, sizeof err);
	if (!d) {
		printf("error %s\n", err);
		return;
	}
	printf("C");
	for (uint64_t c = 0; c < d->n_chroms; c++)
		printf(" %s", d->chrom[c]);
	printf("\nR");
	for (uint64_t r = 0; r < d->n_records; r++)
		printf(" %u", d->rec_chrom[r]);
	printf("\n");
	povu_hip_vcf_doc_free(d);
}

int main()
{
	static const char *CELL[] = {"none", "tp", "fp", "fn"};
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream ls(line);
		std::string cmd;
		ls >> cmd;
		if (cmd == "key") {
			uint64_t pos = 0;
			std::string ref, alt;
			ls >> pos >> ref >> alt;
			const Key k = both_keys(pos, text_of(ref), text_of(alt));
			if (k.skipped)
				printf("skipped\n");
			else
				printf("%llu %llu %llu %s %s %016llx\n", (unsigned long long)k.pos, (unsigned long long)k.s, (unsigned long long)k.p, k.ref.c_str(),
				       k.alt.c_str(), (unsigned long long)k.hash);
		} else if (cmd == "same") {
			uint64_t pa = 0, pb = 0;
			std::string ra, aa, rb, ab;
			ls >> pa >> ra >> aa >> pb >> rb >> ab;
			const std::vector<char> xra = exact(text_of(ra)), xaa = exact(text_of(aa)), xrb = exact(text_of(rb)), xab = exact(text_of(ab));
			const Key a = both_keys(pa, text_of(ra), text_of(aa)), b = both_keys(pb, text_of(rb), text_of(ab));
			bool same = !a.skipped && !b.skipped;
			if (same)
				same = vm_same_key(a.pos, xra.data() + a.p, xra.size() - a.s - a.p, xaa.data() + a.p, xaa.size() - a.s - a.p, b.pos, xrb.data() + b.p,
						   xrb.size() - b.s - b.p, xab.data() + b.p, xab.size() - b.s - b.p);
			if (same && a.hash != b.hash) {
				fprintf(stderr, "vcfcmp_check: equal keys, unequal hashes: %s\n", line.c_str());
				return 1;
			}
			printf("%d\n", same ? 1 : 0);
		} else if (cmd == "cell") {
			uint32_t a = 0, b = 0;
			ls >> a >> b;
			printf("%s %d\n", CELL[vm_cell(a, b)], vm_gteq(a, b) ? 1 : 0);
		} else if (cmd == "chroms") {
			uint32_t threads = 1;
			size_t bytes = 0;
			ls >> threads >> bytes;
			std::string text(bytes, '\0');
			std::cin.read(&text[0], (std::streamsize)bytes);
			if ((size_t)std::cin.gcount() != bytes) {
				fprintf(stderr, "vcfcmp_check: short input\n");
				return 1;
			}
			do_chroms(text, threads);
		} else if (!cmd.empty()) {
			fprintf(stderr, "vcfcmp_check: unknown block %s\n", cmd.c_str());
			return 1;
		}
	}
	printf("vcfcmp_check: ok\n");
	return 0;
}
