// vcfcmp_check.cpp -- the rules of the VCF comparison as the device runs them (hip/vcfcmp_rules.hpp) and the CHROM table of
// the VCF reader (host/vcfcheck.cpp), on the CPU.  Built with -fsanitize=address,undefined (`make vcfcmp_check`) and driven by
// tests/test_vcfcmp_ref.py, which compares every line with the restatement.  Blocks on stdin (a text `_` is the empty text):
//   key <pos> <ref> <alt>            -> `skipped`, or `<POS'> <suffix> <prefix> <REF'> <ALT'> <hash>`: the lane's loops, and again
//                                    through the wave loops the tier-2 kernel calls (wave_skipped, wave_suffix, wave_prefix,
//                                    wave_text_hash) over an emulated wave (wave_emu.hpp); the two must agree or the program fails
//   same <pos> <ref> <alt> <pos> <ref> <alt>  -> 1 when the trimmed keys are equal (and then their hashes are), else 0
//   cell <dose a> <dose b>           -> `<class> <gteq>`, the class none, tp, fp or fn
//   chroms <threads> <bytes>         then the bytes of a VCF  -> `C` and the CHROM strings, `R` and every record's index
//                                    among them, or `error <message>`
#include "../../../include/povu_hip.h"
#include "../hip/vcfcmp_rules.hpp"
#include "wave_emu.hpp"

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

// the key as tier_items_wave of hip/vcf_pair.hpp computes it: the same calls, the wave emulated
static Key wave_key(uint64_t pos, const std::vector<char> &ref, const std::vector<char> &alt)
{
	Key k{};
	const EmuWave w;
	const uint64_t nr = ref.size(), na = alt.size();
	const auto limit = [](uint64_t a, uint64_t b) { return vm_trim_limit(a, b); };
	if ((k.skipped = wave_skipped(ref.data(), nr, alt.data(), na, w)))
		return k;
	k.s = wave_suffix(ref.data(), nr, alt.data(), na, limit, w);
	k.p = wave_prefix(ref.data(), nr, alt.data(), na, k.s, limit, w);
	k.pos = pos + k.p;
	k.hash = vm_key_hash(k.pos, nr - k.s - k.p, na - k.s - k.p, wave_text_hash(ref.data() + k.p, nr - k.s - k.p, w),
			     wave_text_hash(alt.data() + k.p, na - k.s - k.p, w));
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
