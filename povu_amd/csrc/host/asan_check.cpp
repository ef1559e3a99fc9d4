// asan_check.cpp -- CPU-only sanitizer harness for the host-side code of the decompose path (built by
// `make -C povu_amd/csrc asan` with -fsanitize=address,undefined; GPU sanitizers are not available on the test pool).
// Usage: host_asan_check <file.gfa|file.pvst>...   Every .gfa goes through the tokenizer (1 and 4 threads, with
// labels and paths), every .pvst through the reader and, where it parses, through the sites of the call's host half
// (host/vcf.cpp); the names builder and the VCF writer run once over a small hand-made povu_hip_calls.  Malformed inputs
// must fail with an error, not with a fault.
#include "../../../include/povu_hip.h"
#include "gfa.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>

static bool ends_with(const std::string &s, const char *suf)
{
	const std::string t(suf);
	return s.size() >= t.size() && s.compare(s.size() - t.size(), t.size(), t) == 0;
}

// two records of one bubble >1>4 on reference path 0: an anchored multi-allelic one whose REF is allele 1 of its block, and
// one with a missing slot; names -> slots, the writer on 1 and 2 threads and for one prefix; the same with an inversion (SUBR)
// record between them; everything freed
static int check_vcf_writer()
{
	const char *path_name[] = {"R#1#c", "S#1#c", "S#2#c", "lone"}, *prefix[] = {"R#", "nobody"};
	char err[256];
	err[0] = 0;
	if (povu_hip_call_names_make(4, path_name, 1, prefix + 1, err, sizeof err) || !strstr(err, "nobody"))
		return 4;
	povu_hip_call_names *nm = povu_hip_call_names_make(4, path_name, 2, prefix, err, sizeof err);
	if (!nm || nm->refs.n_refs != 1 || nm->refs.n_samples != 3 || nm->refs.n_slots != 4)
		return 5;
	const char *text = "H\t0.0.3\t.\t.\t.\nD\t0\t.\t1\t.\nF\t1\t>1>4\t.\tL\n";
	povu_pvst_doc *doc = povu_pvst_parse(text, strlen(text), err, sizeof err);
	povu_hip_sites *sites = doc ? povu_hip_sites_of_docs(&doc, 1) : nullptr;
	if (!sites || sites->n != 1 || sites->height[0] != 1)
		return 6;
	const uint32_t query[] = {0, 0}, path[] = {0, 0}, first[] = {0, 3}, ref_allele[] = {1, 0}, n_alleles[] = {3, 2}, an[] = {4, 3},
		       ns[] = {3, 2}, block[] = {0, 1}, ac[] = {1, 1, 2};
	const uint64_t pos[] = {2, 9}, ac_off[] = {0, 2, 3}, block_off[] = {0, 3, 5}, seq_off[] = {0, 1, 5, 7, 8, 10},
		       at_off[] = {0, 2, 6, 10, 12, 14}, contig_len[] = {12};
	const uint8_t flags[] = {POVU_HIP_CALL_ANCHORED | POVU_HIP_CALL_DEL, POVU_HIP_CALL_TANGLED};
	const uint16_t gt[] = {0, 1, 2, 0, 0, 1, POVU_HIP_GT_MISSING, 1};
	const povu_hip_calls c = {2, 4, 2, 5, 10, 14, 1, query, path, first, ref_allele, n_alleles, an, ns, block, pos, flags, ac_off,
				  ac, gt, block_off, seq_off, at_off, "CCGGTCTAGT", ">1>1>2>1>3>2>3", contig_len, 0.0};
	for (uint32_t threads : {1u, 2u})
		for (const char *only : {(const char *)nullptr, "R#", "S#"}) {
			size_t len = 0;
			char *vcf = povu_hip_calls_vcf(&c, sites, nm, path_name, threads == 1 ? "20240229" : nullptr, only, threads, &len);
			if (!vcf || strlen(vcf) != len)
				return 7;
			const char *rec = strstr(vcf, "\tlone\n"); // (the column line ends with the last sample; then the records)
			if (!rec || std::count(rec + 6, (const char *)vcf + len, '\n') != (only && only[0] == 'S' ? 0 : 2) ||
			    (!(only && only[0] == 'S') && (strncmp(rec + 6, "R#1#c\t2\t>1>4\tCGGT\tC,CT\t", 22) || !strstr(rec, "\t0\t1|.\t1\n"))))
				return 8;
			povu_hip_buffer_free(vcf);
		}
	// the SUBR writer path: an inversion record between the bubble's two (no site: query NIL), REF then ALT in its own block,
	// both steps backwards (the ID is written forward); then one whose AT strings are empty -- an ID of nothing, no fault
	{
		const uint32_t query2[] = {0, POVU_HIP_NIL, 0}, path2[] = {0, 0, 0}, first2[] = {0, 1, 3}, ref2[] = {1, 0, 0}, nal2[] = {3, 2, 2},
			       an2[] = {4, 2, 3}, ns2[] = {3, 2, 2}, block2[] = {0, 2, 1}, ac2[] = {1, 1, 1, 2}, n_steps2[] = {0, 2, 0};
		const uint64_t pos2[] = {2, 3, 9}, ac_off2[] = {0, 2, 3, 4}, block_off2[] = {0, 3, 5, 7},
			       seq_off2[] = {0, 1, 5, 7, 8, 10, 12, 14}, at_off2[] = {0, 2, 6, 10, 12, 14, 19, 24};
		uint64_t at_off3[] = {0, 2, 6, 10, 12, 14, 14, 14};
		const uint8_t flags2[] = {POVU_HIP_CALL_ANCHORED | POVU_HIP_CALL_DEL, POVU_HIP_CALL_SUBR, POVU_HIP_CALL_TANGLED};
		const uint16_t gt2[] = {0, 1, 2, 0, 0, POVU_HIP_GT_MISSING, 1, POVU_HIP_GT_MISSING, 0, 1, POVU_HIP_GT_MISSING, 1};
		povu_hip_calls c2 = {3, 4, 3, 7, 14, 24, 1, query2, path2, first2, ref2, nal2, an2, ns2, block2, pos2, flags2, ac_off2,
				     ac2, gt2, block_off2, seq_off2, at_off2, "CCGGTCTAGTACGT", ">1>1>2>1>3>2>3<12<7>7>12", contig_len, 0.0,
				     n_steps2, 1, 1, 0, 0};
		for (int round = 0; round < 2; round++) {
			size_t len = 0;
			char *vcf = povu_hip_calls_vcf(&c2, sites, nm, path_name, "20240229", nullptr, 2, &len);
			if (!vcf || strlen(vcf) != len)
				return 10;
			const char *want = round ? "R#1#c\t3\t\tAC\tGT\t60\tPASS\tAC=1;AF=0.5;AN=2;NS=2;AT=,;VARTYPE=SUBR;TANGLED=F\tGT\t0\t.|1\t.\n"
						 : "R#1#c\t3\t>12>7\tAC\tGT\t60\tPASS\tAC=1;AF=0.5;AN=2;NS=2;AT=<12<7,>7>12;VARTYPE=SUBR;TANGLED=F\tGT\t0\t.|1\t.\n";
			if (!strstr(vcf, want) || std::count((const char *)vcf, (const char *)vcf + len, '\n') < 3)
				return 11;
			povu_hip_buffer_free(vcf);
			c2.at_off = at_off3;
			c2.n_at_bytes = 14;
		}
		const uint32_t nal3[] = {3, 3, 2}; // an inversion record of three alleles is refused
		c2.n_alleles = nal3;
		size_t len = 0;
		if (povu_hip_calls_vcf(&c2, sites, nm, path_name, "20240229", nullptr, 1, &len))
			return 12;
	}
	povu_hip_sites_free(sites);
	povu_pvst_doc_free(doc);
	povu_hip_call_names_free(nm);
	return 0;
}

int main(int argc, char **argv)
{
	unsigned long ok = 0, rejected = 0;
	if (int rc = check_vcf_writer())
		return rc;
	for (int i = 1; i < argc; i++) {
		const std::string path = argv[i];
		if (ends_with(path, ".gfa")) {
			for (int threads : {1, 4}) {
				try {
					povu_host::GfaGraph g = povu_host::load_gfa(path, threads == 4, threads == 4, threads);
					if (g.v1.size() != g.v2.size() || g.v1.size() != g.s1.size() || g.v1.size() != g.s2.size())
						throw std::logic_error("link arrays of different length");
					for (size_t e = 0; e < g.v1.size(); e++)
						if (g.v1[e] >= g.vid.size() || g.v2[e] >= g.vid.size() || g.s1[e] > 1 || g.s2[e] > 1)
							throw std::logic_error("link out of range");
					ok++;
				} catch (const std::runtime_error &) {
					rejected++;
				}
			}
		} else if (ends_with(path, ".pvst")) {
			std::ifstream in(path, std::ios::binary);
			std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
			// the text as it is, then truncated at every length: the reader must never read past the buffer
			for (size_t len = text.size();; len = len > 64 ? len - 17 : len - 1) {
				char err[256];
				povu_pvst_doc *d = povu_pvst_parse(text.data(), len, err, sizeof err);
				if (d) {
					for (uint32_t k = 0; k < d->n; k++)
						if (d->parent[k] != POVU_HIP_NIL && d->parent[k] >= d->n)
							return 3;
					povu_hip_sites *s = povu_hip_sites_of_docs(&d, 1);
					if (!s || s->n > d->n)
						return 9;
					for (uint32_t q = 0; q < s->n; q++)
						if ((s->parent[q] != POVU_HIP_NIL && s->parent[q] >= s->n) || s->height[q] > d->n)
							return 9;
					povu_hip_sites_free(s);
					povu_pvst_doc_free(d);
					ok++;
				} else {
					rejected++;
				}
				if (len == 0)
					break;
			}
		}
	}
	printf("host_asan_check: %lu parsed, %lu rejected\n", ok, rejected);
	return 0;
}
