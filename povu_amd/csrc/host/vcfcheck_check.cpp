// vcfcheck_check.cpp -- the rules of the VCF checks as the device runs them (hip/vcfcheck_rules.hpp) and the VCF reader around
// them (host/vcfcheck.cpp), on the CPU.  Built with -fsanitize=address,undefined (`make vcfcheck_check`) and driven by
// tests/test_vcfcheck_ref.py, which compares every line with the restatement.  Blocks on stdin:
//   walk <text>                      -> the steps `<id>:<or> ...`, or `bad`
//   occ <rev> <m> <paths>            then a line of the m path words of the walk, a line of paths + 1 step offsets and a line of
//                                    the path words  -> the paths the walk occurs in (entirely inside), searched by the
//                                    occurrences of its anchor as the device does
//   vcf <threads> <bytes>            then the bytes of a VCF  -> the document (`S` samples, `R` record, `A` allele, `T` task
//                                    lines), or `error <message>`
//   report <paths> <bytes>           then a line `<sample column> <phase> <path words ...>` per path and the bytes of a VCF  -> the
//                                    report of `povu vcf --report` as the device makes it, over the document's tasks: a line `V
//                                    <record> ok`, or `V <record> <status> <allele>` of the record's first failing task, the
//                                    allele states and the task statuses by the rules (a walk's steps are path words as written:
//                                    <id> << 1 | '<'), searched in the path of the task's (column, phase)
#include "../../../include/povu_hip.h"
#include "../hip/vcfcheck_rules.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace povu_hip;

static void do_walk(const std::string &text)
{
	size_t i = 0;
	uint32_t id = 0;
	uint8_t rev = 0;
	int t;
	std::string out;
	while ((t = vc_next_step(text.data(), text.size(), &i, &id, &rev)) == VC_TOKEN_STEP)
		out += (out.empty() ? "" : " ") + std::to_string(id) + ":" + std::to_string(rev);
	printf("%s\n", t == VC_TOKEN_BAD ? "bad" : out.c_str());
}

static void do_occ(std::istream &in, bool rev, uint32_t m, uint32_t P)
{
	// (exact sizes: a read beyond a walk or beyond the last path is the sanitizer's to report)
	std::vector<uint32_t> w(m);
	std::vector<uint64_t> off(P + 1);
	for (auto &x : w)
		in >> x;
	for (auto &x : off)
		in >> x;
	std::vector<uint32_t> steps(off[P]);
	for (auto &x : steps)
		in >> x;
	std::vector<char> hit(P, 0);
	const uint32_t anchor = m ? vc_anchor(w.data(), m, rev) : 0;
	for (uint32_t p = 0; m && p < P; p++)
		for (uint64_t g = off[p]; g < off[p + 1]; g++)
			if (steps[g] == anchor && vc_occurs_at(steps.data(), g, off[p + 1], w.data(), m, rev))
				hit[p] = 1;
	std::string out;
	for (uint32_t p = 0; p < P; p++)
		if (hit[p])
			out += (out.empty() ? "" : " ") + std::to_string(p);
	printf("%s\n", out.c_str());
}

static void do_vcf(const std::string &text, uint32_t threads)
{
	char err[256] = {0};
	povu_hip_vcf_doc *d = povu_hip_vcf_parse(text.data(), text.size(), threads, err, sizeof err);
	if (!d) {
		printf("error %s\n", err);
		return;
	}
	printf("S");
	for (uint64_t c = 0; c < d->n_samples; c++)
		printf(" %s", d->sample[c]);
	printf("\n");
	for (uint64_t r = 0; r < d->n_records; r++) {
		printf("R %llu %llu %.*s\n", (unsigned long long)d->rec_line[r], (unsigned long long)d->rec_pos[r],
		       (int)(d->rec_id_off[r + 1] - d->rec_id_off[r]), d->ids + d->rec_id_off[r]);
		for (uint64_t a = d->allele_off[r]; a < d->allele_off[r + 1]; a++) {
			printf("A %u %.*s |", d->allele_walk[a], (int)(d->text_off[a + 1] - d->text_off[a]), d->text + d->text_off[a]);
			for (uint64_t k = d->step_off[a]; k < d->step_off[a + 1]; k++)
				printf(" %u:%u", d->step_id[k], d->step_or[k]);
			printf("\n");
		}
		for (uint64_t t = d->task_off[r]; t < d->task_off[r + 1]; t++)
			printf("T %u %u %u %u\n", d->task_record[t], d->task_allele[t], d->task_col[t], d->task_phase[t]);
	}
	povu_hip_vcf_doc_free(d);
}

static const char *const STATUS[] = {"found_fwd", "found_rev", "absent", "no_at", "bad_step", "no_slot"};
static int do_report(std::istream &in, uint32_t P, size_t bytes)
{
	struct Path {
		uint32_t col, phase;
		std::vector<uint32_t> steps;
	};
	std::vector<Path> paths(P);
	std::string line;
	for (Path &p : paths) {
		std::getline(in, line);
		std::istringstream ls(line);
		ls >> p.col >> p.phase;
		for (uint32_t x; ls >> x;)
			p.steps.push_back(x);
	}
	std::string text(bytes, '\0');
	in.read(&text[0], (std::streamsize)bytes);
	if ((size_t)in.gcount() != bytes)
		return 1;
	char err[256] = {0};
	povu_hip_vcf_doc *d = povu_hip_vcf_parse(text.data(), text.size(), 1, err, sizeof err);
	if (!d) {
		printf("error %s\n", err);
		return 0;
	}
	for (uint64_t r = 0; r < d->n_records; r++) {
		bool failed = false;
		for (uint64_t t = d->task_off[r]; t < d->task_off[r + 1] && !failed; t++) {
			const uint32_t al = d->task_allele[t], c = d->task_col[t], j = d->task_phase[t];
			const bool has = al < d->allele_off[r + 1] - d->allele_off[r];
			const uint64_t a = d->allele_off[r] + al;
			std::vector<uint32_t> w;
			uint8_t as = 0;
			if (has) {
				for (uint64_t k = d->step_off[a]; k < d->step_off[a + 1]; k++)
					w.push_back(d->step_id[k] << 1 | d->step_or[k]);
				as = vc_allele_state(d->allele_walk[a] & 2u, d->text + d->text_off[a], d->text_off[a + 1] - d->text_off[a], d->allele_walk[a] & 1u,
						     w.size(), false);
			}
			bool no_slot = true, fwd = false, rev = false;
			for (const Path &p : paths) {
				if (p.col != c || p.phase != j)
					continue;
				no_slot = false;
				for (uint64_t g = 0; has && !as && g < p.steps.size(); g++) {
					fwd |= vc_occurs_at(p.steps.data(), g, p.steps.size(), w.data(), (uint32_t)w.size(), false);
					rev |= vc_occurs_at(p.steps.data(), g, p.steps.size(), w.data(), (uint32_t)w.size(), true);
				}
			}
			const uint8_t st = vc_task_status(has, as, no_slot, fwd, rev, false);
			if (st > 1) {
				printf("V %llu %s %u\n", (unsigned long long)r, STATUS[st], al);
				failed = true;
			}
		}
		if (!failed)
			printf("V %llu ok\n", (unsigned long long)r);
	}
	povu_hip_vcf_doc_free(d);
	return 0;
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream ls(line);
		std::string cmd;
		ls >> cmd;
		if (cmd == "walk") {
			std::string text;
			ls >> text;
			do_walk(text);
		} else if (cmd == "occ") {
			uint32_t rev = 0, m = 0, P = 0;
			ls >> rev >> m >> P;
			do_occ(std::cin, rev != 0, m, P);
			std::getline(std::cin, line); // (the rest of the last line)
		} else if (cmd == "vcf") {
			uint32_t threads = 1;
			size_t bytes = 0;
			ls >> threads >> bytes;
			std::string text(bytes, '\0');
			std::cin.read(&text[0], (std::streamsize)bytes);
			if ((size_t)std::cin.gcount() != bytes) {
				fprintf(stderr, "vcfcheck_check: short input\n");
				return 1;
			}
			do_vcf(text, threads);
		} else if (cmd == "report") {
			uint32_t P = 0;
			size_t bytes = 0;
			ls >> P >> bytes;
			if (do_report(std::cin, P, bytes)) {
				fprintf(stderr, "vcfcheck_check: short input\n");
				return 1;
			}
		} else if (!cmd.empty()) {
			fprintf(stderr, "vcfcheck_check: unknown block %s\n", cmd.c_str());
			return 1;
		}
	}
	printf("vcfcheck_check: ok\n");
	return 0;
}
