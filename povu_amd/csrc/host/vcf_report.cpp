// vcf_report.cpp -- `povu vcf --report` (INTEGRATION.md "VCF checks"): the GFA's paths (and, with --spelling, sequences) to the
// GPU, the VCF parsed and checked against them (povu_hip_vcf_check), report.tsv and summary.txt written.  The reader, the
// slots and both texts are the library's (host/vcfcheck.cpp); what stays here is the command line and the files.
#include "decompose.hpp"
#include "gfa.hpp"

#include "povu_hip.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <sys/stat.h>

namespace povu_host
{

namespace
{
struct VcfArgs {
	std::string vcf, out_dir = ".";
	bool report = false, spelling = false, forward_only = false;
};

VcfArgs parse_vcf_args(const std::vector<std::string> &a)
{
	VcfArgs c;
	// `-x <v>`, `-x<v>`, `--name <v>` or `--name=<v>`
	auto value = [&](size_t &i, const std::string &shortf, const std::string &longf, std::string &out) {
		const std::string &x = a[i];
		if (x == shortf || x == longf) {
			if (i + 1 >= a.size())
				throw std::runtime_error("Flag '" + x + "' requires an argument but received none");
			out = a[++i];
		} else if (!x.compare(0, longf.size() + 1, longf + "=")) {
			out = x.substr(longf.size() + 1);
		} else if (x.size() > shortf.size() && !x.compare(0, shortf.size(), shortf) && x[1] != '-') {
			out = x.substr(shortf.size());
		} else {
			return false;
		}
		return true;
	};
	for (size_t i = 0; i < a.size(); i++) {
		const std::string &x = a[i];
		if (value(i, "-c", "--vcf", c.vcf) || value(i, "-o", "--output-dir", c.out_dir))
			continue;
		if (x == "--report")
			c.report = true;
		else if (x == "--spelling")
			c.spelling = true;
		else if (x == "--forward-only")
			c.forward_only = true;
		else if (x == "--tui")
			throw std::runtime_error("the interactive --tui is not provided by this build's `vcf`: use --report");
		else
			throw std::runtime_error("Flag could not be matched: " + x);
	}
	if (!c.report)
		throw std::runtime_error("vcf needs --report (the interactive --tui is not provided by this build)");
	if (c.vcf.empty())
		throw std::runtime_error("Flag 'vcf' is required (-c <vcf>)");
	return c;
}
} // namespace

void do_vcf(const Config &cfg, const std::vector<std::string> &args)
{
	const VcfArgs va = parse_vcf_args(args);
	std::string text;
	{
		std::ifstream in(va.vcf, std::ios::binary);
		if (!in)
			throw std::runtime_error("cannot read the VCF " + va.vcf);
		std::stringstream buf;
		buf << in.rdbuf();
		text = buf.str();
	}
	char err[512] = {0};
	const uint32_t threads = (uint32_t)std::max(1, cfg.threads);
	povu_hip_vcf_doc *doc = povu_hip_vcf_parse(text.data(), text.size(), threads, err, sizeof err);
	if (!doc)
		throw std::runtime_error(va.vcf + ": " + err);
	GfaGraph g = load_gfa(cfg.input_gfa, va.spelling, true, std::max(1, cfg.threads));
	const uint32_t V = (uint32_t)g.vid.size(), P = (uint32_t)g.paths.size();
	std::vector<const char *> names(P);
	for (uint32_t k = 0; k < P; k++)
		names[k] = g.paths[k].name.c_str();
	povu_hip_call_names *nm = povu_hip_vcf_names_make(P, names.data(), err, sizeof err);
	if (!nm) {
		povu_hip_vcf_doc_free(doc);
		throw std::runtime_error(err);
	}
	povu_hip_ctx *ctx = povu_hip_create(cfg.device, err, sizeof err);
	auto fail = [&](const std::string &what) {
		if (ctx)
			povu_hip_destroy(ctx);
		povu_hip_call_names_free(nm);
		povu_hip_vcf_doc_free(doc);
		throw std::runtime_error(what + ": " + err);
	};
	if (!ctx)
		fail("povu_hip");
	if (povu_hip_graph_upload(ctx, V, g.vid.data(), (uint32_t)g.v1.size(), g.v1.data(), g.s1.data(), g.v2.data(), g.s2.data(), nullptr, err,
				  sizeof err) != 0)
		fail("povu_hip");
	const FlatPaths fp = flatten_paths(g.paths);
	if (povu_hip_paths_upload(ctx, P, fp.off.data(), fp.ids.data(), fp.rev.data(), err, sizeof err) != 0)
		fail("paths");
	if (va.spelling) {
		std::vector<uint64_t> seq_off((size_t)V + 1, 0);
		std::string seq;
		for (uint32_t v = 0; v < V; v++) {
			if (g.seq[v] == "*") {
				snprintf(err, sizeof err, "segment %u has no sequence ('*'): --spelling needs every sequence", g.vid[v]);
				fail("sequences");
			}
			seq_off[v + 1] = seq_off[v] + g.seq[v].size();
			seq += g.seq[v];
		}
		if (povu_hip_segments_upload(ctx, V, seq_off.data(), seq.data(), err, sizeof err) != 0)
			fail("sequences");
	}
	const povu_hip_vcf_opts opts{(va.spelling ? POVU_HIP_V_SPELLING : 0u) | (va.forward_only ? POVU_HIP_V_FORWARD_ONLY : 0u)};
	povu_hip_vcf_report *rep = povu_hip_vcf_check(ctx, doc, nm, &opts, err, sizeof err);
	if (!rep)
		fail("vcf");
	size_t rlen = 0, slen = 0;
	char *summary = nullptr;
	char *report = povu_hip_vcf_report_text(rep, doc, nm, &rlen, &summary, &slen);
	std::string bad;
	if (!report) {
		bad = "cannot format the report";
	} else if (mkdir(va.out_dir.c_str(), 0777) != 0 && errno != EEXIST) {
		bad = "cannot create the output directory " + va.out_dir;
	} else {
		std::ofstream r(va.out_dir + "/report.tsv", std::ios::binary), s(va.out_dir + "/summary.txt", std::ios::binary);
		r.write(report, (std::streamsize)rlen);
		s.write(summary, (std::streamsize)slen);
		if (!r || !s)
			bad = "cannot write report.tsv and summary.txt to " + va.out_dir;
	}
	povu_hip_buffer_free(report);
	povu_hip_buffer_free(summary);
	povu_hip_vcf_report_free(rep);
	povu_hip_destroy(ctx);
	povu_hip_call_names_free(nm);
	povu_hip_vcf_doc_free(doc);
	if (!bad.empty())
		throw std::runtime_error(bad);
}

} // namespace povu_host
