// vcf_report.cpp -- `povu vcf --report` (INTEGRATION.md "VCF checks"): the GFA's paths (and, with --spelling, sequences) to the
// GPU, the VCF parsed and checked against them (povu_hip_vcf_check), report.tsv and summary.txt written.  The reader, the
// slots and both texts are the library's (host/vcfcheck.cpp); what stays here is the command line and the files.
// `povu vcf --compare` (INTEGRATION.md "VCF comparison") likewise: two VCFs parsed and compared on a fresh context
// (povu_hip_vcf_compare), compare.tsv and summary.txt written; the GFA is not read.  With --haplotypes (INTEGRATION.md
// "Haplotype comparison") the haplotypes the two spell are compared too (povu_hip_vcf_haplotypes) and haplotypes.tsv and
// hap_summary.txt written beside them: against the paths and sequences of the GFA when -i names one, else by the REF fields.
// `povu vcf --consensus` (INTEGRATION.md "Consensus haplotypes"): the GFA's graph, paths and sequences to the GPU, the VCF's calls
// applied to the paths its CHROMs name (povu_hip_vcf_consensus, one call per CHROM so that a cohort does not meet the output
// limit at once), consensus.fa, roundtrip.tsv and cons_summary.txt written.
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
	std::string vcf, other_vcf, out_dir = ".";
	bool report = false, compare = false, spelling = false, forward_only = false, haplotypes = false, have_max_reach = false;
	uint32_t max_reach = POVU_HIP_H_MAX_REACH_DEFAULT;
	bool consensus = false, roundtrip = false, no_fasta = false, have_line_width = false;
	uint32_t line_width = 60;
	std::vector<std::string> samples, chroms;
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
		if (value(i, "-c", "--vcf", c.vcf) || value(i, "-o", "--output-dir", c.out_dir) || value(i, "-d", "--other-input-vcf", c.other_vcf))
			continue;
		std::string reach;
		if (value(i, "--max-reach", "--max-reach", reach)) {
			char *end = nullptr;
			const unsigned long long v = strtoull(reach.c_str(), &end, 10);
			if (reach.empty() || *end || reach[0] == '-' || v > POVU_HIP_H_MAX_REACH_MOST)
				throw std::runtime_error("Flag '--max-reach' expects a number of bases between 0 and " + std::to_string(POVU_HIP_H_MAX_REACH_MOST));
			c.max_reach = (uint32_t)v, c.have_max_reach = true;
			continue;
		}
		std::string one;
		if (value(i, "--sample", "--sample", one)) {
			c.samples.push_back(one);
			continue;
		}
		if (value(i, "--chrom", "--chrom", one)) {
			c.chroms.push_back(one);
			continue;
		}
		if (value(i, "--line-width", "--line-width", one)) {
			char *end = nullptr;
			const unsigned long long v = strtoull(one.c_str(), &end, 10);
			if (one.empty() || *end || one[0] == '-' || v > 0xFFFFFFFFull)
				throw std::runtime_error("Flag '--line-width' expects a number of bases, 0 for no wrap");
			c.line_width = (uint32_t)v, c.have_line_width = true;
			continue;
		}
		if (x == "--consensus")
			c.consensus = true;
		else if (x == "--roundtrip")
			c.roundtrip = true;
		else if (x == "--no-fasta")
			c.no_fasta = true;
		else if (x == "--tui" && std::find(a.begin(), a.end(), "--consensus") != a.end())
			throw std::runtime_error("--consensus and --tui exclude each other (the interactive --tui is not provided by this build)");
		else if (x == "--report")
			c.report = true;
		else if (x == "--haplotypes")
			c.haplotypes = true;
		else if (x == "--compare")
			c.compare = true;
		else if (x == "--spelling")
			c.spelling = true;
		else if (x == "--forward-only")
			c.forward_only = true;
		else if (x == "--tui")
			throw std::runtime_error("the interactive --tui is not provided by this build's `vcf`: use --report");
		else
			throw std::runtime_error("Flag could not be matched: " + x);
	}
	if (!c.consensus) {
		const char *sub = c.roundtrip ? "--roundtrip" : c.no_fasta ? "--no-fasta" : !c.samples.empty() ? "--sample" : !c.chroms.empty() ? "--chrom" :
				  c.have_line_width ? "--line-width" : nullptr;
		if (sub)
			throw std::runtime_error(std::string(sub) + " is read by --consensus only");
	} else {
		if (c.report || c.compare)
			throw std::runtime_error(std::string("--consensus and ") + (c.report ? "--report" : "--compare") + " exclude each other");
		const char *other = c.haplotypes ? "--haplotypes" : c.have_max_reach ? "--max-reach" : c.spelling ? "--spelling" : c.forward_only ? "--forward-only" :
				    !c.other_vcf.empty() ? "-d (--other-input-vcf)" : nullptr;
		if (other)
			throw std::runtime_error(std::string(other) + " is not read by --consensus");
		if (c.vcf.empty())
			throw std::runtime_error("Flag 'vcf' is required (-c <vcf>)");
		return c;
	}
	if ((c.haplotypes || c.have_max_reach) && (c.report || !c.compare))
		throw std::runtime_error(std::string(c.haplotypes ? "--haplotypes" : "--max-reach") +
					 (c.report ? " belongs to --compare, not to --report" : " is read by --compare only"));
	if (c.have_max_reach && !c.haplotypes)
		throw std::runtime_error("--max-reach is read by --haplotypes only");
	if (c.report && c.compare)
		throw std::runtime_error("--compare and --report exclude each other");
	if (!c.other_vcf.empty() && !c.compare)
		throw std::runtime_error("Flag '-d' (--other-input-vcf) is read by --compare only");
	if (!c.report && !c.compare)
		throw std::runtime_error("vcf needs --report (the interactive --tui is not provided by this build)");
	if (c.compare && c.other_vcf.empty())
		throw std::runtime_error("--compare needs the other VCF: Flag 'other-input-vcf' is required (-d <vcf>)");
	if (c.compare && (c.spelling || c.forward_only))
		throw std::runtime_error(std::string(c.spelling ? "--spelling" : "--forward-only") + " belongs to --report, not to --compare");
	if (c.vcf.empty())
		throw std::runtime_error("Flag 'vcf' is required (-c <vcf>)");
	return c;
}

std::string read_vcf(const std::string &path)
{
	std::ifstream in(path, std::ios::binary);
	if (!in)
		throw std::runtime_error("cannot read the VCF " + path);
	std::stringstream buf;
	buf << in.rdbuf();
	return buf.str();
}

// The haplotypes of both documents compared on `ctx`: with a GFA (-i) its graph, paths and sequences go to the context first and
// the paths are the reference, else the REF fields are
povu_hip_vcf_hap *compare_haplotypes(const Config &cfg, const VcfArgs &va, povu_hip_ctx *ctx, const povu_hip_vcf_doc *a, const povu_hip_vcf_doc *b)
{
	char err[512] = {0};
	const povu_hip_vcf_hap_opts opts{0u, va.max_reach};
	povu_hip_vcf_hap *hap = nullptr;
	if (cfg.input_gfa.empty()) {
		hap = povu_hip_vcf_haplotypes(ctx, a, b, nullptr, 0, &opts, err, sizeof err);
	} else {
		GfaGraph g = load_gfa(cfg.input_gfa, true, true, std::max(1, cfg.threads));
		const uint32_t V = (uint32_t)g.vid.size(), P = (uint32_t)g.paths.size();
		std::vector<const char *> names(P);
		for (uint32_t k = 0; k < P; k++)
			names[k] = g.paths[k].name.c_str();
		if (povu_hip_graph_upload(ctx, V, g.vid.data(), (uint32_t)g.v1.size(), g.v1.data(), g.s1.data(), g.v2.data(), g.s2.data(), nullptr, err,
					  sizeof err) != 0)
			throw std::runtime_error(std::string("povu_hip: ") + err);
		const FlatPaths fp = flatten_paths(g.paths);
		if (povu_hip_paths_upload(ctx, P, fp.off.data(), fp.ids.data(), fp.rev.data(), err, sizeof err) != 0)
			throw std::runtime_error(std::string("paths: ") + err);
		std::vector<uint64_t> seq_off((size_t)V + 1, 0);
		std::string seq;
		for (uint32_t v = 0; v < V; v++) {
			if (g.seq[v] == "*")
				throw std::runtime_error("sequences: segment " + std::to_string(g.vid[v]) + " has no sequence ('*'): a reference needs every sequence");
			seq_off[v + 1] = seq_off[v] + g.seq[v].size();
			seq += g.seq[v];
		}
		if (povu_hip_segments_upload(ctx, V, seq_off.data(), seq.data(), err, sizeof err) != 0)
			throw std::runtime_error(std::string("sequences: ") + err);
		hap = povu_hip_vcf_haplotypes(ctx, a, b, names.data(), P, &opts, err, sizeof err);
	}
	if (!hap)
		throw std::runtime_error(std::string("vcf: ") + err);
	return hap;
}

void do_compare(const Config &cfg, const VcfArgs &va)
{
	char err[512] = {0};
	const uint32_t threads = (uint32_t)std::max(1, cfg.threads);
	povu_hip_vcf_doc *doc[2] = {nullptr, nullptr};
	povu_hip_ctx *ctx = nullptr;
	povu_hip_vcf_cmp *cmp = nullptr;
	povu_hip_vcf_hap *hap = nullptr;
	char *table = nullptr, *summary = nullptr, *hap_table = nullptr, *hap_summary = nullptr;
	std::string bad;
	for (int k = 0; k < 2 && bad.empty(); k++) {
		const std::string &path = k ? va.other_vcf : va.vcf;
		try {
			const std::string text = read_vcf(path);
			doc[k] = povu_hip_vcf_parse(text.data(), text.size(), threads, err, sizeof err);
			if (!doc[k])
				bad = path + ": " + err;
		} catch (const std::runtime_error &e) {
			bad = e.what();
		}
	}
	if (bad.empty() && !(ctx = povu_hip_create(cfg.device, err, sizeof err)))
		bad = std::string("povu_hip: ") + err;
	if (bad.empty() && !(cmp = povu_hip_vcf_compare(ctx, doc[0], doc[1], nullptr, err, sizeof err)))
		bad = std::string("vcf: ") + err;
	size_t tlen = 0, slen = 0;
	if (bad.empty() && !(table = povu_hip_vcf_cmp_text(cmp, doc[0], doc[1], &tlen, &summary, &slen)))
		bad = "cannot format the comparison";
	if (bad.empty() && mkdir(va.out_dir.c_str(), 0777) != 0 && errno != EEXIST)
		bad = "cannot create the output directory " + va.out_dir;
	if (bad.empty()) {
		std::ofstream t(va.out_dir + "/compare.tsv", std::ios::binary), s(va.out_dir + "/summary.txt", std::ios::binary);
		t.write(table, (std::streamsize)tlen);
		s.write(summary, (std::streamsize)slen);
		if (!t || !s)
			bad = "cannot write compare.tsv and summary.txt to " + va.out_dir;
	}
	if (bad.empty() && va.haplotypes) {
		try {
			hap = compare_haplotypes(cfg, va, ctx, doc[0], doc[1]);
		} catch (const std::runtime_error &e) {
			bad = e.what();
		}
		size_t hlen = 0, hslen = 0;
		if (bad.empty() && !(hap_table = povu_hip_vcf_hap_text(hap, doc[0], doc[1], &hlen, &hap_summary, &hslen)))
			bad = "cannot format the haplotype comparison";
		if (bad.empty()) {
			std::ofstream t(va.out_dir + "/haplotypes.tsv", std::ios::binary), s(va.out_dir + "/hap_summary.txt", std::ios::binary);
			t.write(hap_table, (std::streamsize)hlen);
			s.write(hap_summary, (std::streamsize)hslen);
			if (!t || !s)
				bad = "cannot write haplotypes.tsv and hap_summary.txt to " + va.out_dir;
		}
	}
	povu_hip_buffer_free(hap_table);
	povu_hip_buffer_free(hap_summary);
	if (hap)
		povu_hip_vcf_hap_free(hap);
	povu_hip_buffer_free(table);
	povu_hip_buffer_free(summary);
	if (cmp)
		povu_hip_vcf_cmp_free(cmp);
	if (ctx)
		povu_hip_destroy(ctx);
	for (povu_hip_vcf_doc *d : doc)
		if (d)
			povu_hip_vcf_doc_free(d);
	if (!bad.empty())
		throw std::runtime_error(bad);
}

// The graph, paths and sequences of the GFA made resident in `ctx`; gives the path names
std::vector<std::string> upload_reference(const Config &cfg, povu_hip_ctx *ctx)
{
	char err[512] = {0};
	GfaGraph g = load_gfa(cfg.input_gfa, true, true, std::max(1, cfg.threads));
	const uint32_t V = (uint32_t)g.vid.size(), P = (uint32_t)g.paths.size();
	if (povu_hip_graph_upload(ctx, V, g.vid.data(), (uint32_t)g.v1.size(), g.v1.data(), g.s1.data(), g.v2.data(), g.s2.data(), nullptr, err, sizeof err) != 0)
		throw std::runtime_error(std::string("povu_hip: ") + err);
	const FlatPaths fp = flatten_paths(g.paths);
	if (povu_hip_paths_upload(ctx, P, fp.off.data(), fp.ids.data(), fp.rev.data(), err, sizeof err) != 0)
		throw std::runtime_error(std::string("paths: ") + err);
	std::vector<uint64_t> seq_off((size_t)V + 1, 0);
	std::string seq;
	for (uint32_t v = 0; v < V; v++) {
		if (g.seq[v] == "*")
			throw std::runtime_error("sequences: segment " + std::to_string(g.vid[v]) + " has no sequence ('*'): a consensus needs every sequence");
		seq_off[v + 1] = seq_off[v] + g.seq[v].size();
		seq += g.seq[v];
	}
	if (povu_hip_segments_upload(ctx, V, seq_off.data(), seq.data(), err, sizeof err) != 0)
		throw std::runtime_error(std::string("sequences: ") + err);
	std::vector<std::string> names;
	for (const auto &p : g.paths)
		names.push_back(p.name);
	return names;
}

struct ConsRun {
	povu_hip_vcf_doc *doc = nullptr;
	povu_hip_ctx *ctx = nullptr;
	povu_hip_call_names *names = nullptr;
	std::vector<povu_hip_vcf_cons *> parts;
	~ConsRun()
	{
		for (povu_hip_vcf_cons *c : parts)
			povu_hip_vcf_cons_free(c);
		if (names)
			povu_hip_call_names_free(names);
		if (ctx)
			povu_hip_destroy(ctx);
		if (doc)
			povu_hip_vcf_doc_free(doc);
	}
};

void do_consensus(const Config &cfg, const VcfArgs &va)
{
	char err[512] = {0};
	ConsRun run;
	const std::string text = read_vcf(va.vcf);
	if (!(run.doc = povu_hip_vcf_parse(text.data(), text.size(), (uint32_t)std::max(1, cfg.threads), err, sizeof err)))
		throw std::runtime_error(va.vcf + ": " + err);
	const povu_hip_vcf_doc *doc = run.doc;
	// the selection, by name
	std::vector<uint32_t> cols, chroms;
	for (const std::string &n : va.samples) {
		const size_t before = cols.size();
		for (uint64_t c = 0; c < doc->n_samples; c++)
			if (n == doc->sample[c])
				cols.push_back((uint32_t)c);
		if (cols.size() == before)
			throw std::runtime_error("--sample " + n + ": the VCF has no such sample column");
	}
	for (uint64_t c = 0; c < doc->n_chroms; c++)
		if (va.chroms.empty() || std::find(va.chroms.begin(), va.chroms.end(), doc->chrom[c]) != va.chroms.end())
			chroms.push_back((uint32_t)c);
	for (const std::string &n : va.chroms)
		if (std::find_if(chroms.begin(), chroms.end(), [&](uint32_t c) { return n == doc->chrom[c]; }) == chroms.end())
			throw std::runtime_error("--chrom " + n + ": the VCF has no record with that CHROM");
	if (!(run.ctx = povu_hip_create(cfg.device, err, sizeof err)))
		throw std::runtime_error(std::string("povu_hip: ") + err);
	const std::vector<std::string> path_names = upload_reference(cfg, run.ctx);
	std::vector<const char *> names(path_names.size());
	for (size_t k = 0; k < names.size(); k++)
		names[k] = path_names[k].c_str();
	if (!(run.names = povu_hip_vcf_names_make((uint32_t)names.size(), names.data(), err, sizeof err)))
		throw std::runtime_error(err);
	// one call per CHROM (one call without a CHROM for a document without records: it gives the empty result)
	const uint32_t flags = (va.roundtrip ? POVU_HIP_C_ROUNDTRIP : 0u) | (va.no_fasta ? POVU_HIP_C_NO_TEXT : 0u);
	std::string fasta;
	std::vector<uint32_t> u32[9];
	std::vector<uint64_t> u64[4];
	std::vector<uint8_t> status;
	povu_hip_vcf_cons all{};
	for (size_t k = 0; k < std::max<size_t>(chroms.size(), 1); k++) {
		const uint32_t n = (uint32_t)std::max<size_t>(cols.size(), chroms.empty() ? 0 : 1);
		std::vector<uint32_t> sel_col(cols), sel_chrom(n, chroms.empty() ? 0u : chroms[k]);
		sel_col.resize(n, cols.empty() ? 0u : cols[0]);
		const povu_hip_vcf_cons_opts opts{flags, n, cols.empty() ? nullptr : sel_col.data(), chroms.empty() ? nullptr : sel_chrom.data()};
		povu_hip_vcf_cons *c = povu_hip_vcf_consensus(run.ctx, doc, names.data(), (uint32_t)names.size(), &opts, err, sizeof err);
		if (!c)
			throw std::runtime_error(std::string("vcf: ") + err);
		run.parts.push_back(c);
		size_t fl = 0, rl = 0, sl = 0;
		char *rt = nullptr, *sum = nullptr;
		char *fa = povu_hip_vcf_cons_text(c, doc, run.names, names.data(), va.line_width, &fl, &rt, &rl, &sum, &sl);
		if (!fa)
			throw std::runtime_error("cannot format the consensus");
		fasta.append(fa, fl);
		povu_hip_buffer_free(fa), povu_hip_buffer_free(rt), povu_hip_buffer_free(sum);
		const uint32_t *a32[9] = {c->hap_chrom, c->hap_col, c->hap_phase, c->n_applied, c->n_duplicate, c->n_enclosed, c->n_overlap, c->n_unspelled, c->n_nocall};
		const uint64_t *a64[4] = {c->hap_len, c->hap_off, c->rt_path_len, c->rt_first_diff};
		for (int x = 0; x < 9; x++)
			u32[x].insert(u32[x].end(), a32[x], a32[x] + c->n_haps);
		for (int x = 0; x < 4; x++)
			u64[x].insert(u64[x].end(), a64[x], a64[x] + c->n_haps);
		status.insert(status.end(), c->rt_status, c->rt_status + c->n_haps);
		all.n_haps += c->n_haps, all.n_text_bytes += c->n_text_bytes, all.n_unplaced = c->n_unplaced, all.roundtrip = c->roundtrip;
	}
	std::vector<uint32_t> paths;
	for (const povu_hip_vcf_cons *c : run.parts)
		paths.insert(paths.end(), c->rt_path, c->rt_path + c->n_haps);
	all.hap_chrom = u32[0].data(), all.hap_col = u32[1].data(), all.hap_phase = u32[2].data(), all.n_applied = u32[3].data(), all.n_duplicate = u32[4].data();
	all.n_enclosed = u32[5].data(), all.n_overlap = u32[6].data(), all.n_unspelled = u32[7].data(), all.n_nocall = u32[8].data();
	all.hap_len = u64[0].data(), all.hap_off = u64[1].data(), all.rt_path_len = u64[2].data(), all.rt_first_diff = u64[3].data();
	all.rt_status = status.data(), all.rt_path = paths.data();
	size_t fl = 0, rl = 0, sl = 0;
	char *rt = nullptr, *sum = nullptr;
	char *none = povu_hip_vcf_cons_text(&all, doc, run.names, names.data(), va.line_width, &fl, &rt, &rl, &sum, &sl);
	if (!none)
		throw std::runtime_error("cannot format the consensus");
	std::string bad;
	if (mkdir(va.out_dir.c_str(), 0777) != 0 && errno != EEXIST) {
		bad = "cannot create the output directory " + va.out_dir;
	} else {
		std::ofstream r(va.out_dir + "/roundtrip.tsv", std::ios::binary), s(va.out_dir + "/cons_summary.txt", std::ios::binary);
		r.write(rt, (std::streamsize)rl);
		s.write(sum, (std::streamsize)sl);
		bool ok = r && s;
		if (!va.no_fasta) {
			std::ofstream f(va.out_dir + "/consensus.fa", std::ios::binary);
			f.write(fasta.data(), (std::streamsize)fasta.size());
			ok = ok && f;
		}
		if (!ok)
			bad = "cannot write the consensus files to " + va.out_dir;
	}
	povu_hip_buffer_free(none), povu_hip_buffer_free(rt), povu_hip_buffer_free(sum);
	if (!bad.empty())
		throw std::runtime_error(bad);
}
} // namespace

// cli.cpp does not require -i for these arguments of `vcf`: they ask for --compare, which reads no GFA, or for --consensus,
// which refuses a missing -i in its own words
bool vcf_args_check_gfa_themselves(const std::vector<std::string> &args)
{
	return std::find(args.begin(), args.end(), "--compare") != args.end() || std::find(args.begin(), args.end(), "--consensus") != args.end();
}

void do_vcf(const Config &cfg, const std::vector<std::string> &args)
{
	const VcfArgs va = parse_vcf_args(args);
	if (va.consensus) {
		if (cfg.input_gfa.empty())
			throw std::runtime_error("--consensus needs the graph whose paths the CHROMs name: Flag 'gfa' is required (-i <gfa>)");
		do_consensus(cfg, va);
		return;
	}
	if (va.compare) {
		do_compare(cfg, va);
		return;
	}
	const std::string text = read_vcf(va.vcf);
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
