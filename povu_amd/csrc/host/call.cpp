// call.cpp -- `povu call` (INTEGRATION.md "Variant calls"): the GFA's paths and sequences and the PVSTs of a forest
// directory to the GPU (povu_hip_call), the records written as VCF.  References, slots, sites and the VCF text are the
// library's (host/vcf.cpp); what stays here is the command line and the files.
#include "decompose.hpp"
#include "gfa.hpp"

#include "../hip/call_modes.hpp"
#include "../hip/span_rules.hpp"
#include "povu_hip.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <dirent.h>
#include <fstream>
#include <iostream>
#include <sys/stat.h>
#include <sstream>
#include <stdexcept>

namespace povu_host
{

namespace
{

struct CallArgs {
	std::string forest_dir = ".", out_dir;
	std::vector<std::string> prefixes;
	bool to_stdout = true;
	bool inversions = false; // --inversions: SUBR records too (INTEGRATION.md "Inversion calls")
	bool nested = false;	 // --nested, or implied by a profile (INTEGRATION.md "Nested calls")
	bool merge = false;	 // --merge-primitives, with --profile decomposed alone (INTEGRATION.md "Merged primitives")
	bool offref = false;	 // --off-reference: sites no reference path crosses, on a surrogate path (INTEGRATION.md "Off-reference calls")
	bool untangle = false;	 // --untangle: per-copy genotypes where a path laps a site (INTEGRATION.md "Untangled calls")
	bool spanning = false;	 // --spanning-alleles: an option of the nested call (INTEGRATION.md "Spanning alleles")
	std::vector<std::string> regions; // --region <name:start-end>, repeatable (INTEGRATION.md "Region calls")
	uint32_t cluster_ppm = 0;	  // --cluster <F>: F * 10^6, 0 without the flag (INTEGRATION.md "Clustered calls")
	povu_hip_call_profile_opts prof{POVU_HIP_PROFILE_RAW_GRAPH, 0, 0, 0};
};

// the POVU_HIP_T_* flags of the call
uint32_t call_flags(const CallArgs &c)
{
	return (c.inversions ? POVU_HIP_T_INVERSIONS : 0u) | (c.nested ? POVU_HIP_T_NESTED : 0u) | (c.merge ? POVU_HIP_T_MERGE : 0u) |
	       (c.offref ? POVU_HIP_T_OFFREF : 0u) | (c.untangle ? POVU_HIP_T_UNTANGLE : 0u) | (c.spanning ? POVU_HIP_T_SPANNING : 0u);
}

CallArgs parse_call_args(const std::vector<std::string> &a)
{
	CallArgs c;
	int forms = 0;
	bool by_p = false, by_pos = false;
	std::string ref_file, gpus; // gpus: a --gpus flag as it was given (it belongs to `decompose`)
	auto need =[&](size_t &i) -> const std::string & {
		if (i + 1 >= a.size())
			throw std::runtime_error("Flag '" + a[i] + "' requires an argument but received none");
		return a[++i];
	};
	// `--name <n>` or `--name=<n>`, n a decimal number
	uint64_t n64 = 0;
	auto number = [&](size_t &i, const std::string &name, uint64_t &out) {
		std::string v;
		if (a[i] == name)
			v = need(i);
		else if (!a[i].compare(0, name.size() + 1, name + "="))
			v = a[i].substr(name.size() + 1);
		else
			return false;
		if (v.empty() || !std::all_of(v.begin(), v.end(), [](char ch) { return ch >= '0' && ch <= '9'; }) || v.size() > 18)
			throw std::runtime_error("Flag '" + name + "' expects a number, not " + v);
		out = std::stoull(v);
		return true;
	};
	for (size_t i = 0; i < a.size(); i++) {
		const std::string &x = a[i];
		if (x == "-f" || x == "--forest-dir") {
			c.forest_dir = need(i);
		} else if (x == "-P" || x == "--path-prefix") {
			c.prefixes.push_back(need(i));
			by_p = true;
		} else if (x == "-r" || x == "--ref-list") {
			ref_file = need(i);
		} else if (x == "-o" || x == "--output-dir") {
			c.out_dir = need(i);
			c.to_stdout = false;
		} else if (x == "--stdout") {
			c.to_stdout = true;
		} else if (x == "--inversions") {
			c.inversions = true;
		} else if (x == "--nested") {
			c.nested = true;
		} else if (x == "--merge-primitives") {
			c.merge = true;
		} else if (x == "--off-reference") {
			c.offref = true;
		} else if (x == "--untangle") {
			c.untangle = true;
		} else if (x == "--spanning-alleles") {
			c.spanning = true;
		} else if (x == "--profile" || !x.compare(0, 10, "--profile=")) {
			const std::string v = x == "--profile" ? need(i) : x.substr(10);
			uint32_t k = 0;
			while (k < modes::N_PROFILES && v != modes::PROFILE_NAME[k])
				k++;
			c.prof.profile = k;
			if (k == modes::N_PROFILES)
				throw std::runtime_error("Flag '--profile' expects raw-graph, top-level-only, popped, left-normalized or decomposed, not " + v);
		} else if (number(i, "--max-level", n64)) {
			if (n64 > 0x7FFFFFFFull)
				throw std::runtime_error("Flag '--max-level' is too large");
			c.prof.max_level = (uint32_t)n64;
		} else if (number(i, "--max-ref-length", n64)) {
			c.prof.max_ref_length = n64;
		} else if (number(i, "--max-allele-length", n64)) {
			c.prof.max_allele_length = n64;
		} else if (x == "-c" || x == "--chunk-size" || x == "-q" || x == "--queue-length") {
			need(i); // (streaming has no meaning here: accepted and ignored)
		} else if (x == "--region" || !x.compare(0, 9, "--region=")) {
			c.regions.push_back(x == "--region" ? need(i) : x.substr(9));
			povu_hip_region r; // (the form alone: the names are not read yet)
			char err[512] = {0};
			const std::string &text = c.regions.back();
			const size_t colon = text.rfind(':');
			const std::string name = colon == std::string::npos ? std::string() : text.substr(0, colon);
			const char *one[1] = {name.c_str()};
			if (povu_hip_region_parse(text.c_str(), 1, one, &r, err, sizeof err) != 0)
				throw std::runtime_error(std::string("Flag '--region': ") + err);
		} else if (x == "--cluster" || !x.compare(0, 10, "--cluster=")) {
			const std::string v = x == "--cluster" ? need(i) : x.substr(10);
			char err[512] = {0};
			if (povu_hip_cluster_parse(v.c_str(), &c.cluster_ppm, err, sizeof err) != 0)
				throw std::runtime_error(std::string("Flag '--cluster': ") + err);
		} else if (x == "--gpus" || !x.compare(0, 7, "--gpus=")) {
			gpus = x;
			if (x == "--gpus" && i + 1 < a.size())
				i++;
		} else if (x == "-g" || x == "--restrict" || !x.compare(0, 11, "--restrict=")) {
			throw std::runtime_error("--restrict regions are not supported by this build's `call`: its --region <name:start-end> "
						 "(repeatable; 1-based start, exclusive end) restricts a call (INTEGRATION.md \"Region calls\")");
		} else if (x == "--structure-export" || !x.compare(0, 19, "--structure-export=")) {
			throw std::runtime_error("--structure-export variant frames are not supported by this build's `call`");
		} else if (!x.empty() && x[0] == '-') {
			throw std::runtime_error("Flag could not be matched: " + x);
		} else {
			c.prefixes.push_back(x);
			by_pos = true;
		}
	}
	// which modes combine: call_modes.hpp.  --gpus belongs to `decompose`: behind the refusals of --cluster, in front of the others
	const modes::Rule *no = modes::refused(modes::COMMAND_LINE, modes::set_of(call_flags(c), !c.regions.empty(), c.cluster_ppm != 0), c.prof.profile);
	if (!gpus.empty() && !(no && no->who == modes::CLUSTER))
		throw std::runtime_error(c.cluster_ppm ? "Flag '--cluster' cannot be combined with --gpus" : "Flag could not be matched: " + gpus);
	if (no)
		throw std::runtime_error(modes::message(*no, modes::COMMAND_LINE, c.prof.profile));
	// the spanning alleles are an option of the nested call, no mode of the table: refused without one, and under the profiles
	// that rewrite alleles
	if (c.spanning) {
		const bool nested = c.nested || c.prof.profile == POVU_HIP_PROFILE_TOP_LEVEL_ONLY || c.prof.profile == POVU_HIP_PROFILE_POPPED;
		if (const char *why = povu_hip::span_refused(true, nested, c.prof.profile))
			throw std::runtime_error(why);
	}
	forms = (int)by_p + (int)!ref_file.empty() + (int)by_pos;
	if (forms != 1)
		throw std::runtime_error("call needs exactly one of the reference options: -r <file>, -P <prefix> (repeatable), or "
					 "positional prefixes");
	if (!ref_file.empty()) {
		std::ifstream in(ref_file);
		if (!in)
			throw std::runtime_error("cannot read the reference list " + ref_file);
		for (std::string ln; std::getline(in, ln);) {
			while (!ln.empty() && (ln.back() == '\r' || ln.back() == ' ' || ln.back() == '\t'))
				ln.pop_back();
			if (!ln.empty())
				c.prefixes.push_back(ln);
		}
		if (c.prefixes.empty())
			throw std::runtime_error("the reference list " + ref_file + " names no prefix");
	}
	return c;
}

// the sites of every <component id>.pvst of `dir`, in component order
povu_hip_sites *read_forest(const std::string &dir)
{
	std::vector<std::pair<unsigned long, std::string>> files;
	DIR *d = opendir(dir.c_str());
	if (!d)
		throw std::runtime_error("cannot open the forest directory " + dir);
	while (dirent *e = readdir(d)) {
		const std::string nm = e->d_name;
		if (nm.size() > 5 && nm.compare(nm.size() - 5, 5, ".pvst") == 0 &&
		    std::all_of(nm.begin(), nm.end() - 5, [](char ch) { return ch >= '0' && ch <= '9'; }))
			files.emplace_back(std::stoul(nm.substr(0, nm.size() - 5)), dir + "/" + nm);
	}
	closedir(d);
	std::sort(files.begin(), files.end());
	std::vector<povu_pvst_doc *> docs;
	std::string bad;
	for (auto &[cid, path] : files) {
		std::ifstream in(path, std::ios::binary);
		std::stringstream buf;
		buf << in.rdbuf();
		const std::string text = buf.str();
		char err[512] = {0};
		docs.push_back(povu_pvst_parse(text.data(), text.size(), err, sizeof err));
		if (!docs.back()) {
			bad = path + ": " + err;
			break;
		}
		(void)cid;
	}
	povu_hip_sites *s = bad.empty() ? povu_hip_sites_of_docs(docs.data(), (uint32_t)docs.size()) : nullptr;
	for (povu_pvst_doc *x : docs)
		povu_pvst_doc_free(x);
	if (!s)
		throw std::runtime_error(bad.empty() ? "cannot build the sites of " + dir : bad);
	return s;
}

} // namespace

void do_call(const Config &cfg, const std::vector<std::string> &args)
{
	const CallArgs ca = parse_call_args(args);
	GfaGraph g = load_gfa(cfg.input_gfa, true, true, std::max(1, cfg.threads));
	const uint32_t V = (uint32_t)g.vid.size(), P = (uint32_t)g.paths.size();
	std::vector<uint64_t> seq_off((size_t)V + 1, 0);
	for (uint32_t v = 0; v < V; v++) {
		if (g.seq[v] == "*")
			throw std::runtime_error("segment " + std::to_string(g.vid[v]) + " has no sequence ('*'): call needs every sequence");
		seq_off[v + 1] = seq_off[v] + g.seq[v].size();
	}
	std::string seq;
	seq.reserve(seq_off[V]);
	for (auto &x : g.seq)
		seq += x;
	std::vector<const char *> names(P), prefixes;
	for (uint32_t k = 0; k < P; k++)
		names[k] = g.paths[k].name.c_str();
	for (auto &p : ca.prefixes)
		prefixes.push_back(p.c_str());
	char err[512] = {0};
	povu_hip_call_names *nm = povu_hip_call_names_make(P, names.data(), (uint32_t)prefixes.size(), prefixes.data(), err, sizeof err);
	if (!nm)
		throw std::runtime_error(err);
	std::vector<povu_hip_region> regions(ca.regions.size());
	for (size_t k = 0; k < regions.size(); k++)
		if (povu_hip_region_parse(ca.regions[k].c_str(), P, names.data(), &regions[k], err, sizeof err) != 0) {
			povu_hip_call_names_free(nm);
			throw std::runtime_error(std::string("Flag '--region': ") + err);
		}
	const povu_hip_call_regions rg{(uint32_t)regions.size(), 0, regions.data()};
	povu_hip_sites *sites = read_forest(ca.forest_dir);

	povu_hip_ctx *ctx = povu_hip_create(cfg.device, err, sizeof err);
	if (!ctx)
		throw std::runtime_error(std::string("povu_hip: ") + err);
	auto fail = [&](const char *what) {
		povu_hip_destroy(ctx);
		throw std::runtime_error(std::string(what) + ": " + err);
	};
	if (povu_hip_graph_upload(ctx, V, g.vid.data(), (uint32_t)g.v1.size(), g.v1.data(), g.s1.data(), g.v2.data(), g.s2.data(), nullptr,
				  err, sizeof err) != 0)
		fail("povu_hip");
	const FlatPaths fp = flatten_paths(g.paths);
	if (povu_hip_paths_upload(ctx, P, fp.off.data(), fp.ids.data(), fp.rev.data(), err, sizeof err) != 0)
		fail("paths");
	if (povu_hip_segments_upload(ctx, V, seq_off.data(), seq.data(), err, sizeof err) != 0)
		fail("sequences");
	const povu_hip_trav_opts opts{0, call_flags(ca)};
	const povu_hip_call_cluster_opts cl{ca.cluster_ppm, 0};
	povu_hip_calls *c = povu_hip_call_clustered(ctx, sites, &nm->refs, nm->slot_of_path, &opts, &ca.prof, regions.empty() ? nullptr : &rg,
						    ca.cluster_ppm ? &cl : nullptr, err, sizeof err);
	if (!c)
		fail("call");

	// ---- the files: one VCF of every reference (--stdout), or <dir>/<prefix>.vcf per prefix with its references' records
	auto write = [&](std::ostream &os, const char *only) {
		size_t len = 0;
		char *text = povu_hip_calls_vcf_profile(c, sites, nm, names.data(), nullptr, only, (uint32_t)std::max(1, cfg.threads), ca.prof.profile, &len);
		if (!text)
			throw std::runtime_error("cannot format the calls as VCF");
		os.write(text, (std::streamsize)len);
		povu_hip_buffer_free(text);
	};
	if (ca.to_stdout) {
		write(std::cout, nullptr);
		std::cout.flush();
	} else {
		if (mkdir(ca.out_dir.c_str(), 0777) != 0 && errno != EEXIST)
			throw std::runtime_error("cannot create the output directory " + ca.out_dir);
		for (auto &p : ca.prefixes) {
			std::ofstream os(ca.out_dir + "/" + p + ".vcf");
			if (!os)
				throw std::runtime_error("cannot write " + ca.out_dir + "/" + p + ".vcf");
			write(os, p.c_str());
		}
		// the off-reference records no prefix takes
		bool rest = false;
		for (uint64_t i = 0; ca.offref && !rest && i < c->n_records; i++)
			rest = c->rec_offref[i] && std::none_of(ca.prefixes.begin(), ca.prefixes.end(), [&](const std::string &p) {
				       return !strncmp(names[c->path[i]], p.c_str(), p.size());
			       });
		if (rest) {
			size_t len = 0;
			char *text = povu_hip_calls_vcf_rest(c, sites, nm, names.data(), nullptr, prefixes.data(), (uint32_t)prefixes.size(),
							     (uint32_t)std::max(1, cfg.threads), ca.prof.profile, &len);
			std::ofstream os(ca.out_dir + "/off-reference.vcf");
			if (!text || !os)
				throw std::runtime_error("cannot write " + ca.out_dir + "/off-reference.vcf");
			os.write(text, (std::streamsize)len);
			povu_hip_buffer_free(text);
		}
	}
	povu_hip_calls_free(c);
	povu_hip_destroy(ctx);
	povu_hip_sites_free(sites);
	povu_hip_call_names_free(nm);
}

} // namespace povu_host
