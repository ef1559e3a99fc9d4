// call.cpp -- `povu call` (INTEGRATION.md "Variant calls"): the GFA's paths and sequences and the PVSTs of a forest
// directory to the GPU (povu_hip_call), the records formatted on up to -t threads and written as VCF.
#include "decompose.hpp"
#include "gfa.hpp"

#include "povu_hip.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <dirent.h>
#include <fstream>
#include <iostream>
#include <sys/stat.h>
#include <map>
#include <sstream>
#include <stdexcept>
#include <thread>

namespace povu_host
{

namespace
{

const char *VCF_HEADER =
	"##source=povu\n"
	"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
	"##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Total number of alternate alleles in called genotypes\">\n"
	"##INFO=<ID=AT,Number=R,Type=String,Description=\"Allele traversal path through the graph\">\n"
	"##INFO=<ID=AN,Number=1,Type=String,Description=\"Total number of alleles in called genotypes\">\n"
	"##INFO=<ID=AF,Number=A,Type=Float,Description=\"Allele frequency in the population\">\n"
	"##INFO=<ID=NS,Number=1,Type=Integer,Description=\"Number of samples with data\">\n"
	"##INFO=<ID=VARTYPE,Number=1,Type=String,Description=\"Type of variation: INS (insertion), DEL (deletion), SUB (substitution), "
	"SUBR(substitution in reverse) \">\n"
	"##INFO=<ID=TANGLED,Number=1,Type=String,Description=\"Variant lies in a tangled region of the graph: T or F\">\n"
	"##INFO=<ID=LV,Number=1,Type=Integer,Description=\"Level in the PVST (0=top level)\">\n"
	"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";

struct CallArgs {
	std::string forest_dir = ".", out_dir;
	std::vector<std::string> prefixes;
	bool to_stdout = true;
};

CallArgs parse_call_args(const std::vector<std::string> &a)
{
	CallArgs c;
	int forms = 0;
	bool by_p = false, by_pos = false;
	std::string ref_file;
	auto need = [&](size_t &i) -> const std::string & {
		if (i + 1 >= a.size())
			throw std::runtime_error("Flag '" + a[i] + "' requires an argument but received none");
		return a[++i];
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
		} else if (x == "-c" || x == "--chunk-size" || x == "-q" || x == "--queue-length") {
			need(i); // (streaming has no meaning here: accepted and ignored)
		} else if (x == "-g" || x == "--restrict" || !x.compare(0, 11, "--restrict=")) {
			throw std::runtime_error("--restrict regions are not supported by this build's `call`");
		} else if (x == "--structure-export" || !x.compare(0, 19, "--structure-export=")) {
			throw std::runtime_error("--structure-export variant frames are not supported by this build's `call`");
		} else if (!x.empty() && x[0] == '-') {
			throw std::runtime_error("Flag could not be matched: " + x);
		} else {
			c.prefixes.push_back(x);
			by_pos = true;
		}
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

std::pair<std::string, long> pansn(const std::string &n)
{
	const size_t a = n.find('#');
	if (a != std::string::npos) {
		const size_t b = n.find('#', a + 1);
		if (b != std::string::npos && b > a + 1 && std::all_of(n.begin() + a + 1, n.begin() + b, [](char ch) { return ch >= '0' && ch <= '9'; }))
			return {n.substr(0, a), std::stol(n.substr(a + 1, b - a - 1))};
	}
	return {n, -1};
}

struct Sites {
	std::vector<uint32_t> id1, id2, parent, height, tree;
	std::vector<uint8_t> or1, or2, fam;
	std::vector<std::string> label;
};

// every <component id>.pvst of `dir`, in component order
Sites read_forest(const std::string &dir)
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
	Sites s;
	uint32_t tree = 0;
	for (auto &[cid, path] : files) {
		std::ifstream in(path, std::ios::binary);
		std::stringstream buf;
		buf << in.rdbuf();
		const std::string text = buf.str();
		char err[512] = {0};
		povu_pvst_doc *doc = povu_pvst_parse(text.data(), text.size(), err, sizeof err);
		if (!doc)
			throw std::runtime_error(path + ": " + err);
		std::vector<uint32_t> qnum(doc->n, POVU_HIP_NIL);
		uint32_t next = (uint32_t)s.id1.size();
		for (uint32_t v = 0; v < doc->n; v++)
			if (doc->type[v] != 'D')
				qnum[v] = next++;
		for (uint32_t v = 0; v < doc->n; v++) {
			if (doc->type[v] == 'D')
				continue;
			s.id1.push_back(doc->a_id[v]);
			s.id2.push_back(doc->z_id[v]);
			s.or1.push_back(doc->a_or[v]);
			s.or2.push_back(doc->z_or[v]);
			const uint32_t p = doc->parent[v];
			s.parent.push_back(p == POVU_HIP_NIL || p >= doc->n ? POVU_HIP_NIL : qnum[p]);
			s.height.push_back(doc->height[v]);
			s.fam.push_back((uint8_t)doc->type[v]);
			s.tree.push_back(tree);
			s.label.push_back(std::string(doc->a_or[v] ? "<" : ">") + std::to_string(doc->a_id[v]) + (doc->z_or[v] ? "<" : ">") +
					  std::to_string(doc->z_id[v]));
		}
		povu_pvst_doc_free(doc);
		tree++;
		(void)cid;
	}
	return s;
}

std::string today()
{
	char b[16];
	const time_t t = time(nullptr);
	struct tm tmv;
	localtime_r(&t, &tmv);
	strftime(b, sizeof b, "%Y%m%d", &tmv);
	return b;
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
	std::vector<std::string> names(P);
	for (uint32_t k = 0; k < P; k++)
		names[k] = g.paths[k].name;
	std::vector<uint32_t> ref_path;
	for (uint32_t k = 0; k < P; k++)
		for (auto &p : ca.prefixes)
			if (!names[k].compare(0, p.size(), p)) {
				ref_path.push_back(k);
				break;
			}
	if (ref_path.empty()) {
		std::string l;
		for (auto &p : ca.prefixes)
			l += (l.empty() ? "" : ", ") + p;
		throw std::runtime_error("no path name starts with any of the reference prefixes " + l);
	}
	// PanSN slots
	std::vector<std::string> samples;
	std::map<std::string, std::vector<long>> haps;
	for (auto &n : names) {
		auto [sm, h] = pansn(n);
		if (!haps.count(sm))
			samples.push_back(sm);
		auto &hv = haps[sm];
		if (std::find(hv.begin(), hv.end(), h) == hv.end())
			hv.push_back(h);
	}
	std::map<std::pair<std::string, long>, uint32_t> slot_id;
	std::vector<uint32_t> sample_of_slot, slot_first{0};
	for (uint32_t si = 0; si < samples.size(); si++) {
		auto hv = haps[samples[si]];
		std::sort(hv.begin(), hv.end());
		for (long h : hv) {
			slot_id[{samples[si], h}] = (uint32_t)sample_of_slot.size();
			sample_of_slot.push_back(si);
		}
		slot_first.push_back((uint32_t)sample_of_slot.size());
	}
	std::vector<uint32_t> slot_of_path(P);
	for (uint32_t k = 0; k < P; k++)
		slot_of_path[k] = slot_id[pansn(names[k])];
	const Sites st = read_forest(ca.forest_dir);

	char err[512] = {0};
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
	povu_hip_sites sites{(uint32_t)st.id1.size(), st.id1.data(), st.id2.data(), st.or1.data(), st.or2.data(), st.parent.data(),
			     st.height.data(), st.fam.data(), st.tree.data()};
	povu_hip_call_refs refs{(uint32_t)ref_path.size(), ref_path.data(), (uint32_t)sample_of_slot.size(), (uint32_t)samples.size(),
				sample_of_slot.data()};
	povu_hip_calls *c = povu_hip_call(ctx, &sites, &refs, slot_of_path.data(), nullptr, err, sizeof err);
	if (!c)
		fail("call");

	// ---- the records as text, in chunks of records on up to -t threads
	const uint64_t n = c->n_records, S = c->n_slots;
	const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, cfg.threads), (n + 1023) / 1024));
	std::vector<std::string> chunk(T);
	auto format = [&](int t) {
		std::string &o = chunk[t];
		const uint64_t lo = n * t / T, hi = n * (t + 1) / T;
		std::vector<uint64_t> order;
		char num[32];
		for (uint64_t i = lo; i < hi; i++) {
			const uint32_t q = c->query[i], na = c->n_alleles[i], ra = c->ref_allele[i];
			const uint64_t b = c->block_off[c->block[i]];
			order.clear();
			order.push_back(b + ra);
			for (uint32_t a = 0; a < na; a++)
				if (a != ra)
					order.push_back(b + a);
			o += names[c->path[i]];
			o += '\t';
			o += std::to_string(c->pos[i]);
			o += '\t';
			o += st.label[q];
			for (size_t k = 0; k < order.size(); k++) {
				o += k <= 1 ? '\t' : ',';
				o.append(c->seq + c->seq_off[order[k]], c->seq_off[order[k] + 1] - c->seq_off[order[k]]);
			}
			o += "\t60\tPASS\tAC=";
			const uint64_t a0 = c->ac_off[i], a1 = c->ac_off[i + 1];
			const uint32_t an = c->an[i];
			for (uint64_t k = a0; k < a1; k++)
				o += (k > a0 ? "," : "") + std::to_string(c->ac[k]);
			o += ";AF=";
			for (uint64_t k = a0; k < a1; k++) {
				snprintf(num, sizeof num, "%.1f", an ? (double)c->ac[k] / an : 0.0);
				o += (k > a0 ? "," : "");
				o += num;
			}
			o += ";AN=" + std::to_string(an) + ";NS=" + std::to_string(c->ns[i]) + ";AT=";
			for (size_t k = 0; k < order.size(); k++) {
				if (k)
					o += ',';
				o.append(c->at + c->at_off[order[k]], c->at_off[order[k] + 1] - c->at_off[order[k]]);
			}
			const uint8_t f = c->flags[i];
			o += (f & POVU_HIP_CALL_INS) ? ";VARTYPE=INS" : (f & POVU_HIP_CALL_DEL) ? ";VARTYPE=DEL" : ";VARTYPE=SUB";
			o += (f & POVU_HIP_CALL_TANGLED) ? ";TANGLED=T" : ";TANGLED=F";
			o += ";ES=" + st.label[q] + ";LV=" + std::to_string((long)st.height[q] - 1) + "\tGT";
			const uint16_t *row = c->gt + i * S;
			for (uint32_t sm = 0; sm < samples.size(); sm++) {
				o += '\t';
				bool any = false;
				for (uint32_t sl = slot_first[sm]; sl < slot_first[sm + 1]; sl++)
					any |= row[sl] != POVU_HIP_GT_MISSING;
				if (!any) {
					o += '.';
					continue;
				}
				for (uint32_t sl = slot_first[sm]; sl < slot_first[sm + 1]; sl++) {
					if (sl > slot_first[sm])
						o += '|';
					o += row[sl] == POVU_HIP_GT_MISSING ? "." : std::to_string(row[sl]);
				}
			}
			o += '\n';
		}
	};
	std::vector<std::thread> th;
	for (int t = 1; t < T; t++)
		th.emplace_back(format, t);
	format(0);
	for (auto &x : th)
		x.join();

	// ---- the files: one VCF of every reference (--stdout), or <dir>/<prefix>.vcf per prefix with its references' records
	const std::string head = "##fileformat=VCFv4.2\n##fileDate=" + today() + "\n" + VCF_HEADER;
	std::string cols = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
	for (auto &sm : samples)
		cols += "\t" + sm;
	cols += "\n";
	auto write = [&](std::ostream &os, const std::string *only) {
		os << head;
		for (uint32_t r = 0; r < ref_path.size(); r++) {
			const std::string &nm = names[ref_path[r]];
			if (only && nm.compare(0, only->size(), *only))
				continue;
			os << "##contig=<ID=" << nm << ",length=" << c->contig_len[r] << ">\n";
		}
		os << cols;
		if (!only) {
			for (auto &x : chunk)
				os << x;
			return;
		}
		for (auto &x : chunk) { // (records of the prefix's references only: lines start with the path name)
			size_t at = 0;
			while (at < x.size()) {
				const size_t e = x.find('\n', at);
				const size_t tab = x.find('\t', at);
				const std::string nm = x.substr(at, tab - at);
				if (!nm.compare(0, only->size(), *only))
					os.write(x.data() + at, e + 1 - at);
				at = e + 1;
			}
		}
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
			write(os, &p);
		}
	}
	povu_hip_calls_free(c);
	povu_hip_destroy(ctx);
}

} // namespace povu_host
