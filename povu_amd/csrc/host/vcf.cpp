// vcf.cpp -- the host half of a variant call (INTEGRATION.md "Variant calls"), host only: path names to reference paths and
// PanSN slots, PVST vertices to sites, and the records of povu_hip_call to VCF text.  The one place that holds these rules
// for `povu call` and for povu_amd/hip.py alike; tests/vcf_ref.py restates them as the yardstick.
#include "../../../include/povu_hip.h"
#include "../hip/call_modes.hpp"
#include "../hip/cluster_rules.hpp"
#include "../hip/region_rules.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

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
// a nested call's own line ("Nested calls"), and the lines of the keys a profile appends (the reference fixture's texts)
const char *PS_LINE = "##INFO=<ID=PS,Number=1,Type=String,Description=\"ID of the enclosing record of the same reference path\">\n";
const char *PROFILE_LINES[] = {
	"",
	"##INFO=<ID=ORIGIN,Number=1,Type=String,Description=\"Raw record id\">\n"
	"##INFO=<ID=PROFILE,Number=1,Type=String,Description=\"Downstream profile name\">\n"
	"##INFO=<ID=PASSTHROUGH,Number=1,Type=String,Description=\"Record was kept without allele rewrite\">\n",
	"##INFO=<ID=ORIGIN,Number=1,Type=String,Description=\"Raw record id\">\n"
	"##INFO=<ID=PARENT,Number=1,Type=String,Description=\"Raw parent record id\">\n"
	"##INFO=<ID=PROFILE,Number=1,Type=String,Description=\"Downstream profile name\">\n"
	"##INFO=<ID=PASSTHROUGH,Number=1,Type=String,Description=\"Record was kept without allele rewrite\">\n"
	"##INFO=<ID=RESCUED_CHILD,Number=1,Type=String,Description=\"Child was kept because its parent was popped\">\n"
	"##INFO=<ID=POPPED_PARENT,Number=1,Type=String,Description=\"Popped parent id that enabled rescue\">\n",
	// "Left-normalised calls" (RAW_ALT_INDEX and RAW_ALT per ALT: a record here may have several)
	"##INFO=<ID=ORIGIN,Number=1,Type=String,Description=\"Raw record id\">\n"
	"##INFO=<ID=RAW_ALT_INDEX,Number=A,Type=Integer,Description=\"Raw ALT index\">\n"
	"##INFO=<ID=PROFILE,Number=1,Type=String,Description=\"Downstream profile name\">\n"
	"##INFO=<ID=LEFT_NORMALIZED,Number=1,Type=String,Description=\"Record was left-normalized\">\n"
	"##INFO=<ID=RAW_POS,Number=1,Type=Integer,Description=\"Raw POS before profile rewrite\">\n"
	"##INFO=<ID=RAW_REF,Number=1,Type=String,Description=\"Raw REF before profile rewrite\">\n"
	"##INFO=<ID=RAW_ALT,Number=A,Type=String,Description=\"Raw ALT before profile rewrite\">\n",
	// "Decomposed calls" (a row has one ALT)
	"##INFO=<ID=ORIGIN,Number=1,Type=String,Description=\"Raw record id\">\n"
	"##INFO=<ID=RAW_ALT_INDEX,Number=1,Type=Integer,Description=\"Raw ALT index\">\n"
	"##INFO=<ID=PROFILE,Number=1,Type=String,Description=\"Downstream profile name\">\n"
	"##INFO=<ID=DECOMPOSED,Number=1,Type=String,Description=\"Record came from allele decomposition\">\n"
	"##INFO=<ID=PASSTHROUGH,Number=1,Type=String,Description=\"Record was kept because policy forbids decomposition\">\n"
	"##INFO=<ID=PASS_THROUGH_REASON,Number=1,Type=String,Description=\"Reason pass-through was selected\">\n"
	"##INFO=<ID=RAW_POS,Number=1,Type=Integer,Description=\"Raw POS before profile rewrite\">\n"
	"##INFO=<ID=RAW_REF,Number=1,Type=String,Description=\"Raw REF before profile rewrite\">\n"
	"##INFO=<ID=RAW_ALT,Number=1,Type=String,Description=\"Raw ALT before profile rewrite\">\n"
	"##INFO=<ID=SUBR_ORIGIN,Number=1,Type=String,Description=\"Raw SUBR semantics were preserved\">\n",
};
// "Merged primitives": behind the lines of the decomposed profile when the merged rows are written
const char *MERGE_LINES = "##INFO=<ID=MERGED,Number=1,Type=Integer,Description=\"Rows of equal primitives merged into this record\">\n"
			  "##INFO=<ID=MERGED_FROM,Number=.,Type=String,Description=\"Decomposed ids of the merged rows\">\n";
const char *ROW_KIND_NAME[] = {"raw", "snp", "ins", "del", "passthrough"};
const char *ROW_REASON_NAME[] = {"", "max_allele_length", "contig_start", "empty_allele", "equals_ref", "subr_inversion_preservation"};

// (sample, hap) of a path name: `sample#hap#rest` with an all-digit hap, any other name a sample of its own with hap -1
std::pair<std::string, long long> pansn(const std::string &n)
{
	const size_t a = n.find('#');
	if (a != std::string::npos) {
		const size_t b = n.find('#', a + 1);
		if (b != std::string::npos && b > a + 1 && std::all_of(n.begin() + a + 1, n.begin() + b, [](char ch) { return ch >= '0' && ch <= '9'; }))
			return {n.substr(0, a), strtoll(n.c_str() + a + 1, nullptr, 10)};
	}
	return {n, -1};
}

void set_err(char *err, size_t n, const std::string &m)
{
	if (err && n)
		snprintf(err, n, "%s", m.c_str());
}

struct Names {
	povu_hip_call_names pub; // (first: the handle points at it)
	std::vector<uint32_t> ref_path, sample_of_slot, slot_of_path;
	std::vector<std::string> sample;
	std::vector<const char *> sample_ptr;
	std::vector<int64_t> slot_hap;
};

template <class T> bool grow(const T *&p, size_t n)
{
	void *q = realloc(const_cast<T *>(p), (n + 1) * sizeof(T));
	if (q)
		p = static_cast<const T *>(q);
	return q != nullptr;
}

} // namespace

// `name:start-end` to a region of the path named exactly so (INTEGRATION.md "Region calls"; the reading: region_rules.hpp)
extern "C" int povu_hip_region_parse(const char *text, uint32_t n_paths, const char *const *names, povu_hip_region *out, char *err, size_t errlen)
try {
	if (!text || !out || (n_paths && !names)) {
		set_err(err, errlen, "region: bad arguments");
		return 1;
	}
	std::string name;
	uint64_t s = 0, e = 0;
	const std::string bad = region::parse(text, name, s, e);
	if (!bad.empty()) {
		set_err(err, errlen, bad);
		return 1;
	}
	for (uint32_t k = 0; k < n_paths; k++)
		if (names[k] && name == names[k]) {
			*out = povu_hip_region{k, 0, s, e};
			return 0;
		}
	set_err(err, errlen, "region '" + std::string(text) + "': no path is named " + name);
	return 1;
} catch (const std::exception &x) {
	set_err(err, errlen, std::string("region: ") + x.what());
	return 1;
}

// the threshold of "Clustered calls" (the reading: cluster_rules.hpp)
extern "C" int povu_hip_cluster_parse(const char *text, uint32_t *ppm, char *err, size_t errlen)
try {
	if (!text || !ppm) {
		set_err(err, errlen, "cluster threshold: bad arguments");
		return 1;
	}
	const std::string bad = cluster::parse(text, ppm);
	if (!bad.empty()) {
		set_err(err, errlen, bad);
		return 1;
	}
	return 0;
} catch (const std::exception &x) {
	set_err(err, errlen, std::string("cluster threshold: ") + x.what());
	return 1;
}

// need_ref: a call's names (no reference path is refused); else the samples and slots alone ("VCF checks")
static povu_hip_call_names *names_make(uint32_t n_paths, const char *const *path_name, uint32_t n_prefixes, const char *const *prefix,
				       bool need_ref, char *err, size_t errlen)
try {
	if ((n_paths && !path_name) || (n_prefixes && !prefix)) {
		set_err(err, errlen, "call names: bad arguments");
		return nullptr;
	}
	std::unique_ptr<Names> nm(new Names);
	std::map<std::string, std::vector<long long>> haps;
	std::vector<std::pair<std::string, long long>> key(n_paths);
	for (uint32_t k = 0; k < n_paths; k++) {
		const std::string name = path_name[k];
		for (uint32_t p = 0; p < n_prefixes; p++)
			if (!name.compare(0, strlen(prefix[p]), prefix[p])) {
				nm->ref_path.push_back(k);
				break;
			}
		key[k] = pansn(name);
		if (!haps.count(key[k].first))
			nm->sample.push_back(key[k].first);
		auto &hv = haps[key[k].first];
		if (std::find(hv.begin(), hv.end(), key[k].second) == hv.end())
			hv.push_back(key[k].second);
	}
	if (need_ref && nm->ref_path.empty()) {
		std::string l;
		for (uint32_t p = 0; p < n_prefixes; p++)
			l += std::string(l.empty() ? "" : ", ") + prefix[p];
		set_err(err, errlen, "no path name starts with any of the reference prefixes " + l);
		return nullptr;
	}
	std::map<std::pair<std::string, long long>, uint32_t> slot_id;
	for (uint32_t si = 0; si < nm->sample.size(); si++) {
		auto &hv = haps[nm->sample[si]];
		std::sort(hv.begin(), hv.end());
		for (long long h : hv) {
			slot_id[{nm->sample[si], h}] = (uint32_t)nm->sample_of_slot.size();
			nm->sample_of_slot.push_back(si);
			nm->slot_hap.push_back(h);
		}
		nm->sample_ptr.push_back(nm->sample[si].c_str());
	}
	for (uint32_t k = 0; k < n_paths; k++)
		nm->slot_of_path.push_back(slot_id[key[k]]);
	nm->pub = {{(uint32_t)nm->ref_path.size(), nm->ref_path.data(), (uint32_t)nm->sample_of_slot.size(), (uint32_t)nm->sample.size(),
		    nm->sample_of_slot.data()},
		   n_paths, nm->slot_of_path.data(), nm->sample_ptr.data(), nm->slot_hap.data()};
	return &nm.release()->pub;
} catch (const std::bad_alloc &) {
	set_err(err, errlen, "call names: out of memory");
	return nullptr;
}

extern "C" povu_hip_call_names *povu_hip_call_names_make(uint32_t n_paths, const char *const *path_name, uint32_t n_prefixes,
							 const char *const *prefix, char *err, size_t errlen)
{
	return names_make(n_paths, path_name, n_prefixes, prefix, true, err, errlen);
}

extern "C" povu_hip_call_names *povu_hip_vcf_names_make(uint32_t n_paths, const char *const *path_name, char *err, size_t errlen)
{
	return names_make(n_paths, path_name, 0, nullptr, false, err, errlen);
}

extern "C" void povu_hip_call_names_free(povu_hip_call_names *n) { delete reinterpret_cast<Names *>(n); }

extern "C" int povu_hip_sites_add_tree(povu_hip_sites *s, uint32_t tree, uint32_t n, const uint32_t *id1, const uint32_t *id2,
				       const uint8_t *or1, const uint8_t *or2, const uint32_t *parent, const uint8_t *family)
try {
	if (!s || (n && (!id1 || !id2 || !or1 || !or2 || !parent)) || (uint64_t)s->n + n >= POVU_HIP_NIL)
		return 1;
	auto root = [&](uint32_t v) { return family ? family[v] == 'D' : v == 0; };
	auto up = [&](uint32_t v) { return root(v) || parent[v] >= n ? POVU_HIP_NIL : parent[v]; };
	// heights without recursion, whatever the order of the vertices: walk up to the first vertex seen before, number the
	// chain on the way back (a vertex on a cycle of parent pointers counts as seen with height 0: the walk ends)
	std::vector<uint32_t> qnum(n, POVU_HIP_NIL), height(n, 0), chain;
	std::vector<char> seen(n, 0);
	uint32_t m = s->n;
	for (uint32_t v = 0; v < n; v++) {
		if (!root(v))
			qnum[v] = m++;
		for (uint32_t u = v; u != POVU_HIP_NIL && !seen[u]; u = up(u)) {
			seen[u] = 1;
			chain.push_back(u);
		}
		for (; !chain.empty(); chain.pop_back())
			height[chain.back()] = up(chain.back()) == POVU_HIP_NIL ? 0 : height[up(chain.back())] + 1;
	}
	if (!grow(s->id1, m) || !grow(s->id2, m) || !grow(s->or1, m) || !grow(s->or2, m) || !grow(s->parent, m) || !grow(s->height, m) ||
	    !grow(s->family, m) || !grow(s->tree, m))
		return 1;
	for (uint32_t v = 0; v < n; v++) {
		const uint32_t q = qnum[v];
		if (q == POVU_HIP_NIL)
			continue;
		const_cast<uint32_t *>(s->id1)[q] = id1[v];
		const_cast<uint32_t *>(s->id2)[q] = id2[v];
		const_cast<uint8_t *>(s->or1)[q] = or1[v];
		const_cast<uint8_t *>(s->or2)[q] = or2[v];
		const_cast<uint32_t *>(s->parent)[q] = up(v) == POVU_HIP_NIL ? POVU_HIP_NIL : qnum[up(v)];
		const_cast<uint32_t *>(s->height)[q] = height[v];
		const_cast<uint8_t *>(s->family)[q] = family ? family[v] : (uint8_t)'F';
		const_cast<uint32_t *>(s->tree)[q] = tree;
	}
	s->n = m;
	return 0;
} catch (const std::bad_alloc &) {
	return 1;
}

extern "C" povu_hip_sites *povu_hip_sites_of_docs(const povu_pvst_doc *const *docs, uint32_t n)
{
	auto *s = static_cast<povu_hip_sites *>(calloc(1, sizeof(povu_hip_sites)));
	for (uint32_t k = 0; s && k < n; k++) {
		const povu_pvst_doc *d = docs[k];
		if (!d || povu_hip_sites_add_tree(s, k, d->n, d->a_id, d->z_id, d->a_or, d->z_or, d->parent, (const uint8_t *)d->type)) {
			povu_hip_sites_free(s);
			s = nullptr;
		}
	}
	return s;
}

extern "C" void povu_hip_sites_free(povu_hip_sites *s)
{
	if (!s)
		return;
	for (const void *p : {(const void *)s->id1, (const void *)s->id2, (const void *)s->or1, (const void *)s->or2, (const void *)s->parent,
			      (const void *)s->height, (const void *)s->family, (const void *)s->tree})
		free(const_cast<void *>(p));
	free(s);
}

namespace
{
// the lines of "Off-reference calls", behind the header of a call made with POVU_HIP_T_OFFREF
const char OFFREF_LINES[] =
	"##INFO=<ID=OFFREF,Number=0,Type=Flag,Description=\"Called off the reference paths: CHROM is the surrogate path, the first path that "
	"traverses the site\">\n"
	"##INFO=<ID=HOST,Number=1,Type=String,Description=\"ID of the tightest site called on the reference paths that encloses the record on "
	"its path\">\n"
	"##INFO=<ID=HA,Number=1,Type=Integer,Description=\"Allele of the record's path in HOST, numbered in traversal order\">\n";

// the lines of "Untangled calls", behind those of a call made with POVU_HIP_T_UNTANGLE
const char UNTANGLE_LINES[] =
	"##INFO=<ID=LN,Number=1,Type=Integer,Description=\"Lap of the reference path through the site this record is, from 1\">\n"
	"##INFO=<ID=LC,Number=1,Type=Integer,Description=\"Laps of the reference path through the site\">\n"
	"##FORMAT=<ID=CN,Number=.,Type=Integer,Description=\"Laps of the sample's haplotypes through the site\">\n";

// the lines of "Clustered calls", behind those of a call made with a threshold (and one line that states it)
const char CLUSTER_LINES[] =
	"##INFO=<ID=NX,Number=R,Type=Integer,Description=\"Exact alleles of the site behind every written allele, the cluster of REF first\">\n"
	"##INFO=<ID=MINSIM,Number=1,Type=Integer,Description=\"Lowest similarity, in parts per million, of an exact allele of the site to the "
	"representative of its cluster\">\n";

// what a writer is asked for
struct VcfRequest {
	const povu_hip_calls *c;
	const povu_hip_sites *sites;
	const povu_hip_call_names *names;
	const char *const *path_name;
	const char *date; // (NULL: today)
	// the paths whose lines and records are written: those of only_prefix (NULL: every one), or with `rest` those of no prefix
	const char *only_prefix;
	const char *const *rest_prefix;
	uint32_t n_rest;
	bool rest;
	uint32_t threads, profile;
	bool nested_fields; // false: the entry of before, which reads nothing of `c` behind n_inv_tier2
};

// which array groups of the calls are read, and the counts the text is made with: the one place that looks at nested_fields
// and at the optional pointers
struct VcfShape {
	bool level, parent_query, ref_spelled; // the fields of "Nested calls", each absent for the entry of before or where a hand-made record leaves it out
	bool nested;			       // PS is written
	bool normalized;		       // the fields of "Left-normalised calls", under that profile alone (absent: no record was changed)
	bool rows;			       // the rows of "Decomposed calls", under that profile alone (absent: the raw records are written)
	bool merged;			       // the merged rows of "Merged primitives", written instead of the rows when they are there
	bool merged_lines;		       // (a call with the flag and no row has no array to show for it: the header still names the fields)
	bool offref;			       // the arrays of "Off-reference calls" (`offref` speaks for a call without a record)
	bool untangled;			       // the arrays of "Untangled calls" (`untangled` speaks for a call without a record)
	bool clustered;			       // the arrays of "Clustered calls" (one left out: no record says NX or MINSIM)
	uint64_t cluster_ppm;		       // 0: the text of the call without a threshold
	bool star;			       // rec_star of "Spanning alleles" (absent: no record has a `*` ALT)
	uint64_t n;			       // rows of text: merged rows, rows or records
	uint32_t S, P, n_samples;
	std::vector<uint32_t> slot_first; // (the slots of a sample are consecutive)
};

// false: the request or an index of the calls is out of bounds
bool calls_shape(const VcfRequest &rq, VcfShape &sh)
{
	const povu_hip_calls *c = rq.c;
	const povu_hip_sites *sites = rq.sites;
	const povu_hip_call_names *names = rq.names;
	const uint32_t profile = rq.profile;
	const bool nested_fields = rq.nested_fields;
	if (!c || !sites || !names || !rq.path_name || c->n_slots != names->refs.n_slots || c->n_refs != names->refs.n_refs ||
	    profile > POVU_HIP_PROFILE_DECOMPOSED)
		return false;
	const uint32_t *parent_query = nested_fields ? c->parent_query : nullptr;
	const uint64_t *ref_spelled = nested_fields ? c->ref_spelled : nullptr;
	sh.level = nested_fields && c->level;
	sh.parent_query = parent_query, sh.ref_spelled = ref_spelled;
	sh.nested = nested_fields && c->nested;
	sh.normalized = nested_fields && profile == POVU_HIP_PROFILE_LEFT_NORMALIZED && c->raw_pos && c->norm_block;
	sh.rows = nested_fields && profile == POVU_HIP_PROFILE_DECOMPOSED && c->row_record && c->row_alt && c->row_kind && c->row_reason &&
		  c->row_index && c->row_pos && c->row_ref_start && c->row_ref_len && c->row_alt_start && c->row_alt_len && c->row_lead && c->row_ac &&
		  c->row_an && c->row_ns;
	sh.merged = sh.rows && c->mrow_off;
	sh.merged_lines = sh.merged || (nested_fields && profile == POVU_HIP_PROFILE_DECOMPOSED && c->merged && !c->n_rows);
	sh.offref = nested_fields && (c->rec_offref || c->offref);
	if (sh.offref && ((c->n_records && (!c->rec_offref || !c->host_query || !c->host_allele)) ||
			  (c->n_off_contigs && (!c->off_contig_path || !c->off_contig_len))))
		return false;
	sh.untangled = nested_fields && (c->rec_unt || c->untangled);
	if (sh.untangled && c->n_records && (!c->rec_unt || !c->lap || !c->n_laps || !c->lap_count))
		return false;
	sh.cluster_ppm = nested_fields ? c->cluster_ppm : 0;
	if (sh.cluster_ppm > cluster::PPM)
		return false;
	sh.clustered = sh.cluster_ppm && c->rec_clustered && c->cl_minsim && c->cl_nx;
	sh.star = nested_fields && c->rec_star;
	if (sh.merged && (!c->mrow_member || !c->mrow_gt || !c->mrow_ac || !c->mrow_an || !c->mrow_ns))
		return false;
	const uint64_t n_records = c->n_records, n = sh.merged ? c->n_mrows : sh.rows ? c->n_rows : n_records;
	sh.n = n, sh.S = c->n_slots, sh.P = names->n_paths, sh.n_samples = names->refs.n_samples;
	for (uint64_t i = 0; i < n_records; i++) {
		const bool subr = c->flags[i] & POVU_HIP_CALL_SUBR; // (its query is POVU_HIP_NIL: it belongs to no site)
		if ((!subr && c->query[i] >= sites->n) || c->path[i] >= sh.P || (subr && (c->n_alleles[i] != 2 || c->ref_allele[i] != 0)))
			return false;
		if (parent_query && parent_query[i] != POVU_HIP_NIL && parent_query[i] >= sites->n)
			return false;
		if (ref_spelled && ref_spelled[i] >= c->n_spelled)
			return false;
		if (sh.offref && c->host_query[i] != POVU_HIP_NIL && c->host_query[i] >= sites->n)
			return false;
		// a `*` ALT is the last of at least three alleles (REF, an ALT of the site, `*`), has an AC entry and no spelled
		// allele; never on an inversion record, and no profile rewrites such a record
		if (sh.star && c->rec_star[i] &&
		    (subr || c->n_alleles[i] < 3 || c->ref_allele[i] >= c->n_alleles[i] - 1 || c->ac_off[i + 1] - c->ac_off[i] != c->n_alleles[i] - 1 ||
		     sh.rows || sh.normalized))
			return false;
		if (sh.normalized && (c->flags[i] & POVU_HIP_CALL_NORMALIZED) &&
		    (subr || c->norm_block[i] >= c->n_blocks || c->block_off[c->norm_block[i]] + c->n_alleles[i] > c->n_spelled))
			return false;
	}
	for (uint64_t k = 0; sh.rows && k < c->n_rows; k++) {
		const uint64_t i = c->row_record[k];
		if (i >= n_records || !c->row_alt[k] || c->row_alt[k] >= c->n_alleles[i] || c->row_kind[k] > POVU_HIP_ROW_PASS ||
		    c->row_reason[k] > POVU_HIP_REASON_SUBR)
			return false;
		// its stretches lie inside the record's REF and that ALT
		const uint32_t ra = c->ref_allele[i], a = c->row_alt[k] - 1 < ra ? c->row_alt[k] - 1 : c->row_alt[k];
		const uint64_t sr = ref_spelled ? ref_spelled[i] : c->block_off[c->block[i]] + ra, sa = c->block_off[c->block[i]] + a;
		if (sa >= c->n_spelled || (uint64_t)c->row_ref_start[k] + c->row_ref_len[k] > c->seq_off[sr + 1] - c->seq_off[sr] ||
		    (uint64_t)c->row_alt_start[k] + c->row_alt_len[k] > c->seq_off[sa + 1] - c->seq_off[sa])
			return false;
	}
	// every merged row has members, all of them rows, and together they are the rows
	if (sh.merged && (c->mrow_off[0] != 0 || c->mrow_off[n] != c->n_rows))
		return false;
	for (uint64_t g = 0; sh.merged && g < n; g++)
		if (c->mrow_off[g] >= c->mrow_off[g + 1] || c->mrow_off[g + 1] > c->n_rows)
			return false;
	for (uint64_t k = 0; sh.merged && k < c->n_rows; k++)
		if (c->mrow_member[k] >= c->n_rows)
			return false;
	sh.slot_first.assign(sh.n_samples + 1, 0);
	for (uint32_t sl = 0; sl < sh.S; sl++) {
		if (names->refs.sample_of_slot[sl] >= sh.n_samples)
			return false;
		sh.slot_first[names->refs.sample_of_slot[sl] + 1] = sl + 1;
	}
	// the paths that give a contig line: the reference paths, and the surrogates that are none
	for (uint32_t r = 0; r < names->refs.n_refs; r++)
		if (names->refs.ref_path[r] >= sh.P)
			return false;
	for (uint64_t k = 0; sh.offref && k < c->n_off_contigs; k++)
		if (c->off_contig_path[k] >= sh.P)
			return false;
	return true;
}

bool takes(const VcfRequest &rq, const char *name)
{
	if (!rq.rest)
		return !rq.only_prefix || !strncmp(name, rq.only_prefix, strlen(rq.only_prefix));
	for (uint32_t k = 0; k < rq.n_rest; k++)
		if (!strncmp(name, rq.rest_prefix[k], strlen(rq.rest_prefix[k])))
			return false;
	return true;
}

// fixed lines, the blocks of the modes, a contig line per path that is taken (`keep` marks it), the column line
std::string vcf_header(const VcfRequest &rq, const VcfShape &sh, std::vector<char> &keep)
{
	const povu_hip_calls *c = rq.c;
	char today[16];
	const char *date = rq.date;
	if (!date) {
		const time_t t = time(nullptr);
		struct tm tmv;
		localtime_r(&t, &tmv);
		strftime(today, sizeof today, "%Y%m%d", &tmv);
		date = today;
	}
	std::string head = std::string("##fileformat=VCFv4.2\n##fileDate=") + date + "\n" + VCF_HEADER + (sh.nested ? PS_LINE : "") + PROFILE_LINES[rq.profile] +
			   (sh.merged_lines ? MERGE_LINES : "") + (sh.offref ? OFFREF_LINES : "") + (sh.untangled ? UNTANGLE_LINES : "");
	if (sh.cluster_ppm) {
		char f[64];
		snprintf(f, sizeof f, "##povu_call_cluster=%u.%06u\n", (unsigned)(sh.cluster_ppm / cluster::PPM), (unsigned)(sh.cluster_ppm % cluster::PPM));
		head += std::string(CLUSTER_LINES) + f;
	}
	auto contig = [&](uint32_t p, uint64_t length) {
		if (!takes(rq, rq.path_name[p]))
			return;
		keep[p] = 1;
		head += std::string("##contig=<ID=") + rq.path_name[p] + ",length=" + std::to_string(length) + ">\n";
	};
	for (uint32_t r = 0; r < rq.names->refs.n_refs; r++)
		contig(rq.names->refs.ref_path[r], c->contig_len[r]);
	for (uint64_t k = 0; sh.offref && k < c->n_off_contigs; k++)
		contig(c->off_contig_path[k], c->off_contig_len[k]);
	head += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
	for (uint32_t sm = 0; sm < sh.n_samples; sm++)
		head += std::string("\t") + rq.names->sample[sm];
	head += "\n";
	return head;
}

std::string site_label(const povu_hip_sites *sites, uint32_t q)
{
	return (sites->or1[q] ? "<" : ">") + std::to_string(sites->id1[q]) + (sites->or2[q] ? "<" : ">") + std::to_string(sites->id2[q]);
}
// the kind of a row as a primitive: a _ROW_RAW row is the one primitive of its record
uint32_t primitive_kind(const povu_hip_calls *c, uint64_t y)
{
	if (c->row_kind[y] != POVU_HIP_ROW_RAW)
		return c->row_kind[y];
	return !c->row_ref_len[y] ? POVU_HIP_ROW_INS : !c->row_alt_len[y] ? POVU_HIP_ROW_DEL : POVU_HIP_ROW_SNP;
}
const char *vartype(uint8_t f)
{
	return (f & POVU_HIP_CALL_SUBR) ? ";VARTYPE=SUBR" : (f & POVU_HIP_CALL_INS) ? ";VARTYPE=INS" : (f & POVU_HIP_CALL_DEL) ? ";VARTYPE=DEL" : ";VARTYPE=SUB";
}

// one row of the text and what both kinds of row are made of
struct Row {
	uint64_t mrow, at, members, i; // the row, the row that is written (a merged row's representative), its members, its record
	// a row of "Decomposed calls" that is no raw record: one ALT, its own POS, texts and counts, the GT row projected (a merged
	// row of two or more is none even when its representative is one)
	bool prim;
	bool subr;
	bool star; // its last ALT is `*`: no spelled allele, nothing of `seq` / `at` is read for it
	std::vector<uint64_t> order; // its spelled alleles: REF first, the others in the query's allele order
	std::string label;	     // its ID: the site, or the ends of an inversion
};
// false: the row's path is not written
bool row_of(const VcfRequest &rq, const VcfShape &sh, const std::vector<char> &keep, uint64_t mrow, Row &r)
{
	const povu_hip_calls *c = rq.c;
	r.mrow = mrow;
	r.at = sh.merged ? c->mrow_member[c->mrow_off[mrow]] : mrow;
	r.members = sh.merged ? c->mrow_off[mrow + 1] - c->mrow_off[mrow] : 1;
	const uint64_t i = r.i = sh.rows ? c->row_record[r.at] : r.at;
	if (!keep[c->path[i]])
		return false;
	r.prim = sh.rows && (c->row_kind[r.at] != POVU_HIP_ROW_RAW || r.members > 1);
	r.star = sh.star && c->rec_star[i];
	const uint32_t na = c->n_alleles[i] - (r.star ? 1u : 0u), ra = c->ref_allele[i]; // (the alleles the block spells)
	const uint64_t b = c->block_off[c->block[i]];
	r.order.clear();
	r.order.push_back(sh.ref_spelled ? c->ref_spelled[i] : b + ra);
	for (uint32_t a = 0; a < na; a++)
		if (a != ra)
			r.order.push_back(b + a);
	r.subr = c->flags[i] & POVU_HIP_CALL_SUBR;
	if (!r.subr) {
		r.label = site_label(rq.sites, c->query[i]);
		return true;
	}
	// the first and the last step of the REF AT string, both written '>' when both are '<'
	const char *at = c->at + c->at_off[b], *end = c->at + c->at_off[b + 1], *last = end;
	while (last > at && last[-1] != '<' && last[-1] != '>')
		last--;
	const char *first_end = at == end ? at : at + 1;
	while (first_end < end && *first_end != '<' && *first_end != '>')
		first_end++;
	r.label.assign(at, first_end);
	if (last > at)
		r.label.append(last - 1, end);
	if (at < end && *at == '<' && last > at && last[-1] == '<')
		r.label[0] = r.label[first_end - at] = '>';
	return true;
}

// a number of a sample column (nearly always one digit)
void put_number(std::string &o, uint32_t v)
{
	if (v < 10)
		o += (char)('0' + v);
	else
		o += std::to_string(v);
}
// the sample columns: the values of a sample's slots joined by '|', one '.' where no slot has a value.  value(slot): what is
// written for it, POVU_HIP_GT_MISSING for '.'.  laps (NULL: none): behind a ':' the laps of the sample's slots, '.' for none
template <class Value> void genotype_columns(const VcfShape &sh, Value &&value, const uint16_t *laps, std::string &o)
{
	for (uint32_t sm = 0; sm < sh.n_samples; sm++) {
		const uint32_t s0 = sh.slot_first[sm], s1 = sh.slot_first[sm + 1];
		o += '\t';
		bool any = false;
		for (uint32_t sl = s0; sl < s1; sl++)
			any |= value(sl) != POVU_HIP_GT_MISSING;
		if (!any)
			o += '.';
		for (uint32_t sl = s0; any && sl < s1; sl++) {
			if (sl > s0)
				o += '|';
			if (value(sl) == POVU_HIP_GT_MISSING)
				o += '.';
			else
				put_number(o, value(sl));
		}
		for (uint32_t sl = s0; laps && sl < s1; sl++) {
			o += sl > s0 ? ',' : ':';
			if (!laps[sl])
				o += '.';
			else
				put_number(o, laps[sl]);
		}
	}
	o += '\n';
}
// a slot of a merged row: 0, 1 or none
uint32_t merged_value(uint8_t v) { return v <= 1 ? v : POVU_HIP_GT_MISSING; }

void primitive_row(const VcfRequest &rq, const VcfShape &sh, const Row &r, std::string &o)
{
	const povu_hip_calls *c = rq.c;
	const uint64_t at = r.at, i = r.i, mrow = r.mrow;
	const bool merged = sh.merged, subr = r.subr;
	const std::string &label = r.label;
	const uint8_t f = c->flags[i];
	char num[32];
	const uint32_t k = c->row_alt[at], kind = primitive_kind(c, at);
	const uint32_t index = c->row_kind[at] == POVU_HIP_ROW_RAW ? 1 : c->row_index[at];
	const bool passed = kind == POVU_HIP_ROW_PASS;
	const uint64_t sr = r.order[0], sa = r.order[k];
	const char lead = (char)c->row_lead[at];
	o += rq.path_name[c->path[i]];
	o += '\t';
	o += std::to_string(c->row_pos[at]);
	o += '\t';
	o += label;
	if (subr)
		o += ":subr-passthrough";
	else
		o += ":" + std::to_string(k) + ":" + ROW_KIND_NAME[kind] + (passed ? std::string() : std::to_string(index));
	o += '\t';
	if (lead)
		o += lead;
	o.append(c->seq + c->seq_off[sr] + c->row_ref_start[at], c->row_ref_len[at]);
	o += '\t';
	if (lead)
		o += lead;
	o.append(c->seq + c->seq_off[sa] + c->row_alt_start[at], c->row_alt_len[at]);
	const uint32_t ac = merged ? c->mrow_ac[mrow] : c->row_ac[at], an = merged ? c->mrow_an[mrow] : c->row_an[at];
	snprintf(num, sizeof num, "%.1f", an ? (double)ac / an : 0.0);
	o += "\t60\tPASS\tAC=" + std::to_string(ac) + ";AF=" + num + ";AN=" + std::to_string(an) +
	     ";NS=" + std::to_string(merged ? c->mrow_ns[mrow] : c->row_ns[at]) + ";AT=";
	o.append(c->at + c->at_off[sr], c->at_off[sr + 1] - c->at_off[sr]);
	o += ',';
	o.append(c->at + c->at_off[sa], c->at_off[sa + 1] - c->at_off[sa]);
	if (passed)
		o += vartype(f);
	else
		o += kind == POVU_HIP_ROW_SNP ? ";VARTYPE=SUB" : kind == POVU_HIP_ROW_INS ? ";VARTYPE=INS" : ";VARTYPE=DEL";
	o += passed && (f & POVU_HIP_CALL_TANGLED) ? ";TANGLED=T" : ";TANGLED=F";
	o += ";ORIGIN=" + label + ";RAW_ALT_INDEX=" + std::to_string(k) + ";PROFILE=decomposed;";
	o += passed ? std::string("PASSTHROUGH=T;PASS_THROUGH_REASON=") + ROW_REASON_NAME[c->row_reason[at]] : std::string("DECOMPOSED=T");
	if (r.members > 1) { // the members' decomposed IDs, the representative's first
		o += ";MERGED=" + std::to_string(r.members) + ";MERGED_FROM=";
		for (uint64_t m = c->mrow_off[mrow]; m < c->mrow_off[mrow + 1]; m++) {
			const uint64_t y = c->mrow_member[m], iy = c->row_record[y];
			const bool raw = c->row_kind[y] == POVU_HIP_ROW_RAW;
			if (m > c->mrow_off[mrow])
				o += ',';
			o += ((c->flags[iy] & POVU_HIP_CALL_SUBR) ? label : site_label(rq.sites, c->query[iy])) + ":" + std::to_string(c->row_alt[y]) + ":" +
			     ROW_KIND_NAME[primitive_kind(c, y)] + std::to_string(raw ? 1 : c->row_index[y]);
		}
	}
	if (subr) {
		o += ";SUBR_ORIGIN=T";
	} else {
		o += ";RAW_POS=" + std::to_string(c->pos[i]) + ";RAW_REF=";
		o.append(c->seq + c->seq_off[sr], c->seq_off[sr + 1] - c->seq_off[sr]);
		o += ";RAW_ALT=";
		o.append(c->seq + c->seq_off[sa], c->seq_off[sa + 1] - c->seq_off[sa]);
	}
	o += "\tGT";
	// the merged row's value, else the record's projected on the ALT
	const uint16_t *gt = c->gt + i * sh.S;
	const uint8_t *mgt = merged ? c->mrow_gt + mrow * sh.S : nullptr;
	genotype_columns(sh, [&](uint32_t sl) -> uint32_t { return mgt ? merged_value(mgt[sl]) : gt[sl] == 0 ? 0u : gt[sl] == k ? 1u : POVU_HIP_GT_MISSING; },
			 nullptr, o);
}

void record_row(const VcfRequest &rq, const VcfShape &sh, const Row &r, std::string &o)
{
	const povu_hip_calls *c = rq.c;
	const uint64_t i = r.i, mrow = r.mrow;
	const uint32_t profile = rq.profile, q = c->query[i], na = c->n_alleles[i];
	const bool merged = sh.merged, subr = r.subr;
	const std::vector<uint64_t> &order = r.order;
	const std::string &label = r.label;
	const uint8_t f = c->flags[i];
	char num[32];
	const bool has_parent = !subr && sh.parent_query && c->parent_query[i] != POVU_HIP_NIL;
	const std::string parent = has_parent ? site_label(rq.sites, c->parent_query[i]) : std::string(".");
	const bool rescued = !subr && profile == POVU_HIP_PROFILE_POPPED && (f & POVU_HIP_CALL_RESCUED);
	const bool norm = sh.normalized && (f & POVU_HIP_CALL_NORMALIZED);
	const uint64_t nbase = norm ? c->block_off[c->norm_block[i]] : 0; // (its alleles in written order)
	o += rq.path_name[c->path[i]];
	o += '\t';
	o += std::to_string(c->pos[i]);
	o += '\t';
	o += label;
	if (!subr && profile == POVU_HIP_PROFILE_TOP_LEVEL_ONLY)
		o += ":top";
	if (rescued)
		o += ":rescued";
	if (norm)
		o += ":norm";
	for (size_t k = 0; k < order.size(); k++) {
		const uint64_t sa = norm ? nbase + k : order[k];
		o += k <= 1 ? '\t' : ',';
		o.append(c->seq + c->seq_off[sa], c->seq_off[sa + 1] - c->seq_off[sa]);
	}
	if (r.star)
		o += ",*";
	o += "\t60\tPASS\tAC=";
	// (a _ROW_RAW row of a merged call: its record has one ALT, the counts and the GT are the merged row's)
	const uint64_t a0 = c->ac_off[i], a1 = c->ac_off[i + 1];
	const uint32_t an = merged ? c->mrow_an[mrow] : c->an[i];
	auto ac_of = [&](uint64_t k) { return merged ? c->mrow_ac[mrow] : c->ac[k]; };
	for (uint64_t k = a0; k < a1; k++)
		o += (k > a0 ? "," : "") + std::to_string(ac_of(k));
	o += ";AF=";
	for (uint64_t k = a0; k < a1; k++) {
		snprintf(num, sizeof num, "%.1f", an ? (double)ac_of(k) / an : 0.0);
		o += (k > a0 ? "," : "");
		o += num;
	}
	o += ";AN=" + std::to_string(an) + ";NS=" + std::to_string(merged ? c->mrow_ns[mrow] : c->ns[i]) + ";AT=";
	for (size_t k = 0; k < order.size(); k++) {
		if (k)
			o += ',';
		o.append(c->at + c->at_off[order[k]], c->at_off[order[k] + 1] - c->at_off[order[k]]);
	}
	if (r.star)
		o += ",*";
	o += vartype(f);
	o += (f & POVU_HIP_CALL_TANGLED) ? ";TANGLED=T" : ";TANGLED=F";
	if (!subr) {
		o += ";ES=" + label + ";LV=" + std::to_string(sh.level ? (long)(int32_t)c->level[i] : (long)rq.sites->height[q] - 1);
		if (sh.nested && has_parent)
			o += ";PS=" + parent;
		if (sh.clustered && c->rec_clustered[i]) {
			const uint32_t *nx = c->cl_nx + c->ac_off[i] + i;
			for (uint32_t k = 0; k < na; k++)
				o += (k ? "," : ";NX=") + std::to_string(nx[k]);
			o += ";MINSIM=" + std::to_string(c->cl_minsim[i]);
		}
		if (sh.offref && c->rec_offref[i]) {
			o += ";OFFREF=T";
			if (c->host_query[i] != POVU_HIP_NIL)
				o += ";HOST=" + site_label(rq.sites, c->host_query[i]) + ";HA=" + std::to_string(c->host_allele[i]);
		}
		if (sh.untangled && c->rec_unt[i])
			o += ";LN=" + std::to_string(c->lap[i]) + ";LC=" + std::to_string(c->n_laps[i]);
		if (norm) {
			o += ";ORIGIN=" + label + ";RAW_ALT_INDEX=";
			for (size_t k = 1; k < order.size(); k++)
				o += (k > 1 ? "," : "") + std::to_string(k);
			o += ";PROFILE=left-normalized;LEFT_NORMALIZED=T;RAW_POS=" + std::to_string(c->raw_pos[i]);
			for (size_t k = 0; k < order.size(); k++) {
				o += k == 0 ? ";RAW_REF=" : k == 1 ? ";RAW_ALT=" : ",";
				o.append(c->seq + c->seq_off[order[k]], c->seq_off[order[k] + 1] - c->seq_off[order[k]]);
			}
		} else if (profile == POVU_HIP_PROFILE_TOP_LEVEL_ONLY || profile == POVU_HIP_PROFILE_POPPED) {
			o += ";ORIGIN=" + label + (rescued ? ";PARENT=" + parent : std::string()) + ";PROFILE=" + modes::PROFILE_NAME[profile] +
			     (rescued ? ";RESCUED_CHILD=T;POPPED_PARENT=" + parent : std::string(";PASSTHROUGH=T"));
		}
	}
	// an untangled record: every sample column is <GT>:<CN>, CN the laps of the sample's slots
	const bool with_cn = sh.untangled && !subr && c->rec_unt[i];
	o += with_cn ? "\tGT:CN" : "\tGT";
	const uint16_t *gt = c->gt + i * sh.S;
	const uint8_t *mgt = merged ? c->mrow_gt + mrow * sh.S : nullptr;
	genotype_columns(sh, [&](uint32_t sl) -> uint32_t { return mgt ? merged_value(mgt[sl]) : gt[sl]; }, with_cn ? c->lap_count + i * sh.S : nullptr, o);
}

char *calls_vcf(const VcfRequest &rq, size_t *len)
try {
	VcfShape sh;
	if (!len || !calls_shape(rq, sh))
		return nullptr;
	std::vector<char> keep(sh.P, 0);
	const std::string head = vcf_header(rq, sh, keep);
	// ---- the rows as text, in chunks of rows on up to `threads` threads
	const uint64_t n = sh.n;
	const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>(rq.threads, (n + 1023) / 1024));
	std::vector<std::string> chunk(T);
	auto format = [&](int t) {
		Row r;
		for (uint64_t mrow = n * t / T; mrow < n * (t + 1) / T; mrow++)
			if (!row_of(rq, sh, keep, mrow, r))
				continue;
			else if (r.prim)
				primitive_row(rq, sh, r, chunk[t]);
			else
				record_row(rq, sh, r, chunk[t]);
	};
	auto on_threads = [&](auto &&work) {
		std::vector<std::thread> th;
		for (int t = 1; t < T; t++)
			th.emplace_back(work, t);
		work(0);
		for (auto &x : th)
			x.join();
	};
	on_threads(format);
	// ---- one buffer: every thread copies its own chunk into place (the pages of a large text are first touched in parallel)
	std::vector<size_t> first(T + 1, head.size());
	for (int t = 0; t < T; t++)
		first[t + 1] = first[t] + chunk[t].size();
	const size_t total = first[T];
	char *out = static_cast<char *>(malloc(total + 1));
	if (!out)
		return nullptr;
	head.copy(out, head.size());
	on_threads([&](int t) { chunk[t].copy(out + first[t], chunk[t].size()); });
	char *at = out + total;
	*at = 0;
	*len = total;
	return out;
} catch (const std::bad_alloc &) {
	return nullptr;
}
} // namespace

extern "C" char *povu_hip_calls_vcf(const povu_hip_calls *c, const povu_hip_sites *sites, const povu_hip_call_names *names,
				    const char *const *path_name, const char *date, const char *only_prefix, uint32_t threads, size_t *len)
{
	// a caller of before may hold a povu_hip_calls that ends with n_inv_tier2: nothing behind it is read
	return calls_vcf({c, sites, names, path_name, date, only_prefix, nullptr, 0, false, threads, POVU_HIP_PROFILE_RAW_GRAPH, false}, len);
}

extern "C" char *povu_hip_calls_vcf_profile(const povu_hip_calls *c, const povu_hip_sites *sites, const povu_hip_call_names *names,
					    const char *const *path_name, const char *date, const char *only_prefix, uint32_t threads,
					    uint32_t profile, size_t *len)
{
	return calls_vcf({c, sites, names, path_name, date, only_prefix, nullptr, 0, false, threads, profile, true}, len);
}

extern "C" char *povu_hip_calls_vcf_rest(const povu_hip_calls *c, const povu_hip_sites *sites, const povu_hip_call_names *names,
					 const char *const *path_name, const char *date, const char *const *prefix, uint32_t n_prefixes,
					 uint32_t threads, uint32_t profile, size_t *len)
{
	if (n_prefixes && !prefix)
		return nullptr;
	for (uint32_t k = 0; k < n_prefixes; k++)
		if (!prefix[k])
			return nullptr;
	return calls_vcf({c, sites, names, path_name, date, nullptr, prefix, n_prefixes, true, threads, profile, true}, len);
}
