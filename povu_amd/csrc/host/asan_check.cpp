// asan_check.cpp -- CPU-only sanitizer harness for the host-side code of the decompose path (built by
// `make -C povu_amd/csrc asan` with -fsanitize=address,undefined; GPU sanitizers are not available on the test pool).
// Usage: host_asan_check <file.gfa|file.pvst>...   Every .gfa goes through the tokenizer (1 and 4 threads, with
// labels and paths), every .pvst through the reader and, where it parses, through the sites of the call's host half
// (host/vcf.cpp); the names builder and the VCF writer run once over a small hand-made povu_hip_calls.  Malformed inputs
// must fail with an error, not with a fault.  The forest's wire formats (hip/forest_wire.hpp: what one process reads of
// another's forest) run first, on hand-made tables, headers and extended trees: good ones round-trip, bad ones are refused.
// Then the PVST writer (host/pvst_io.cpp) against the plain std::string writer it replaced, kept here as its restatement, on
// generated trees, and its refusals; every .pvst that parses in full is also written back and compared byte for byte.  Then
// the environment hooks of a pass (hip/pass_hooks.hpp) against a table of what the code they came from gave.
#include "../../../include/povu_hip.h"
#include "../hip/forest_wire.hpp"
#include "../hip/pass_hooks.hpp"
#include "gfa.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

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

// hip/forest_wire.hpp; returns 0 or the line of the first check that failed
static int check_forest_wire()
{
	using namespace forest_wire;
#define WANT(x)                                                                                                                              \
	do {                                                                                                                                 \
		if (!(x))                                                                                                                    \
			return __LINE__;                                                                                                     \
	} while (0)
	// ---- the five arrays of a PVST block: a | z | parent | a_or | z_or, each padded to 64 B, inside the linear bound
	for (size_t total : {size_t(0), size_t(1), size_t(15), size_t(16), size_t(17), size_t(1000)}) {
		std::vector<char> blk(PvstArrays::bound(total) + 1);
		char *q = blk.data();
		PvstArrays v;
		const size_t w = pad64(4 * total), b = pad64(total), bytes = PvstArrays::layout(q, total, &v);
		WANT(bytes == 3 * w + 2 * b && bytes == PvstArrays::layout(nullptr, total) && bytes <= PvstArrays::bound(total));
		WANT(w == PvstArrays::word_bytes(total) && b == PvstArrays::flag_bytes(total));
		WANT((char *)v.a == q && (char *)v.z == q + w && (char *)v.parent == q + 2 * w);
		WANT((char *)v.aor == q + 3 * w && (char *)v.zor == q + 3 * w + b);
	}
	// ---- tree tables: 0, 1 and 5 trees, with and without the extras words; the last tree's offset needs the high word
	const uint64_t big = (1ull << 32) + 1000;
	const TreeRecord five[5] = {{1, 10, 12, 7, 0, 0, 2, 0}, {2, 3, 2, 0, 7, 2, 0, 1}, {4, 9, 9, 5, 7, 2, 1, 2}, {7, 1, 0, 1, 12, 3, 0, 2},
				    {9, 50, 70, 900, big - 900, 3, 3, 3}};
	for (size_t n : {size_t(0), size_t(1), size_t(5)})
		for (bool extras : {false, true}) {
			std::vector<uint32_t> w(TREE_WORDS * n + 1, 0xABABABABu);
			WANT(encode_tree_table(w.data(), five, n, big, extras) && w[TREE_WORDS * n] == 0xABABABABu);
			std::vector<TreeRecord> got;
			WANT(!decode_tree_table(w.data(), TREE_WORDS * n, n, big, extras, 6, 5, got) && got.size() == n);
			for (size_t i = 0; i < n; i++) {
				WANT(got[i].component_id == five[i].component_id && got[i].n_vtx == five[i].n_vtx && got[i].n_links == five[i].n_links);
				WANT(got[i].n_pvst == five[i].n_pvst && got[i].off == five[i].off);
				WANT(got[i].n_hairpins == (extras ? five[i].n_hairpins : 0) && got[i].sub_c == (extras ? five[i].sub_c : 0));
				WANT(!extras || got[i].hp_off == five[i].hp_off);
			}
			if (n == 5)
				WANT(w[TREE_WORDS * 4 + 5] == 1 && w[5] == 0); // (the high word: only where the offset needs it)
		}
	{
		std::vector<TreeRecord> got;
		std::vector<uint32_t> w(TREE_WORDS * 5);
		WANT(encode_tree_table(w.data(), five, 5, big, true));
		WANT(!encode_tree_table(w.data(), five, 5, big - 1, true)); // (the sender's own table: the last tree ends behind the block)
		WANT(encode_tree_table(w.data(), five, 5, big, true));
		WANT(decode_tree_table(w.data(), w.size(), 5, big - 1, true, 6, 5, got));	  // n_pvst > total - off
		// off > total and nothing else wrong (n_pvst 0: `total - off` alone would wrap and let it through), decoded and encoded
		const TreeRecord behind = {3, 1, 0, 0, 12, 0, 0, 0};
		uint32_t qb[TREE_WORDS] = {3, 1, 0, 0, 12, 0, 0, 0};
		std::vector<TreeRecord> edge;
		WANT(decode_tree_table(qb, TREE_WORDS, 1, 11, false, 0, 0, edge) && !encode_tree_table(qb, &behind, 1, 11, false) && edge.empty());
		WANT(encode_tree_table(qb, &behind, 1, 12, false) && !decode_tree_table(qb, TREE_WORDS, 1, 12, false, 0, 0, edge) && edge.size() == 1);
		WANT(decode_tree_table(w.data(), w.size(), 5, big, true, 6, 4, got));		  // sub_c + 1 >= c1
		WANT(decode_tree_table(w.data(), w.size(), 5, big, true, 5, 5, got));		  // hairpin counts beyond `pairs`
		WANT(decode_tree_table(w.data(), w.size() - 1, 5, big, true, 6, 5, got));	  // more trees than the buffer holds
		WANT(decode_tree_table(w.data(), w.size(), ~size_t(0) / 2, big, true, 6, 5, got)); // (and a count whose size would wrap)
		got.clear();
		WANT(!decode_tree_table(w.data(), w.size(), 5, big, false, 0, 0, got) && got.size() == 5 && got[4].n_hairpins == 0);
		// off + n_pvst wraps in 32 bits / in 64 bits
		uint32_t q32[TREE_WORDS] = {1, 1, 1, 0x20, 0xFFFFFFF0u, 0, 0, 0}, q64[TREE_WORDS] = {1, 1, 1, 16, 0xFFFFFFFBu, 0xFFFFFFFFu, 0, 0};
		WANT(decode_tree_table(q32, TREE_WORDS, 1, 0xFFFFFFF8ull, false, 0, 0, got));
		WANT(decode_tree_table(q64, TREE_WORDS, 1, ~0ull, false, 0, 0, got));
		WANT(got.size() == 5);
	}
	// ---- the packed forest's header
	{
		const ForestLayout L(5, 1000);
		WANT(L.meta == 64 && L.a == 64 + 128 && L.z == L.a + 4032 && L.parent == L.z + 4032 && L.aor == L.parent + 4032);
		WANT(L.zor == L.aor + 1024 && L.bytes == L.zor + 1024);
		uint64_t h[8];
		size_t n_trees = 0, total = 0;
		ForestLayout::write_header(h, 5, 1000, 9);
		WANT(!ForestLayout::read_header(h, L.bytes, n_trees, total) && n_trees == 5 && total == 1000 && h[2] == 9);
		WANT(ForestLayout::read_header(h, L.bytes - 1, n_trees, total)); // the buffer is shorter than the plan
		h[0] = ~0ull / 16;
		WANT(ForestLayout::read_header(h, L.bytes, n_trees, total)); // sizes beyond the buffer (their bytes would wrap)
		h[0] = 5, h[1] = ~0ull / 4;
		WANT(ForestLayout::read_header(h, L.bytes, n_trees, total));
		h[1] = 1000, h[3] ^= 1;
		WANT(ForestLayout::read_header(h, L.bytes, n_trees, total)); // bad magic word
	}
	// ---- the extras segment: every combination of the three flags
	for (unsigned flags = 0; flags < 8; flags++) {
		XLayout L;
		L.labels = flags & 1u, L.hp = flags & 2u, L.sub = flags & 4u;
		L.total = 77, L.pairs = L.hp ? 5 : 0;
		if (L.sub)
			L.c1 = 4, L.nv = 130, L.nc = 129;
		L.plan();
		size_t want = 128;
		if (L.labels) {
			WANT(L.o_ai == want && L.o_zi == want + 320 && L.o_fam == want + 640);
			want += 640 + 128;
		}
		if (L.hp) {
			WANT(L.o_hp == want);
			want += 128;
		}
		if (L.sub) {
			WANT(L.o_voff == want && L.o_cnt == want + 64 && L.x.fam == want + 128);
			want += 128;
			WANT(L.x.or1 == want + 192 && L.x.or2 == want + 384 && L.x.route == want + 576 && L.x.id1 == want + 768);
			WANT(L.x.id2 == L.x.id1 + 576 && L.x.coff == L.x.id2 + 576 && L.x.child == L.x.coff + 576 && L.x.end == L.x.child + 576);
			want = L.x.end;
		}
		WANT(L.bytes == want);
		uint64_t h[16];
		L.write_header(h);
		XLayout R;
		WANT(!R.read_header(h, L.bytes, 77) && R.bytes == L.bytes && R.labels == L.labels && R.hp == L.hp && R.sub == L.sub);
		WANT(R.o_ai == L.o_ai && R.o_hp == L.o_hp && R.o_voff == L.o_voff && R.x.child == L.x.child && R.x.end == L.x.end);
		WANT(R.read_header(h, L.bytes, 78));	  // another forest's
		WANT(R.read_header(h, L.bytes + 64, 77)); // `bytes` disagrees with what is mapped
		h[7] += 64;
		WANT(R.read_header(h, L.bytes + 64, 77)); // ... and with the plan
		h[7] -= 64;
		for (int k : {2, 4, 5, 6}) { // sizes beyond the segment
			const uint64_t keep = h[k];
			h[k] = ~0ull / 8;
			WANT(R.read_header(h, L.bytes, 77));
			h[k] = keep;
		}
		WANT(!R.read_header(h, L.bytes, 77));
	}
	{ // the -s result block: the same eight sections with one spare entry each, from 0
		const SubBlockLayout B(130, 129, 0, 1);
		WANT(B.fam == 0 && B.or1 == 192 && B.id1 == 768 && B.id2 == 768 + 576 && B.coff == B.id2 + 576 && B.child == B.coff + 576);
		WANT(B.end == B.child + 576);
		const SubBlockLayout Z(63, 15, 0, 1); // (the spare entry takes a section over a boundary)
		WANT(Z.or1 == 64 && Z.id1 == 256 && Z.coff == 256 + 512 && Z.child == Z.coff + 256 && Z.end == Z.child + 64);
	}
	// ---- extended trees: three components (the second without vertices) of 3 and 2 vertices
	{
		const uint64_t voff[4] = {0, 3, 3, 5};
		const uint32_t coff[6] = {0, 2, 2, 2, 3, 3}, child[3] = {1, 2, 1};
		WANT(!validate_subforest(voff, 4, coff, 5, child, 3));
		WANT(!validate_subforest(voff, 0, coff, 0, child, 0) && validate_subforest(voff, 0, coff, 5, child, 3));
		auto bad = [&](int what) {
			std::vector<uint64_t> v(voff, voff + 4);
			std::vector<uint32_t> c(coff, coff + 6), ch(child, child + 3);
			size_t nv = 5, nc = 3;
			switch (what) {
			case 0: v[1] = 4, v[2] = 3; break;	// voff decreasing
			case 1: v[3] = 4; break;		// voff.back() != nv
			case 2: c[2] = 1; break;		// coff decreasing
			case 3: c[5] = 2; break;		// coff[nv] != nc
			case 4: ch[2] = 2; break;		// a child equal to its component's vertex count
			case 5: ch[0] = 3; break;		// (the same in the first component)
			case 6: v[0] = 1; break;		// vertices before the first component
			case 7: c[1] = 0xFFFFFFF0u; break; // (an offset far behind `child`: found before anything is read there)
			}
			return validate_subforest(v.data(), 4, c.data(), nv, ch.data(), nc) != nullptr;
		};
		for (int what = 0; what < 8; what++)
			WANT(bad(what));
	}
#undef WANT
	return 0;
}

// ---- the PVST writer
// The writer the library had for a tree with its -s vertices before pvst_emit served every form: a growing string and a
// library call per number.  Kept only here, as the naive restatement of the line format.
static std::string naive_pvst_text(const povu_hip_subtree *t)
{
	std::string o;
	o += "H\t0.0.3\t.\t.\t.\n";
	for (uint32_t v = 0; v < t->n_total; v++) {
		o += (char)t->fam[v];
		o += '\t';
		o += std::to_string(v);
		o += '\t';
		if (t->fam[v] == 'D') {
			o += '.';
		} else { // id_or_t::as_str, include/povu/graph/types.hpp:85-95
			o += t->or1[v] ? '<' : '>';
			o += std::to_string(t->id1[v]);
			o += t->or2[v] ? '<' : '>';
			o += std::to_string(t->id2[v]);
		}
		o += '\t';
		const uint32_t c0 = t->child_off[v], c1 = t->child_off[v + 1];
		if (c0 == c1) {
			o += '.';
		} else { // print_with_comma, include/povu/common/utils.hpp:44-55
			for (uint32_t k = c0; k < c1; k++) {
				o += std::to_string(t->child[k]);
				if (k + 1 < c1)
					o += ", ";
			}
		}
		o += '\t';
		if (t->route[v])
			o += (char)t->route[v];
		else
			o += '.';
		o += '\n';
	}
	return o;
}

// a tree in both forms of the writer's input: the arrays of a PVST (parent) and the extended tree of -s (children lists)
struct TextTree {
	std::vector<uint8_t> fam, or1, or2, route;
	std::vector<uint32_t> id1, id2, parent, coff, child;
	void add(char letter, uint32_t par, uint32_t a, uint32_t z, uint8_t o1 = 0, uint8_t o2 = 0, char r = 'L')
	{
		fam.push_back((uint8_t)letter), parent.push_back(par), id1.push_back(a), id2.push_back(z), or1.push_back(o1), or2.push_back(o2);
		route.push_back(letter == 'D' ? 0 : (uint8_t)r);
	}
	void children_from_parents()
	{
		const uint32_t n = (uint32_t)fam.size();
		coff.assign(n + 1, 0);
		for (uint32_t v = 1; v < n; v++)
			coff[parent[v] + 1]++;
		for (uint32_t v = 0; v < n; v++)
			coff[v + 1] += coff[v];
		child.assign(coff[n] + 1, 0); // (+1: never an empty vector's null data())
		std::vector<uint32_t> at(coff.begin(), coff.end() - 1);
		for (uint32_t v = 1; v < n; v++)
			child[at[parent[v]]++] = v;
	}
	povu_hip_subtree view() const
	{
		povu_hip_subtree t{};
		t.n_total = t.n_flubble_like = (uint32_t)fam.size();
		t.fam = fam.data(), t.or1 = or1.data(), t.or2 = or2.data(), t.route = route.data();
		t.id1 = id1.data(), t.id2 = id2.data(), t.child_off = coff.data(), t.child = child.data();
		return t;
	}
};

// the subtree form against the restatement; with `arrays` also the array form (the letters given, and left out when they are
// D / F) against the same bytes
static bool same_text(const TextTree &x, bool arrays)
{
	const povu_hip_subtree t = x.view();
	const std::string want = naive_pvst_text(&t);
	auto is = [&](char *got, size_t len) {
		const bool eq = got && len == want.size() && memcmp(got, want.data(), len) == 0 && got[len] == 0;
		povu_hip_buffer_free(got);
		return eq;
	};
	size_t len = 0;
	char *got = povu_hip_pvst_format_subtree(&t, &len);
	if (!is(got, len))
		return false;
	if (!arrays)
		return true;
	const uint32_t n = t.n_total;
	got = povu_hip_pvst_format_fam(n, t.id1, t.id2, t.or1, t.or2, x.parent.data(), t.fam, &len);
	if (!is(got, len))
		return false;
	bool plain = true;
	for (uint32_t v = 1; v < n; v++)
		plain = plain && t.fam[v] == 'F';
	if (plain) {
		got = povu_hip_pvst_format(n, t.id1, t.id2, t.or1, t.or2, x.parent.data(), &len);
		if (!is(got, len))
			return false;
	}
	return true;
}

static int check_pvst_writer()
{
#define WANT(c)                                                                                                                   \
	do {                                                                                                                      \
		if (!(c))                                                                                                         \
			return __LINE__;                                                                                          \
	} while (0)
	const uint32_t NIL = POVU_HIP_NIL;
	// every line letter, both routes and none, both orientations (the letters C M S and the route R: the subtree form only)
	{
		TextTree x;
		x.add('D', NIL, 0, 0);
		const char letters[] = "FTOCMS";
		for (int k = 0; k < 6; k++)
			x.add(letters[k], k < 3 ? 0 : (uint32_t)k - 2, 10 + k, 20 + k, k & 1, (k >> 1) & 1, k % 3 == 0 ? 'L' : k % 3 == 1 ? 'R' : 0);
		x.children_from_parents();
		WANT(same_text(x, false));
		TextTree y; // (the letters and the route the array form knows)
		y.add('D', NIL, 0, 0);
		for (int k = 0; k < 6; k++)
			y.add(letters[k % 3], (uint32_t)k / 2, 10 + k, 20 + k, k & 1, (k >> 1) & 1);
		y.children_from_parents();
		WANT(same_text(y, true));
	}
	// segment ids at every edge of the digit count
	{
		TextTree x;
		x.add('D', NIL, 0, 0);
		const uint32_t edge[] = {0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000,
					 99999999, 100000000, 999999999, 1000000000, 4294967295u};
		const uint32_t ne = sizeof edge / sizeof *edge;
		for (uint32_t k = 0; k < ne; k++)
			x.add('F', 0, edge[k], edge[ne - 1 - k], k & 1, ~k & 1);
		x.children_from_parents();
		WANT(same_text(x, true));
	}
	// vertices with 1 000, 2, 1 and 0 children
	{
		TextTree x;
		x.add('D', NIL, 0, 0);
		for (uint32_t v = 1; v <= 1003; v++)
			x.add('F', v <= 1000 ? 0 : v <= 1002 ? 1 : 2, v, v + 1);
		x.children_from_parents();
		WANT(x.coff[1] == 1000 && x.coff[2] - x.coff[1] == 2 && x.coff[3] - x.coff[2] == 1 && x.coff[4] == x.coff[3]);
		WANT(same_text(x, true));
	}
	// chains and stars of 1, 2 and 3 vertices
	for (uint32_t n = 1; n <= 3; n++)
		for (int star = 0; star < 2; star++) {
			TextTree x;
			x.add('D', NIL, 0, 0);
			for (uint32_t v = 1; v < n; v++)
				x.add('F', star ? 0 : v - 1, 2 * v, 2 * v + 1);
			x.children_from_parents();
			WANT(same_text(x, true));
		}
	// every id ten digits wide: no text of that many lines is longer
	{
		TextTree x;
		x.add('D', NIL, 0, 0);
		for (uint32_t v = 1; v < 50; v++)
			x.add('F', (v - 1) / 2, 4294967295u, 4000000000u + v, 1, 1);
		x.children_from_parents();
		WANT(same_text(x, true));
	}
	// an extended tree that lists its vertices far more often than once (a concealed vertex is listed under two parents;
	// here every vertex under every vertex, 40 times): the text is much longer than a tree's of as many lines
	{
		TextTree x;
		x.add('D', NIL, 0, 0);
		x.add('C', 0, 4294967295u, 4294967294u, 1, 1, 'R');
		x.add('M', 0, 4294967293u, 4294967292u, 1, 1, 'R');
		x.coff.assign(1, 0);
		for (uint32_t v = 0; v < 3; v++) {
			for (uint32_t k = 0; k < 120; k++)
				x.child.push_back(k % 3);
			x.coff.push_back((uint32_t)x.child.size());
		}
		WANT(x.child.size() > 3 - 1);
		WANT(same_text(x, false));
	}
	// the refusals
	{
		const uint32_t id[] = {0, 1, 2}, par[] = {NIL, 0, 1}, par_self[] = {NIL, 1, 1}, par_late[] = {NIL, 0, 5};
		const uint8_t orr[] = {0, 0, 1}, fam[] = {'D', 'T', 'O'};
		size_t len = 0;
		char *ok = povu_hip_pvst_format_fam(3, id, id, orr, orr, par, fam, &len);
		WANT(ok && len);
		povu_hip_buffer_free(ok);
		WANT(!povu_hip_pvst_format_fam(0, id, id, orr, orr, par, fam, &len) && !povu_hip_pvst_format(0, id, id, orr, orr, par, &len));
		WANT(!povu_hip_pvst_format_fam(3, nullptr, id, orr, orr, par, fam, &len) && !povu_hip_pvst_format(3, nullptr, id, orr, orr, par, &len));
		WANT(!povu_hip_pvst_format_fam(3, id, nullptr, orr, orr, par, fam, &len) && !povu_hip_pvst_format(3, id, nullptr, orr, orr, par, &len));
		WANT(!povu_hip_pvst_format_fam(3, id, id, nullptr, orr, par, fam, &len) && !povu_hip_pvst_format(3, id, id, nullptr, orr, par, &len));
		WANT(!povu_hip_pvst_format_fam(3, id, id, orr, nullptr, par, fam, &len) && !povu_hip_pvst_format(3, id, id, orr, nullptr, par, &len));
		WANT(!povu_hip_pvst_format_fam(3, id, id, orr, orr, nullptr, fam, &len) && !povu_hip_pvst_format(3, id, id, orr, orr, nullptr, &len));
		for (const char *bad : {"FTO", "DDO", "DTD", "DCO", "DTM", "DSF", "DXF", "dTO"}) // (a letter outside D / F, T, O, or in the other's place)
			WANT(!povu_hip_pvst_format_fam(3, id, id, orr, orr, par, reinterpret_cast<const uint8_t *>(bad), &len));
		WANT(!povu_hip_pvst_format_fam(3, id, id, orr, orr, par_self, fam, &len) && !povu_hip_pvst_format(3, id, id, orr, orr, par_self, &len));
		WANT(!povu_hip_pvst_format_fam(3, id, id, orr, orr, par_late, fam, &len) && !povu_hip_pvst_format(3, id, id, orr, orr, par_late, &len));
		WANT(!povu_hip_pvst_format_subtree(nullptr, &len));
	}
#undef WANT
	return 0;
}

// a .pvst that parsed, written back through the array form of the writer (the letters of the file given): the bytes of the
// file.  Only for files that number their lines by row and hold the letters that form knows.
static bool pvst_round_trip(const povu_pvst_doc *d, const std::string &text)
{
	size_t len = 0;
	char *got = povu_hip_pvst_format_fam(d->n, d->a_id, d->z_id, d->a_or, d->z_or, d->parent, reinterpret_cast<const uint8_t *>(d->type), &len);
	const bool eq = got && len == text.size() && memcmp(got, text.data(), len) == 0;
	povu_hip_buffer_free(got);
	return eq;
}

// ---- the environment hooks of a pass: read_pass_hooks() against what the expressions it replaced gave for the same text.
// Those stood at their points of use (the line numbers: the files as they were before pass_hooks.hpp), `ev` = the variable's text:
//   POVU_HIP_WIDE_COUNTS  povu_hip.hip:911-912      ev ? atoi(ev) : 0
//   POVU_HIP_WORD_PREFIX  par_kernels.hip:1513      ev ? atoi(ev) : 0
//   POVU_HIP_LSZ_FIELD    par_kernels.hip:1515      ev ? (unsigned)min(max(atoi(ev), 0), (int)LSZ_FIELD_CAP) : LSZ_FIELD_CAP    (the cap: 8)
//   POVU_HIP_WALK_ROUTE   tree_kernels.hip:1832     ev ? (uint32_t)atoi(ev) : 0u
//   POVU_HIP_DFS_BLOCKS   tree_kernels.hip:1876-78  min(all_blocks, ev ? max(1u, (unsigned)atoi(ev)) : 49152u)    (the value before the min)
//   POVU_HIP_CLASS_BUDGET tree_kernels.hip:1880-82  ev ? (uint32_t)max(16, atoi(ev)) : CLASS_BUDGET    (256)
//   POVU_HIP_RANK_STATS   tree_kernels.hip:1761     ev != nullptr
//   POVU_HIP_RANK_BITS    list_rank.hip:27-29       ev ? (unsigned)min(6, max(2, atoi(ev))) : 3u
// atoi of "" and of text without digits is 0; a negative number converted to unsigned wraps.
static int check_pass_hooks()
{
	using povu_hip::PassHooks;
	struct Row {
		const char *text; // null: unset
		int64_t want;
	};
	struct Hook {
		const char *name;
		int64_t (*get)(const PassHooks &);
		std::vector<Row> rows;
	};
	const std::vector<Hook> hooks = {
		{"POVU_HIP_WIDE_COUNTS", [](const PassHooks &h) { return (int64_t)h.wide_counts; },
		 {{nullptr, 0}, {"1", 1}, {"2", 2}, {"3", 3}, {"0", 0}, {"-1", -1}, {"9", 9}, {"", 0}, {"words", 0}}},
		{"POVU_HIP_WORD_PREFIX", [](const PassHooks &h) { return (int64_t)h.word_prefix; },
		 {{nullptr, 0}, {"1", 1}, {"2", 2}, {"3", 3}, {"0", 0}, {"-1", -1}, {"9", 9}, {"", 0}, {"words", 0}}},
		{"POVU_HIP_LSZ_FIELD", [](const PassHooks &h) { return (int64_t)h.lsz_field; },
		 {{nullptr, 8}, {"5", 5}, {"0", 0}, {"8", 8}, {"-3", 0}, {"9", 8}, {"99", 8}, {"", 0}, {"wide", 0}}},
		{"POVU_HIP_WALK_ROUTE", [](const PassHooks &h) { return (int64_t)h.walk_route; },
		 {{nullptr, 0}, {"1", 1}, {"2", 2}, {"-1", 4294967295ll}, {"", 0}, {"left", 0}}},
		{"POVU_HIP_DFS_BLOCKS", [](const PassHooks &h) { return (int64_t)h.dfs_blocks; },
		 {{nullptr, 49152}, {"3072", 3072}, {"1", 1}, {"0", 1}, {"-5", 4294967291ll}, {"196608", 196608}, {"", 1}, {"many", 1}}},
		{"POVU_HIP_CLASS_BUDGET", [](const PassHooks &h) { return (int64_t)h.class_budget; },
		 {{nullptr, 256}, {"64", 64}, {"16", 16}, {"15", 16}, {"0", 16}, {"-7", 16}, {"100000", 100000}, {"", 16}, {"big", 16}}},
		{"POVU_HIP_RANK_STATS", [](const PassHooks &h) { return (int64_t)h.rank_stats; },
		 {{nullptr, 0}, {"1", 1}, {"0", 1}, {"", 1}, {"no", 1}}},
		{"POVU_HIP_RANK_BITS", [](const PassHooks &h) { return (int64_t)h.rank_bits; },
		 {{nullptr, 3}, {"4", 4}, {"2", 2}, {"6", 6}, {"1", 2}, {"-4", 2}, {"7", 6}, {"40", 6}, {"", 2}, {"bits", 2}}},
	};
	for (const Hook &k : hooks)
		unsetenv(k.name);
	for (const Hook &k : hooks) {
		for (const Row &r : k.rows) {
			if (r.text)
				setenv(k.name, r.text, 1);
			else
				unsetenv(k.name);
			const PassHooks h = povu_hip::read_pass_hooks();
			if (k.get(h) != r.want) {
				fprintf(stderr, "host_asan_check: %s=%s gives %lld, not %lld\n", k.name, r.text ? r.text : "(unset)", (long long)k.get(h),
					(long long)r.want);
				return 1;
			}
			for (const Hook &o : hooks) // (a variable moves its own field only)
				if (&o != &k && o.get(h) != o.rows[0].want)
					return 2;
		}
		unsetenv(k.name);
	}
	return 0;
}

int main(int argc, char **argv)
{
	unsigned long ok = 0, rejected = 0, written_back = 0;
	if (int line = check_forest_wire()) {
		fprintf(stderr, "host_asan_check: forest_wire check failed at line %d\n", line);
		return 13;
	}
	printf("host_asan_check: forest_wire ok\n");
	if (int rc = check_vcf_writer())
		return rc;
	if (int line = check_pvst_writer()) {
		fprintf(stderr, "host_asan_check: PVST writer check failed at line %d\n", line);
		return 14;
	}
	printf("host_asan_check: pvst_writer ok\n");
	if (check_pass_hooks())
		return 15;
	printf("host_asan_check: pass_hooks ok\n");
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
					if (len == text.size()) {
						if (!pvst_round_trip(d, text)) {
							fprintf(stderr, "host_asan_check: %s is not what the writer makes of its parse\n", path.c_str());
							return 16;
						}
						written_back++;
					}
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
	printf("host_asan_check: %lu parsed, %lu rejected, %lu written back\n", ok, rejected, written_back);
	return 0;
}
