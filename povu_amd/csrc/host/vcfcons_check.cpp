// vcfcons_check.cpp -- the rules of the consensus haplotypes (hip/vcfcons_rules.hpp) on the CPU, under the sanitizers: the
// order, the drop rule one edit after another and in the kernel's chunks of 64 with carries (the wave of wave_emu.hpp), the
// kept edits' offsets, and the materialiser's walk -- tiles, lanes of 16 bytes, vc_seek once and vc_source from there --
// against a byte-by-byte apply; on the hand-made lists of INTEGRATION.md "Consensus haplotypes" and on a small seeded fuzz.
// Built by `make vcfcons_check`, run by tests/test_vcfcons_ref.py.  Prints `vcfcons_check: ok` and exits 0, or says what failed.
#include "../hip/vcfcons_rules.hpp"
#include "wave_emu.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

using namespace povu_hip;

namespace
{
int failures = 0;
#define CHECK(cond, ...)                                                                  \
	do {                                                                              \
		if (!(cond)) {                                                            \
			failures++;                                                       \
			fprintf(stderr, "vcfcons_check: %s:%d: ", __FILE__, __LINE__);    \
			fprintf(stderr, __VA_ARGS__);                                     \
			fprintf(stderr, "\n");                                            \
		}                                                                         \
	} while (0)

struct Edit {
	uint64_t s, e; // 0-based, half-open
	std::string t;
	uint32_t group;
};
VcOrdered ordered(const Edit &x) { return {x.s + 1, x.e + 1, x.group}; }
void sort_edits(std::vector<Edit> &v)
{
	std::stable_sort(v.begin(), v.end(), [](const Edit &a, const Edit &b) { return vc_before(ordered(a), ordered(b)); });
}
// the order as the device makes it: VC_SORT_PASSES stable passes, least significant part first, each over the low
// vc_sort_bits bits of its part alone (a radix sort reads no more)
void sort_edits_by_passes(std::vector<Edit> &v, unsigned group_bits)
{
	for (int which = 0; which < VC_SORT_PASSES; which++) {
		const unsigned bits = vc_sort_bits(which, group_bits);
		const uint32_t mask = bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1;
		std::stable_sort(v.begin(), v.end(), [&](const Edit &a, const Edit &b) {
			const VcOrdered x = ordered(a), y = ordered(b);
			return (vc_sort_key(which, x.bs, x.be, x.group) & mask) < (vc_sort_key(which, y.bs, y.be, y.group) & mask);
		});
	}
}
void check_passes(std::vector<Edit> v, const char *what)
{
	std::vector<Edit> by_passes = v;
	sort_edits(v);
	sort_edits_by_passes(by_passes, 8);
	for (size_t k = 0; k < v.size(); k++)
		CHECK(v[k].s == by_passes[k].s && v[k].e == by_passes[k].e && v[k].group == by_passes[k].group,
		      "%s: place %zu holds [%llu, %llu) by the passes, [%llu, %llu) by the order", what, k, (unsigned long long)by_passes[k].s,
		      (unsigned long long)by_passes[k].e, (unsigned long long)v[k].s, (unsigned long long)v[k].e);
}
// the verdicts one edit after another
std::vector<uint32_t> decide_plain(const std::vector<Edit> &v)
{
	std::vector<uint32_t> out;
	uint64_t most = 0;
	for (size_t k = 0; k < v.size(); k++) {
		const VcOrdered a = ordered(v[k]), p = k ? ordered(v[k - 1]) : VcOrdered{0, 0, 0};
		out.push_back(vc_decide(a.bs, a.be, a.group, k > 0, most, p.bs, p.be, p.group));
		most = std::max(most, a.be);
	}
	return out;
}
// ... and as k_vc_lists does: 64 edits a chunk, an inclusive max-scan inside it, carries between; the kept edits ranked by a
// ballot and placed by the sum of their length changes
struct Listed {
	std::vector<uint32_t> verdict, kept; // kept: indices into the ordered list
	std::vector<uint64_t> start;	     // of every kept edit, in the haplotype
	uint64_t delta = 0;
};
Listed decide_chunked(const std::vector<Edit> &v)
{
	Listed L;
	L.verdict.resize(v.size());
	const EmuWave w;
	uint64_t carry_end = 0, carry_d = 0;
	VcOrdered carry_prev{0, 0, 0};
	for (size_t c0 = 0; c0 < v.size(); c0 += 64) {
		uint64_t incl[64], d[64], dincl[64];
		VcOrdered a[64];
		bool in[64];
		for (uint32_t lane = 0; lane < 64; lane++) {
			in[lane] = c0 + lane < v.size();
			a[lane] = in[lane] ? ordered(v[c0 + lane]) : VcOrdered{0, 0, 0};
			incl[lane] = std::max(lane ? incl[lane - 1] : 0, a[lane].be);
		}
		uint32_t verdict[64];
		for (uint32_t lane = 0; lane < 64; lane++) {
			const uint64_t before = std::max(lane ? incl[lane - 1] : 0, carry_end);
			const VcOrdered p = lane ? a[lane - 1] : carry_prev;
			verdict[lane] = in[lane] ? vc_decide(a[lane].bs, a[lane].be, a[lane].group, c0 + lane > 0, before, p.bs, p.be, p.group) : (uint32_t)VC_DUPLICATE;
			d[lane] = in[lane] && verdict[lane] == VC_KEEP ? vc_delta(a[lane].bs, a[lane].be, v[c0 + lane].t.size()) : 0;
			dincl[lane] = (lane ? dincl[lane - 1] : 0) + d[lane];
		}
		const uint64_t km = w.ballot([&](uint32_t lane) { return in[lane] && verdict[lane] == VC_KEEP; });
		const size_t chunk_base = L.kept.size();
		for (uint32_t lane = 0; lane < 64; lane++) {
			if (!in[lane])
				continue;
			L.verdict[c0 + lane] = verdict[lane];
			if (km >> lane & 1) {
				// (the kernel's place: the kept of the chunks in front, then the kept lanes below this one)
				CHECK(L.kept.size() == chunk_base + (size_t)__builtin_popcountll(km & ((1ull << lane) - 1)), "the ballot's rank");
				L.kept.push_back((uint32_t)(c0 + lane));
				L.start.push_back((a[lane].bs - 1) + carry_d + (dincl[lane] - d[lane]));
			}
		}
		carry_end = std::max(carry_end, incl[63]);
		carry_d += dincl[63];
		carry_prev = a[63];
	}
	L.delta = carry_d;
	return L;
}
std::string apply_plain(const std::string &path, const std::vector<Edit> &v, const std::vector<uint32_t> &kept)
{
	std::string out;
	uint64_t at = 0;
	for (uint32_t k : kept) {
		out += path.substr(at, v[k].s - at) + v[k].t;
		at = v[k].e;
	}
	return out + path.substr(at);
}

// several haplotypes one after another, written as k_vc_materialise writes them
struct Hap {
	std::string path;
	std::vector<Edit> edits; // ordered
	Listed L;
	uint64_t len;
};
std::string materialise(const std::vector<Hap> &haps, uint32_t tile_bytes)
{
	std::vector<uint64_t> hoff(1, 0);
	for (const Hap &h : haps)
		hoff.push_back(hoff.back() + h.len);
	const uint64_t total = hoff.back();
	const uint32_t nH = (uint32_t)haps.size();
	std::string out((total + 15) / 16 * 16, '?');
	for (uint64_t tile0 = 0; tile0 < total; tile0 += tile_bytes) {
		const uint32_t ht = span_of(hoff.data(), nH, tile0);
		for (uint64_t g0 = tile0; g0 < tile0 + tile_bytes && g0 < total; g0 += 16) {
			uint32_t h = ht + span_of(hoff.data() + ht, nH - ht, g0);
			uint64_t h_end = hoff[h + 1], o = g0 - hoff[h];
			const Hap *H = &haps[h];
			uint32_t n = (uint32_t)H->L.kept.size();
			auto edit = [&](uint32_t u) {
				CHECK(u < H->L.kept.size(), "edit %u of %zu", u, H->L.kept.size());
				const Edit &e = H->edits[H->L.kept[u]];
				return VcKept{H->L.start[u], e.t.size(), e.e};
			};
			VcWalk w;
			if (h == ht) { // as the kernel: between the tile's first and last edit
				const uint64_t ot = tile0 - hoff[ht];
				auto start = [&](uint32_t u) { return H->L.start[u]; };
				w = vc_seek_between(o, vh_locate(ot, n, start), vh_locate(ot + (tile_bytes - 1), n, start), n, edit);
				const VcWalk whole = vc_seek(o, n, edit);
				CHECK(w.k == whole.k && w.nx == whole.nx && w.next_start == whole.next_start, "the seek between the tile's edits finds another edit");
			} else {
				w = vc_seek(o, n, edit);
			}
			if (g0 + 16 <= h_end) {
				const VhSource src = vc_source(w, o, n, edit);
				if (!src.from_edit && vc_ref_run(w, o, n) >= 16) {
					CHECK(src.at + 16 <= H->path.size(), "a run of 16 past the path's end");
					out.replace(g0, 16, H->path, src.at, 16);
					continue;
				}
			}
			for (uint32_t b = 0; b < 16; b++) {
				const uint64_t g = g0 + b;
				char byte = 0;
				if (g < total) {
					while (g >= h_end) {
						h++;
						CHECK(h < nH, "a haplotype past the last");
						H = &haps[h], h_end = hoff[h + 1], o = 0, n = (uint32_t)H->L.kept.size();
						w = vc_seek(0, n, edit);
					}
					const VhSource src = vc_source(w, o, n, edit);
					if (src.from_edit) {
						CHECK(w.k < n && src.at < H->edits[H->L.kept[w.k]].t.size(), "a byte past T");
						byte = H->edits[H->L.kept[w.k]].t[src.at];
					} else {
						CHECK(src.at < H->path.size(), "a base past the path: %llu of %zu", (unsigned long long)src.at, H->path.size());
						byte = H->path[src.at];
					}
					o++;
				}
				out[g] = byte;
			}
		}
	}
	out.resize(total);
	return out;
}
Hap make_hap(const std::string &path, std::vector<Edit> edits)
{
	Hap h{path, std::move(edits), {}, 0};
	sort_edits(h.edits);
	h.L = decide_chunked(h.edits);
	const std::vector<uint32_t> plain = decide_plain(h.edits);
	CHECK(plain == h.L.verdict, "the chunks decide otherwise than one edit after another (%zu edits)", h.edits.size());
	h.len = path.size() + h.L.delta;
	const std::string want = apply_plain(path, h.edits, h.L.kept);
	CHECK(want.size() == h.len, "length %zu, the sum of the changes says %llu", want.size(), (unsigned long long)h.len);
	return h;
}
std::vector<uint32_t> counts(const Hap &h)
{
	std::vector<uint32_t> n(4, 0);
	for (uint32_t v : h.L.verdict)
		n[v]++;
	return n;
}

void hand_cases()
{
	const std::string P = "ACGTACGTACGTACGTACGTACGT";
	const Edit span{2, 8, "CCC", 0};
	struct Case {
		std::vector<Edit> edits;
		std::vector<uint32_t> want; // kept, duplicate, enclosed, overlap
		const char *text;
	} cases[] = {
		{{span, {3, 4, "A", 1}, {5, 6, "G", 2}}, {1, 0, 2, 0}, "ACCCCACGTACGTACGTACGT"},
		{{{3, 4, "C", 0}, {3, 4, "C", 0}}, {1, 1, 0, 0}, "ACGCACGTACGTACGTACGTACGT"},
		{{span, {2, 2, "TT", 1}}, {2, 0, 0, 0}, "ACTTCCCACGTACGTACGTACGT"},
		{{span, {8, 8, "GG", 1}}, {2, 0, 0, 0}, "ACCCCGGACGTACGTACGTACGT"},
		{{span, {5, 5, "GG", 1}}, {1, 0, 1, 0}, "ACCCCACGTACGTACGTACGT"},
		{{{2, 2, "TT", 0}, {2, 2, "GG", 1}}, {1, 0, 0, 1}, "ACTTGTACGTACGTACGTACGTACGT"},
		{{{0, 10, "TTG", 0}, {5, 20, "AA", 1}, {12, 15, "TT", 2}}, {1, 0, 1, 1}, "TTGGTACGTACGTACGT"},
		{{{0, 24, "", 0}}, {1, 0, 0, 0}, ""},						     // the whole path deleted
		{{{0, 0, "GG", 0}, {24, 24, "TT", 1}, {0, 1, "C", 2}, {23, 24, "", 3}}, {4, 0, 0, 0}, "GGCCGTACGTACGTACGTACGTACGTT"}, // both ends
	};
	for (const Case &c : cases) {
		const Hap h = make_hap(P, c.edits);
		CHECK(counts(h) == c.want, "counts of the case with text %s", c.text);
		CHECK(apply_plain(P, h.edits, h.L.kept) == c.text, "text %s, want %s", apply_plain(P, h.edits, h.L.kept).c_str(), c.text);
		for (uint32_t tile : {16u, 32u, 4096u})
			CHECK(materialise({h}, tile) == c.text, "the walk writes %s, want %s", materialise({h}, tile).c_str(), c.text);
	}
	// the order itself: s, insertions first, e descending, group
	std::vector<Edit> v = {{5, 9, "", 3}, {5, 5, "A", 2}, {5, 12, "", 1}, {4, 6, "", 0}, {5, 9, "", 1}};
	sort_edits(v);
	const uint32_t want[] = {0, 2, 1, 1, 3};
	for (size_t k = 0; k < v.size(); k++)
		CHECK(v[k].group == want[k], "order: place %zu holds group %u", k, v[k].group);
	// ... and by the device's passes: equal starts whose ends straddle a multiple of 1024, lie more than 1024 and more than
	// 2^32 apart; starts that differ in the high word only
	check_passes(v, "the hand list");
	check_passes({{1000, 1010, "", 0}, {1000, 1030, "", 1}, {1000, 3000, "", 2}, {1000, 1000, "A", 3}, {1000, 1023, "", 4}, {1000, 1024, "", 5}}, "ends around 1024");
	check_passes({{7, (1ull << 32) + 5, "", 0}, {7, 9, "", 1}, {7, (1ull << 33) + 1, "", 2}, {7, 1ull << 32, "", 3}}, "ends around 2^32");
	check_passes({{(1ull << 32) + 3, (1ull << 32) + 9, "", 0}, {5, 6, "", 1}, {(1ull << 33) + 3, (1ull << 33) + 4, "", 2}, {3, 1ull << 34, "", 3}}, "starts around 2^32");
	CHECK(vc_key_e(1) > vc_key_e(2) && vc_key_e((1ull << VC_COORD_BITS) - 1) == 0, "the e key descends");
}

void fuzz()
{
	std::mt19937_64 rng(20261021);
	auto upto = [&](uint64_t n) { return (uint64_t)(rng() % (n + 1)); };
	const char *B = "ACGTacgtN";
	for (int round = 0; round < 300; round++) {
		std::vector<Hap> haps;
		const uint32_t n_haps = 1 + (uint32_t)upto(5);
		for (uint32_t k = 0; k < n_haps; k++) {
			std::string path(upto(round % 3 ? 90 : 400), 'A');
			for (char &c : path)
				c = B[upto(3)];
			std::vector<Edit> edits;
			const uint32_t n = (uint32_t)upto(round % 5 ? 12 : 150);
			for (uint32_t i = 0; i < n; i++) {
				Edit e;
				e.s = upto(path.size());
				e.e = std::min<uint64_t>(path.size(), e.s + (upto(3) ? upto(4) : upto(40)));
				e.t = std::string(upto(2) ? upto(3) : upto(40), 'x');
				for (char &c : e.t)
					c = B[4 + upto(4)];
				e.group = (uint32_t)edits.size();
				if (!edits.empty() && !upto(6)) // a copy of an earlier edit: the same group
					e = edits[upto(edits.size() - 1)];
				edits.push_back(e);
			}
			check_passes(edits, "fuzz");
			haps.push_back(make_hap(path, edits));
		}
		std::string want;
		for (const Hap &h : haps)
			want += apply_plain(h.path, h.edits, h.L.kept);
		for (uint32_t tile : {16u, 64u, 4096u})
			CHECK(materialise(haps, tile) == want, "round %d, tile %u: the walk and the plain apply differ", round, tile);
		for (const Hap &h : haps) { // the kept edits are free of overlaps, in order
			uint64_t at = 0;
			for (uint32_t k : h.L.kept) {
				CHECK(h.edits[k].s >= at, "round %d: a kept edit begins inside the one in front", round);
				at = h.edits[k].e;
			}
		}
	}
}
} // namespace

int main()
{
	hand_cases();
	fuzz();
	if (failures) {
		fprintf(stderr, "vcfcons_check: %d failures\n", failures);
		return 1;
	}
	printf("vcfcons_check: ok\n");
	return 0;
}
