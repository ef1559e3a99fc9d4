// vcfhap_check.cpp -- the rules of the haplotype comparison as the device runs them (hip/vcfhap_rules.hpp), on the CPU.  Built
// with -fsanitize=address,undefined (`make vcfhap_check`) and driven by tests/test_vcfhap_ref.py, which compares every line
// with the restatement.  Blocks on stdin (a text `_` is the empty text):
//   edit <pos> <ref> <alt>          -> `<s> <e> <suffix> <prefix> <T> <hash>`: the lane's loops, and again through the wave loops
//                                   the tier-2 kernel calls (wave_suffix, wave_prefix, wave_text_hash of hip/vcfcmp_rules.hpp)
//                                   over an emulated wave (wave_emu.hpp); the two must agree or the program fails
//   reach <path> <s> <e> <unit> <max>  -> `<left> <right> <capped>`: k_vh_reach's two calls of wave_first, to the right, then to
//                                   the left, one step beyond the cap
//   heads <n> then n marks          -> a 0 or 1 per sorted span: the running maximum in chunks of 64 with a carry, then the test
//   conflict <n> then n pairs s e   -> 0 or 1: the sorted list in chunks of 64, the maximum end and the last edit carried
//   hap <text> <lo> <n> then n triples s e T  -> the haplotype, every byte by the locator
//   status <7 flags>                -> the status, or `compare`;  compared <equal> <edits a> <edits b> -> the status
#include "../../../include/povu_hip.h"
#include "../hip/vcfhap_rules.hpp"
#include "wave_emu.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace povu_hip;

// (exact sizes: a read beyond a text is the sanitizer's to report)
static std::vector<char> exact(const std::string &t) { return std::vector<char>(t.begin(), t.end()); }
static std::string text_of(const std::string &token) { return token == "_" ? "" : token; }

struct Edit {
	uint64_t s, p, hash;
	VhEdit e;
};
static Edit lane_edit(uint64_t pos, const std::vector<char> &ref, const std::vector<char> &alt)
{
	Edit k{};
	const uint64_t nr = ref.size(), na = alt.size();
	k.s = vh_suffix(ref.data(), nr, alt.data(), na);
	k.p = vh_prefix(ref.data(), nr, alt.data(), na, k.s);
	k.e = vh_edit(pos, nr, na, k.s, k.p);
	k.hash = vh_edit_hash(k.e.bs, k.e.be, k.e.t_len, vm_text_hash(alt.data() + k.p, na - k.s - k.p));
	return k;
}
// the edit as tier_items_wave of hip/vcf_pair.hpp computes it: the same calls, the wave emulated
static Edit wave_edit(uint64_t pos, const std::vector<char> &ref, const std::vector<char> &alt)
{
	Edit k{};
	const EmuWave w;
	const uint64_t nr = ref.size(), na = alt.size();
	const auto limit = [](uint64_t a, uint64_t b) { return vh_trim_limit(a, b); };
	k.s = wave_suffix(ref.data(), nr, alt.data(), na, limit, w);
	k.p = wave_prefix(ref.data(), nr, alt.data(), na, k.s, limit, w);
	k.e = vh_edit(pos, nr, na, k.s, k.p);
	k.hash = vh_edit_hash(k.e.bs, k.e.be, k.e.t_len, wave_text_hash(alt.data() + k.p, na - k.s - k.p, w));
	return k;
}

// the reach as k_vh_reach runs it: `limit` = max_reach + 1 steps at the most, 64 a ballot
static void do_reach(const std::vector<char> &path, uint64_t s0, uint64_t e0, const std::vector<char> &unit, uint64_t max_reach)
{
	const uint64_t limit = max_reach + 1, plen = path.size(), m = unit.size();
	const EmuWave w;
	const uint64_t kr = wave_first(limit, w, [&](uint64_t x) { return !(e0 + x < plen && vh_reach_right_ok(unit.data(), m, x, (uint8_t)path[e0 + x])); });
	const uint64_t kl = wave_first(limit, w, [&](uint64_t x) { return !(x < s0 && vh_reach_left_ok(unit.data(), m, x, (uint8_t)path[s0 - 1 - x])); });
	printf("%llu %llu %d\n", (unsigned long long)std::min(kl, max_reach), (unsigned long long)std::min(kr, max_reach), kl > max_reach || kr > max_reach ? 1 : 0);
}

// the conflicts as side_conflict runs them: chunks of 64 lanes, an inclusive maximum of the ends, a carry
static bool chunked_conflict(const std::vector<uint64_t> &bs, const std::vector<uint64_t> &be)
{
	const size_t n = bs.size();
	uint64_t carry_end = 0, carry_bs = 0, carry_be = 0;
	for (size_t c0 = 0; c0 < n; c0 += 64) {
		uint64_t incl[64], s[64], e[64];
		for (size_t l = 0; l < 64; l++) {
			s[l] = c0 + l < n ? bs[c0 + l] : 0, e[l] = c0 + l < n ? be[c0 + l] : 0;
			incl[l] = std::max(e[l], l ? incl[l - 1] : 0);
		}
		const uint64_t hit = EmuWave{}.ballot([&](uint32_t l) {
			const uint64_t before = std::max(l ? incl[l - 1] : 0, carry_end);
			return c0 + l < n && vh_conflict(s[l], e[l], c0 + l > 0, before, l ? s[l - 1] : carry_bs, l ? e[l - 1] : carry_be);
		});
		if (hit)
			return true;
		carry_end = std::max(carry_end, incl[63]), carry_bs = s[63], carry_be = e[63];
	}
	return false;
}

int main()
{
	static const char *STATUS[] = {"inconsistent", "nocall_a", "nocall_b", "unspelled_a", "unspelled_b", "conflict_a", "conflict_b", "equal_ref", "equal", "differ"};
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream ls(line);
		std::string cmd;
		ls >> cmd;
		if (cmd == "edit") {
			uint64_t pos = 0;
			std::string ref, alt;
			ls >> pos >> ref >> alt;
			const std::vector<char> r = exact(text_of(ref)), a = exact(text_of(alt));
			const Edit l = lane_edit(pos, r, a), w = wave_edit(pos, r, a);
			if (l.s != w.s || l.p != w.p || l.hash != w.hash || l.e.bs != w.e.bs || l.e.be != w.e.be || l.e.t_len != w.e.t_len) {
				fprintf(stderr, "vcfhap_check: the lane and the wave disagree on %s\n", line.c_str());
				return 1;
			}
			std::string t;
			for (uint64_t i = 0; i < l.e.t_len; i++)
				t += (char)vm_fold(a[l.e.t_at + i]);
			printf("%lld %lld %llu %llu %s %016llx\n", (long long)l.e.bs - 1, (long long)l.e.be - 1, (unsigned long long)l.s, (unsigned long long)l.p,
			       t.empty() ? "_" : t.c_str(), (unsigned long long)l.hash);
		} else if (cmd == "reach") {
			std::string path, unit;
			uint64_t s = 0, e = 0, most = 0;
			ls >> path >> s >> e >> unit >> most;
			do_reach(exact(text_of(path)), s, e, exact(unit), most);
		} else if (cmd == "heads") {
			size_t n = 0;
			ls >> n;
			std::vector<uint32_t> mark(n);
			for (uint32_t &m : mark)
				ls >> m;
			uint32_t reached = 0; // the exclusive running maximum
			std::string out;
			for (size_t k = 0; k < n; k++) {
				out += vh_window_head(reached, (uint32_t)k) ? "1" : "0";
				reached = std::max(reached, mark[k]);
			}
			printf("%s\n", out.empty() ? "_" : out.c_str());
		} else if (cmd == "conflict") {
			size_t n = 0;
			ls >> n;
			std::vector<uint64_t> bs(n), be(n);
			for (size_t k = 0; k < n; k++) {
				ls >> bs[k] >> be[k];
				bs[k] += 1, be[k] += 1; // (as the device keeps them)
			}
			printf("%d\n", chunked_conflict(bs, be) ? 1 : 0);
		} else if (cmd == "hap") {
			std::string text_token;
			uint64_t lo = 0;
			size_t n = 0;
			ls >> text_token >> lo >> n;
			const std::vector<char> text = exact(text_of(text_token));
			std::vector<uint64_t> s(n), e(n), start(n);
			std::vector<std::vector<char>> t(n);
			uint64_t change = 0; // modulo 2^64
			for (size_t k = 0; k < n; k++) {
				std::string tt;
				ls >> s[k] >> e[k] >> tt;
				t[k] = exact(text_of(tt));
				start[k] = s[k] - lo + change;
				change += (uint64_t)t[k].size() - (e[k] - s[k]);
			}
			const uint64_t len = text.size() + change;
			std::string out;
			for (uint64_t h = 0; h < len; h++) {
				const uint32_t k = vh_locate(h, (uint32_t)n, [&](uint32_t u) { return start[u]; });
				const VhSource src = k == n ? vh_source(h, true, 0, 0, 0) : vh_source(h, false, start[k], t[k].size(), e[k] - lo);
				out += (char)vm_fold(src.from_edit ? t[k][src.at] : text[src.at]);
			}
			printf("%s\n", out.empty() ? "_" : out.c_str());
		} else if (cmd == "status") {
			int f[7] = {0};
			for (int &x : f)
				ls >> x;
			const uint8_t st = vh_status(f[0], f[1], f[2], f[3], f[4], f[5], f[6]);
			printf("%s\n", st == VH_COMPARE ? "compare" : STATUS[st]);
		} else if (cmd == "compared") {
			int equal = 0;
			uint32_t ea = 0, eb = 0;
			ls >> equal >> ea >> eb;
			printf("%s\n", STATUS[vh_compared(equal, ea, eb)]);
		} else if (!cmd.empty()) {
			fprintf(stderr, "vcfhap_check: unknown block %s\n", cmd.c_str());
			return 1;
		}
	}
	printf("vcfhap_check: ok\n");
	return 0;
}
