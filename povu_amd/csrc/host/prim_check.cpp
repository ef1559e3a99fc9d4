// prim_check.cpp -- the aligner of the `decomposed` profile (hip/prim_align.hpp) on the CPU, built with -fsanitize=address,undefined
// (make prim_check; run by tests/test_prim_core.py).  One wave is 64 lane states stepped in lockstep: a step first reads what
// every left neighbour handed on at the step before (the device's one shuffle is this array read), then steps every lane.
// Both tiers run as prim_kernels.hip runs them: the register words of tier 1, the stripes, the column between stripes and
// the slab of codes of tier 2 are plain arrays here, every index checked before it is used.
//
// stdin: lines `REF ALT POS CONTEXT_BASE CAP [ONE_ALT]`, an empty text written `.`; CONTEXT_BASE is the reference path's base in
// front of POS (`.` when POS is 1); ONE_ALT 1 applies the _ROW_RAW rule of a record with one ALT.  --force-tier2: every aligned
// pair through the striped sweep.  stdout, per line: `pair <cells> <tier> <rows>` and then per row
// `kind reason index pos ref_start ref_len alt_start alt_len lead` (lead `.` for none).
#include "../hip/prim_align.hpp"

#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace pa = prim_align;

#define CHECK(cond)                                                                        \
	do {                                                                               \
		if (!(cond)) {                                                             \
			fprintf(stderr, "prim_check: %s failed (line %d)\n", #cond, __LINE__); \
			abort();                                                           \
		}                                                                          \
	} while (0)

namespace
{
struct Wave {
	std::array<pa::Lane, pa::LANES> lane{};
	// what the shuffle up by one gives every lane: the `out` of its left neighbour before this step (lane 0: its own)
	std::array<uint32_t, pa::LANES> shuffled_up() const
	{
		std::array<uint32_t, pa::LANES> in{};
		for (uint32_t l = 0; l < pa::LANES; l++)
			in[l] = lane[l ? l - 1 : 0].out;
		return in;
	}
};

// tier 1: one stripe, the codes in two words a lane
template <class Sink>
void align_tier1(const std::string &a, const std::string &b, Sink &sink)
{
	const uint32_t n = (uint32_t)a.size(), m = (uint32_t)b.size();
	CHECK(n >= 1 && m >= 1 && n <= pa::TIER1_MAX && m <= pa::TIER1_MAX);
	std::array<uint8_t, pa::LANES> areg{}, breg{};
	std::array<std::array<uint64_t, 2>, pa::LANES> w{};
	for (uint32_t l = 0; l < pa::LANES; l++) {
		areg[l] = l < n ? pa::upper((uint8_t)a[l]) : 0;
		breg[l] = l < m ? pa::upper((uint8_t)b[l]) : 0;
	}
	Wave wave;
	const uint32_t steps = n + m + 1;
	for (uint32_t t = 0; t < steps; t++) {
		std::array<uint32_t, pa::LANES> in = wave.shuffled_up();
		const uint32_t row = t < n ? t : n; // (lane 0 has no cell behind row n)
		in[0] = pa::pack(row, row ? areg[row - 1] : 0);
		for (uint32_t l = 0; l < pa::LANES; l++) {
			const pa::Flush f = pa::lane_step(wave.lane[l], t, l, n, l < m, l + 1, breg[l], in[l]);
			if (f.full) {
				CHECK(f.index < 2);
				w[l][f.index] = f.word;
			}
		}
	}
	uint32_t i = n, j = m;
	pa::Run run;
	const uint32_t trace = n + m;
	for (uint32_t k = 0; k < trace; k++) {
		if (i == 0 && j == 0)
			break;
		const uint32_t ii = i ? i - 1 : 0, jj = j ? j - 1 : 0;
		CHECK(ii < pa::LANES && jj < pa::LANES);
		const uint64_t word = w[jj][ii / pa::WORD_ROWS];
		const pa::TraceStep s = pa::trace_step(pa::code_of(word, ii + 1), i, j, areg[ii] != breg[jj]);
		i = s.i, j = s.j;
		pa::feed(run, s.col, i, j, sink);
	}
	CHECK(i == 0 && j == 0);
	pa::close_run(run, sink);
}

// tier 2: stripes of 64 columns, the last column of a stripe handed to the next through `col`, the codes in a slab
template <class Sink>
void align_tier2(const std::string &a, const std::string &b, Sink &sink)
{
	const uint32_t n = (uint32_t)a.size(), m = (uint32_t)b.size();
	CHECK(n >= 1 && m >= 1 && n <= pa::MAX_LENGTH && m <= pa::MAX_LENGTH);
	std::vector<uint8_t> sa(pa::MAX_LENGTH), sb(pa::MAX_LENGTH);
	std::vector<uint16_t> col(pa::MAX_LENGTH + 1);
	for (uint32_t x = 0; x < n; x++)
		sa[x] = pa::upper((uint8_t)a[x]);
	for (uint32_t x = 0; x < m; x++)
		sb[x] = pa::upper((uint8_t)b[x]);
	const uint64_t words = pa::slab_words(n, m);
	CHECK(words * 8 <= 64 * 1024);
	std::vector<uint64_t> slab(words);
	const uint32_t n_stripes = pa::stripes(m);
	for (uint32_t st = 0; st < n_stripes; st++) {
		const uint32_t c0 = st * pa::LANES, width = m - c0 < pa::LANES ? m - c0 : pa::LANES;
		Wave wave;
		const uint32_t steps = n + width + 1;
		for (uint32_t t = 0; t < steps; t++) {
			std::array<uint32_t, pa::LANES> in = wave.shuffled_up();
			const uint32_t row = t < n ? t : n;
			CHECK(row < col.size());
			in[0] = pa::pack(st ? col[row] : row, row ? sa[row - 1] : 0);
			for (uint32_t l = 0; l < pa::LANES; l++) {
				const bool live = l < width;
				const pa::Flush f = pa::lane_step(wave.lane[l], t, l, n, live, c0 + l + 1, live ? sb[c0 + l] : 0, in[l]);
				if (f.full) {
					const uint64_t at = pa::slab_index(st, n, f.index, l);
					CHECK(at < words);
					slab[at] = f.word;
				}
				if (l == pa::LANES - 1 && live && t >= l && t - l <= n) { // the stripe's last column, for the next stripe
					CHECK(t - l < col.size());
					col[t - l] = (uint16_t)wave.lane[l].up;
				}
			}
		}
	}
	uint32_t i = n, j = m;
	pa::Run run;
	const uint32_t trace = n + m;
	for (uint32_t k = 0; k < trace; k++) {
		if (i == 0 && j == 0)
			break;
		const uint32_t ii = i ? i - 1 : 0, jj = j ? j - 1 : 0;
		const uint64_t at = pa::slab_index(jj / pa::LANES, n, ii / pa::WORD_ROWS, jj % pa::LANES);
		CHECK(at < words && ii < n && jj < m);
		const pa::TraceStep s = pa::trace_step(pa::code_of(slab[at], ii + 1), i, j, sa[ii] != sb[jj]);
		i = s.i, j = s.j;
		pa::feed(run, s.col, i, j, sink);
	}
	CHECK(i == 0 && j == 0);
	pa::close_run(run, sink);
}

template <class Sink>
void align(uint32_t tier, const std::string &a, const std::string &b, Sink &sink)
{
	if (tier == 1)
		align_tier1(a, b, sink);
	else
		align_tier2(a, b, sink);
}

struct Writer {
	std::vector<pa::Row> rows;
	std::vector<bool> set;
	uint8_t context;
	void put(uint32_t slot, pa::Row r)
	{
		CHECK(slot < rows.size() && !set[slot]);
		if (r.context)
			r.lead = context;
		rows[slot] = r, set[slot] = true;
	}
};

void print_row(const pa::Row &r)
{
	printf("%u %u %u %llu %u %u %u %u %c\n", r.kind, r.reason, r.index, (unsigned long long)r.pos, r.ref_start, r.ref_len, r.alt_start, r.alt_len,
	       r.lead ? (char)r.lead : '.');
}
} // namespace

int main(int argc, char **argv)
{
	bool force_tier2 = false;
	for (int k = 1; k < argc; k++) {
		if (!strcmp(argv[k], "--force-tier2")) {
			force_tier2 = true;
		} else {
			fprintf(stderr, "usage: prim_check [--force-tier2] < lines of `REF ALT POS CONTEXT_BASE CAP [ONE_ALT]`\n");
			return 2;
		}
	}
	std::string line;
	while (std::getline(std::cin, line)) {
		if (line.empty())
			continue;
		std::istringstream is(line);
		std::string ref, alt, ctx;
		unsigned long long pos = 0;
		uint32_t cap = 0, one_alt = 0;
		if (!(is >> ref >> alt >> pos >> ctx >> cap) || ctx.size() != 1 || !cap || cap > pa::MAX_LENGTH) {
			fprintf(stderr, "prim_check: bad line: %s\n", line.c_str());
			return 2;
		}
		is >> one_alt;
		if (ref == ".")
			ref.clear();
		if (alt == ".")
			alt.clear();
		const uint32_t reason = pa::unaligned_reason(false, ref.size(), alt.size(), cap);
		if (reason) {
			printf("pair 0 0 1\n");
			print_row(pa::whole_row(reason, pos, (uint32_t)ref.size(), (uint32_t)alt.size()));
			continue;
		}
		const uint32_t n = (uint32_t)ref.size(), m = (uint32_t)alt.size(), tier = pa::tier_of(n, m, force_tier2);
		pa::CountSink count;
		align(tier, ref, alt, count);
		const pa::Counted c = pa::counted(count, pos, one_alt != 0, ref.data(), n, alt.data(), m);
		printf("pair %llu %u %u\n", (unsigned long long)(n + 1) * (m + 1), tier, c.n_rows);
		if (c.reason) {
			print_row(pa::whole_row(c.reason, pos, n, m));
			continue;
		}
		Writer w{std::vector<pa::Row>(c.n_rows), std::vector<bool>(c.n_rows, false), ctx == "." ? (uint8_t)0 : (uint8_t)ctx[0]};
		pa::EmitSink<Writer> emit(w, c, pos, ref.data());
		align(tier, ref, alt, emit);
		CHECK(emit.seen == c.n_rows);
		for (const pa::Row &r : w.rows)
			print_row(r);
	}
	return 0;
}
