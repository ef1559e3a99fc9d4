// untangle_check.cpp -- the rules of the untangled calls (hip/untangle_rules.hpp) on the CPU, built with
// -fsanitize=address,undefined (make untangle_check; run by tests/test_untangle_core.py).  One wave is 64 lane states stepped
// in lockstep, as untangle_kernels.hip steps them: a step first reads what every left neighbour handed on at the step before
// (the device's one shuffle is this array read), then steps every lane; the traceback reads the words of the codes from the
// lane that owns the column.  Every index is checked before it is used.
//
// argv[1]: a file of lines `n m a_0 .. a_{n-1} b_0 .. b_{m-1}` (lap sequences as allele numbers, b already oriented), both
// lengths 1 .. 64.  stdout, per line: `partner_0 .. partner_{n-1} | extra` with `-` for a row without a partner.
#include "../hip/untangle_rules.hpp"

#include <array>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

namespace pa = prim_align;
namespace un = untangle;

#define CHECK(cond)                                                                            \
	do {                                                                                   \
		if (!(cond)) {                                                                 \
			fprintf(stderr, "untangle_check: %s failed (line %d)\n", #cond, __LINE__); \
			abort();                                                               \
		}                                                                              \
	} while (0)

namespace
{
void rules()
{
	CHECK(un::entry_state(3, false, 0, 1, 1, 2, false) == un::ENTRY_TASK && un::entry_state(1, false, 0, 1, 1, 1, false) == un::ENTRY_TRIVIAL);
	CHECK(un::entry_state(1, false, 0, 1, 1, 2, false) == un::ENTRY_TASK && un::entry_state(64, false, 0, 1, 1, 64, false) == un::ENTRY_TASK);
	CHECK(un::entry_state(65, false, 0, 1, 1, 3, false) == un::ENTRY_OLD && un::entry_state(64, false, 0, 1, 1, 65, false) == un::ENTRY_OLD);
	CHECK(un::entry_state(3, true, 0, 1, 1, 2, false) == un::ENTRY_OLD && un::entry_state(3, false, 0, 1, 1, 2, true) == un::ENTRY_OLD);
	CHECK(un::entry_state(3, false, 1, 1, 1, 2, false) == un::ENTRY_OLD && un::entry_state(3, false, 0, 1, 2, 2, false) == un::ENTRY_OLD);
	CHECK(un::entry_state(3, false, 0, 1, 0, 0, false) == un::ENTRY_OLD);
	CHECK(un::oriented_lap(0, 4, true) == 3 && un::oriented_lap(3, 4, true) == 0 && un::oriented_lap(2, 4, false) == 2);
	CHECK(un::code_of_allele(2, 2) == 0 && un::code_of_allele(0, 2) == 1 && un::code_of_allele(3, 2) == 3);
	CHECK(un::packed_value(un::pack(128, 65534)) == 128 && un::packed_symbol(un::pack(128, 65534)) == 65534);
}

void align(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b)
{
	const uint32_t n = (uint32_t)a.size(), m = (uint32_t)b.size();
	CHECK(n >= 1 && m >= 1 && n <= un::MAX_LAPS && m <= un::MAX_LAPS);
	std::array<uint32_t, pa::LANES> areg{}, breg{};
	for (uint32_t l = 0; l < pa::LANES; l++) {
		areg[l] = l < n ? a[l] : 0;
		breg[l] = l < m ? b[l] : 0;
	}
	std::array<un::Lane, pa::LANES> lane{};
	const uint32_t steps = n + m + 1;
	for (uint32_t t = 0; t < steps; t++) {
		std::array<uint32_t, pa::LANES> in{};
		for (uint32_t l = 0; l < pa::LANES; l++)
			in[l] = lane[l ? l - 1 : 0].out;
		const uint32_t row = t < n ? t : n; // (lane 0 has no cell behind row n)
		in[0] = un::pack(row, row ? areg[row - 1] : 0);
		for (uint32_t l = 0; l < pa::LANES; l++)
			un::lane_step(lane[l], t, l, n, l < m, breg[l], in[l]);
	}
	std::vector<uint8_t> partner(n, 0xEE);
	uint32_t i = n, j = m, extra = 0;
	const uint32_t trace = n + m;
	for (uint32_t k = 0; k < trace && (i || j); k++) {
		const uint32_t jj = j ? j - 1 : 0;
		CHECK(jj < pa::LANES && i <= n);
		const un::Trace ts = un::trace_step(un::word_of(lane[jj], i ? i : 1), i, j);
		if (ts.row_done) {
			CHECK(ts.row < n && partner[ts.row] == 0xEE);
			partner[ts.row] = ts.partner;
		}
		extra += ts.extra;
		i = ts.i, j = ts.j;
	}
	CHECK(i == 0 && j == 0);
	for (uint32_t r = 0; r < n; r++) {
		CHECK(partner[r] != 0xEE);
		if (partner[r] == un::NO_PARTNER)
			printf("- ");
		else
			printf("%u ", (unsigned)partner[r]);
	}
	printf("| %u\n", extra);
}
} // namespace

int main(int argc, char **argv)
{
	rules();
	if (argc < 2) {
		fprintf(stderr, "usage: untangle_check <cases>\n");
		return 2;
	}
	std::ifstream in(argv[1]);
	if (!in) {
		fprintf(stderr, "untangle_check: cannot read %s\n", argv[1]);
		return 2;
	}
	for (std::string ln; std::getline(in, ln);) {
		if (ln.empty())
			continue;
		std::istringstream is(ln);
		uint32_t n = 0, m = 0;
		is >> n >> m;
		CHECK(is && n >= 1 && m >= 1 && n <= un::MAX_LAPS && m <= un::MAX_LAPS);
		std::vector<uint32_t> a(n), b(m);
		for (auto &x : a)
			is >> x;
		for (auto &x : b)
			is >> x;
		CHECK(!is.fail());
		for (uint32_t x : a)
			CHECK(x <= 0xFFFFu);
		for (uint32_t x : b)
			CHECK(x <= 0xFFFFu);
		align(a, b);
	}
	printf("untangle_check: ok\n");
	return 0;
}
