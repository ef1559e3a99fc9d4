// merge_kernels.hip -- equal primitives of a decomposed call merged into one row with joint genotypes (POVU_HIP_T_MERGE).
//
// The definition is this project's own (INTEGRATION.md "Merged primitives"; restated in tests/merge_ref.py); what a member says
// about a slot is prim_merge.hpp, which host/merge_check.cpp runs on the CPU.  The step reads what prim_rows left on the device:
// the sorted rows, the rows before the sort with the stretch of every (record, ALT) among them, the spelled bytes and the GT rows:
//   keys    a lane per row: the dense number of its (reference, POS) run (head flags and a scan over the sorted rows), its two
//           written lengths, a 64-bit hash of its upper-cased written texts; a row kept whole gets a hash of its own index and
//           equals no row;
//   groups  exact_groups.hpp over those keys, the comparison byte for byte over the spelled texts; the groups numbered by a
//           scan over their first members, hence in the order of the representatives among the rows; the member list is the
//           rows stably sorted by that number, the offsets the heads of its runs;
//   votes   one wave per group, a lane per sample (its slots are consecutive), a loop over the members; another ALT of a
//           member's record is looked up among the rows before the sort, where its rows ascend, by bisection.
// The rules at the head of prim_kernels.hip hold here too: trip counts are fixed before the loop, no kernel waits for another
// wave, every shuffle runs with all 64 lanes, every store is checked against the range the host carved.
#include "merge_kernels.hpp"

#include "exact_groups.hpp"
#include "prim_align.hpp"
#include "prim_merge.hpp"

namespace povu_hip
{

namespace
{

namespace pa = prim_align;
namespace pm = prim_merge;

constexpr int WAVES = Q_TPB / 64;
constexpr unsigned LEN_BITS = 10; // a written text of a primitive row has at most POVU_HIP_PRIM_MAX_LENGTH + 1 bytes
// words[]: what the vote tells the host
enum { W_GROUPS = 0, W_MEMBERS, W_REF_CONSISTENT, W_CONFLICTS, W_WORDS = 8 };

// the written texts of the sorted rows, over the spelled bytes
struct RowTexts {
	const uint32_t *record, *alt, *ref_start, *ref_len, *alt_start, *alt_len;
	const uint8_t *kind, *lead;
	const uint32_t *ref_allele, *block;
	const uint64_t *ref_spelled, *block_off, *sp_off;
	const char *seq;
	struct Text {
		const char *p;
		uint32_t n; // written bytes, the lead counted
		uint8_t lead;
		__device__ __forceinline__ uint8_t at(uint32_t i) const { return pa::upper(lead ? (i ? (uint8_t)p[i - 1] : lead) : (uint8_t)p[i]); }
	};
	__device__ __forceinline__ Text ref(uint32_t x) const
	{
		const uint8_t l = lead[x];
		return {seq + sp_off[ref_spelled[record[x]]] + ref_start[x], ref_len[x] + (l ? 1u : 0u), l};
	}
	__device__ __forceinline__ Text alt_text(uint32_t x) const
	{
		const uint32_t j = record[x], k = alt[x], ra = ref_allele[j];
		const uint8_t l = lead[x];
		return {seq + sp_off[block_off[block[j]] + (k - 1 < ra ? k - 1 : k)] + alt_start[x], alt_len[x] + (l ? 1u : 0u), l};
	}
	__device__ __forceinline__ bool whole(uint32_t x) const { return kind[x] == pa::ROW_PASS; }
};

// head of a (reference, POS) run of the sorted rows; flag[n] = 0
__global__ void k_mg_heads(uint32_t n, const uint32_t *__restrict__ record, const uint64_t *__restrict__ pos, PrimIn I, uint32_t *__restrict__ flag)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x <= n; x += (uint64_t)gridDim.x * Q_TPB) {
		bool head = x == 0;
		if (x && x < n)
			head = pos[x] != pos[x - 1] || I.ref.ref_of_path[I.path[record[x]]] != I.ref.ref_of_path[I.path[record[x - 1]]];
		flag[x] = x < n && head;
	}
}

__device__ __forceinline__ uint64_t hash_text(uint64_t h, const RowTexts::Text &t)
{
	const uint32_t n = t.n;
	for (uint32_t i = 0; i < n; i++)
		h = mix64(h ^ t.at(i));
	return mix64(h ^ 0x100u); // (no byte: the end of a text)
}

// the keys of every row: run, lengths, hash
__global__ void k_mg_keys(uint32_t n, RowTexts T, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ run_before, uint32_t mask_hi,
			  uint32_t mask_lo, uint32_t *__restrict__ rq, uint32_t *__restrict__ rlen, uint64_t *__restrict__ rhash)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x < n; x += (uint64_t)gridDim.x * Q_TPB) {
		rq[x] = run_before[x] + flag[x] - 1;
		uint64_t h;
		if (T.whole((uint32_t)x)) {
			rlen[x] = 0;
			h = mix64(x + 1);
		} else {
			const RowTexts::Text a = T.ref((uint32_t)x), b = T.alt_text((uint32_t)x);
			const uint32_t top = (1u << LEN_BITS) - 1;
			rlen[x] = (min(a.n, top) << LEN_BITS) | min(b.n, top);
			h = hash_text(hash_text(0x9e3779b97f4a7c15ull, a), b);
		}
		rhash[x] = h & (((uint64_t)mask_hi << 32) | mask_lo);
	}
}

// rows a and b of one (reference, POS) run are equal: neither kept whole, the same written texts after upper-casing
struct SameRow {
	RowTexts T;
	__device__ __forceinline__ bool operator()(uint32_t a, uint32_t b) const
	{
		if (T.whole(a) || T.whole(b))
			return false;
		const RowTexts::Text ra = T.ref(a), rb = T.ref(b), aa = T.alt_text(a), ab = T.alt_text(b);
		if (ra.n != rb.n || aa.n != ab.n)
			return false;
		bool same = true;
		const uint32_t nr = ra.n, na = aa.n;
		for (uint32_t i = 0; i < nr; i++)
			same &= ra.at(i) == rb.at(i);
		for (uint32_t i = 0; i < na; i++)
			same &= aa.at(i) == ab.at(i);
		return same;
	}
};

__global__ void k_mg_group_key(uint32_t n, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ gid, uint32_t *__restrict__ key)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x < n; x += (uint64_t)gridDim.x * Q_TPB)
		key[x] = gid[perm[x]];
}

// the member list (the rows sorted by group) and where every group begins in it
__global__ void k_mg_members(uint32_t n, uint32_t n_mrows, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ gid,
			     uint32_t *__restrict__ member, uint64_t *__restrict__ off)
{
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x <= n; x += (uint64_t)gridDim.x * Q_TPB) {
		if (x == n) {
			off[n_mrows] = n;
			continue;
		}
		const uint32_t r = sorted[x], g = gid[r];
		member[x] = r;
		if ((x == 0 || gid[sorted[x - 1]] != g) && g < n_mrows)
			off[g] = x;
	}
}

struct VoteIn {
	PrimIn I;
	PrimPre pre;
	uint64_t n_pre; // rows before the sort
	const uint32_t *record, *alt, *ref_len;
	const uint8_t *kind, *lead;
	const uint64_t *pos;
};
struct VoteOut {
	uint64_t n_mrows, n_rows;
	const uint64_t *off;
	const uint32_t *member;
	uint8_t *gt;
	uint32_t *ac, *an, *ns;
	unsigned long long *words;
};

// one wave per group, a lane per sample
__global__ __launch_bounds__(Q_TPB) void k_mg_vote(VoteIn V, VoteOut o)
{
	const PrimIn &I = V.I;
	const uint32_t lane = threadIdx.x & 63u, S = I.slots.S, n_samples = I.slots.NS;
	const uint32_t *__restrict__ slot_first = I.slots.slot_first;
	const pm::Rows pre{V.pre.pos, V.pre.ref_len, V.pre.lead};
	const uint64_t waves = (uint64_t)gridDim.x * WAVES;
	for (uint64_t gi = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); gi < o.n_mrows; gi += waves) {
		const uint64_t m1 = min(o.off[gi + 1], o.n_rows), m0 = min(o.off[gi], m1 ? m1 - 1 : 0); // (a group has a member)
		const uint32_t first = o.member[m0];
		const uint64_t a = V.pos[first], b = pm::span_end(a, V.ref_len[first], V.lead[first]);
		const bool rule = V.kind[first] != pa::ROW_PASS;
		uint32_t ac = 0, an = 0, ns = 0, n_cons = 0, n_conf = 0;
		for (uint32_t sm = lane; sm < n_samples; sm += 64) {
			bool any = false;
			const uint32_t s0 = slot_first[sm], s1 = min(slot_first[sm + 1], S);
			for (uint32_t sl = s0; sl < s1; sl++) {
				pm::Tally tally;
				for (uint64_t m = m0; m < m1; m++) {
					const uint32_t x = o.member[m], j = V.record[x], k = V.alt[x];
					const uint64_t p0 = I.ac_off[j], n_alts = I.ac_off[j + 1] - p0;
					const uint32_t v = pm::vote(I.gt[(uint64_t)j * S + sl], k, (uint32_t)n_alts, rule, pre, a, b, [&](uint32_t other) {
						const uint64_t p = p0 + other - 1, lo = V.pre.row_off[p], hi = V.pre.row_off[p + 1];
						return pm::OtherAlt{V.pre.reason[p] == 0 && hi <= V.n_pre, lo, hi};
					});
					pm::cast(tally, v);
				}
				const uint8_t value = pm::slot_value(tally);
				o.gt[gi * S + sl] = value; // (gi < n_mrows and sl < S: inside the n_mrows * S bytes)
				any |= value != pm::SLOT_MISSING;
				an += value != pm::SLOT_MISSING;
				ac += value == 1;
				n_cons += pm::ref_consistent(tally);
				n_conf += pm::conflict(tally);
			}
			ns += any;
		}
		ac = wave_sum(ac), an = wave_sum(an), ns = wave_sum(ns), n_cons = wave_sum(n_cons), n_conf = wave_sum(n_conf);
		if (lane == 0) {
			o.ac[gi] = ac, o.an[gi] = an, o.ns[gi] = ns;
			if (m1 - m0 > 1) {
				atomicAdd(o.words + W_GROUPS, 1ull);
				atomicAdd(o.words + W_MEMBERS, (unsigned long long)(m1 - m0));
			}
			if (n_cons)
				atomicAdd(o.words + W_REF_CONSISTENT, (unsigned long long)n_cons);
			if (n_conf)
				atomicAdd(o.words + W_CONFLICTS, (unsigned long long)n_conf);
		}
	}
}

} // namespace

MergedRows merge_rows(povu_hip_ctx *ctx, const PrimIn &in, const PrimRows &rows)
{
	hipStream_t s = ctx->stream;
	MergedRows out;
	const uint32_t n = (uint32_t)rows.n_rows, S = in.slots.S, hbits = hash_bits_hook(); // (prim_rows refused 2^32 rows)
	const size_t n1 = (size_t)n + 1;
	uint32_t *flag, *run_before, *rq, *rlen, *firstf, *gidx, *gid, *count;
	uint64_t *rhash;
	unsigned long long *splits;
	GroupWs gw;
	gw.tmp_bytes = prim_tmp_bytes(n1, true) + 256;
	carve(ctx->mg_ws, [&](Spans &take) {
		take(n1, flag, run_before, rq, rlen, firstf, gidx, gid, gw.pa, gw.pb, gw.key, gw.kout, gw.mark, gw.hmax, gw.head, gw.rep, gw.blist);
		take(n1, rhash);
		take(n1, gw.rbad);
		take(2, count);
		take(1, splits);
		take(gw.tmp_bytes, gw.tmp);
	});
	if (n) {
		const RowTexts T{rows.record,	rows.alt, rows.ref_start, rows.ref_len,	  rows.alt_start, rows.alt_len, rows.kind,
				 rows.lead,	in.ref_allele, in.block,  in.ref_spelled, in.block_off,	  in.sp_off,	in.seq};
		// ---- keys
		KLAUNCH(k_mg_heads, dim3(stride_blocks(n1)), dim3(Q_TPB), 0, s, n, rows.record, rows.pos, in, flag);
		scan_exclusive_u32(flag, run_before, n1, gw.tmp, gw.tmp_bytes, s);
		KLAUNCH(k_mg_keys, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, T, flag, run_before, hash_mask_hi(hbits), hash_mask_lo(hbits), rq, rlen, rhash);
		// ---- groups (a run number is below n)
		const uint32_t *sp = group_exact(n, rq, rlen, rhash, hbits, 2 * LEN_BITS, bits_for(n), SameRow{T}, gw, count, splits, &out.n_splits, s);
		number_groups(n, sp, gw.rep, firstf, gidx, nullptr, gw.tmp, gw.tmp_bytes, s);
		out.n_mrows = read_back(gidx + n, s); // (waits for the stream: n_splits has arrived)
		KLAUNCH(k_eg_group_of, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, sp, gw.rep, gidx, nullptr, gid);
	}
	const uint64_t nm = out.n_mrows;
	refuse_2_32(nm * S, "the merged primitives need ", "(group, slot) entries");
	unsigned long long *words;
	carve(ctx->mg_rows, [&](Spans &take) {
		take(nm + 1, out.off);
		take(n1, out.member);
		take(nm * S + 1, out.gt);
		take(nm + 1, out.ac, out.an, out.ns);
		take(W_WORDS, words);
	});
	if (!n) {
		HIP_CHECK(hipMemsetAsync(out.off, 0, 8, s)); // (no rows: no merged rows, the one offset)
		return out;
	}
	// ---- members: the rows stably sorted by group, so those of a group stay in row order
	launch_iota(n, gw.pa, s);
	LsdSort sort{gw.pa, gw.pb, gw.key, gw.kout, n, gw.tmp, gw.tmp_bytes, s};
	sort.pass(0, bits_for(nm), [&](int, const uint32_t *cur, uint32_t *k) { KLAUNCH(k_mg_group_key, dim3(stride_blocks(n)), dim3(Q_TPB), 0, s, n, cur, gid, k); });
	KLAUNCH(k_mg_members, dim3(stride_blocks(n1)), dim3(Q_TPB), 0, s, n, (uint32_t)nm, sort.cur, gid, out.member, out.off);
	// ---- votes
	HIP_CHECK(hipMemsetAsync(words, 0, W_WORDS * 8, s));
	const VoteIn V{in, rows.pre, rows.n_rows, rows.record, rows.alt, rows.ref_len, rows.kind, rows.lead, rows.pos};
	const VoteOut O{nm, rows.n_rows, out.off, out.member, out.gt, out.ac, out.an, out.ns, words};
	KLAUNCH(k_mg_vote, dim3(wave_blocks(nm)), dim3(Q_TPB), 0, s, V, O);
	unsigned long long h_words[W_WORDS] = {};
	HIP_CHECK(copy_async(h_words, words, W_WORDS * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	out.n_groups = h_words[W_GROUPS], out.n_members = h_words[W_MEMBERS];
	out.n_ref_consistent = h_words[W_REF_CONSISTENT], out.n_conflicts = h_words[W_CONFLICTS];
	return out;
}

} // namespace povu_hip
