// untangle_kernels.hip -- the untangled calls of povu_hip_call with POVU_HIP_T_UNTANGLE (include/povu_hip.h).
//
// The definition is this project's own ("Untangled calls (decided here, modelled on `ita::untangle`)";
// restated in tests/untangle_ref.py; the rules that need no wave live in untangle_rules.hpp).  Where a path walks a called
// site more than once its traversals ("laps") are contiguous in the traversal table, which is sorted by (site, path, first
// step).  The step runs behind the spelling, when every record has its row, and rewrites the rows of the looped sites:
//   lap runs    a lane a traversal; the first traversal of a (kept site, path) walks its run: every lap learns its run's
//               head, the head the lap count and whether the laps differ in direction; the (kept site, slot) cell takes the
//               number of traversing paths, the lowest head and the sum of the laps (atomics).  The heads of the record
//               paths' runs are compacted into the list of the reference runs;
//   task list   a lane per (reference run, slot) entry: its state (untangle::entry_state).  The entries that need an
//               alignment are compacted into the task list; a u64 scan of their row counts gives the offsets of partner[];
//   align       one wave per task, lane l owns column l + 1: n + m + 1 anti-diagonal steps with one __shfl_up each, the codes
//               in two 64-bit registers a lane, the traceback reading the words by __shfl; lane 0 writes partner[];
//   genotypes   AC of the candidate records (those whose reference run has an aligned entry) zeroed, then one wave per
//               flubble record, a lane per sample: the loop of k_cl_records with the aligned entries read from partner[];
//               lap, n_laps, lap_count and rec_unt for every flubble record.
//
// What cannot hang or leave its arrays: every trip count is fixed before its loop (a run ends at the table's end at the
// latest; the sweep takes n + m + 1 steps, the traceback at most n + m); no kernel waits on another wave; the shuffles run
// outside every divergent branch (the conditions around them are the same in all 64 lanes); a task or a record whose indices
// are not what the host listed is left alone by its whole wave and reported (W_BROKEN), and the call is refused.
#include "untangle_kernels.hpp"
#include "untangle_rules.hpp"

namespace povu_hip
{

namespace un = untangle;

namespace
{
constexpr uint32_t WAVES = Q_TPB / 64;
// workgroups of the wave-per-item kernels: enough to fill the device several times over, few enough that the counters, which
// every wave adds once, stay cheap; the waves stride over the items
inline unsigned wave_grid(size_t n) { return std::min(wave_blocks(n), 8192u); }
// the counter words
enum : uint32_t { W_MISSING = 0, W_EXTRA = 1, W_RECORDS = 2, W_FALLBACK = 3, W_BROKEN = 4, W_WORDS = 8 };

// the lap runs: per traversal the head of its run, per head the laps and whether they differ in direction; the cells
struct Runs {
	uint32_t R, S;
	uint32_t *head, *len; // [R]
	uint8_t *mixed;	      // [R]
	uint32_t *spaths, *shead, *slaps; // [nQ * S] paths of the slot that traverse the site, the lowest head, the laps
};
// the reference runs, the entries and the tasks
struct Tasks {
	uint32_t nRH, nT;
	const uint32_t *rh;   // [nRH] head traversal of every reference run, ascending
	uint32_t *rr_of;      // [R] reference run of a head traversal
	uint32_t *rr_any;     // [nRH] OR of the states of the run's entries
	uint8_t *state;	      // [nRH * S] untangle::ENTRY_*
	uint32_t *task_of;    // [nRH * S] task of an ENTRY_TASK entry
	const uint32_t *tl;   // [nT] entry of every task, ascending
	const uint64_t *poff; // [nT + 1] offsets into partner
	uint8_t *partner;
};
} // namespace

// ---- lap runs
__global__ void k_un_runs(Runs r, TravView T, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ qidx,
			  const uint32_t *__restrict__ slot_of_path, const uint32_t *__restrict__ on_ref, uint8_t *__restrict__ refflag)
{
	for (uint32_t t = blockIdx.x * Q_TPB + threadIdx.x; t < r.R; t += gridDim.x * Q_TPB) {
		const uint32_t q = T.rq[t], p = T.op[t];
		const bool head = keep[q] && (t == 0 || T.rq[t - 1] != q || T.op[t - 1] != p);
		refflag[t] = head && on_ref[p] != NO_QUERY;
		if (!head)
			continue;
		const uint8_t dir = T.orv[t];
		bool mixed = false;
		uint32_t e = t;
		for (; e < r.R && T.rq[e] == q && T.op[e] == p; e++) {
			r.head[e] = t;
			mixed |= T.orv[e] != dir;
		}
		r.len[t] = e - t;
		r.mixed[t] = mixed;
		const uint64_t cell = (uint64_t)qidx[q] * r.S + slot_of_path[p];
		atomicAdd(r.spaths + cell, 1u);
		atomicMin(r.shead + cell, t);
		atomicAdd(r.slaps + cell, e - t);
	}
}
__global__ void k_un_rr_of(uint32_t nRH, uint32_t R, const uint32_t *__restrict__ rh, uint32_t *__restrict__ rr_of)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < nRH; k += gridDim.x * Q_TPB)
		if (rh[k] < R)
			rr_of[rh[k]] = k;
}

// ---- task list: the state of every (reference run, slot) entry
__global__ void k_un_entries(Runs r, Tasks k, TravView T, const uint32_t *__restrict__ qidx, const uint32_t *__restrict__ slot_of_path,
			     uint8_t *__restrict__ tflag)
{
	const uint64_t X = (uint64_t)k.nRH * r.S;
	for (uint64_t x = (uint64_t)blockIdx.x * Q_TPB + threadIdx.x; x < X; x += (uint64_t)gridDim.x * Q_TPB) {
		const uint32_t rr = (uint32_t)(x / r.S), sl = (uint32_t)(x % r.S), h = k.rh[rr];
		uint8_t st = un::ENTRY_OLD;
		if (h < r.R) {
			const uint64_t cell = (uint64_t)qidx[T.rq[h]] * r.S + sl;
			const uint32_t sp = r.spaths[cell], hp = r.shead[cell];
			const bool one = sp == 1 && hp < r.R;
			st = un::entry_state(r.len[h], r.mixed[h] != 0, slot_of_path[T.op[h]], sl, sp, one ? r.len[hp] : 0, one && r.mixed[hp] != 0);
		}
		k.state[x] = st;
		tflag[x] = st == un::ENTRY_TASK;
		if (st != un::ENTRY_OLD)
			atomicOr(k.rr_any + rr, (uint32_t)st);
	}
}
__global__ void k_un_tasks(Runs r, Tasks k, uint64_t *__restrict__ pcnt)
{
	for (uint32_t x = blockIdx.x * Q_TPB + threadIdx.x; x <= k.nT; x += gridDim.x * Q_TPB) {
		uint64_t n = 0;
		if (x < k.nT) {
			const uint32_t e = k.tl[x], rr = e / r.S;
			k.task_of[e] = x;
			n = rr < k.nRH && k.rh[rr] < r.R ? r.len[k.rh[rr]] : 0;
		}
		pcnt[x] = n;
	}
}

// ---- align: one wave per task
__global__ __launch_bounds__(Q_TPB) void k_un_align(Runs r, Tasks k, TravView T, const uint32_t *__restrict__ oa, const uint32_t *__restrict__ qidx,
						    uint64_t partner_bytes, unsigned long long *__restrict__ words)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = (uint64_t)gridDim.x * WAVES;
	uint32_t missing = 0, extra = 0; // of the wave's tasks: one atomic each behind the loop, not one a task on one address
	for (uint64_t x = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); x < k.nT; x += waves) {
		// a task that is not what the host listed cannot be: the whole wave leaves it before any shuffle and the call is refused
		const uint32_t e = k.tl[x], rr = e / r.S, sl = e % r.S;
		const uint32_t h = rr < k.nRH ? k.rh[rr] : NO_QUERY;
		const uint32_t n = h < r.R ? r.len[h] : 0;
		const uint32_t hp = h < r.R ? r.shead[(uint64_t)qidx[T.rq[h]] * r.S + sl] : NO_QUERY;
		const uint32_t m = hp < r.R ? r.len[hp] : 0;
		const uint64_t p0 = k.poff[x];
		if (!n || !m || n > un::MAX_LAPS || m > un::MAX_LAPS || (uint64_t)h + n > r.R || (uint64_t)hp + m > r.R || p0 + n > partner_bytes) {
			if (lane == 0)
				atomicOr(words + W_BROKEN, 1ull);
			continue;
		}
		const bool flipped = T.orv[hp] != T.orv[h];
		const uint32_t areg = lane < n ? oa[h + lane] : 0, breg = lane < m ? oa[hp + un::oriented_lap(lane, m, flipped)] : 0;
		un::Lane s;
		const uint32_t steps = n + m + 1;
		for (uint32_t t = 0; t < steps; t++) {
			uint32_t in = __shfl_up(s.out, 1, 64);
			const uint32_t row = t < n ? t : n; // (lane 0 has no cell behind row n)
			const uint32_t a_row = __shfl(areg, (int)(row ? row - 1 : 0), 64);
			if (lane == 0)
				in = un::pack(row, row ? a_row : 0);
			un::lane_step(s, t, lane, n, lane < m, breg, in);
		}
		uint32_t i = n, j = m;
		const uint32_t trace = n + m;
		for (uint32_t c = 0; c < trace; c++) {
			if (i == 0 && j == 0)
				break;
			const unsigned long long mine = un::word_of(s, i ? i : 1);
			const uint64_t word = __shfl(mine, (int)((j ? j - 1 : 0) & 63u), 64);
			const un::Trace ts = un::trace_step(word, i, j);
			if (ts.row_done && ts.row < n) {
				if (lane == 0)
					k.partner[p0 + ts.row] = ts.partner;
				missing += ts.partner == un::NO_PARTNER;
			}
			extra += ts.extra;
			i = ts.i, j = ts.j;
		}
	}
	if (lane == 0) {
		if (missing)
			atomicAdd(words + W_MISSING, (unsigned long long)missing);
		if (extra)
			atomicAdd(words + W_EXTRA, (unsigned long long)extra);
	}
}

// ---- genotypes
// the reference run of sorted flubble record i0, NO_QUERY when its indices are not what the host listed
__device__ __forceinline__ uint32_t run_of_record(const Runs &r, const Tasks &k, const CallView &V, const uint32_t *__restrict__ perm, uint32_t i0,
						  uint32_t *t_out, uint32_t *h_out)
{
	const uint32_t j = perm[i0], t = j < V.nfl ? V.rlist[j] : NO_QUERY;
	const uint32_t h = t < r.R ? r.head[t] : NO_QUERY;
	const uint32_t rr = h < r.R && h <= t ? k.rr_of[h] : NO_QUERY;
	*t_out = t, *h_out = h;
	return rr < k.nRH ? rr : NO_QUERY;
}
__global__ __launch_bounds__(Q_TPB) void k_un_zero_ac(uint32_t nfl, uint32_t nrec, Runs r, Tasks k, CallView V, const uint32_t *__restrict__ perm,
						      const uint32_t *__restrict__ dst, const uint64_t *__restrict__ ac_off, uint32_t *__restrict__ ac)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * WAVES;
	for (uint32_t i0 = blockIdx.x * WAVES + (threadIdx.x >> 6); i0 < nfl; i0 += waves) {
		const uint32_t i = dst ? dst[i0] : i0;
		uint32_t t, h;
		const uint32_t rr = run_of_record(r, k, V, perm, i0, &t, &h);
		if (rr == NO_QUERY || i >= nrec || !k.rr_any[rr])
			continue;
		for (uint64_t a = ac_off[i] + lane; a < ac_off[i + 1]; a += 64)
			ac[a] = 0;
	}
}
// one wave per flubble record, a lane per sample (its slots are consecutive): k_cl_records' loop, the aligned entries from
// partner[]
__global__ __launch_bounds__(Q_TPB) void k_un_records(UntangleIn I, Runs r, Tasks k, UntangleRows out, unsigned long long *__restrict__ words)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * WAVES;
	const CallView &V = I.v;
	const uint32_t *__restrict__ slot_first = I.slots.slot_first, *__restrict__ oa = V.oa;
	const uint8_t *__restrict__ orv = V.trav.orv;
	uint16_t *__restrict__ gt = I.rows.gt;
	const uint32_t n_samples = I.slots.NS, S = I.slots.S;
	uint32_t n_unt = 0, n_fallback = 0, any_broken = 0; // of the wave's records: one atomic each behind the loop
	for (uint32_t i0 = blockIdx.x * WAVES + (threadIdx.x >> 6); i0 < I.nfl; i0 += waves) {
		const uint32_t i = I.dst ? I.dst[i0] : i0;
		uint32_t t, h;
		const uint32_t rr = run_of_record(r, k, V, I.perm, i0, &t, &h);
		if (rr == NO_QUERY || i >= I.nrec) { // (the same in every lane)
			any_broken = 1;
			continue;
		}
		const uint32_t q = V.trav.rq[t], ra = I.rows.o_ref[i], own = I.slots.slot_of_path[I.rows.o_path[i]];
		const uint32_t lap = t - h, n = r.len[h];
		const uint64_t base = (uint64_t)I.qidx[q] * S, xb = (uint64_t)rr * S;
		const bool cand = k.rr_any[rr] != 0;
		uint32_t n_an = 0, n_ns = 0, amb = 0, unt = 0, fallback = 0, broken = 0;
		for (uint32_t sm = lane; sm < n_samples; sm += 64) {
			bool any = false;
			for (uint32_t sl = slot_first[sm]; sl < slot_first[sm + 1]; sl++) {
				const uint32_t laps = r.slaps[base + sl];
				out.lap_count[(uint64_t)i * S + sl] = (uint16_t)(laps < un::CN_MAX ? laps : un::CN_MAX);
				const uint8_t st = k.state[xb + sl];
				uint32_t code = POVU_HIP_GT_MISSING;
				if (st == un::ENTRY_OLD) {
					fallback += laps >= 2;
					if (sl == own) {
						code = 0;
					} else {
						const uint32_t mn = I.smin[base + sl], mx = I.smax[base + sl];
						if (mn != 0xFFFFFFFFu && mn == mx)
							code = un::code_of_allele(mn, ra);
						else if (mn != 0xFFFFFFFFu)
							amb = 1;
					}
				} else {
					const uint32_t hp = r.shead[base + sl], m = hp < r.R ? r.len[hp] : 0;
					uint32_t pj = 0;
					if (st == un::ENTRY_TASK) {
						const uint32_t task = k.task_of[xb + sl];
						pj = un::NO_PARTNER;
						if (task < k.nT && lap < n)
							pj = k.partner[k.poff[task] + lap];
						else
							broken = 1;
						unt = 1;
					}
					if (pj != un::NO_PARTNER) {
						if (pj < m && (uint64_t)hp + m <= r.R)
							code = un::code_of_allele(oa[hp + un::oriented_lap(pj, m, orv[hp] != orv[h])], ra);
						else
							broken = 1;
					}
				}
				if (!cand)
					continue;
				gt[(uint64_t)i * S + sl] = (uint16_t)code;
				if (code != POVU_HIP_GT_MISSING) {
					any = true;
					n_an++;
					if (code)
						atomicAdd(I.ac + I.ac_off[i] + code - 1, 1u);
				}
			}
			n_ns += any;
		}
		n_an = wave_sum(n_an);
		n_ns = wave_sum(n_ns);
		amb = wave_sum(amb);
		unt = wave_sum(unt);
		fallback = wave_sum(fallback);
		broken = wave_sum(broken);
		if (lane == 0) {
			out.lap[i] = lap + 1;
			out.n_laps[i] = n;
			out.rec_unt[i] = unt != 0;
			if (cand) {
				I.rows.o_an[i] = n_an;
				I.rows.o_ns[i] = n_ns;
				const uint8_t f = I.rows.o_flags[i] & (uint8_t)~POVU_HIP_CALL_TANGLED;
				I.rows.o_flags[i] = f | ((V.trav.qstatus[q] || amb) ? POVU_HIP_CALL_TANGLED : 0);
			}
		}
		n_unt += unt != 0;
		n_fallback += fallback;
		any_broken |= broken;
	}
	if (lane == 0) {
		if (n_unt)
			atomicAdd(words + W_RECORDS, (unsigned long long)n_unt);
		if (n_fallback)
			atomicAdd(words + W_FALLBACK, (unsigned long long)n_fallback);
		if (any_broken)
			atomicOr(words + W_BROKEN, 1ull);
	}
}

UntangleRows untangle_rows(povu_hip_ctx *ctx, const UntangleIn &in)
{
	hipStream_t s = ctx->stream;
	const uint32_t R = in.v.trav.R, S = in.slots.S, nfl = in.nfl, nrec = in.nrec;
	const size_t R1 = (size_t)R + 1, r1 = (size_t)nrec + 1, cells = (size_t)in.nQ * S + 1;
	UntangleRows out;
	unsigned long long *words;
	carve(ctx->un_rows, [&](Spans &take) {
		take(r1, out.rec_unt, out.lap, out.n_laps);
		take((size_t)nrec * S + 1, out.lap_count);
		take(W_WORDS, words);
	});
	HIP_CHECK(hipMemsetAsync(out.rec_unt, 0, r1, s));
	HIP_CHECK(hipMemsetAsync(out.lap, 0, r1 * 4, s));
	HIP_CHECK(hipMemsetAsync(out.n_laps, 0, r1 * 4, s));
	HIP_CHECK(hipMemsetAsync(out.lap_count, 0, ((size_t)nrec * S + 1) * 2, s));
	HIP_CHECK(hipMemsetAsync(words, 0, W_WORDS * 8, s));
	if (!nfl || !R || !in.nQ)
		return out;

	// ---- lap runs
	Runs r{R, S};
	Tasks k{};
	uint8_t *refflag;
	uint32_t *rh, *count;
	void *tmp;
	const size_t tmp_bytes = prim_tmp_bytes(R1, false) + 256;
	carve(ctx->un_ws, [&](Spans &take) {
		take(R1, r.head, r.len, r.mixed, refflag, rh, k.rr_of);
		take(cells, r.spaths, r.shead, r.slaps);
		take(2, count);
		take(tmp_bytes, tmp);
	});
	HIP_CHECK(hipMemsetAsync(r.spaths, 0, cells * 4, s));
	HIP_CHECK(hipMemsetAsync(r.shead, 0xFF, cells * 4, s));
	HIP_CHECK(hipMemsetAsync(r.slaps, 0, cells * 4, s));
	HIP_CHECK(hipMemsetAsync(k.rr_of, 0xFF, R1 * 4, s));
	HIP_CHECK(hipMemsetAsync(count, 0, 8, s));
	KLAUNCH(k_un_runs, dim3(stride_blocks(R)), dim3(Q_TPB), 0, s, r, in.v.trav, in.v.keep, in.qidx, in.slots.slot_of_path, in.v.on_ref, refflag);
	compact_flagged_u8(refflag, R, rh, count, tmp, tmp_bytes, s);
	k.nRH = read_back(count, s);
	k.rh = rh;
	if (!k.nRH)
		throw HipError("untangled calls: the flubble records have no reference run (internal)");
	KLAUNCH(k_un_rr_of, dim3(stride_blocks(k.nRH)), dim3(Q_TPB), 0, s, k.nRH, R, rh, k.rr_of);

	// ---- task list
	const uint64_t X = (uint64_t)k.nRH * S;
	refuse_2_32(X, "POVU_HIP_T_UNTANGLE needs ", "(reference run, slot) entries");
	uint8_t *tflag;
	uint32_t *tl, *tcount;
	void *tmp2;
	const size_t tmp2_bytes = prim_tmp_bytes((size_t)X + 1, false) + 256;
	carve(ctx->un_task, [&](Spans &take) {
		take((size_t)X + 1, k.state, tflag, k.task_of, tl);
		take((size_t)k.nRH + 1, k.rr_any);
		take(2, tcount);
		take(tmp2_bytes, tmp2);
	});
	HIP_CHECK(hipMemsetAsync(k.task_of, 0xFF, ((size_t)X + 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(k.rr_any, 0, ((size_t)k.nRH + 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(tcount, 0, 8, s));
	KLAUNCH(k_un_entries, dim3(stride_blocks(X)), dim3(Q_TPB), 0, s, r, k, in.v.trav, in.qidx, in.slots.slot_of_path, tflag);
	compact_flagged_u8(tflag, X, tl, tcount, tmp2, tmp2_bytes, s);
	k.nT = read_back(tcount, s);
	k.tl = tl;
	refuse_2_32(k.nT, "POVU_HIP_T_UNTANGLE needs ", "alignments");
	uint64_t *pcnt, *poff, *s64;
	carve(ctx->un_part, [&](Spans &take) {
		take((size_t)k.nT + 1, pcnt, poff);
		take(scan_exclusive_u64_tmp((size_t)k.nT + 1), s64);
	});
	KLAUNCH(k_un_tasks, dim3(stride_blocks((size_t)k.nT + 1)), dim3(Q_TPB), 0, s, r, k, pcnt);
	scan_exclusive_u64(pcnt, poff, (size_t)k.nT + 1, s64, s);
	k.poff = poff;
	const uint64_t partner_bytes = read_back(poff + k.nT, s);
	if (partner_bytes > (uint64_t)k.nT * un::MAX_LAPS)
		throw HipError("untangled calls: a task of more than 64 rows (internal)");
	size_t free_b = 0, total_b = 0;
	HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
	if (partner_bytes > total_b)
		throw HipError("POVU_HIP_T_UNTANGLE: the partner table of " + std::to_string(k.nT) + " alignments (" + std::to_string(partner_bytes >> 20) +
			       " MiB) does not fit device memory");
	carve(ctx->un_pair, [&](Spans &take) { take((size_t)partner_bytes + 1, k.partner); });

	// ---- align
	if (k.nT)
		KLAUNCH(k_un_align, dim3(wave_grid(k.nT)), dim3(Q_TPB), 0, s, r, k, in.v.trav, in.v.oa, in.qidx, partner_bytes, words);

	// ---- genotypes
	KLAUNCH(k_un_zero_ac, dim3(wave_blocks(nfl)), dim3(Q_TPB), 0, s, nfl, nrec, r, k, in.v, in.perm, in.dst, in.ac_off, in.ac);
	KLAUNCH(k_un_records, dim3(wave_grid(nfl)), dim3(Q_TPB), 0, s, in, r, k, out, words);
	unsigned long long hw[W_WORDS] = {0};
	HIP_CHECK(copy_async(hw, words, sizeof hw, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	if (hw[W_BROKEN])
		throw HipError("untangled calls: a task or a record is not what the host listed (internal)");
	out.n_tasks = k.nT, out.n_records = hw[W_RECORDS], out.n_missing = hw[W_MISSING], out.n_extra = hw[W_EXTRA], out.n_fallback = hw[W_FALLBACK];
	return out;
}

} // namespace povu_hip
