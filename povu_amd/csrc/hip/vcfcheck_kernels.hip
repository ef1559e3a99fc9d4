// vcfcheck_kernels.hip -- povu_hip_vcf_check (include/povu_hip.h): does a parsed VCF still describe the resident graph?
//
// The definition is INTEGRATION.md "VCF checks" (restated in tests/vcfcheck_ref.py; the rules that are plain arithmetic are
// vcfcheck_rules.hpp).  All of it runs on the graph, paths and sequences resident in the context:
//   walks        every step id to a path word (find_vertex), every allele to its state (no walk, a step the graph lacks);
//   step index   the occurrences of every path word (build_step_index, the inversion calls' index);
//   search       the unit of work is an (allele, direction), not a task: many slots carry one allele and it is searched once.
//                A unit walks the occurrences of its anchor (w[0] forward, flip(w[m - 1]) reverse), finds the path of each
//                (span_of), rejects what would run past the path's end, compares the m steps and marks (allele, slot of the
//                path) in a byte table of hits.  A lane per unit while the walk has at most TIER1_STEPS steps and the anchor
//                at most TIER1_CANDIDATES occurrences, else a wave per unit: lanes across the occurrences while the walk has
//                at most 64 steps, across the steps (64 a ballot) when it is longer;
//   spelling     a wave per allele, lanes across the bytes of a step, REF / ALT compared in place with both readings;
//   tasks        a lane per task reads its status from the table;
//   records      a wave per record reduces its tasks and alleles to the first failure.
// A row of the table belongs to one unit: its bytes are written with plain vector stores of the same value, no atomics.
#include "call_common.hpp"
#include "vcfcheck_rules.hpp"

namespace povu_hip
{

static constexpr uint32_t TIER1_STEPS = 64, TIER1_CANDIDATES = 64;
// (the state of an allele is VC_AS_* of vcfcheck_rules.hpp: no walk, a step the graph lacks, a `*` allele; 0: it is searched)
// counters: [0, POVU_HIP_V_N_STATUS) tasks of every status, then invalid records, misspelled alleles
static constexpr uint32_t CN_INVALID = POVU_HIP_V_N_STATUS, CN_MISSPELLED = CN_INVALID + 1, CN_WORDS = 8;
// the kernels that count stride over a grid of at most this many workgroups (the device's wave slots at 256 lanes a workgroup):
// a wave adds what it counted once, at its end, so the eight counters see thousands of atomics, not one a wave of tasks
static constexpr unsigned COUNT_BLOCKS = 2048;

// what the kernels read of the document, the paths and the index; what a kernel writes is a parameter of its own, but the hits
struct VcView {
	PathsView paths;
	const uint32_t *ioff, *occ;	// the step index (null without path steps: nothing is searched)
	const uint32_t *slot_of_path;	// [P]
	uint32_t S;			// slots
	uint32_t nA;			// alleles
	const uint32_t *soff;		// [nA + 1] steps of an allele
	const uint32_t *w;		// the walks as path words, NO_QUERY for a step the graph lacks
	const uint8_t *astate;		// [nA] VC_AS_*
	uint8_t *hit;			// [2][nA][S] the forward plane, then the reverse plane
	__device__ __forceinline__ uint8_t *hit_of(uint32_t a, bool rev, uint32_t slot) const
	{
		return hit + ((uint64_t)(rev ? nA : 0) + a) * S + slot;
	}
};

__global__ void k_vc_resolve(uint32_t n, const uint32_t *__restrict__ sid, const uint8_t *__restrict__ sor, const uint32_t *__restrict__ vid,
			     uint32_t V, uint32_t *__restrict__ w)
{
	for (uint32_t k = blockIdx.x * Q_TPB + threadIdx.x; k < n; k += gridDim.x * Q_TPB) {
		const uint32_t v = find_vertex(vid, V, sid[k]);
		w[k] = v == NO_QUERY ? NO_QUERY : (v << 1) | (sor[k] & 1u);
	}
}
__global__ void k_vc_alleles(uint32_t nA, const uint32_t *__restrict__ soff, const uint32_t *__restrict__ w, const uint8_t *__restrict__ awalk,
			     const uint64_t *__restrict__ toff, const char *__restrict__ text, uint8_t *__restrict__ astate)
{
	for (uint32_t a = blockIdx.x * Q_TPB + threadIdx.x; a < nA; a += gridDim.x * Q_TPB) {
		bool unknown = false;
		for (uint32_t k = soff[a]; !unknown && k < soff[a + 1]; k++)
			unknown = w[k] == NO_QUERY;
		astate[a] = vc_allele_state(awalk[a] & 2u, text + toff[a], toff[a + 1] - toff[a], awalk[a] & 1u, soff[a + 1] - soff[a], unknown);
	}
}

// the occurrence of the unit's anchor at global position g: marks the slot of g's path when the walk stands there
__device__ __forceinline__ void try_candidate(const VcView &A, uint32_t a, bool rev, const uint32_t *__restrict__ wp, uint32_t m, uint32_t g)
{
	const uint32_t p = span_of(A.paths.path_off, A.paths.n_paths, g);
	uint8_t *h = A.hit_of(a, rev, A.slot_of_path[p]);
	if (*h)
		return; // (another occurrence has marked the slot)
	if (vc_occurs_at(A.paths.steps, g, A.paths.path_off[p + 1], wp, m, rev))
		*h = 1;
}

// tier 1: a lane per unit u = allele << 1 | direction; the long walks and the long lists (or every unit, with force) go to `t2`
__global__ void k_vc_search(uint32_t nU, VcView A, uint32_t force, uint32_t forward_only, uint32_t *__restrict__ t2, uint32_t *__restrict__ n_t2)
{
	for (uint32_t u = blockIdx.x * Q_TPB + threadIdx.x; u < nU; u += gridDim.x * Q_TPB) {
		const uint32_t a = u >> 1;
		const bool rev = u & 1u;
		if ((rev && forward_only) || A.astate[a])
			continue;
		const uint32_t m = A.soff[a + 1] - A.soff[a];
		const uint32_t *wp = A.w + A.soff[a];
		const uint32_t x = vc_anchor(wp, m, rev), e0 = A.ioff[x], e1 = A.ioff[x + 1];
		if (force || m > TIER1_STEPS || e1 - e0 > TIER1_CANDIDATES) {
			t2[atomicAdd(n_t2, 1u)] = u;
			continue;
		}
		for (uint32_t e = e0; e < e1; e++)
			try_candidate(A, a, rev, wp, m, A.occ[e]);
	}
}
// tier 2: a wave per unit of `t2`
__global__ __launch_bounds__(Q_TPB) void k_vc_search_wave(const uint32_t *__restrict__ t2, uint32_t n2, VcView A)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	for (uint32_t i = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); i < n2; i += waves) {
		const uint32_t u = t2[i], a = u >> 1;
		const bool rev = u & 1u;
		const uint32_t m = A.soff[a + 1] - A.soff[a];
		const uint32_t *wp = A.w + A.soff[a];
		const uint32_t x = vc_anchor(wp, m, rev), e0 = A.ioff[x], e1 = A.ioff[x + 1];
		if (m <= 64) { // lanes across the occurrences (e1 + 64 < 2^32: 2^32 - 4096 path steps or more are refused)
			for (uint32_t b = e0; b < e1; b += 64)
				if (b + lane < e1)
					try_candidate(A, a, rev, wp, m, A.occ[b + lane]);
			continue;
		}
		for (uint32_t e = e0; e < e1; e++) { // lanes across the steps, an occurrence at a time (all of this is wave-uniform)
			const uint32_t g = A.occ[e], p = span_of(A.paths.path_off, A.paths.n_paths, g);
			uint8_t *h = A.hit_of(a, rev, A.slot_of_path[p]);
			if (*h || !vc_fits(g, m, A.paths.path_off[p + 1]))
				continue;
			bool same = true;
			for (uint32_t k0 = 0; same && k0 < m; k0 += 64) {
				const uint32_t k = k0 + lane;
				same = !__ballot(k < m && A.paths.steps[(uint64_t)g + k] != vc_pattern_step(wp, m, rev, k));
			}
			if (same && lane == 0)
				*h = 1;
		}
	}
}

// ---- spelling: a wave per allele that has a walk of known steps and a text.  Whole: the text is every step's bases; anchored: the
// first step's last base, then the other steps' bases
__global__ __launch_bounds__(Q_TPB) void k_vc_spell(VcView A, const uint8_t *__restrict__ awalk, const uint64_t *__restrict__ toff,
						    const char *__restrict__ text, uint8_t *__restrict__ spell, unsigned long long *__restrict__ cnt)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	const PathsView &P = A.paths;
	unsigned long long n_misspelled = 0; // of the wave's alleles: one atomic at its end
	for (uint32_t a = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); a < A.nA; a += waves) {
		if (A.astate[a] || (awalk[a] & 3u) != 3u)
			continue; // (POVU_HIP_V_SPELL_NONE: the array was cleared)
		const uint32_t m = A.soff[a + 1] - A.soff[a];
		const uint32_t *wp = A.w + A.soff[a];
		const char *T = text + toff[a];
		const uint64_t L = toff[a + 1] - toff[a];
		uint64_t total = 0;
		for (uint32_t k = lane; k < m; k += 64)
			total += path_step_len(P, wp[k]);
		total = wave_sum(total);
		const uint64_t len0 = path_step_len(P, wp[0]);
		bool whole = L == total, anchored = len0 > 0 && L == total - len0 + 1;
		uint64_t at = 0; // bases in front of step k
		for (uint32_t k = 0; k < m && (whole || anchored); k++) {
			const uint32_t x = wp[k];
			const uint64_t b0 = P.seq_off[x >> 1], n = P.seq_off[(x >> 1) + 1] - b0;
			bool bad_w = false, bad_a = false;
			for (uint64_t i = lane; i < n; i += 64) {
				const uint8_t c = (uint8_t)P.seq[(x & 1u) ? b0 + n - 1 - i : b0 + i], rc = comp(c), o = (x & 1u) ? rc : c;
				if (whole && (!rc || (uint8_t)T[at + i] != o))
					bad_w = true;
				if (anchored && (k ? (!rc || (uint8_t)T[at - len0 + 1 + i] != o) : (i == n - 1 && (!rc || (uint8_t)T[0] != o))))
					bad_a = true;
			}
			whole = whole && !__ballot(bad_w);
			anchored = anchored && !__ballot(bad_a);
			at += n;
		}
		if (lane == 0) {
			spell[a] = whole ? POVU_HIP_V_SPELL_WHOLE : anchored ? POVU_HIP_V_SPELL_ANCHORED : POVU_HIP_V_SPELL_MISSPELLED;
			n_misspelled += !whole && !anchored;
		}
	}
	if (lane == 0 && n_misspelled)
		atomicAdd(cnt + CN_MISSPELLED, n_misspelled);
}

// ---- tasks: a lane per task (the loop is by waves: every lane of a wave takes part in the counts)
struct VcTasks {
	uint32_t nK;
	const uint32_t *t_rec, *t_al, *t_col, *t_phase; // [nK]
	const uint32_t *aoff;				  // [nR + 1] alleles of a record
	const uint32_t *col_first, *col_slots;		  // [columns]
};
__global__ __launch_bounds__(Q_TPB) void k_vc_tasks(VcTasks K, VcView A, uint32_t forward_only, uint8_t *__restrict__ status,
						    unsigned long long *__restrict__ cnt)
{
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long mine[POVU_HIP_V_N_STATUS] = {0}; // the wave's tasks of every status: one atomic a status at its end
	for (uint64_t b = ((uint64_t)blockIdx.x * Q_TPB + threadIdx.x) & ~63ull; b < K.nK; b += (uint64_t)gridDim.x * Q_TPB) {
		const uint64_t t = b + lane;
		uint32_t st = POVU_HIP_V_N_STATUS; // (no task)
		if (t < K.nK) {
			const uint32_t r = K.t_rec[t], al = K.t_al[t], c = K.t_col[t], j = K.t_phase[t];
			const uint32_t a = K.aoff[r] + al; // (read only when the record has the allele)
			const bool has = al < K.aoff[r + 1] - K.aoff[r];
			const uint8_t as = has ? A.astate[a] : 0;
			const bool no_slot = j >= K.col_slots[c];
			bool fwd = false, rev = false;
			if (has && !as && !no_slot) {
				fwd = *A.hit_of(a, false, K.col_first[c] + j);
				rev = *A.hit_of(a, true, K.col_first[c] + j);
			}
			st = vc_task_status(has, as, no_slot, fwd, rev, forward_only != 0);
			status[t] = (uint8_t)st;
		}
#pragma unroll
		for (uint32_t s = 0; s < POVU_HIP_V_N_STATUS; s++)
			mine[s] += __popcll(__ballot(st == s));
	}
#pragma unroll
	for (uint32_t s = 0; s < POVU_HIP_V_N_STATUS; s++)
		if (lane == 0 && mine[s])
			atomicAdd(cnt + s, mine[s]);
}

// ---- records: a wave per record.  Its first failure in (allele, column, phase) order -- the order of its tasks --, a misspelled
// allele in front of the tasks of that allele
__global__ __launch_bounds__(Q_TPB) void k_vc_records(uint32_t nR, const uint32_t *__restrict__ aoff, const uint32_t *__restrict__ tkoff,
						      const uint32_t *__restrict__ t_al, const uint8_t *__restrict__ status,
						      const uint8_t *__restrict__ spell, uint8_t *__restrict__ r_inv, uint8_t *__restrict__ r_reason,
						      uint32_t *__restrict__ r_al, uint32_t *__restrict__ r_task, unsigned long long *__restrict__ cnt)
{
	const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (Q_TPB / 64);
	unsigned long long n_invalid = 0; // of the wave's records: one atomic at its end
	for (uint32_t r = blockIdx.x * (Q_TPB / 64) + (threadIdx.x >> 6); r < nR; r += waves) {
		uint32_t ft = NO_QUERY, fm = NO_QUERY; // the first failing task, the first misspelled allele (within the record)
		for (uint32_t b = tkoff[r]; b < tkoff[r + 1] && ft == NO_QUERY; b += 64) {
			const uint32_t t = b + lane; // (tkoff[r + 1] + 64 < 2^32: 2^32 - 64 tasks or more are refused)
			const unsigned long long m = __ballot(t < tkoff[r + 1] && status[t] > POVU_HIP_V_FOUND_REV);
			if (m)
				ft = b + (uint32_t)__ffsll((long long)m) - 1;
		}
		for (uint32_t b = aoff[r]; b < aoff[r + 1] && fm == NO_QUERY; b += 64) {
			const uint32_t a = b + lane;
			const unsigned long long m = __ballot(a < aoff[r + 1] && spell[a] == POVU_HIP_V_SPELL_MISSPELLED);
			if (m)
				fm = b + (uint32_t)__ffsll((long long)m) - 1 - aoff[r];
		}
		if (lane)
			continue;
		const uint32_t fal = ft == NO_QUERY ? NO_QUERY : t_al[ft];
		const bool by_spelling = fm != NO_QUERY && (ft == NO_QUERY || fm <= fal);
		r_inv[r] = ft != NO_QUERY || fm != NO_QUERY;
		r_reason[r] = by_spelling ? POVU_HIP_V_MISSPELLED : ft != NO_QUERY ? status[ft] : 0xFF;
		r_al[r] = by_spelling ? fm : fal;
		r_task[r] = by_spelling ? NO_QUERY : ft;
		n_invalid += ft != NO_QUERY || fm != NO_QUERY;
	}
	if (lane == 0 && n_invalid)
		atomicAdd(cnt + CN_INVALID, n_invalid);
}

namespace
{
struct ReportOwner {
	povu_hip_vcf_report view{}; // first member: the owner is recovered from it in povu_hip_vcf_report_free
	PinnedVec<uint8_t> task_status, allele_spell, rec_invalid, rec_reason;
	PinnedVec<uint32_t> rec_allele, rec_task;
};
// a copy of 64-bit offsets as the 32-bit ones the device reads (the caller has refused what does not fit)
std::vector<uint32_t> narrow(const uint64_t *off, size_t n)
{
	std::vector<uint32_t> v(n);
	for (size_t k = 0; k < n; k++)
		v[k] = (uint32_t)off[k];
	return v;
}
// what the kernels index by must lie within what they index: offsets that ascend to their totals, tasks of their records and
// of the document's columns, paths in the names' slots (all true of povu_hip_vcf_parse and the names makers)
void check_doc(const povu_hip_vcf_doc *d, const povu_hip_call_names *names, uint32_t S)
{
	auto ascends = [](const uint64_t *off, uint64_t n, uint64_t total) {
		if (!off || off[0] != 0 || off[n] != total)
			return false;
		for (uint64_t k = 0; k < n; k++)
			if (off[k] > off[k + 1])
				return false;
		return true;
	};
	bool ok = ascends(d->allele_off, d->n_records, d->n_alleles) && ascends(d->task_off, d->n_records, d->n_tasks) &&
		  ascends(d->step_off, d->n_alleles, d->n_steps) && ascends(d->text_off, d->n_alleles, d->n_text_bytes);
	for (uint64_t r = 0; ok && r < d->n_records; r++)
		for (uint64_t t = d->task_off[r]; ok && t < d->task_off[r + 1]; t++)
			ok = d->task_record[t] == r && d->task_col[t] < d->n_samples && (t == d->task_off[r] || d->task_allele[t - 1] <= d->task_allele[t]);
	if (!ok)
		throw HipError("the VCF document's offsets and tasks do not belong together");
	for (uint32_t p = 0; p < names->n_paths; p++)
		if (names->slot_of_path[p] >= S)
			throw HipError("the names put path " + std::to_string(p) + " in a slot they do not have");
}
} // namespace

static povu_hip_vcf_report *vcf_check(povu_hip_ctx *ctx, const povu_hip_vcf_doc *doc, const povu_hip_call_names *names, uint32_t flags,
				      CallTimer &timer)
{
	if (!ctx || !doc || !names)
		throw HipError("null context, document or names");
	if (!ctx->g.block)
		throw HipError("the VCF checks need a resident graph (povu_hip_graph_upload first)");
	if (!ctx->paths_valid || ctx->paths_gen != ctx->g.gen)
		throw HipError("no paths are resident for the graph now uploaded (povu_hip_paths_upload after povu_hip_graph_upload)");
	const bool spelling = flags & POVU_HIP_V_SPELLING, forward_only = flags & POVU_HIP_V_FORWARD_ONLY, force = flags & POVU_HIP_V_FORCE_TIER2;
	if (spelling && (!ctx->seq_valid || ctx->seq_gen != ctx->g.gen))
		throw HipError("the spelling check needs the sequences of the graph now uploaded (povu_hip_segments_upload after povu_hip_graph_upload)");
	if (names->n_paths != ctx->n_paths)
		throw HipError("the names are of " + std::to_string(names->n_paths) + " paths, " + std::to_string(ctx->n_paths) + " are resident");
	const uint64_t N = ctx->n_path_steps;
	if (N >= 0xFFFFFFFFull - 4096) // (the sort of the step index takes fewer)
		throw HipError("the VCF checks index every path step: " + std::to_string(N) + " steps, 2^32 or more are refused");
	refuse_2_32(doc->n_records + 64, "the VCF checks need ", "records");
	refuse_2_32(2 * doc->n_alleles + 64, "the VCF checks need ", "searches (two an allele)");
	refuse_2_32(doc->n_steps + 64, "the VCF checks need ", "walk steps");
	refuse_2_32(doc->n_tasks + 64, "the VCF checks need ", "tasks");
	const uint32_t nR = (uint32_t)doc->n_records, nA = (uint32_t)doc->n_alleles, nS = (uint32_t)doc->n_steps, nK = (uint32_t)doc->n_tasks;
	const uint32_t nC = (uint32_t)doc->n_samples, S = names->refs.n_slots, P = ctx->n_paths;
	refuse_2_32((uint64_t)nA * S, "the VCF checks need ", "(allele, slot) pairs");
	const size_t cells = (size_t)nA * S;
	std::vector<uint32_t> col_first((size_t)nC + 1), col_slots((size_t)nC + 1);
	if (povu_hip_vcf_columns(doc, names, col_first.data(), col_slots.data()))
		throw HipError("the names do not name their slots' samples");
	check_doc(doc, names, S);
	const std::vector<uint32_t> h_soff = narrow(doc->step_off, (size_t)nA + 1), h_aoff = narrow(doc->allele_off, (size_t)nR + 1),
				    h_tkoff = narrow(doc->task_off, (size_t)nR + 1);

	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->wait_tail();
	hipStream_t s = ctx->stream;
	// ---- the layout: what is uploaded, what the kernels work on, the results
	uint32_t *soff, *sid, *aoff, *tkoff, *t_rec, *t_al, *t_col, *t_phase, *d_first, *d_slots, *slot_of_path, *w, *t2, *words, *r_al, *r_task;
	uint64_t *toff;
	uint8_t *awalk, *sor, *astate, *status, *spell, *r_inv, *r_reason, *hit;
	char *text;
	unsigned long long *cnt;
	auto layout = [&](Spans &take) {
		take((size_t)nA + 1, soff, toff, awalk, astate, spell);
		take((size_t)nS + 1, sid, sor, w);
		take(doc->n_text_bytes + 1, text);
		take((size_t)nR + 1, aoff, tkoff, r_inv, r_reason, r_al, r_task);
		take((size_t)nK + 1, t_rec, t_al, t_col, t_phase, status);
		take((size_t)nC + 1, d_first, d_slots);
		take((size_t)P + 1, slot_of_path);
		take(2 * (size_t)nA + 1, t2);
		take(8, words);
		take(CN_WORDS, cnt);
	};
	timer.start(s);
	StepIndex ix{nullptr, nullptr};
	if (N)
		ix = build_step_index(ctx, ctx->vc_ws, layout);
	else
		carve(ctx->vc_ws, layout);
	carve(ctx->vc_hit, [&](Spans &take) { take(2 * cells + 1, hit); });
	auto up = [&](void *dst, const void *src, size_t bytes) {
		if (bytes)
			HIP_CHECK(copy_async(dst, src, bytes, hipMemcpyHostToDevice, s));
	};
	up(soff, h_soff.data(), ((size_t)nA + 1) * 4);
	up(toff, doc->text_off, ((size_t)nA + 1) * 8);
	up(awalk, doc->allele_walk, nA);
	up(sid, doc->step_id, (size_t)nS * 4);
	up(sor, doc->step_or, nS);
	up(text, doc->text, doc->n_text_bytes);
	up(aoff, h_aoff.data(), ((size_t)nR + 1) * 4);
	up(tkoff, h_tkoff.data(), ((size_t)nR + 1) * 4);
	up(t_rec, doc->task_record, (size_t)nK * 4);
	up(t_al, doc->task_allele, (size_t)nK * 4);
	up(t_col, doc->task_col, (size_t)nK * 4);
	up(t_phase, doc->task_phase, (size_t)nK * 4);
	up(d_first, col_first.data(), (size_t)nC * 4);
	up(d_slots, col_slots.data(), (size_t)nC * 4);
	up(slot_of_path, names->slot_of_path, (size_t)P * 4);
	HIP_CHECK(hipMemsetAsync(words, 0, 32, s));
	HIP_CHECK(hipMemsetAsync(cnt, 0, CN_WORDS * 8, s));
	HIP_CHECK(hipMemsetAsync(hit, 0, 2 * cells + 1, s));
	HIP_CHECK(hipMemsetAsync(spell, 0, (size_t)nA + 1, s));
	launch_vid_ascending(ctx->g.V, ctx->g.vid, words, s);
	query_refusals(read_back(words, s), "VCF checks");

	// ---- walks, search, spelling
	const VcView A{paths_view(ctx), ix.ioff, ix.occ, slot_of_path, S, nA, soff, w, astate, hit};
	if (nS)
		KLAUNCH(k_vc_resolve, dim3(stride_blocks(nS)), dim3(Q_TPB), 0, s, nS, sid, sor, ctx->g.vid, ctx->g.V, w);
	if (nA)
		KLAUNCH(k_vc_alleles, dim3(stride_blocks(nA)), dim3(Q_TPB), 0, s, nA, soff, w, awalk, toff, text, astate);
	uint32_t n_t2 = 0;
	if (N && nA && S) {
		KLAUNCH(k_vc_search, dim3(stride_blocks(2 * (size_t)nA)), dim3(Q_TPB), 0, s, 2 * nA, A, force ? 1u : 0u, forward_only ? 1u : 0u, t2, words + 1);
		n_t2 = read_back(words + 1, s);
		if (n_t2)
			KLAUNCH(k_vc_search_wave, dim3(wave_blocks(n_t2)), dim3(Q_TPB), 0, s, t2, n_t2, A);
	}
	if (spelling && nA)
		KLAUNCH(k_vc_spell, dim3(std::min(wave_blocks(nA), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, A, awalk, toff, text, spell, cnt);
	// ---- tasks, records
	if (nK) {
		const VcTasks K{nK, t_rec, t_al, t_col, t_phase, aoff, d_first, d_slots};
		KLAUNCH(k_vc_tasks, dim3(std::min(stride_blocks(nK), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, K, A, forward_only ? 1u : 0u, status, cnt);
	}
	if (nR)
		KLAUNCH(k_vc_records, dim3(std::min(wave_blocks(nR), COUNT_BLOCKS)), dim3(Q_TPB), 0, s, nR, aoff, tkoff, t_al, status, spell, r_inv, r_reason, r_al, r_task, cnt);

	// ---- to the host
	auto o = std::make_unique<ReportOwner>();
	uint64_t h_cnt[CN_WORDS] = {0};
	hand_off(o->task_status, (size_t)nK + 1, status, nK, ctx);
	hand_off(o->allele_spell, (size_t)nA + 1, spell, nA, ctx);
	hand_off(o->rec_invalid, (size_t)nR + 1, r_inv, nR, ctx);
	hand_off(o->rec_reason, (size_t)nR + 1, r_reason, nR, ctx);
	hand_off(o->rec_allele, (size_t)nR + 1, r_al, nR, ctx);
	hand_off(o->rec_task, (size_t)nR + 1, r_task, nR, ctx);
	HIP_CHECK(copy_async(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, s));
	povu_hip_vcf_report &v = o->view;
	v.device_ms = timer.stop(s);
	v.n_records = nR, v.n_tasks = nK, v.n_alleles = nA;
	v.task_status = o->task_status.data();
	v.allele_spell = o->allele_spell.data();
	v.rec_invalid = o->rec_invalid.data();
	v.rec_reason = o->rec_reason.data();
	v.rec_allele = o->rec_allele.data();
	v.rec_task = o->rec_task.data();
	for (uint32_t k = 0; k < POVU_HIP_V_N_STATUS; k++)
		v.n_status[k] = h_cnt[k];
	v.n_invalid = h_cnt[CN_INVALID];
	v.n_misspelled = h_cnt[CN_MISSPELLED];
	v.n_tier2 = n_t2;
	return &o.release()->view;
}

} // namespace povu_hip

// ---- C ABI

extern "C" povu_hip_vcf_report *povu_hip_vcf_check(povu_hip_ctx *ctx, const povu_hip_vcf_doc *doc, const povu_hip_call_names *names,
						   const povu_hip_vcf_opts *opts, char *err, size_t errlen)
{
	CallTimer timer;
	return guarded_call(ctx, err, errlen, (povu_hip_vcf_report *)nullptr, [&] { return vcf_check(ctx, doc, names, opts ? opts->flags : 0u, timer); });
}
extern "C" void povu_hip_vcf_report_free(povu_hip_vcf_report *r)
{
	delete reinterpret_cast<ReportOwner *>(r);
}
