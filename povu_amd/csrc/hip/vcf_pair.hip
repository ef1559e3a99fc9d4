// vcf_pair.hip -- the host's half of vcf_pair.hpp: two parsed VCFs verified and laid end to end, before anything is uploaded.
#include "vcf_pair.hpp"

#include <algorithm>
#include <unordered_map>

namespace povu_hip
{

namespace
{

// what the kernels index by must lie within what they index (all true of povu_hip_vcf_parse)
void check_pair_doc(const povu_hip_vcf_doc *d, const char *which, const PairWant &need)
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
		  ascends(d->text_off, d->n_alleles, d->n_text_bytes) && (!d->n_records || (d->rec_chrom && d->chrom && d->rec_pos)) &&
		  (!d->n_alleles || d->allele_walk) && (!d->n_text_bytes || d->text) && (!d->n_samples || d->sample) &&
		  (!d->n_tasks || (d->task_record && d->task_allele && d->task_col && (!need.t_ph || d->task_phase)));
	for (uint64_t c = 0; ok && c < d->n_samples; c++)
		ok = d->sample[c] != nullptr;
	for (uint64_t r = 0; ok && r < d->n_records; r++) {
		ok = d->rec_chrom[r] < d->n_chroms && d->chrom[d->rec_chrom[r]];
		for (uint64_t t = d->task_off[r]; ok && t < d->task_off[r + 1]; t++)
			ok = d->task_record[t] == r && d->task_col[t] < d->n_samples &&
			     (!need.tkoff || t == d->task_off[r] || d->task_allele[t - 1] <= d->task_allele[t]);
	}
	if (!ok)
		throw HipError(std::string("the offsets, tasks and CHROM ids of document ") + which + " do not belong together");
}
// the ALTs of record r: its alleles with a text, REF first, but REF
uint64_t alts_of(const povu_hip_vcf_doc *d, uint64_t r)
{
	uint64_t n = 0;
	for (uint64_t a = d->allele_off[r]; a < d->allele_off[r + 1] && (d->allele_walk[a] & 2u); a++)
		n++;
	return n ? n - 1 : 0;
}

} // namespace

PairUpload pair_build(const povu_hip_ctx *ctx, const povu_hip_vcf_doc *da, const povu_hip_vcf_doc *db, const char *who, const PairWant &want,
		      uint64_t pos_limit)
{
	if (!ctx || !da || !db)
		throw HipError("null context or document");
	const povu_hip_vcf_doc *docs[2] = {da, db};
	for (const povu_hip_vcf_doc *d : docs) { // (a side first: the sums below do not wrap)
		refuse_2_32(d->n_records + 64, who, "records of a document");
		refuse_2_32(d->n_alleles + 64, who, "alleles of a document");
		refuse_2_32(d->n_tasks + 64, who, "tasks of a document");
		refuse_2_32(d->n_text_bytes + 64, who, "text bytes of a document");
		refuse_2_32(d->n_samples + 64, who, "sample columns of a document");
	}
	refuse_2_32(da->n_records + db->n_records + 64, who, "records");
	refuse_2_32(da->n_alleles + db->n_alleles + 64, who, "alleles");
	refuse_2_32(da->n_tasks + db->n_tasks + 64, who, "tasks");
	refuse_2_32(da->n_text_bytes + db->n_text_bytes + 64, who, "text bytes");
	check_pair_doc(da, "A", want);
	check_pair_doc(db, "B", want);
	PairUpload U;
	U.da = da, U.db = db;
	U.nRa = (uint32_t)da->n_records, U.nR = U.nRa + (uint32_t)db->n_records, U.nAl = (uint32_t)(da->n_alleles + db->n_alleles);
	U.nT = (uint32_t)(da->n_tasks + db->n_tasks), U.n_text = da->n_text_bytes + db->n_text_bytes;
	U.n_cols_a = (uint32_t)da->n_samples, U.n_cols = U.n_cols_a + (uint32_t)db->n_samples;
	const uint32_t nR = U.nR, nAl = U.nAl, nT = U.nT;

	// ---- both documents as one; the items' offsets; the CHROM ids
	U.aoff.resize((size_t)nR + 1), U.ioff.resize((size_t)nR + 1), U.chrom.resize(nR), U.toff.resize((size_t)nAl + 1), U.pos.resize(nR);
	U.tkoff.resize(want.tkoff ? (size_t)nR + 1 : 0);
	U.t_rec.resize(want.t_rec ? nT : 0), U.t_al.resize(want.t_al ? nT : 0), U.t_col.resize(want.t_col ? nT : 0), U.t_ph.resize(want.t_ph ? nT : 0);
	std::unordered_map<std::string, uint32_t> chrom_of;
	uint64_t n_items = 0, n_items_a = 0, r0 = 0, a0 = 0, t0 = 0, x0 = 0;
	for (int side = 0; side < 2; side++) { // (by side, not by pointer: a document may be compared with itself)
		const povu_hip_vcf_doc *d = docs[side];
		std::vector<uint32_t> id(d->n_chroms);
		for (uint64_t k = 0; k < d->n_chroms; k++) {
			id[k] = d->chrom[k] ? chrom_of.emplace(d->chrom[k], (uint32_t)chrom_of.size()).first->second : 0u;
			if (U.chrom_name.size() < chrom_of.size())
				U.chrom_name.push_back(d->chrom[k]);
		}
		for (uint64_t r = 0; r < d->n_records; r++) {
			if (pos_limit && d->rec_pos[r] >= pos_limit)
				throw HipError(std::string("document ") + (side ? "B" : "A") + ", record " + std::to_string(r) + ": POS " +
					       std::to_string(d->rec_pos[r]) + ": 2^40 or more is refused");
			U.aoff[r0 + r] = (uint32_t)(a0 + d->allele_off[r]);
			if (want.tkoff)
				U.tkoff[r0 + r] = (uint32_t)(t0 + d->task_off[r]);
			U.ioff[r0 + r] = (uint32_t)std::min<uint64_t>(n_items, 0xFFFFFFFFull);
			U.pos[r0 + r] = d->rec_pos[r];
			U.chrom[r0 + r] = id[d->rec_chrom[r]];
			const uint64_t alts = alts_of(d, r), ar = d->allele_off[r];
			n_items += alts;
			for (uint64_t k = 0; k <= alts && ar + k < d->allele_off[r + 1]; k++)
				U.longest = std::max(U.longest, d->text_off[ar + k + 1] - d->text_off[ar + k]);
		}
		for (uint64_t a = 0; a < d->n_alleles; a++)
			U.toff[a0 + a] = x0 + d->text_off[a];
		const uint64_t n = d->n_tasks;
		if (want.t_rec)
			for (uint64_t t = 0; t < n; t++)
				U.t_rec[t0 + t] = (uint32_t)(r0 + d->task_record[t]);
		if (want.t_al)
			std::copy(d->task_allele, d->task_allele + n, U.t_al.begin() + t0);
		if (want.t_col)
			std::copy(d->task_col, d->task_col + n, U.t_col.begin() + t0);
		if (want.t_ph) {
			std::copy(d->task_phase, d->task_phase + n, U.t_ph.begin() + t0);
			for (uint64_t t = 0; t < n; t++)
				U.max_phase = std::max(U.max_phase, d->task_phase[t]);
		}
		r0 += d->n_records, a0 += d->n_alleles, t0 += d->n_tasks, x0 += d->n_text_bytes;
		if (side == 0)
			n_items_a = n_items;
	}
	U.aoff[nR] = nAl, U.toff[nAl] = U.n_text;
	if (want.tkoff)
		U.tkoff[nR] = nT;
	refuse_2_32(n_items + 64, who, "(record, ALT) items");
	U.ioff[nR] = (uint32_t)n_items;
	U.nI = (uint32_t)n_items, U.nIa = (uint32_t)n_items_a, U.n_chroms = (uint32_t)chrom_of.size();

	// ---- the common samples
	U.colmap.assign(want.colmap ? (size_t)U.n_cols + 1 : 0, NO_QUERY);
	std::unordered_map<std::string, uint32_t> col_of_b; // (of several columns of one name the first counts)
	for (uint64_t c = 0; c < db->n_samples; c++)
		col_of_b.emplace(db->sample[c], (uint32_t)c);
	for (uint64_t c = 0; c < da->n_samples; c++) {
		const auto at = col_of_b.find(da->sample[c]);
		if (at == col_of_b.end())
			continue;
		if (want.colmap)
			U.colmap[c] = U.colmap[U.n_cols_a + at->second] = (uint32_t)U.col_a.size();
		U.col_a.push_back((uint32_t)c), U.col_b.push_back(at->second);
		col_of_b.erase(at);
	}
	U.nC = (uint32_t)U.col_a.size();
	return U;
}

} // namespace povu_hip
