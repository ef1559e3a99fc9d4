// vcfcheck.cpp -- the host half of the VCF checks (INTEGRATION.md "VCF checks"), host only: VCF text to the alleles, walks and
// tasks povu_hip_vcf_check takes (records parsed in chunks on several threads), the sample columns to slots, and a report to the
// two files of `povu vcf --report`.  tests/vcfcheck_ref.py restates it as the yardstick.
#include "../../../include/povu_hip.h"
#include "../hip/vcfcheck_rules.hpp"
#include "../hip/vcfcmp_rules.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace
{

using povu_hip::vc_next_step;

void set_err(char *err, size_t n, const std::string &m)
{
	if (err && n)
		snprintf(err, n, "%s", m.c_str());
}

struct Span {
	const char *p;
	size_t n;
	bool is(const char *s) const { return n == strlen(s) && !memcmp(p, s, n); }
};
// the pieces of [p, p + n) between the separators `seps` (one or two bytes)
void split(const char *p, size_t n, const char *seps, std::vector<Span> &out)
{
	out.clear();
	size_t b = 0;
	for (size_t i = 0; i <= n; i++)
		if (i == n || p[i] == seps[0] || (seps[1] && p[i] == seps[1])) {
			out.push_back({p + b, i - b});
			b = i + 1;
		}
}
bool number(const Span &s, uint64_t max, uint64_t *v)
{
	if (!s.n || s.n > 19)
		return false;
	uint64_t x = 0;
	for (size_t i = 0; i < s.n; i++) {
		if (s.p[i] < '0' || s.p[i] > '9')
			return false;
		x = x * 10 + (uint64_t)(s.p[i] - '0');
	}
	*v = x;
	return x <= max;
}

struct Line {
	size_t off, len;
	uint64_t no;
};
struct Task {
	uint32_t allele, col, phase;
};
// what a chunk of records parses to; offsets are the chunk's own
struct Chunk {
	std::vector<uint64_t> line, pos, id_off{0}, allele_off{0}, task_off{0}, step_off{0}, text_off{0};
	std::vector<uint8_t> allele_walk, step_or;
	std::vector<uint32_t> step_id, task_allele, task_col, task_phase;
	std::string ids, text;
	// the CHROM strings of the chunk in order of first appearance, and every record's among them
	std::vector<std::string> chrom;
	std::unordered_map<std::string, uint32_t> chrom_of;
	std::vector<uint32_t> rec_chrom;
	uint64_t bad_line = 0; // the first malformed line, 0: none
	std::string bad;
};

struct Malformed {
	std::string why;
};

void parse_record(const char *text, const Line &ln, size_t n_samples, Chunk &c)
{
	std::vector<Span> f, part, sub, gt;
	split(text + ln.off, ln.len, "\t", f);
	if (f.size() < 8)
		throw Malformed{"a record needs at least 8 columns, this one has " + std::to_string(f.size())};
	if (f.size() > 8 && f.size() != 9 + n_samples)
		throw Malformed{"the #CHROM line names " + std::to_string(n_samples) + " sample columns, this record has " +
				std::to_string(f.size() - 9)};
	uint64_t pos = 0;
	if (!number(f[1], ~0ull, &pos))
		throw Malformed{"POS is no number: " + std::string(f[1].p, f[1].n)};
	// the texts: REF, then the ALTs
	std::vector<Span> texts{f[3]};
	if (!f[4].is(".")) {
		split(f[4].p, f[4].n, ",", part);
		texts.insert(texts.end(), part.begin(), part.end());
	}
	// the walks
	std::vector<Span> walks;
	split(f[7].p, f[7].n, ";", part);
	for (const Span &kv : part)
		if (kv.n >= 3 && !memcmp(kv.p, "AT=", 3)) {
			split(kv.p + 3, kv.n - 3, ",", walks);
			break;
		}
	const size_t n_al = std::max(texts.size(), walks.size());
	for (size_t a = 0; a < n_al; a++) {
		// (the AT entry of a spanning allele is the one character `*`: a walk without steps, no bad step)
		if (a < walks.size() && !povu_hip::vc_star_text(walks[a].p, walks[a].n)) {
			size_t i = 0;
			uint32_t id = 0;
			uint8_t rev = 0;
			int t;
			while ((t = vc_next_step(walks[a].p, walks[a].n, &i, &id, &rev)) == povu_hip::VC_TOKEN_STEP) {
				c.step_id.push_back(id);
				c.step_or.push_back(rev);
			}
			if (t == povu_hip::VC_TOKEN_BAD)
				throw Malformed{"AT walk " + std::to_string(a) + " is no walk of [<>]id steps: " + std::string(walks[a].p, walks[a].n)};
		}
		if (a < texts.size())
			c.text.append(texts[a].p, texts[a].n);
		c.allele_walk.push_back((uint8_t)((a < walks.size() ? 1 : 0) | (a < texts.size() ? 2 : 0)));
		c.step_off.push_back(c.step_id.size());
		c.text_off.push_back(c.text.size());
	}
	// the tasks, in (allele, column, phase) order
	std::vector<Task> tasks;
	if (f.size() > 8) {
		split(f[8].p, f[8].n, ":", part);
		size_t at = part.size();
		for (size_t k = 0; k < part.size() && at == part.size(); k++)
			if (part[k].is("GT"))
				at = k;
		for (size_t s = 0; at < part.size() && s < n_samples; s++) {
			split(f[9 + s].p, f[9 + s].n, ":", sub);
			if (at >= sub.size())
				continue;
			split(sub[at].p, sub[at].n, "|/", gt);
			for (size_t j = 0; j < gt.size(); j++) {
				if (gt[j].is("."))
					continue;
				uint64_t a = 0;
				if (!number(gt[j], 0xFFFFFFFEull, &a))
					throw Malformed{"GT of sample column " + std::to_string(s) + " is no genotype: " + std::string(sub[at].p, sub[at].n)};
				tasks.push_back({(uint32_t)a, (uint32_t)s, (uint32_t)j});
			}
		}
	}
	std::stable_sort(tasks.begin(), tasks.end(), [](const Task &x, const Task &y) { return x.allele < y.allele; });
	for (const Task &t : tasks) {
		c.task_allele.push_back(t.allele);
		c.task_col.push_back(t.col);
		c.task_phase.push_back(t.phase);
	}
	c.line.push_back(ln.no);
	c.pos.push_back(pos);
	const auto at_chrom = c.chrom_of.emplace(std::string(f[0].p, f[0].n), (uint32_t)c.chrom.size());
	if (at_chrom.second)
		c.chrom.push_back(at_chrom.first->first);
	c.rec_chrom.push_back(at_chrom.first->second);
	c.ids.append(f[2].p, f[2].n);
	c.id_off.push_back(c.ids.size());
	c.allele_off.push_back(c.allele_walk.size());
	c.task_off.push_back(c.task_allele.size());
}

void parse_chunk(const char *text, const Line *lines, size_t n, size_t n_samples, Chunk &c)
{
	for (size_t k = 0; k < n; k++) {
		// (what a malformed line has appended so far stays in no array: the chunk is dropped with the parse)
		try {
			parse_record(text, lines[k], n_samples, c);
		} catch (const Malformed &m) {
			c.bad_line = lines[k].no;
			c.bad = m.why;
			return;
		}
	}
}

struct Doc {
	povu_hip_vcf_doc pub{}; // (first: the handle points at it)
	std::vector<std::string> sample;
	std::vector<const char *> sample_ptr;
	std::vector<uint64_t> line, pos, id_off{0}, allele_off{0}, task_off{0}, step_off{0}, text_off{0};
	std::vector<uint8_t> allele_walk, step_or;
	std::vector<uint32_t> step_id, task_record, task_allele, task_col, task_phase;
	std::string ids, text;
	std::vector<std::string> chrom;
	std::vector<const char *> chrom_ptr;
	std::vector<uint32_t> rec_chrom;
};

template <class T> void append(std::vector<T> &to, const std::vector<T> &from) { to.insert(to.end(), from.begin(), from.end()); }
// offsets of a chunk behind those of the document: from[0] is 0
void append_off(std::vector<uint64_t> &to, const std::vector<uint64_t> &from)
{
	const uint64_t base = to.back();
	for (size_t k = 1; k < from.size(); k++)
		to.push_back(base + from[k]);
}

const char *STATUS_NAME[] = {"found_fwd", "found_rev", "absent", "no_at", "bad_step", "no_slot", "misspelled"};

// the sample named `name`, or n_samples
uint32_t sample_of(const povu_hip_call_names *names, const char *name)
{
	for (uint32_t s = 0; s < names->refs.n_samples; s++)
		if (!strcmp(names->sample[s], name))
			return s;
	return names->refs.n_samples;
}

char *to_buffer(const std::string &s, size_t *len)
{
	char *p = static_cast<char *>(malloc(s.size() + 1));
	if (!p)
		return nullptr;
	memcpy(p, s.data(), s.size());
	p[s.size()] = 0;
	if (len)
		*len = s.size();
	return p;
}

} // namespace

extern "C" povu_hip_vcf_doc *povu_hip_vcf_parse(const char *text, size_t len, uint32_t threads, char *err, size_t errlen)
try {
	if (!text && len) {
		set_err(err, errlen, "vcf parse: bad arguments");
		return nullptr;
	}
	std::unique_ptr<Doc> d(new Doc);
	// ---- the lines: the #CHROM line, the records
	std::vector<Line> lines;
	bool have_columns = false;
	uint64_t no = 0;
	for (size_t b = 0; b < len;) {
		const char *nl = static_cast<const char *>(memchr(text + b, '\n', len - b));
		size_t e = nl ? (size_t)(nl - text) : len, n = e - b;
		no++;
		if (n && text[b + n - 1] == '\r')
			n--;
		if (n && text[b] == '#') {
			if (n >= 6 && !memcmp(text + b, "#CHROM", 6) && (n == 6 || text[b + 6] == '\t')) {
				if (have_columns) {
					set_err(err, errlen, "line " + std::to_string(no) + ": a second #CHROM line");
					return nullptr;
				}
				std::vector<Span> f;
				split(text + b, n, "\t", f);
				if (f.size() < 8) {
					set_err(err, errlen, "line " + std::to_string(no) + ": the #CHROM line needs at least 8 columns, this one has " +
								     std::to_string(f.size()));
					return nullptr;
				}
				for (size_t k = 9; k < f.size(); k++)
					d->sample.emplace_back(f[k].p, f[k].n);
				have_columns = true;
			}
		} else if (n) {
			if (!have_columns) {
				set_err(err, errlen, "line " + std::to_string(no) + ": a record in front of the #CHROM line");
				return nullptr;
			}
			lines.push_back({b, n, no});
		}
		b = e + 1;
	}
	// ---- the records, in chunks
	const size_t R = lines.size();
	const size_t n_chunks = std::max<size_t>(1, std::min<size_t>(std::max<uint32_t>(1, threads), (R + 255) / 256));
	std::vector<Chunk> chunks(n_chunks);
	std::vector<std::string> thrown(n_chunks);
	auto work = [&](size_t k) {
		const size_t b = R * k / n_chunks, e = R * (k + 1) / n_chunks;
		try {
			parse_chunk(text, lines.data() + b, e - b, d->sample.size(), chunks[k]);
		} catch (const std::exception &x) {
			thrown[k] = x.what();
		}
	};
	{
		std::vector<std::thread> pool;
		for (size_t k = 1; k < n_chunks; k++)
			pool.emplace_back(work, k);
		work(0);
		for (auto &t : pool)
			t.join();
	}
	for (size_t k = 0; k < n_chunks; k++) {
		if (!thrown[k].empty()) {
			set_err(err, errlen, "vcf parse: " + thrown[k]);
			return nullptr;
		}
		if (chunks[k].bad_line) {
			set_err(err, errlen, "line " + std::to_string(chunks[k].bad_line) + ": " + chunks[k].bad);
			return nullptr;
		}
	}
	std::unordered_map<std::string, uint32_t> chrom_of; // of the document: a chunk's new strings behind those of the chunks before
	for (const Chunk &c : chunks) {
		const uint64_t r0 = d->line.size();
		std::vector<uint32_t> global(c.chrom.size());
		for (size_t k = 0; k < c.chrom.size(); k++) {
			const auto at = chrom_of.emplace(c.chrom[k], (uint32_t)d->chrom.size());
			if (at.second)
				d->chrom.push_back(c.chrom[k]);
			global[k] = at.first->second;
		}
		for (uint32_t k : c.rec_chrom)
			d->rec_chrom.push_back(global[k]);
		for (size_t r = 0; r + 1 < c.task_off.size(); r++)
			d->task_record.insert(d->task_record.end(), c.task_off[r + 1] - c.task_off[r], (uint32_t)(r0 + r));
		append(d->line, c.line);
		append(d->pos, c.pos);
		append_off(d->id_off, c.id_off);
		append_off(d->allele_off, c.allele_off);
		append_off(d->task_off, c.task_off);
		append_off(d->step_off, c.step_off);
		append_off(d->text_off, c.text_off);
		append(d->allele_walk, c.allele_walk);
		append(d->step_or, c.step_or);
		append(d->step_id, c.step_id);
		append(d->task_allele, c.task_allele);
		append(d->task_col, c.task_col);
		append(d->task_phase, c.task_phase);
		d->ids += c.ids;
		d->text += c.text;
	}
	if (d->line.size() >= 0xFFFFFFFFull) {
		set_err(err, errlen, "vcf parse: 2^32 records or more are refused");
		return nullptr;
	}
	for (auto &s : d->sample)
		d->sample_ptr.push_back(s.c_str());
	for (auto &s : d->chrom)
		d->chrom_ptr.push_back(s.c_str());
	povu_hip_vcf_doc &p = d->pub;
	p.n_samples = d->sample.size();
	p.n_records = d->line.size();
	p.n_alleles = d->allele_walk.size();
	p.n_steps = d->step_id.size();
	p.n_text_bytes = d->text.size();
	p.n_tasks = d->task_allele.size();
	p.n_id_bytes = d->ids.size();
	p.sample = d->sample_ptr.data();
	p.rec_line = d->line.data();
	p.rec_pos = d->pos.data();
	p.rec_id_off = d->id_off.data();
	p.ids = d->ids.data();
	p.allele_off = d->allele_off.data();
	p.task_off = d->task_off.data();
	p.step_off = d->step_off.data();
	p.text_off = d->text_off.data();
	p.allele_walk = d->allele_walk.data();
	p.step_id = d->step_id.data();
	p.step_or = d->step_or.data();
	p.text = d->text.data();
	p.task_record = d->task_record.data();
	p.task_allele = d->task_allele.data();
	p.task_col = d->task_col.data();
	p.task_phase = d->task_phase.data();
	p.n_chroms = d->chrom.size();
	p.chrom = d->chrom_ptr.data();
	p.rec_chrom = d->rec_chrom.data();
	return &d.release()->pub;
} catch (const std::exception &x) {
	set_err(err, errlen, std::string("vcf parse: ") + x.what());
	return nullptr;
}

extern "C" void povu_hip_vcf_doc_free(povu_hip_vcf_doc *d) { delete reinterpret_cast<Doc *>(d); }

extern "C" int povu_hip_vcf_columns(const povu_hip_vcf_doc *doc, const povu_hip_call_names *names, uint32_t *col_first, uint32_t *col_slots)
{
	if (!doc || !names || (doc->n_samples && (!col_first || !col_slots)))
		return 1;
	// the slots of a sample are consecutive
	std::vector<uint32_t> first(names->refs.n_samples + 1, 0), count(names->refs.n_samples + 1, 0);
	for (uint32_t sl = names->refs.n_slots; sl-- > 0;) {
		const uint32_t s = names->refs.sample_of_slot[sl];
		if (s >= names->refs.n_samples)
			return 1;
		first[s] = sl;
		count[s]++;
	}
	for (uint64_t c = 0; c < doc->n_samples; c++) {
		const uint32_t s = sample_of(names, doc->sample[c]);
		col_first[c] = first[s];
		col_slots[c] = count[s];
	}
	return 0;
}

extern "C" char *povu_hip_vcf_report_text(const povu_hip_vcf_report *r, const povu_hip_vcf_doc *doc, const povu_hip_call_names *names,
					  size_t *report_len, char **summary, size_t *summary_len)
try {
	if (!r || !doc || !names || !summary || r->n_records != doc->n_records || r->n_tasks != doc->n_tasks || r->n_alleles != doc->n_alleles)
		return nullptr;
	std::vector<uint32_t> col_first(doc->n_samples + 1), col_slots(doc->n_samples + 1);
	if (povu_hip_vcf_columns(doc, names, col_first.data(), col_slots.data()))
		return nullptr;
	std::string out = "rec_idx\tID\tPOS\tAT\tHap ID\tsample\treason\n";
	uint64_t n_invalid = 0;
	for (uint64_t i = 0; i < doc->n_records; i++) {
		if (!r->rec_invalid[i])
			continue;
		n_invalid++;
		const uint32_t reason = r->rec_reason[i], al = r->rec_allele[i], t = r->rec_task[i];
		if (reason > POVU_HIP_V_MISSPELLED || (reason == POVU_HIP_V_MISSPELLED ? t != POVU_HIP_NIL : t >= doc->n_tasks || doc->task_record[t] != i))
			return nullptr;
		out += std::to_string(i) + "\t";
		out.append(doc->ids + doc->rec_id_off[i], doc->rec_id_off[i + 1] - doc->rec_id_off[i]);
		out += "\t" + std::to_string(doc->rec_pos[i]) + "\t";
		const uint64_t a = doc->allele_off[i] + al;
		if (a < doc->allele_off[i + 1])
			for (uint64_t k = doc->step_off[a]; k < doc->step_off[a + 1]; k++)
				out += (doc->step_or[k] ? "<" : ">") + std::to_string(doc->step_id[k]);
		if (reason == POVU_HIP_V_MISSPELLED) {
			out += "\t.\t.";
		} else {
			const uint32_t c = doc->task_col[t], j = doc->task_phase[t];
			long long hap = 1;
			if (c >= doc->n_samples)
				return nullptr;
			if (j < col_slots[c] && names->slot_hap && names->slot_hap[col_first[c] + j] >= 0)
				hap = names->slot_hap[col_first[c] + j];
			out += "\t" + std::to_string(hap) + "\t" + doc->sample[c];
		}
		out += std::string("\t") + STATUS_NAME[reason] + "\n";
	}
	char line[64];
	if (!n_invalid)
		snprintf(line, sizeof line, "No errors\n");
	else
		snprintf(line, sizeof line, "Error rate: %.2f%%\n", (double)n_invalid / (double)doc->n_records * 100.0);
	*summary = to_buffer(line, summary_len);
	char *rep = *summary ? to_buffer(out, report_len) : nullptr;
	if (!rep) {
		free(*summary);
		*summary = nullptr;
	}
	return rep;
} catch (const std::bad_alloc &) {
	return nullptr;
}

// ---- the two files of `povu vcf --compare` (INTEGRATION.md "VCF comparison")

namespace
{
// `num / den` to four decimals, `nan` where the denominator is 0
std::string ratio(uint64_t num, uint64_t den)
{
	if (!den)
		return "nan";
	char b[32];
	snprintf(b, sizeof b, "%.4f", (double)num / (double)den);
	return b;
}
std::string rates(uint64_t both, uint64_t only_a, uint64_t only_b)
{
	return "precision " + ratio(both, both + only_a) + ", recall " + ratio(both, both + only_b) + ", F1 " + ratio(2 * both, 2 * both + only_a + only_b);
}
} // namespace

extern "C" char *povu_hip_vcf_cmp_text(const povu_hip_vcf_cmp *c, const povu_hip_vcf_doc *doc_a, const povu_hip_vcf_doc *doc_b, size_t *compare_len,
				       char **summary, size_t *summary_len)
try {
	using namespace povu_hip;
	if (!c || !doc_a || !doc_b || !summary)
		return nullptr;
	std::string out = "side\tCHROM\tPOS\tREF\tALT\trec_idx\tID\tn\n";
	for (uint64_t g = 0; g < c->n_groups; g++) {
		if (c->group_class[g] == POVU_HIP_M_SHARED)
			continue;
		const bool b = c->group_class[g] == POVU_HIP_M_ONLY_B;
		uint64_t i = c->group_first[g];
		if (b != (i >= c->n_items_a) || i >= c->n_items_a + c->n_items_b)
			return nullptr;
		i -= b ? c->n_items_a : 0;
		const povu_hip_vcf_doc *d = b ? doc_b : doc_a;
		const uint64_t r = (b ? c->item_record_b : c->item_record_a)[i], k = (b ? c->item_alt_b : c->item_alt_a)[i];
		const uint64_t s = (b ? c->item_suffix_b : c->item_suffix_a)[i], p = (b ? c->item_prefix_b : c->item_prefix_a)[i];
		if (r >= d->n_records || !k || d->allele_off[r] + k >= d->allele_off[r + 1] || d->rec_chrom[r] >= d->n_chroms)
			return nullptr;
		const uint64_t ar = d->allele_off[r], aa = ar + k;
		const uint64_t nr = d->text_off[ar + 1] - d->text_off[ar], na = d->text_off[aa + 1] - d->text_off[aa];
		if (s + p > nr || s + p > na)
			return nullptr;
		out += std::string(b ? "B" : "A") + "\t" + d->chrom[d->rec_chrom[r]] + "\t" + std::to_string((b ? c->item_pos_b : c->item_pos_a)[i]) + "\t";
		for (uint64_t x = p; x < nr - s; x++)
			out += (char)vm_fold(d->text[d->text_off[ar] + x]);
		out += "\t";
		for (uint64_t x = p; x < na - s; x++)
			out += (char)vm_fold(d->text[d->text_off[aa] + x]);
		out += "\t" + std::to_string(r) + "\t";
		out.append(d->ids + d->rec_id_off[r], d->rec_id_off[r + 1] - d->rec_id_off[r]);
		out += "\t" + std::to_string((uint64_t)c->group_n_a[g] + c->group_n_b[g]) + "\n";
	}
	uint64_t tp = 0, fp = 0, fn = 0, gteq = 0;
	for (uint64_t x = 0; x < c->n_common_samples; x++)
		tp += c->sample_tp[x], fp += c->sample_fp[x], fn += c->sample_fn[x], gteq += c->sample_gteq[x];
	std::string sum = "Alleles: shared " + std::to_string(c->n_shared) + ", only A " + std::to_string(c->n_only_a) + ", only B " +
			  std::to_string(c->n_only_b) + "\n";
	sum += "Alleles: " + rates(c->n_shared, c->n_only_a, c->n_only_b) + "\n";
	sum += "Genotypes: tp " + std::to_string(tp) + ", fp " + std::to_string(fp) + ", fn " + std::to_string(fn) + ", gteq " + std::to_string(gteq) + "\n";
	sum += "Genotypes: " + rates(tp, fp, fn) + "\n";
	for (uint64_t x = 0; x < c->n_common_samples; x++) {
		if (c->sample_col_a[x] >= doc_a->n_samples)
			return nullptr;
		sum += std::string("Sample ") + doc_a->sample[c->sample_col_a[x]] + ": tp " + std::to_string(c->sample_tp[x]) + ", fp " +
		       std::to_string(c->sample_fp[x]) + ", fn " + std::to_string(c->sample_fn[x]) + ", gteq " + std::to_string(c->sample_gteq[x]) + "\n";
	}
	if (c->n_skipped_a || c->n_skipped_b)
		sum += "Skipped alleles: A " + std::to_string(c->n_skipped_a) + ", B " + std::to_string(c->n_skipped_b) + "\n";
	if (c->n_samples_only_a || c->n_samples_only_b)
		sum += "Unmatched sample columns: A " + std::to_string(c->n_samples_only_a) + ", B " + std::to_string(c->n_samples_only_b) + "\n";
	*summary = to_buffer(sum, summary_len);
	char *rep = *summary ? to_buffer(out, compare_len) : nullptr;
	if (!rep) {
		free(*summary);
		*summary = nullptr;
	}
	return rep;
} catch (const std::bad_alloc &) {
	return nullptr;
}

// ---- the two files of `povu vcf --compare --haplotypes` (INTEGRATION.md "Haplotype comparison")

extern "C" char *povu_hip_vcf_hap_text(const povu_hip_vcf_hap *h, const povu_hip_vcf_doc *doc_a, const povu_hip_vcf_doc *doc_b, size_t *haplotypes_len,
				       char **summary, size_t *summary_len)
try {
	static const char *NAME[POVU_HIP_H_N_STATUS] = {"inconsistent", "nocall_a", "nocall_b", "unspelled_a", "unspelled_b",
							"conflict_a",	"conflict_b", "equal_ref", "equal",	  "differ"};
	if (!h || !doc_a || !doc_b || !summary)
		return nullptr;
	// the CHROM strings as the comparison numbers them: A's in order of first appearance, then B's new ones
	std::vector<std::string> chrom;
	for (const povu_hip_vcf_doc *d : {doc_a, doc_b})
		for (uint64_t k = 0; k < d->n_chroms; k++)
			if (d->chrom[k] && std::find(chrom.begin(), chrom.end(), d->chrom[k]) == chrom.end())
				chrom.push_back(d->chrom[k]);
	std::string out = "CHROM\tSTART\tEND\tsample\tphase\tstatus\tlen_a\tlen_b\tfirst_diff\tedits_a\tedits_b\n";
	for (uint64_t c = 0; c < h->n_cells; c++) {
		const uint32_t st = h->cell_status[c], w = h->cell_window[c], x = h->cell_sample[c];
		if (st >= POVU_HIP_H_N_STATUS || w >= h->n_windows || x >= h->n_common_samples || h->win_chrom[w] >= chrom.size() ||
		    h->sample_col_a[x] >= doc_a->n_samples)
			return nullptr;
		if (st == POVU_HIP_H_EQUAL_REF || st == POVU_HIP_H_EQUAL)
			continue;
		const bool compared = st == POVU_HIP_H_DIFFER;
		out += chrom[h->win_chrom[w]] + "\t" + std::to_string(h->win_lo[w] + 1) + "\t" + std::to_string(h->win_hi[w]) + "\t" +
		       doc_a->sample[h->sample_col_a[x]] + "\t" + std::to_string(h->cell_phase[c]) + "\t" + NAME[st] + "\t";
		out += (compared ? std::to_string(h->cell_len_a[c]) : std::string(".")) + "\t" + (compared ? std::to_string(h->cell_len_b[c]) : std::string(".")) +
		       "\t" + (compared ? std::to_string(h->cell_first_diff[c]) : std::string(".")) + "\t";
		out += std::to_string(h->cell_edits_a[c]) + "\t" + std::to_string(h->cell_edits_b[c]) + "\n";
	}
	auto counts = [&](const uint64_t *n) {
		std::string s;
		for (uint32_t k = 0; k < POVU_HIP_H_N_STATUS; k++)
			s += std::string(k ? ", " : "") + NAME[k] + " " + std::to_string(n[k]);
		return s;
	};
	const uint64_t *n = h->n_status;
	const uint64_t same = n[POVU_HIP_H_EQUAL_REF] + n[POVU_HIP_H_EQUAL];
	std::string sum = "Windows: " + std::to_string(h->n_windows) + ", inconsistent " + std::to_string(h->n_inconsistent) + "\n";
	sum += "Cells: " + counts(n) + "\n";
	sum += "Concordance: " + ratio(same, same + n[POVU_HIP_H_DIFFER]) + "\n";
	sum += "Non-reference concordance: " + ratio(n[POVU_HIP_H_EQUAL], n[POVU_HIP_H_EQUAL] + n[POVU_HIP_H_DIFFER]) + "\n";
	for (uint64_t x = 0; x < h->n_common_samples; x++) {
		if (h->sample_col_a[x] >= doc_a->n_samples)
			return nullptr;
		sum += std::string("Sample ") + doc_a->sample[h->sample_col_a[x]] + ": " + counts(h->sample_status + x * POVU_HIP_H_N_STATUS) + "\n";
	}
	if (h->n_unplaced_a || h->n_unplaced_b)
		sum += "Unplaced records: A " + std::to_string(h->n_unplaced_a) + ", B " + std::to_string(h->n_unplaced_b) + "\n";
	if (h->n_reach_capped)
		sum += "Capped reaches: " + std::to_string(h->n_reach_capped) + "\n";
	*summary = to_buffer(sum, summary_len);
	char *rep = *summary ? to_buffer(out, haplotypes_len) : nullptr;
	if (!rep) {
		free(*summary);
		*summary = nullptr;
	}
	return rep;
} catch (const std::bad_alloc &) {
	return nullptr;
}

// ---- the three files of `povu vcf --consensus` (INTEGRATION.md "Consensus haplotypes")

extern "C" char *povu_hip_vcf_cons_text(const povu_hip_vcf_cons *c, const povu_hip_vcf_doc *doc, const povu_hip_call_names *names,
					const char *const *path_name, uint32_t width, size_t *fasta_len, char **roundtrip, size_t *roundtrip_len,
					char **summary, size_t *summary_len)
try {
	static const char *NAME[POVU_HIP_C_N_RT] = {"none", "equal", "differ", "no_path", "ambiguous"};
	if (!c || !doc || !names || !roundtrip || !summary || (names->n_paths && !path_name))
		return nullptr;
	std::vector<uint32_t> col_first(doc->n_samples + 1), col_slots(doc->n_samples + 1);
	if (povu_hip_vcf_columns(doc, names, col_first.data(), col_slots.data()))
		return nullptr;
	std::string fa, rt = "CHROM\tsample\tphase\tstatus\tlen\tpath\tpath_len\tfirst_diff\tapplied\tduplicate\tenclosed\toverlap\tunspelled\tnocall\n";
	uint64_t n_rt[POVU_HIP_C_N_RT] = {0}, n_kind[6] = {0};
	for (uint64_t h = 0; h < c->n_haps; h++) {
		const uint32_t ch = c->hap_chrom[h], col = c->hap_col[h], j = c->hap_phase[h], st = c->rt_status[h], p = c->rt_path[h];
		if (ch >= doc->n_chroms || !doc->chrom[ch] || col >= doc->n_samples || st >= POVU_HIP_C_N_RT || (p != POVU_HIP_NIL && p >= names->n_paths) ||
		    (c->text && c->hap_off[h] + c->hap_len[h] > c->n_text_bytes))
			return nullptr;
		const uint32_t counts[6] = {c->n_applied[h], c->n_duplicate[h], c->n_enclosed[h], c->n_overlap[h], c->n_unspelled[h], c->n_nocall[h]};
		n_rt[st]++;
		for (int k = 0; k < 6; k++)
			n_kind[k] += counts[k];
		if (c->text) {
			long long hap = j;
			if (j < col_slots[col] && names->slot_hap && names->slot_hap[col_first[col] + j] >= 0)
				hap = names->slot_hap[col_first[col] + j];
			fa += std::string(">") + doc->sample[col] + "#" + std::to_string(hap) + "#" + doc->chrom[ch] + "\n";
			const char *t = c->text + c->hap_off[h];
			const uint64_t n = c->hap_len[h], step = width ? width : (n ? n : 1);
			for (uint64_t k = 0; k < n; k += step) {
				fa.append(t + k, std::min(step, n - k));
				fa += "\n";
			}
		}
		if (st == POVU_HIP_C_RT_EQUAL)
			continue;
		rt += std::string(doc->chrom[ch]) + "\t" + doc->sample[col] + "\t" + std::to_string(j) + "\t" + NAME[st] + "\t" + std::to_string(c->hap_len[h]) + "\t";
		rt += (p != POVU_HIP_NIL ? std::string(path_name[p]) : std::string(".")) + "\t" + (p != POVU_HIP_NIL ? std::to_string(c->rt_path_len[h]) : std::string(".")) + "\t";
		rt += st == POVU_HIP_C_RT_DIFFER ? std::to_string(c->rt_first_diff[h]) : std::string(".");
		for (int k = 0; k < 6; k++)
			rt += "\t" + std::to_string(counts[k]);
		rt += "\n";
	}
	static const char *KIND[6] = {"applied", "duplicate", "enclosed", "overlap", "unspelled", "nocall"};
	std::string sum = "Haplotypes: " + std::to_string(c->n_haps) + ", bases " + std::to_string(c->n_text_bytes) + "\nRound trip: ";
	for (uint32_t k = 0; k < POVU_HIP_C_N_RT; k++)
		sum += std::string(k ? ", " : "") + NAME[k] + " " + std::to_string(n_rt[k]);
	sum += "\nEdits: ";
	for (int k = 0; k < 6; k++)
		sum += std::string(k ? ", " : "") + KIND[k] + " " + std::to_string(n_kind[k]);
	sum += "\n";
	if (c->n_unplaced)
		sum += "Unplaced records: " + std::to_string(c->n_unplaced) + "\n";
	*summary = to_buffer(sum, summary_len);
	*roundtrip = *summary ? to_buffer(rt, roundtrip_len) : nullptr;
	char *out = *roundtrip ? to_buffer(fa, fasta_len) : nullptr;
	if (!out) {
		free(*summary);
		free(*roundtrip);
		*summary = *roundtrip = nullptr;
	}
	return out;
} catch (const std::bad_alloc &) {
	return nullptr;
}
