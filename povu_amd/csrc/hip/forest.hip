// forest.hip -- what a caller does with a finished forest (include/povu_hip.h): its counts, waits and times, the views of a
// tree's PVST arrays, of its labels and of its extended tree of -s, the site table, and the PVST text of a tree, a thin
// selector over the writer of host/pvst_io.cpp.
#include "context.hpp"

#include <algorithm>
#include <cstdlib>
#include <vector>

using namespace povu_hip;

extern "C" uint32_t povu_hip_forest_total_components(const povu_hip_forest *f) { return f ? f->total_components : 0; }
extern "C" uint32_t povu_hip_forest_tree_count(const povu_hip_forest *f) { return f ? (uint32_t)f->trees.size() : 0; }

extern "C" int povu_hip_forest_wait(povu_hip_forest *f)
{
	if (!f)
		return 1;
	f->ready();
	return 0;
}
extern "C" double povu_hip_forest_pass_ms(povu_hip_forest *f)
{
	if (!f)
		return -1.0;
	f->ready();
	return f->pass_ms;
}

extern "C" double povu_hip_forest_span_ms(povu_hip_forest *first, povu_hip_forest *last)
{
	if (!first || !last || !first->ev0 || !last->ev1)
		return -1.0;
	first->ready();
	last->ready();
	float ms = 0;
	return hipEventElapsedTime(&ms, first->ev0, last->ev1) == hipSuccess ? (double)ms : -1.0;
}

extern "C" int povu_hip_forest_get(const povu_hip_forest *f, uint32_t i, povu_hip_tree *out)
{
	if (!f || !out || i >= f->trees.size())
		return 1;
	const_cast<povu_hip_forest *>(f)->ready(); // (the arrays of a POVU_HIP_F_ASYNC forest may still be on their way)
	const auto &t = f->trees[i];
	out->component_id = t.component_id;
	out->n_vtx = t.n_vtx;
	out->n_links = t.n_links;
	out->n_pvst = t.n_pvst;
	const auto &b = f->blocks[(size_t)t.blk];
	out->a_id = b.a + t.off;
	out->z_id = b.z + t.off;
	out->a_or = b.aor + t.off;
	out->z_or = b.zor + t.off;
	out->parent = b.parent + t.off;
	out->n_hairpins = t.n_hairpins;
	out->hairpins = t.n_hairpins ? f->hairpins.data() + 2 * t.hp_off : nullptr;
	return 0;
}

extern "C" int povu_hip_forest_raw(const povu_hip_forest *f, const void **block, size_t *bytes, uint64_t *total,
				   uint64_t offsets[5])
{
	if (!f || !block || !bytes || !total || !offsets || f->blocks.size() > 1)
		return 1; // (several blocks -- a merged forest, a mixed pass: no single raw view)
	const_cast<povu_hip_forest *>(f)->ready();
	if (f->blocks.empty()) { // (a forest without trees, of a shard without components)
		*block = nullptr, *bytes = 0, *total = 0;
		std::fill(offsets, offsets + 5, 0ull);
		return 0;
	}
	const auto &b = f->blocks[0];
	*block = b.p;
	*bytes = b.bytes;
	*total = b.total;
	const char *p = static_cast<const char *>(b.p);
	offsets[0] = (uint64_t)((const char *)b.a - p);
	offsets[1] = (uint64_t)((const char *)b.z - p);
	offsets[2] = (uint64_t)((const char *)b.parent - p);
	offsets[3] = (uint64_t)((const char *)b.aor - p);
	offsets[4] = (uint64_t)((const char *)b.zor - p);
	return 0;
}

extern "C" uint64_t povu_hip_forest_first(const povu_hip_forest *f, uint32_t i)
{
	return (f && i < f->trees.size()) ? (uint64_t)f->trees[i].off : 0;
}

extern "C" void povu_hip_forest_free(povu_hip_forest *f) { delete f; }

// mto::to_pvst::write_pvst, src/mto/to_pvst.cpp:23-109
extern "C" int povu_hip_forest_get_sub(const povu_hip_forest *f, uint32_t i, const uint32_t **ai, const uint32_t **zi,
				       const uint8_t **fam)
{
	if (!f || i >= f->trees.size())
		return 1;
	const auto &t = f->trees[i];
	const auto &b = f->blocks[(size_t)t.blk];
	if (!f->labels || t.off + t.n_pvst > b.sub_fam.size())
		return 3; // the forest was not decomposed with POVU_HIP_F_LEAF_SUBFLUBBLES
	if (ai)
		*ai = b.sub_ai.data() + t.off;
	if (zi)
		*zi = b.sub_zi.data() + t.off;
	if (fam)
		*fam = b.sub_fam.data() + t.off;
	return 0;
}

extern "C" int povu_hip_forest_get_subtree(const povu_hip_forest *f, uint32_t i, povu_hip_subtree *out)
{
	if (!f || !out || i >= f->trees.size())
		return 1;
	const_cast<povu_hip_forest *>(f)->ready();
	const auto &t = f->trees[i];
	const SubForest *x = f->blocks[(size_t)t.blk].subx.get();
	if (!x || t.sub_c + 1 >= x->voff.size())
		return 3; // the forest was not decomposed with POVU_HIP_F_SUBFLUBBLES
	const uint64_t b = x->voff[t.sub_c], e = x->voff[t.sub_c + 1];
	out->n_total = (uint32_t)(e - b);
	out->n_flubble_like = t.n_pvst;
	out->n_concealed = x->counts[3 * (size_t)t.sub_c];
	out->n_midi = x->counts[3 * (size_t)t.sub_c + 1];
	out->n_smothered = x->counts[3 * (size_t)t.sub_c + 2];
	out->fam = x->fam + b;
	out->or1 = x->or1 + b;
	out->or2 = x->or2 + b;
	out->route = x->route + b;
	out->id1 = x->id1 + b;
	out->id2 = x->id2 + b;
	out->child_off = x->coff + b;
	out->child = x->child;
	return 0;
}

// the sites of every tree through povu_hip_sites_add_tree (host/vcf.cpp): the extended tree of -s, else the PVST with the T / O
// letters of --leaf-subflubbles, else the PVST as it is
extern "C" povu_hip_sites *povu_hip_forest_sites(const povu_hip_forest *f)
{
	auto *s = f ? static_cast<povu_hip_sites *>(calloc(1, sizeof(povu_hip_sites))) : nullptr;
	std::vector<uint32_t> par;
	for (uint32_t i = 0; s && i < f->trees.size(); i++) {
		povu_hip_subtree x;
		povu_hip_tree t;
		const uint8_t *fam = nullptr;
		int rc;
		if (povu_hip_forest_get_subtree(f, i, &x) == 0) {
			par.assign(x.n_total, POVU_HIP_NIL);
			for (uint32_t v = 0; v < x.n_total; v++)
				for (uint32_t k = x.child_off[v]; k < x.child_off[v + 1]; k++)
					if (x.child[k] < x.n_total)
						par[x.child[k]] = v;
			rc = povu_hip_sites_add_tree(s, i, x.n_total, x.id1, x.id2, x.or1, x.or2, par.data(), x.fam);
		} else {
			rc = povu_hip_forest_get(f, i, &t);
			povu_hip_forest_get_sub(f, i, nullptr, nullptr, &fam); // (leaves fam null when the forest carries no letters)
			rc = rc ? rc : povu_hip_sites_add_tree(s, i, t.n_pvst, t.a_id, t.z_id, t.a_or, t.z_or, t.parent, fam);
		}
		if (rc) {
			povu_hip_sites_free(s);
			s = nullptr;
		}
	}
	return s;
}

extern "C" char *povu_hip_forest_pvst_text(const povu_hip_forest *f, uint32_t i, size_t *len)
{
	povu_hip_subtree st;
	if (povu_hip_forest_get_subtree(f, i, &st) == 0)
		return povu_hip_pvst_format_subtree(&st, len);
	povu_hip_tree t;
	if (povu_hip_forest_get(f, i, &t) != 0)
		return nullptr;
	const uint8_t *fam = nullptr;
	if (povu_hip_forest_get_sub(f, i, nullptr, nullptr, &fam) != 0)
		fam = nullptr;
	return povu_hip_pvst_format_fam(t.n_pvst, t.a_id, t.z_id, t.a_or, t.z_or, t.parent, fam, len);
}
