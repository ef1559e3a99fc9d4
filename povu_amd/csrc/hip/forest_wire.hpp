// forest_wire.hpp -- every byte format in which a forest leaves its process, and every bound on what comes back in: the
// 8-word tree table (povu_hip_forest_share / _attach, povu_hip_comm_gather), the packed forest "pv_frst1"
// (povu_hip_forest_pack / _merge), the extras segment "v_sharex", the block of the extended trees of -s.  Plain C++17, no
// HIP: host/asan_check.cpp runs it under the sanitizers.  Numbers from another process are bounded here, before they size
// or index anything and without arithmetic that can wrap; a decoder returns null, or what is wrong.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace forest_wire
{
inline size_t pad64(size_t b) { return (b + 63) & ~size_t(63); }

// ---------------------------------------------------------------- a PVST block
// the five arrays of a block of `total` PVST vertices, each padded to 64 B: a | z | parent | a_or | z_or.  The forest's
// page-locked blocks, the class stage's device block and the copies between the two all take their offsets from here.
struct PvstArrays {
	uint32_t *a = nullptr, *z = nullptr, *parent = nullptr;
	uint8_t *aor = nullptr, *zor = nullptr; // 0 forward, 1 reverse
	static size_t word_bytes(size_t total) { return pad64(total * 4); } // one of a, z, parent
	static size_t flag_bytes(size_t total) { return pad64(total); }	    // one of a_or, z_or
	// places the arrays in the block at `q`; returns the bytes they take (out == nullptr: only measures)
	static size_t layout(void *q, size_t total, PvstArrays *out = nullptr)
	{
		const size_t w = word_bytes(total), b = flag_bytes(total);
		if (out) {
			char *c = static_cast<char *>(q);
			out->a = (uint32_t *)c, out->z = (uint32_t *)(c + w), out->parent = (uint32_t *)(c + 2 * w);
			out->aor = (uint8_t *)(c + 3 * w), out->zor = (uint8_t *)(c + 3 * w + b);
		}
		return 3 * w + 2 * b;
	}
	// what layout() takes at most, linear in `total`: 14 bytes a vertex and one 64 B step per array
	static size_t bound(size_t total) { return 3 * (total * 4 + 64) + 2 * (total + 64); }
};

// ---------------------------------------------------------------- the tree table
// one tree of a block: 8 words {component_id, n_vtx, n_links, n_pvst, off lo, off hi, n_hairpins, sub_c}
struct TreeRecord {
	uint32_t component_id, n_vtx, n_links, n_pvst;
	uint64_t off;	 // first PVST vertex in the block's arrays
	uint64_t hp_off; // first hairpin pair (not on the wire: the pairs follow tree order)
	uint32_t n_hairpins;
	uint32_t sub_c; // with POVU_HIP_F_SUBFLUBBLES: its component in the block's extended trees
};
constexpr size_t TREE_WORDS = 8;

inline bool in_block(const TreeRecord &t, uint64_t total) { return t.off <= total && t.n_pvst <= total - t.off; }

// `n` trees (anything derived from TreeRecord) of a block of `total` PVST vertices -> words[8 n]; `extras`: with the
// hairpin count and the component in the extended trees (else zero).  False: a tree lies outside the block.
template <typename Tree>
bool encode_tree_table(uint32_t *words, const Tree *trees, size_t n, uint64_t total, bool extras)
{
	for (size_t i = 0; i < n; i++) {
		const TreeRecord &t = trees[i];
		if (!in_block(t, total))
			return false;
		uint32_t *q = words + TREE_WORDS * i;
		q[0] = t.component_id, q[1] = t.n_vtx, q[2] = t.n_links, q[3] = t.n_pvst;
		q[4] = (uint32_t)(t.off & 0xFFFFFFFFu), q[5] = (uint32_t)(t.off >> 32);
		q[6] = extras ? t.n_hairpins : 0, q[7] = extras ? t.sub_c : 0;
	}
	return true;
}

// words[n_words] -> `n_trees` trees appended to `out`, each inside a block of `total` PVST vertices.  With `has_extras` the
// hairpin counts (together at most `pairs`; hp_off counts from 0) and sub_c (n_sub_components = entries of the extended
// trees' voff, 0 = none: not checked) are read too.
template <typename Tree>
const char *decode_tree_table(const uint32_t *words, size_t n_words, size_t n_trees, uint64_t total, bool has_extras, uint64_t pairs,
			      uint64_t n_sub_components, std::vector<Tree> &out)
{
	if (n_trees > n_words / TREE_WORDS)
		return "the tree table is longer than its buffer";
	uint64_t hp_seen = 0;
	for (size_t i = 0; i < n_trees; i++) {
		const uint32_t *q = words + TREE_WORDS * i;
		Tree t{};
		t.component_id = q[0], t.n_vtx = q[1], t.n_links = q[2], t.n_pvst = q[3];
		t.off = (uint64_t)q[4] | ((uint64_t)q[5] << 32);
		if (!in_block(t, total))
			return "a tree lies outside its block";
		if (has_extras) {
			t.n_hairpins = q[6], t.sub_c = q[7];
			if (n_sub_components && (uint64_t)t.sub_c + 1 >= n_sub_components)
				return "a tree names a component its extended trees do not have";
			if (t.n_hairpins > pairs - hp_seen)
				return "the hairpin boundaries do not add up";
			t.hp_off = hp_seen;
			hp_seen += t.n_hairpins;
		}
		out.push_back(t);
	}
	return nullptr;
}

// ---------------------------------------------------------------- packed forest ("pv_frst1")
// [header 8 x u64 {n_trees, total, total_components, magic} | 4 words per tree | a | z | parent | a_or | z_or], 64-byte sections
constexpr uint64_t FOREST_MAGIC = 0x31747372665F7670ull;
struct ForestLayout {
	size_t meta, a, z, parent, aor, zor, bytes;
	ForestLayout(size_t n_trees, size_t total)
	{
		size_t o = 64;
		meta = o, o += pad64(n_trees * 16);
		a = o, o += pad64(total * 4);
		z = o, o += pad64(total * 4);
		parent = o, o += pad64(total * 4);
		aor = o, o += pad64(total);
		zor = o, o += pad64(total);
		bytes = o;
	}
	static void write_header(uint64_t h[8], size_t n_trees, size_t total, uint32_t total_components)
	{
		for (int i = 0; i < 8; i++)
			h[i] = 0;
		h[0] = n_trees, h[1] = total, h[2] = total_components, h[3] = FOREST_MAGIC;
	}
	// the header of a buffer of `bytes` (>= 64): its counts, bounded by the buffer
	static const char *read_header(const uint64_t *h, size_t bytes, size_t &n_trees, size_t &total)
	{
		if (h[3] != FOREST_MAGIC)
			return "packed forest: bad magic word";
		if (h[0] > bytes / 16 || h[1] > bytes / 4 || ForestLayout(h[0], h[1]).bytes > bytes)
			return "packed forest has the wrong size";
		n_trees = h[0], total = h[1];
		return nullptr;
	}
};

// ---------------------------------------------------------------- the extended trees of -s
// fam | or1 | or2 | route (u8 per vertex) | id1 | id2 (u32 per vertex) | coff (u32, vertices + 1) | child (u32), 64-byte
// sections from `at`; `spare` more entries in every array but coff
struct SubBlockLayout {
	size_t fam = 0, or1 = 0, or2 = 0, route = 0, id1 = 0, id2 = 0, coff = 0, child = 0, end = 0;
	SubBlockLayout() = default;
	SubBlockLayout(size_t nv, size_t nc, size_t at = 0, size_t spare = 0)
	{
		size_t q = at;
		auto sec = [&](size_t b) {
			const size_t r = q;
			q += pad64(b);
			return r;
		};
		fam = sec(nv + spare), or1 = sec(nv + spare), or2 = sec(nv + spare), route = sec(nv + spare);
		id1 = sec((nv + spare) * 4), id2 = sec((nv + spare) * 4), coff = sec((nv + 1) * 4), child = sec((nc + spare) * 4);
		end = q;
	}
};

// voff[c1]: vertices of the components, coff[nv + 1]: children of the vertices, child[nc]: indices inside a component
inline const char *validate_subforest(const uint64_t *voff, size_t c1, const uint32_t *coff, size_t nv, const uint32_t *child, size_t nc)
{
	if (c1 == 0)
		return nv || nc ? "extended trees without components" : nullptr;
	if (voff[0] != 0 || voff[c1 - 1] != nv)
		return "the extended trees do not add up";
	for (size_t c = 0; c + 1 < c1; c++)
		if (voff[c] > voff[c + 1]) // (with the last entry == nv: every entry indexes coff)
			return "the components of the extended trees overlap";
	if (coff[nv] != nc)
		return "the children lists of the extended trees do not add up";
	for (size_t v = 0; v < nv; v++)
		if (coff[v] > coff[v + 1]) // (with the last entry == nc: no component's stretch of `child` runs backwards or past the end)
			return "the children lists of the extended trees overlap";
	for (size_t c = 0; c + 1 < c1; c++) {
		const uint64_t n = voff[c + 1] - voff[c];
		for (size_t k = coff[voff[c]]; k < coff[voff[c + 1]]; k++)
			if (child[k] >= n)
				return "a child of the extended trees lies outside its component";
	}
	return nullptr;
}

// ---------------------------------------------------------------- shared-memory gather ("v_share1", "v_sharex")
// The 64-byte descriptor {magic, segment | ~0, its size, trees, PVST vertices, total components, offset of the tree table,
// rank}; the table's 64-byte header {magic, trees, PVST vertices, extras segment | ~0, its mapped size, its bytes used}.
constexpr uint64_t SHARE_MAGIC = 0x3165726168735F76ull;
constexpr uint64_t SHARE_EMPTY = ~0ull;
// What the five arrays do not hold -- the leaf passes' labels (ai, zi, line letter per PVST vertex), the hairpin boundaries,
// the extended trees of `-s` -- travels in a SECOND shared-memory segment.  Sections, each padded to 64 bytes, behind a
// 128-byte header {magic, PVST vertices, hairpin pairs, flags, components + 1 of the extended trees, their vertices, their
// child entries, bytes}: [ai][zi] u32 x total, [letter] u8 x total | [pairs] 2 x u64 | [voff] u64, [counts] u32 x 3, then a
// SubBlockLayout.
constexpr uint64_t SHAREX_MAGIC = 0x7865726168735F76ull;
struct XLayout {
	size_t total = 0, pairs = 0, c1 = 0, nv = 0, nc = 0;
	bool labels = false, hp = false, sub = false;
	size_t o_ai = 0, o_zi = 0, o_fam = 0, o_hp = 0, o_voff = 0, o_cnt = 0, bytes = 0;
	SubBlockLayout x;
	void plan()
	{
		size_t q = 128;
		auto sec = [&](size_t b) {
			const size_t r = q;
			q += pad64(b);
			return r;
		};
		if (labels)
			o_ai = sec(total * 4), o_zi = sec(total * 4), o_fam = sec(total);
		if (hp)
			o_hp = sec(pairs * 16);
		if (sub) {
			o_voff = sec(c1 * 8), o_cnt = sec((c1 ? c1 - 1 : 0) * 12);
			x = SubBlockLayout(nv, nc, q);
			q = x.end;
		}
		bytes = q;
	}
	void write_header(uint64_t h[16]) const
	{
		for (int i = 0; i < 16; i++)
			h[i] = 0;
		h[0] = SHAREX_MAGIC, h[1] = total, h[2] = pairs, h[3] = (labels ? 1u : 0u) | (hp ? 2u : 0u) | (sub ? 4u : 0u);
		h[4] = c1, h[5] = nv, h[6] = nc, h[7] = bytes;
	}
	// the header of a segment of which `xbytes` (>= 128) are used, beside a block of `want_total` PVST vertices; plans the layout
	const char *read_header(const uint64_t *h, size_t xbytes, size_t want_total)
	{
		if (h[0] != SHAREX_MAGIC || h[1] != want_total || h[7] != xbytes)
			return "does not match its forest";
		total = want_total, pairs = h[2], labels = h[3] & 1u, hp = h[3] & 2u, sub = h[3] & 4u;
		c1 = h[4], nv = h[5], nc = h[6];
		if ((labels && total > xbytes / 4) || pairs > xbytes / 16 || c1 > xbytes / 8 || nv > xbytes || nc > xbytes / 4)
			return "names sizes beyond itself";
		plan();
		return bytes == xbytes ? nullptr : "has another layout than its header says";
	}
};
} // namespace forest_wire
