// sub_kernels.hpp -- the three inserting passes of `povu decompose -s`: find_concealed, find_midi,
// find_smothered, see sub_kernels.hip
#pragma once
#include "forest_wire.hpp"
#include "leaf_kernels.hpp"

#include <memory>
#include <vector>

struct PinnedPool; // (context.hpp: the pool of page-locked result blocks of a context)

namespace povu_hip
{

// PVST line letters of the inserted vertices (include/povu/common/constants.hpp:53-60)
static constexpr uint8_t FAM_CONCEALED = 'C', FAM_MIDI = 'M', FAM_SMOTHERED = 'S';

// The PVSTs of one pass after all five passes of -s, on the host: component c owns the vertices [voff[c], voff[c + 1])
// (its own numbering starts at 0 = the dummy root; the flubble-like vertices keep their indices, the inserted ones
// follow) and every vertex its children in the reference's order.  The arrays lie in ONE page-locked block of the
// context's pool (the copies from the device run at link speed; the block goes back to the pool with the forest).
struct SubForest {
	std::vector<uint64_t> voff;   // [C + 1]
	std::vector<uint32_t> counts; // [3 C] concealed, midi, smothered vertices per component
	uint64_t n_vtx = 0, n_child = 0;
	const uint8_t *fam = nullptr, *or1 = nullptr, *or2 = nullptr, *route = nullptr; // per vertex: line letter, orientations ('>' = 0), 'L' / 'R' / 0
	const uint32_t *id1 = nullptr, *id2 = nullptr; // the two boundaries in print order
	const uint32_t *coff = nullptr;		       // [vertices + 1] children of a vertex: child[coff[x] .. coff[x + 1])
	const uint32_t *child = nullptr;	       // PVST indices inside the component
	std::shared_ptr<::PinnedPool> pool;
	void *blk = nullptr;
	size_t blk_cap = 0;
	int blk_seg = -1;
	SubForest() = default;
	SubForest(const SubForest &) = delete;
	SubForest &operator=(const SubForest &) = delete;
	~SubForest();
	void point(const char *base, const forest_wire::SubBlockLayout &L) // the eight arrays: sections of one block
	{
		fam = (const uint8_t *)(base + L.fam), or1 = (const uint8_t *)(base + L.or1), or2 = (const uint8_t *)(base + L.or2);
		route = (const uint8_t *)(base + L.route), id1 = (const uint32_t *)(base + L.id1), id2 = (const uint32_t *)(base + L.id2);
		coff = (const uint32_t *)(base + L.coff), child = (const uint32_t *)(base + L.child);
	}
};

// The device tables of the inserting passes: one arena per phase, carved when the phase's sizes are known (sub_kernels.hip:
// tables_spans .. out_spans; DESIGN.md §4 lists them).  A context keeps them from one -s pass to the next -- an arena only
// grows, and every pass carves it anew from offset 0 -- and a pass without -s releases them.
// The six are declared once, X(name): the list makes the members and for_each_arena.
#define POVU_SUB_ARENAS(X) X(tables) X(concealed) X(smothered) X(xspace) X(children) X(out)
struct SubArenas {
#define POVU_ARENA_MEMBER(name) Arena name;
	POVU_SUB_ARENAS(POVU_ARENA_MEMBER)
#undef POVU_ARENA_MEMBER
	template <class Self, class F>
	static void visit_arenas(Self &s, F &&f) // f(name, arena), in declaration order
	{
#define POVU_ARENA_VISIT(name) f(#name, s.name);
		POVU_SUB_ARENAS(POVU_ARENA_VISIT)
#undef POVU_ARENA_VISIT
	}
	template <class F>
	void for_each_arena(F &&f) { visit_arenas(*this, f); }
	template <class F>
	void for_each_arena(F &&f) const { visit_arenas(*this, f); }
	void release();
	size_t capacity() const; // bytes held, all six together
	// Where the last pass left the splice's pool layout in `xspace` (tests: povu_hip_debug_splice_pool reads how full each
	// component's stretch got): poff[C + 1], and ptop[C] when the splice ran (null: no PVST vertex, nothing was pushed).
	// Pointers into the arena, valid until the next pass carves or releases it.
	const uint32_t *pool_off = nullptr, *pool_top = nullptr;
	uint32_t pool_comps = 0;
};

// Runs find_concealed, find_midi and find_smothered on the state leaf_prepare / leaf_dense left (an all-parallel pass whose
// tree stage also wrote the depths), all on the stream s; the result is on the host, in `out`, when it returns.  Throws
// HipError when a table outgrows its bound.  Reads its test and debug switches (POVU_HIP_SUB_*) from the environment on
// every call.
void run_subflubbles(const CompState &cs, const SeqWs &sw, const ParWs &pw, const TreeWs &tw, const LeafState &ls, uint32_t C,
		     HostScratch &host, SubForest &out, const std::shared_ptr<::PinnedPool> &pool, hipStream_t s, SubArenas &arenas);

} // namespace povu_hip
