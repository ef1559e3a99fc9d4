// common.hpp -- shared declarations of the gfx950 decompose library.
#pragma once
#include <hip/hip_runtime.h>

#include "forest_wire.hpp"
#include "search_rules.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#define POVU_NIL 0xFFFFFFFFu

// four consecutive words from a 4-byte aligned address in ONE load instruction (global_load_dwordx4 only needs dword
// alignment); the caller makes sure the array carries three words of slack behind the last one it may name
__device__ __forceinline__ uint4 load4_unaligned(const unsigned *__restrict__ p)
{
	typedef unsigned v4a __attribute__((ext_vector_type(4), aligned(4)));
	const v4a v = *reinterpret_cast<const v4a *>(p);
	return make_uint4(v.x, v.y, v.z, v.w);
}

// ---- conditional gathers that leave together.  `cond ? p[i] : dflt` with a per-lane cond compiles to a branch around the
// load, and where the address inside the branch comes from an earlier load the first instruction there drains the memory
// counter (vmcnt(0)): gfx950 counts loads and stores in ONE in-order counter, and the compiler cannot know how many younger
// loads the branches it skipped have issued.  Four "simultaneous" gathers written that way are four round trips.
// gather_if and its kin load UNCONDITIONALLY from a clamped index (a 16-byte record: gather_if<uint4>), so that a batch of
// them is one run of load instructions behind one counted wait.  `safe` is an index the lane may ALWAYS read -- normally its
// own element, or element 0 of an array that is neither null nor empty on that path: the choice is stated at every call.
// A clamped load is a real load whose value is dropped, and it costs what a real one costs: the address unit works through
// every active lane, whatever line it names (all idle lanes on ONE line, element 0, measured slower still than each on its
// own neighbourhood).  So the idiom pays where cond mostly holds, or where the lanes that fail read next to their own data;
// where most lanes fail -- the fourth slot of lists that mostly hold one or two -- the branch, which issues no address for
// them, is the cheaper form (k_events).
// landed(a, b, ...) closes a batch.  The compiler undoes a batch where it can: a value whose uses all lie behind one branch is
// sunk into that branch, its load with it, and waits there on its own again; a select right on a load with no other use is
// turned back into a branch around the load.  landed ties the values to the place where it stands: an empty statement the
// optimiser cannot see through.  It emits no instruction and no wait is written by hand -- the compiler places its counted
// wait in front of it.  One statement per batch, so that the register copies it may need stand behind ALL the loads.  Where
// a value is used although cond failed, the caller selects behind landed().
#define POVU_W2(v) "+v"((v).x), "+v"((v).y)
#define POVU_W4(v) "+v"((v).x), "+v"((v).y), "+v"((v).z), "+v"((v).w)
__device__ __forceinline__ void landed(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
__device__ __forceinline__ void landed(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, uint32_t &e)
{
	asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e));
}
__device__ __forceinline__ void landed(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, uint32_t &e, uint32_t &f)
{
	asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f));
}
__device__ __forceinline__ void landed(uint2 &a, uint2 &b, uint2 &c, uint2 &d, uint32_t &e, uint32_t &f, uint32_t &g, uint32_t &h)
{
	asm volatile("" : POVU_W2(a), POVU_W2(b), POVU_W2(c), POVU_W2(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h));
}
__device__ __forceinline__ void landed(uint4 &a) { asm volatile("" : POVU_W4(a)); }
__device__ __forceinline__ void landed(uint4 &a, uint2 &b) { asm volatile("" : POVU_W4(a), POVU_W2(b)); }
__device__ __forceinline__ void landed(uint32_t &a, uint4 &b, uint4 &c, uint4 &d) { asm volatile("" : "+v"(a), POVU_W4(b), POVU_W4(c), POVU_W4(d)); }
__device__ __forceinline__ void landed(uint32_t &a, uint32_t &b, uint32_t &c, uint4 &d, uint4 &e, uint4 &f)
{
	asm volatile("" : "+v"(a), "+v"(b), "+v"(c), POVU_W4(d), POVU_W4(e), POVU_W4(f));
}
__device__ __forceinline__ void landed(uint4 &a, uint4 &b, uint4 &c, uint4 &d) { asm volatile("" : POVU_W4(a), POVU_W4(b), POVU_W4(c), POVU_W4(d)); }
// ... of a batch kept in arrays of N elements (k_back_edges: N = BE_BATCH sides of a lane at a time; the build takes 4, and 2
// and 8 are there so that POVU_BE_BATCH can be set to them for a measurement)
#define POVU_A2(a, W) W((a)[0]), W((a)[1])
#define POVU_A4(a, W) POVU_A2(a, W), W((a)[2]), W((a)[3])
#define POVU_A8(a, W) POVU_A4(a, W), W((a)[4]), W((a)[5]), W((a)[6]), W((a)[7])
#define POVU_W1(v) "+v"(v)
template <uint32_t N>
__device__ __forceinline__ void landed(uint32_t (&a)[N], uint32_t (&b)[N], uint32_t (&c)[N], uint32_t (&d)[N], uint32_t (&e)[N])
{
	static_assert(N == 2 || N == 4 || N == 8, "a batch of 2, 4 or 8");
	if constexpr (N == 2)
		asm volatile("" : POVU_A2(a, POVU_W1), POVU_A2(b, POVU_W1), POVU_A2(c, POVU_W1), POVU_A2(d, POVU_W1), POVU_A2(e, POVU_W1));
	else if constexpr (N == 4)
		asm volatile("" : POVU_A4(a, POVU_W1), POVU_A4(b, POVU_W1), POVU_A4(c, POVU_W1), POVU_A4(d, POVU_W1), POVU_A4(e, POVU_W1));
	else
		asm volatile("" : POVU_A8(a, POVU_W1), POVU_A8(b, POVU_W1), POVU_A8(c, POVU_W1), POVU_A8(d, POVU_W1), POVU_A8(e, POVU_W1));
}
template <uint32_t N>
__device__ __forceinline__ void landed(uint4 (&a)[N], uint32_t (&b)[N])
{
	static_assert(N == 2 || N == 4 || N == 8, "a batch of 2, 4 or 8");
	if constexpr (N == 2)
		asm volatile("" : POVU_A2(a, POVU_W4), POVU_A2(b, POVU_W1));
	else if constexpr (N == 4)
		asm volatile("" : POVU_A4(a, POVU_W4), POVU_A4(b, POVU_W1));
	else
		asm volatile("" : POVU_A8(a, POVU_W4), POVU_A8(b, POVU_W1));
}
template <uint32_t N>
__device__ __forceinline__ void landed(uint4 (&a)[N])
{
	static_assert(N == 2 || N == 4 || N == 8, "a batch of 2, 4 or 8");
	if constexpr (N == 2)
		asm volatile("" : POVU_A2(a, POVU_W4));
	else if constexpr (N == 4)
		asm volatile("" : POVU_A4(a, POVU_W4));
	else
		asm volatile("" : POVU_A8(a, POVU_W4));
}
#undef POVU_A2
#undef POVU_A4
#undef POVU_A8
#undef POVU_W1
#undef POVU_W2
#undef POVU_W4
template <class T>
__device__ __forceinline__ T gather_if(bool cond, const T *__restrict__ p, uint32_t i, uint32_t safe)
{
	return p[cond ? i : safe];
}
// ... of two words at an even word index (8-byte aligned)
__device__ __forceinline__ uint2 gather2_if(bool cond, const unsigned *__restrict__ p, uint32_t i, uint32_t safe)
{
	return *reinterpret_cast<const uint2 *>(p + (cond ? i : safe));
}
// ... of four words from a 4-byte aligned address (load4_unaligned: three words of slack behind `i` AND behind `safe`)
__device__ __forceinline__ uint4 gather4_unaligned_if(bool cond, const unsigned *__restrict__ p, uint32_t i, uint32_t safe)
{
	return load4_unaligned(p + (cond ? i : safe));
}

// Workgroup index with the 8 XCDs in mind: the dispatcher deals workgroups round-robin over the XCDs (blocks b and b + 8
// share one, MI355X_MICROARCH.md "Workgroup dispatch"), so neighbouring blocks -- which touch neighbouring lines in
// almost every kernel here -- land in eight different L2s.  BIDX renumbers the blocks so that every XCD works on one
// contiguous stretch of the grid (bijective for any grid size); a speed choice only, nothing depends on placement.
#ifdef POVU_XCD_SWIZZLE
__device__ __forceinline__ unsigned povu_xcd_bid()
{
	const unsigned nwg = gridDim.x, q = nwg >> 3, r = nwg & 7u, x = blockIdx.x & 7u, i = blockIdx.x >> 3;
	return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}
#define BIDX povu_xcd_bid()
#else
#define BIDX blockIdx.x
#endif

namespace povu_hip
{

struct HipError : std::runtime_error {
	using std::runtime_error::runtime_error;
};

#define HIP_CHECK(expr)                                                                          \
	do {                                                                                     \
		hipError_t e__ = (expr);                                                         \
		if (e__ != hipSuccess)                                                           \
			throw povu_hip::HipError(std::string(#expr) + ": " + hipGetErrorString(e__) + " (" + \
						 __FILE__ + ":" + std::to_string(__LINE__) + ")");   \
	} while (0)

// kernel launch + launch-configuration check (a bad grid / LDS size / missing code object is not reported by the
// stream synchronisation that follows)
#define KLAUNCH(kernel, grid, block, shmem, stream, ...)                                          \
	do {                                                                                      \
		hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);              \
		HIP_CHECK(hipGetLastError());                                                     \
	} while (0)
// ... of one lane per element on workgroups of TPB lanes; nothing is launched for n == 0
static constexpr int TPB = 256;
static inline unsigned nblk(size_t n) { return (unsigned)((n + TPB - 1) / TPB); }
#define LAUNCH(k, n, s, ...)                                                                     \
	do {                                                                                     \
		if ((n) > 0) {                                                                   \
			hipLaunchKernelGGL(k, dim3(nblk(n)), dim3(TPB), 0, s, __VA_ARGS__);      \
			HIP_CHECK(hipGetLastError());                                            \
		}                                                                                \
	} while (0)

// Bytes that cross PCIe, tallied per thread (a context is used by one thread at a time; the C ABI entry points add the
// difference over a call to their context's totals, povu_hip_transfer_bytes).  Every host<->device copy of the library goes
// through copy_async; results that kernels write straight into page-locked host memory are counted where they are sized.
struct XferTally {
	uint64_t h2d = 0, d2h = 0;
};
inline XferTally &xfer_tally()
{
	static thread_local XferTally t;
	return t;
}
inline hipError_t copy_async(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
	if (kind == hipMemcpyHostToDevice)
		xfer_tally().h2d += n;
	else if (kind == hipMemcpyDeviceToHost)
		xfer_tally().d2h += n;
	return hipMemcpyAsync(dst, src, n, kind, s);
}
inline void count_kernel_d2h(size_t n) { xfer_tally().d2h += n; }

// One growable device arena per context: stages carve typed spans with a bump
// pointer, nothing is hipMalloc'd inside the timed path once the arena is warm.
class Arena
{
public:
	~Arena() { release(); }
	void release()
	{
		if (base_)
			(void)hipFree(base_);
		base_ = nullptr;
		cap_ = 0;
		top_ = 0;
	}
	// make sure `bytes` are available from offset 0; invalidates earlier spans
	// (head_room: an eighth more than asked for, so that the next, slightly larger graph of a long-lived context does not
	// cost a new allocation; a caller that knows there will be no next graph asks for none)
	void reserve(size_t bytes, bool head_room = true)
	{
		if (bytes > cap_) {
			release();
			size_t want = head_room ? bytes + bytes / 8 + (1u << 20) : bytes + 4096;
			if (hipMalloc(&base_, want) != hipSuccess) {
				(void)hipGetLastError();
				base_ = nullptr;
				want = bytes + 4096; // no head room: retry with exactly what this graph needs
				if (hipMalloc(&base_, want) != hipSuccess) {
					(void)hipGetLastError();
					base_ = nullptr;
					size_t free_b = 0, total_b = 0;
					(void)hipMemGetInfo(&free_b, &total_b);
					throw HipError("not enough device memory for the decompose workspace: need " +
						       std::to_string(want >> 20) + " MiB in one arena, " + std::to_string(free_b >> 20) +
						       " MiB free of " + std::to_string(total_b >> 20) +
						       " MiB (povu_hip_workspace_estimate gives the total for a graph)");
				}
			}
			cap_ = want;
		}
		top_ = 0;
	}
	template <typename T>
	T *take(size_t n)
	{
		size_t off = (top_ + 255) & ~size_t(255);
		size_t bytes = n * sizeof(T);
		if (off + bytes > cap_)
			throw HipError("povu_hip arena overflow (internal sizing bug)");
		top_ = off + bytes;
		return reinterpret_cast<T *>(static_cast<char *>(base_) + off);
	}
	bool fits(size_t bytes) const { return ((top_ + 255) & ~size_t(255)) + bytes <= cap_; }
	static size_t padded(size_t n, size_t elem) { return ((n * elem) + 255) & ~size_t(255); }
	size_t capacity() const { return cap_; }
	size_t used() const { return top_; }
	// two groups of arrays that are never live together share a stretch: carve one, rewind to where it began, carve the
	// other, continue behind the longer of the two (rewind(m); ...; advance_to(end of the first))
	void rewind(size_t mark) { top_ = mark; }
	void advance_to(size_t mark)
	{
		if (mark > top_)
			top_ = mark;
	}

private:
	void *base_ = nullptr;
	size_t cap_ = 0, top_ = 0;
};

// An arena layout declared once: a list of spans, `take(n, p...)` for n elements of each pointer's type (n bytes for a
// void *; `take.bytes_for(p, b)` for b bytes behind a typed pointer), run first with no arena behind it to measure, then to
// carve.  The measure holds from any starting offset: every span counts its padded size and one alignment step more.
struct Spans {
	Arena *ar = nullptr; // null: measure only
	size_t bytes = 0;
	template <typename... P>
	void operator()(size_t n, P *&...p)
	{
		(one(p, n), ...);
	}
	template <typename T>
	void one(T *&p, size_t n)
	{
		bytes += Arena::padded(n, sizeof(T)) + 256;
		if (ar)
			p = ar->take<T>(n);
	}
	void one(void *&p, size_t n)
	{
		char *c = nullptr;
		one(c, n);
		if (ar)
			p = c;
	}
	// a span stated in bytes (no whole number of T, or cut up further by its owner)
	template <typename T>
	void bytes_for(T *&p, size_t n_bytes)
	{
		void *v = nullptr;
		one(v, n_bytes);
		if (ar)
			p = static_cast<T *>(v);
	}
};
template <class List>
size_t measure(List &&list)
{
	Spans m;
	list(m);
	return m.bytes;
}
// reserves what `list` measures in `A` (from offset 0: earlier spans are invalidated) and carves it
template <class List>
void carve(Arena &A, List &&list, bool head_room = true)
{
	A.reserve(measure(list), head_room);
	Spans c{&A};
	list(c);
}

// Page-locked host scratch of one context.  Every small read-back (a count that sizes the next
// launch) and every host-built table goes through it, so no copy is staged through pageable
// memory; spans stay valid until the next reset() (= the next decompose on that context).
class HostScratch
{
public:
	~HostScratch()
	{
		for (auto &c : chunks_)
			(void)hipHostFree(c.p);
		for (hipEvent_t e : events_)
			(void)hipEventDestroy(e);
	}
	HostScratch() = default;
	HostScratch(const HostScratch &) = delete;
	HostScratch &operator=(const HostScratch &) = delete;
	// Words a kernel published into a span of this scratch (publish_words, or a kernel that writes page-locked memory itself)
	// are read WITHOUT leaving the stream idle: mark() right behind the publishing kernel, then the stream is given the
	// kernels that do not depend on the words, then wait() on what mark() returned -- the host wakes up while they run.
	// Every mark() of a pass takes an event of its own from a pool the scratch keeps (reset() gives them all back).
	using Token = size_t;
	Token mark(hipStream_t s)
	{
		if (marks_ == events_.size()) {
			hipEvent_t e = nullptr;
			HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
			events_.push_back(e);
		}
		HIP_CHECK(hipEventRecord(events_[marks_], s));
		return marks_++;
	}
	void wait(Token t) { HIP_CHECK(hipEventSynchronize(events_[t])); }
	void reset()
	{
		for (auto &c : chunks_)
			c.top = 0;
		marks_ = 0;
	}
	template <typename T>
	T *take(size_t n)
	{
		const size_t bytes = forest_wire::pad64(n * sizeof(T));
		for (auto &c : chunks_)
			if (c.cap - c.top >= bytes) {
				char *r = c.p + c.top;
				c.top += bytes;
				return reinterpret_cast<T *>(r);
			}
		Chunk c{nullptr, std::max<size_t>(2 * bytes, size_t(1) << 16), bytes};
		HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&c.p), c.cap, hipHostMallocDefault));
		chunks_.push_back(c);
		return reinterpret_cast<T *>(c.p);
	}
	// one 32-bit word of device memory, through the stream
	uint32_t read_u32(const uint32_t *dptr, hipStream_t s)
	{
		uint32_t *h = take<uint32_t>(1);
		HIP_CHECK(copy_async(h, dptr, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		return *h;
	}

private:
	struct Chunk {
		char *p;
		size_t cap, top;
	};
	std::vector<Chunk> chunks_;
	std::vector<hipEvent_t> events_;
	size_t marks_ = 0; // events_[0, marks_) recorded since the last reset()
};

// HIP-event stage timer on the context's stream.
struct StageTimer {
	struct Rec {
		std::string name;
		hipEvent_t a, b;
		uint32_t launches;
	};
	std::vector<Rec> recs;
	std::vector<hipEvent_t> pool;
	size_t pool_used = 0;
	hipStream_t stream = nullptr;
	bool enabled = true; // per-stage event pairs cost a few microseconds each; the pass total is always timed
	hipEvent_t get()
	{
		if (pool_used == pool.size()) {
			hipEvent_t e;
			HIP_CHECK(hipEventCreate(&e));
			pool.push_back(e);
		}
		return pool[pool_used++];
	}
	void reset()
	{
		recs.clear();
		pool_used = 0;
	}
	void begin(const char *name)
	{
		if (!enabled)
			return;
		Rec r{name, get(), get(), 0};
		HIP_CHECK(hipEventRecord(r.a, stream));
		recs.push_back(r);
	}
	void end(uint32_t launches)
	{
		if (!enabled)
			return;
		recs.back().launches = launches;
		HIP_CHECK(hipEventRecord(recs.back().b, stream));
	}
	~StageTimer()
	{
		for (auto e : pool)
			(void)hipEventDestroy(e);
	}
};

// device-wide primitives (primitives.hip)
void scan_exclusive_u32(const uint32_t *in, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes, hipStream_t s);
// two independent scans that are due at the same point of the pass, in the same two launches
void scan_exclusive_u32_pair(const uint32_t *in0, uint32_t *out0, size_t n0, const uint32_t *in1, uint32_t *out1, size_t n1,
			     void *tmp, size_t tmp_bytes, hipStream_t s);
// exclusive running xor of two arrays of the same length (the two halves of 64-bit words), in the same two launches
void scan_exclusive_xor_u32_pair(const uint32_t *in0, uint32_t *out0, const uint32_t *in1, uint32_t *out1, size_t n, void *tmp,
				 size_t tmp_bytes, hipStream_t s);
// exclusive sums of BYTE inputs (flags, counts below 256): one job, or two independent ones in the same two launches
void scan_exclusive_u8(const uint8_t *in0, uint32_t *out0, size_t n0, const uint8_t *in1, uint32_t *out1, size_t n1, void *tmp,
		       size_t tmp_bytes, hipStream_t s);
// exclusive prefix sums of in[i] - sub[i] (mod 2^32)
void scan_exclusive_diff_u32(const uint32_t *in, const uint32_t *sub, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes,
			     hipStream_t s);
// ... of in8[i] - sub[i]: byte counts (below 256 each) minus word counts
void scan_exclusive_diff_u8_u32(const uint8_t *in8, const uint32_t *sub, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes,
				hipStream_t s);
// ... of in8[i] - sub8[i]: byte counts minus byte counts (the difference wraps mod 2^32 where sub8[i] > in8[i], as with words)
void scan_exclusive_diff_u8_u8(const uint8_t *in8, const uint8_t *sub8, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes,
			       hipStream_t s);
// a word job and a byte job that are due at the same point of the pass, in the same launches
void scan_exclusive_u32_u8_pair(const uint32_t *in0, uint32_t *out0, size_t n0, const uint8_t *in1, uint32_t *out1, size_t n1,
				void *tmp, size_t tmp_bytes, hipStream_t s);
// exclusive running xor of 128-bit words (two independent 64-bit hashes side by side)
// (n_dev, device memory, optional: only the first *n_dev + 1 words exist -- n then is the most there can be and sizes the launch)
void scan_exclusive_xor_u128(const ulonglong2 *in, ulonglong2 *out, size_t n, void *tmp, size_t tmp_bytes, hipStream_t s,
			     const uint32_t *n_dev = nullptr);
// inclusive prefix sums of words (out[i] = in[0] + ... + in[i])
void scan_inclusive_u32(const uint32_t *in, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes, hipStream_t s);
// exclusive sums of BYTE inputs as packed count records (cntrec_prefix below): rec0 / rec1 take cntrec_records(n0 / n1)
// records; one job, or two independent ones in the same launches (in1 may be null)
void scan_count_records_u8(const uint8_t *in0, uint4 *rec0, size_t n0, const uint8_t *in1, uint4 *rec1, size_t n1, void *tmp,
			   size_t tmp_bytes, hipStream_t s);
// elements a tile of that scan covers: of its two-launch form / of its one-launch (look-back) form
void scan_count_records_tiles(size_t *chunk_tile, size_t *lookback_tile);
size_t scan_tmp_bytes(size_t n);
// exclusive sums of u64 (in == out allowed); tmp holds scan_exclusive_u64_tmp(n) WORDS of 8 bytes
void scan_exclusive_u64(const uint64_t *in, uint64_t *out, size_t n, uint64_t *tmp, hipStream_t s);
size_t scan_exclusive_u64_tmp(size_t n);

// ---- scans inside a wave and a workgroup, written once.  An operation is a type with an associative, commutative
// operator() whose identity is the all-zero value T{}, and before(inc, v): what the lanes in front of a lane hold together,
// from the lane's inclusive value and its own.  ScanOp<0|1|2> = sum (mod 2^32, 2^64) / maximum / xor of u32 and u64, Xor128 = xor of
// 128-bit words.  Everything is inlined, and LDS comes from the caller: a kernel's layout and barriers are its own.
// (a lane's value from the lane `off` in front / behind / across; any 32- or 64-bit scalar, and 128-bit words)
template <class T> __device__ __forceinline__ T lanes_up(T v, int off) { return __shfl_up(v, off); }
template <class T> __device__ __forceinline__ T lanes_down(T v, int off) { return __shfl_down(v, off); }
template <class T> __device__ __forceinline__ T lanes_xor(T v, int off) { return __shfl_xor(v, off); }
__device__ __forceinline__ uint2 lanes_down(const uint2 v, int off) { return make_uint2(__shfl_down(v.x, off), __shfl_down(v.y, off)); }
__device__ __forceinline__ ulonglong2 lanes_up(const ulonglong2 v, int off) { return make_ulonglong2(__shfl_up(v.x, off), __shfl_up(v.y, off)); }
__device__ __forceinline__ ulonglong2 lanes_down(const ulonglong2 v, int off) { return make_ulonglong2(__shfl_down(v.x, off), __shfl_down(v.y, off)); }
template <int OP>
struct ScanOp {
	__device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return OP == 1 ? (a > b ? a : b) : (OP == 2 ? (a ^ b) : a + b); }
	template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return OP == 1 ? (a > b ? a : b) : (OP == 2 ? (a ^ b) : a + b); } // (64-bit values)
	__device__ __forceinline__ uint32_t before(uint32_t inc, uint32_t v) const
	{
		if (OP == 0)
			return inc - v;
		if (OP == 2)
			return inc ^ v;
		const uint32_t y = __shfl_up(inc, 1); // (a maximum cannot be undone)
		return (threadIdx.x & 63u) ? y : 0u;
	}
};
// the minimum, for reductions alone (its identity is not the zero the scans start from)
struct MinOp {
	template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? a : b; }
};
struct Xor128 {
	__device__ __forceinline__ ulonglong2 operator()(const ulonglong2 a, const ulonglong2 b) const { return make_ulonglong2(a.x ^ b.x, a.y ^ b.y); }
	__device__ __forceinline__ ulonglong2 before(const ulonglong2 inc, const ulonglong2 v) const { return (*this)(inc, v); }
};
// lane l gets the lanes 0 .. l
template <class T, class Op>
__device__ __forceinline__ T wave_inclusive_scan(T v, Op op)
{
	const int lane = (int)(threadIdx.x & 63u);
	for (int off = 1; off < 64; off <<= 1) {
		const T y = lanes_up(v, off);
		if (lane >= off)
			v = op(v, y);
	}
	return v;
}
// lane 0 gets the whole wave
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op)
{
	for (int off = 32; off; off >>= 1)
		v = op(v, lanes_down(v, off));
	return v;
}
// every lane gets the whole wave (a xor butterfly)
template <class T, class Op>
__device__ __forceinline__ T wave_all_reduce(T v, Op op)
{
	for (int off = 32; off; off >>= 1)
		v = op(v, lanes_xor(v, off));
	return v;
}
// the workgroup (WAVES waves), in every lane; sh: WAVES values, free again on return (one barrier in, one out)
template <int WAVES, class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T *sh, Op op)
{
	v = wave_reduce(v, op);
	if ((threadIdx.x & 63u) == 0)
		sh[threadIdx.x >> 6] = v;
	__syncthreads();
	T r = sh[0];
#pragma unroll
	for (int w = 1; w < WAVES; w++)
		r = op(r, sh[w]);
	__syncthreads();
	return r;
}
// Exclusive prefix over the workgroup in two halves, for kernels that put several scans in front of one barrier:
// wave_scan_publish returns the lane's inclusive value within its wave and leaves the wave's total in sh[wave]; behind a
// barrier waves_before returns the waves in front of this one, and the whole workgroup in `total`.
template <class T, class Op>
__device__ __forceinline__ T wave_scan_publish(T v, T *sh, Op op)
{
	const T inc = wave_inclusive_scan(v, op);
	if ((threadIdx.x & 63u) == 63u)
		sh[threadIdx.x >> 6] = inc;
	return inc;
}
template <int WAVES, class T, class Op>
__device__ __forceinline__ T waves_before(const T *sh, T &total, Op op)
{
	const int wave = (int)(threadIdx.x >> 6);
	T before{};
	total = T{};
#pragma unroll
	for (int w = 0; w < WAVES; w++) {
		if (w < wave)
			before = op(before, sh[w]);
		total = op(total, sh[w]);
	}
	return before;
}
// ... and in one piece: what the lanes in front of this one hold together, `total` = the whole workgroup.  ONE barrier; a
// caller that uses `sh` again puts its own behind the last use.
template <int WAVES, class T, class Op>
__device__ __forceinline__ T block_exclusive_scan(T v, T *sh, T &total, Op op)
{
	const T inc = wave_scan_publish(v, sh, op);
	__syncthreads();
	const T before = waves_before<WAVES>(sh, total, op);
	return op(before, op.before(inc, v));
}
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v) { return wave_inclusive_scan(v, ScanOp<0>{}); }
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v) { return wave_inclusive_scan(v, ScanOp<1>{}); }

// indices of the non-zero bytes of flag[0..n), ascending, into out; their number into *count_dev (device memory).  No
// prefix array is written: tiles are counted, the counts scanned, the tiles ranked again.
// ---- bit-rank directory: one 16-byte record per 64 flags = {bits 0..31, bits 32..63, set bits in front of the record, 0}.
// rank(x) = flags set at positions < x is ONE 16-byte load and a popcount, and a table over 2 * 10^8 flags is 50 MB (it
// stays in the Infinity Cache) where the byte flags + their 4-byte prefix sums were 1 GB.  The producer writes the bit
// words (x, y); bitrank_build fills in z (three small launches over n / 64 records).  The array carries one record of
// slack: rank(n) is asked for.
__device__ __forceinline__ uint32_t bitrank(const uint4 *__restrict__ rec, uint32_t x)
{
	const uint4 r = rec[x >> 6];
	const unsigned long long bits = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
	return r.z + (uint32_t)__popcll(bits & ((1ull << (x & 63u)) - 1ull));
}
__device__ __forceinline__ bool bitrank_test(const uint4 *__restrict__ rec, uint32_t x)
{
	const uint4 r = rec[x >> 6];
	return (((x & 32u) ? r.y : r.x) >> (x & 31u)) & 1u;
}
// ---- count records: the same idea for small COUNTS.  One 16-byte record per CNTREC_N = 12 byte counts = {counts 0..3,
// counts 4..7, counts 8..11, sum of every count in front of the record}: "sum of the counts in front of element i" is ONE
// 16-byte load, a mask and three byte sums, and the table is 1.33 bytes an element where the word prefix sums were 4.
// scan_count_records_u8 writes it from the byte array (which stays).  The count bytes of the last record that lie behind
// the array's end are zero; the array carries one record of slack (never written, never read for i < n).
static constexpr uint32_t CNTREC_N = 12;
inline size_t cntrec_records(size_t n) { return (n + CNTREC_N - 1) / CNTREC_N + 1; }
// the sum of the four bytes of x, added to acc (v_sad_u8 against zero)
__device__ __forceinline__ uint32_t cntrec_bytesum(uint32_t x, uint32_t acc) { return __builtin_amdgcn_sad_u8(x, 0u, acc); }
// the record of element i, and i's place k in it (i / 12 by a multiply-high: 0xAAAAAAAB = ceil(2^35 / 12), exact for 32 bits)
__device__ __forceinline__ uint4 cntrec_load(const uint4 *__restrict__ rec, uint32_t i, uint32_t &k)
{
	const uint32_t r = __umulhi(i, 0xAAAAAAABu) >> 3;
	k = i - CNTREC_N * r;
	return rec[r];
}
// the low k bytes of a word (k >= 4: all of it; k <= 0: none)
__device__ __forceinline__ uint32_t cntrec_low_bytes(uint32_t x, int k) { return k >= 4 ? x : k <= 0 ? 0u : x & ((1u << (8 * k)) - 1u); }
__device__ __forceinline__ uint32_t cntrec_prefix(const uint4 *__restrict__ rec, uint32_t i)
{
	uint32_t k;
	const uint4 r = cntrec_load(rec, i, k);
	const int kk = (int)k;
	return cntrec_bytesum(cntrec_low_bytes(r.z, kk - 8), cntrec_bytesum(cntrec_low_bytes(r.y, kk - 4), cntrec_bytesum(cntrec_low_bytes(r.x, kk), r.w)));
}
__device__ __forceinline__ uint32_t cntrec_count(const uint4 *__restrict__ rec, uint32_t i)
{
	uint32_t k;
	const uint4 r = cntrec_load(rec, i, k);
	const uint32_t w = k < 4 ? r.x : k < 8 ? r.y : r.z;
	return (w >> (8 * (k & 3u))) & 0xFFu;
}
// How a kernel reads a prefix-sum array: the words themselves, or count records.  at(i) = the sum in front of element i,
// count(i) = element i itself (words: two gathers; records: the same record again).
struct PrefixWords {
	const uint32_t *__restrict__ p;
	__device__ __forceinline__ uint32_t at(uint32_t i) const { return p[i]; }
	__device__ __forceinline__ uint32_t count(uint32_t i) const { return p[i + 1] - p[i]; }
};
struct PrefixRecords {
	const uint4 *__restrict__ p;
	__device__ __forceinline__ uint32_t at(uint32_t i) const { return cntrec_prefix(p, i); }
	__device__ __forceinline__ uint32_t count(uint32_t i) const { return cntrec_count(p, i); }
};
// Component of a candidate-stack entry, looked up instead of stored (a word per entry was 0.4 GB written and as much read
// by every consumer).  Entry i belongs to the last non-empty component that starts at or before i: `rec` is a bit-rank
// directory over the stack positions with a bit where a non-empty component starts, `list` those components in order.
// The cost is the same for 24 large components and for a million tiny ones: one 16-byte look-up and one word.
struct StackComp {
	const uint4 *rec;
	const uint32_t *list;
	__device__ __forceinline__ uint32_t operator()(uint32_t i) const { return list[bitrank(rec, i + 1) - 1u]; }
};
// Component of a tree vertex / of a slot of the per-component layouts, looked up in the vertex offsets of the C components
// (C > 0): component c owns the tree vertices [2 voff[c] + c, 2 voff[c + 1] + c] and the slots from voff[c] + c.  The keys
// ascend strictly, whatever components are empty.
struct CompSpans {
	const uint32_t *voff;
	uint32_t C;
	__device__ __forceinline__ uint32_t of_tree(uint32_t t) const
	{
		const uint32_t *v = voff;
		return last_upto(0u, C, [=](uint32_t c) { return 2 * v[c] + c <= t; });
	}
	__device__ __forceinline__ uint32_t of_slot(uint32_t slot) const
	{
		const uint32_t *v = voff;
		return last_upto(0u, C, [=](uint32_t c) { return v[c] + c <= slot; });
	}
};
// spreads the low 16 bits of x to every fourth bit position (bit k -> bit 4 k)
__device__ __forceinline__ unsigned long long spread4(unsigned long long x)
{
	x &= 0xFFFFull;
	x = (x | (x << 24)) & 0x000000FF000000FFull;
	x = (x | (x << 12)) & 0x000F000F000F000Full;
	x = (x | (x << 6)) & 0x0303030303030303ull;
	x = (x | (x << 3)) & 0x1111111111111111ull;
	return x;
}
// A wave whose lane l holds four flags f (bits 0..3) of the positions 256 w + 4 l + {0..3} writes the four records of its
// 256 positions (rec = the wave's first record; every lane of the wave calls this)
__device__ __forceinline__ void bitrank_store_wave(uint4 *__restrict__ rec, uint32_t f, bool in_range)
{
	const uint32_t lane = threadIdx.x & 63u;
	const unsigned long long m0 = __ballot(f & 1u), m1 = __ballot(f & 2u), m2 = __ballot(f & 4u), m3 = __ballot(f & 8u);
	if (lane < 4 && in_range) {
		const unsigned sh = 16u * lane;
		const unsigned long long w = spread4(m0 >> sh) | (spread4(m1 >> sh) << 1) | (spread4(m2 >> sh) << 2) | (spread4(m3 >> sh) << 3);
		rec[lane] = make_uint4((uint32_t)w, (uint32_t)(w >> 32), 0u, 0u);
	}
}
// fills the z words of `rec` (n_rec records + one closing record whose bits are cleared here); tmp: (n_rec + 2) words + the scan's scratch
void bitrank_build(uint4 *rec, size_t n_rec, uint32_t *tmp_counts, void *scan_tmp, size_t scan_tmp_bytes, hipStream_t s);

// ---- a workgroup of 256 lanes appends the flagged positions of LIST_ITER rounds x 1024 positions (four a lane and round, bit
// 4 it + j of `fw`: position B0 + 1024 it + 4 tid + j) to a list, IN POSITION ORDER, with ONE atomic add on the list's
// length.  Atomic adds on one word retire at ~90 M/s on this chip (one per wave of 256 positions made such a kernel 8.9 ms
// on 2 * 10^8 positions), so they are kept to one per 16 384 positions.  The order matters for speed, not for results: the
// kernels that work through these lists want neighbouring lanes on neighbouring positions (a list that interleaved a
// workgroup's rounds made the class walks 35 % slower).
static constexpr uint32_t LIST_ITER = 16, LIST_TPB = 256, LIST_SPAN = LIST_TPB * 4 * LIST_ITER;
__device__ __forceinline__ void append_in_order(unsigned long long fw, uint32_t B0, uint32_t *__restrict__ list, uint32_t *__restrict__ n_list)
{
	__shared__ uint32_t tot[LIST_ITER * (LIST_TPB / 64)], base_sh;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
	for (uint32_t it = 0; it < LIST_ITER; it++) {
		const uint32_t f = (uint32_t)(fw >> (4 * it)) & 15u;
		const uint32_t t = (uint32_t)(__popcll(__ballot(f & 1u)) + __popcll(__ballot(f & 2u)) + __popcll(__ballot(f & 4u)) + __popcll(__ballot(f & 8u)));
		if (lane == 0)
			tot[it * (LIST_TPB / 64) + wave] = t;
	}
	__syncthreads();
	if (threadIdx.x < 64) { // rounds first, waves inside a round: exclusive prefix of the 64 counts, the total to the list
		const uint32_t v = tot[threadIdx.x];
		const uint32_t inc = wave_inclusive_sum(v);
		tot[threadIdx.x] = inc - v;
		if (lane == 63)
			base_sh = inc ? atomicAdd(n_list, inc) : 0u;
	}
	__syncthreads();
	const uint32_t base = base_sh;
#pragma unroll
	for (uint32_t it = 0; it < LIST_ITER; it++) {
		uint32_t f = (uint32_t)(fw >> (4 * it)) & 15u;
		// (every lane of the wave takes part in the ballots; lanes without a flag of this round only skip the stores)
		const uint32_t before = (uint32_t)(__popcll(__ballot(f & 1u) & lt) + __popcll(__ballot(f & 2u) & lt) + __popcll(__ballot(f & 4u) & lt) +
						   __popcll(__ballot(f & 8u) & lt));
		uint32_t at = base + tot[it * (LIST_TPB / 64) + wave] + before;
		while (f) {
			const int k = __ffs((int)f) - 1;
			f &= f - 1;
			list[at++] = B0 + it * (LIST_TPB * 4u) + threadIdx.x * 4u + (uint32_t)k;
		}
	}
}

// Up to 8 words of device memory into page-locked host memory by ONE single-lane kernel: a hipMemcpyAsync per word is a
// copy submission each (3-4 us apiece on the stream; config 2's whole pass is 1.1 ms).  `host_dst` is the HOST pointer of
// page-locked memory (HostScratch); read it after the stream is synchronised.
struct WordSrc {
	const uint32_t *p[8];
};
void publish_words(uint32_t *host_dst, const WordSrc &src, int n, hipStream_t s);
void compact_flagged_u8(const uint8_t *flag, size_t n, uint32_t *out, uint32_t *count_dev, void *tmp, size_t tmp_bytes, hipStream_t s);
size_t compact_tmp_bytes(size_t n);
// 64-bit sums of n u32 counts, of `a` into h[0] and of `b` (optional) into h[1], in one launch; tot: as many words of device
// memory (cleared here).  Waits for the stream.
void totals_u32(const uint32_t *a, const uint32_t *b, uint64_t n, unsigned long long *tot, uint64_t *h, hipStream_t s);
// exclusive running maximum (identity 0)
void scan_exclusive_max_u32(const uint32_t *in, uint32_t *out, size_t n, void *tmp, size_t tmp_bytes, hipStream_t s);
// stable LSD radix sort of (key,value) pairs on the low `bits` bits of the key.  Inputs and outputs must not alias (kin !=
// kout, vin != vout): with an odd number of places the first place would scatter into the array it is still reading.
void sort_pairs_u32(const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, size_t n, unsigned bits,
		    void *tmp, size_t tmp_bytes, hipStream_t s);
size_t sort_tmp_bytes(size_t n);
// bytes of ONE span that serves every scan, compaction and (with_sort) sort of up to n elements: the primitives of a phase
// run one after another on one stream and each writes what it reads of its scratch (the scan clears its status words, the
// sort fills its table, the compaction its tile counts), so they share it
size_t prim_tmp_bytes(size_t n, bool with_sort);

inline unsigned bits_for(uint64_t max_value)
{
	unsigned b = 1;
	while (b < 32 && (uint64_t(1) << b) <= max_value)
		b++;
	return b;
}

} // namespace povu_hip
