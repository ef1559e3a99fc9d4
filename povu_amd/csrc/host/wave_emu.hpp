// wave_emu.hpp -- a wave of 64 lanes on the CPU, for the check programs: the `w` that the wave loops of hip/vcfcmp_rules.hpp
// are written over, its lanes taken one after another.
#pragma once
#include <cstdint>

struct EmuWave {
	template <class F> uint64_t ballot(F &&f) const
	{
		uint64_t m = 0;
		for (uint32_t lane = 0; lane < 64; lane++)
			if (f(lane))
				m |= 1ull << lane;
		return m;
	}
	template <class F> uint64_t sum(F &&f) const
	{
		uint64_t v = 0;
		for (uint32_t lane = 0; lane < 64; lane++)
			v += f(lane);
		return v;
	}
};
