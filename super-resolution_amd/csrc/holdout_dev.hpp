// holdout_dev.hpp -- the device copy of the hold-out's index hash (holdout_host.hpp states it and holds its plain-C++
// twin): every kernel that needs to know whether observation i is held out recomputes it from the index.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace srmap {

// i: the flat index into the whole problem's [K][C][h][w]; held out iff lo <= hash24(i, seed) < hi.  A fraction is the
// band [0, floor(fraction * 2^24)), fold f of F the band [floor(f 2^24 / F), floor((f + 1) 2^24 / F)); lo <= hi <= 2^24
__device__ __forceinline__ bool holdout_held_dev(uint64_t i, uint64_t seed, uint32_t lo, uint32_t hi) {
  uint64_t z = i + seed * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const uint32_t v = (uint32_t)(z >> 40);
  return v >= lo && v < hi;
}

}  // namespace srmap
