// The 64-bit finalizer (MurmurHash3's fmix64) that the open-addressing tables of mm_unique_hash.hip (rows of points) and
// mm_boundary.hip (sorted corner ids of faces) hash with.  The tables' probe loops differ -- their empty markers are -1
// and 0 -- and stay with their units.
#pragma once

__device__ __forceinline__ unsigned long long mm_mix64(unsigned long long h)
{
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}
