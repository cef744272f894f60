// Device-side mirror of hs_colstat (include/hairsplitter_hip.h), shared constants, and what the sorted-key routes of hs_kernels_alleles.hip
// (32-bit keys) and hs_kernels_map.hip (64-bit keys) share. Builtins and plain C++ only.
#pragma once
#include <stdint.h>
namespace hsdev {
struct alignas(16) hs_colstat_dev {
    uint8_t key[4];
    uint16_t cnt[5];
    uint16_t depth;
};
static_assert(sizeof(hs_colstat_dev) == 16, "hs_colstat must be 16 bytes");
// result of k_column_top3 == hs_coltop (include/hairsplitter_hip.h)
struct alignas(16) hs_coltop_dev {
    int32_t c0, c1, c2;
    uint8_t k0, k1, tie, pad;
};
static_assert(sizeof(hs_coltop_dev) == 16, "hs_coltop must be 16 bytes");

// the length block_bitonic_sort sorts for n keys: the next power of two, 2 at least
static __host__ __device__ __forceinline__ int pow2_at_least(int n) { int p = 2; while (p < n) p <<= 1; return p; }

// keys[0, n_pow2) ascending, in LDS or in global scratch: the bitonic network, a compare-exchange per thread and step. Every thread of the
// workgroup calls it (blockDim.x threads), behind a __syncthreads() that follows the last write of a key; it ends in one.
template <class Key> static __device__ __forceinline__ void block_bitonic_sort(Key* keys, int n_pow2) {
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    for (int k = 2; k <= n_pow2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n_pow2 >> 1); t += nt) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const Key a = keys[i], b = keys[l];
                if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
}

// an id onto the list of a wide route (one thread of a workgroup calls it): counted always, written never beyond the list's length
static __device__ __forceinline__ void wide_list_push(int32_t* count, int32_t* list, int length, int id) {
    const int at = atomicAdd(count, 1);
    if (at < length) list[at] = id;
}
}  // namespace hsdev
