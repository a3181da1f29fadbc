// Host/device layout of the distance kernels (bg_dist.hip; launched by bg_host.cpp's
// bg_hamming_batch / bg_mismatch_matrix).
#pragma once
#include <stdint.h>

#define BG_DIST_THREADS 256
#define BG_DIST_SEG 65536    // bytes of a pair one workgroup counts (pair kernels)
#define BG_DIST_TILE 64      // rows x columns of counts per workgroup (tile kernel)
#define BG_DIST_SLAB 64      // bytes of every row staged in LDS per step (tile kernel)

// One pair of equal-length byte ranges in the staging buffer.
struct BgDistPair {
  uint64_t off1, off2;
  uint32_t n;
  uint32_t pad;
};

struct BgDistPairsArgs {
  const uint8_t* bytes;
  const BgDistPair* pairs;
  const uint32_t* segBase;        // npairs + 1: first workgroup of each pair (ceil(n / SEG) each)
  unsigned long long* counts;     // [2 p] mismatches, [2 p + 1] transitions; zeroed before the launch
  uint32_t npairs;
};

// Entry (i, j) over min(alen[i], blen[j]) bytes, for rows of different lengths.
struct BgDistRowsArgs {
  const uint8_t* bytes;
  const uint64_t* aoff;
  const uint64_t* boff;
  const uint32_t* alen;
  const uint32_t* blen;
  uint32_t* counts;               // na x nb, zeroed before the launch
  uint32_t na, nb;
  uint32_t segs;                  // workgroups per entry: ceil(longest row / SEG)
  uint32_t row0;                  // first row of this launch (blockIdx.y counts from it)
};

struct BgDistTileArgs {
  const uint8_t* a;               // na rows of `stride` bytes, 16-byte aligned, zero beyond L
  const uint8_t* b;               // nb rows (symmetric: the same pointer)
  uint32_t* counts;               // na x nb
  uint32_t na, nb;
  uint32_t stride;                // a multiple of 16
  uint32_t tilesB;                // ceil(nb / TILE)
  uint32_t symmetric;             // 1: B is A; grid = T (T + 1) / 2 tiles with tj >= ti
};
