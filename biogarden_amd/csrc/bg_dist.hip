// Distances between equal-length rows on gfx950 (DESIGN.md "Distances"): the inner step of
// analysis::seq::hamming_distance (seq.rs:74-83), transition_transversion_ratio (:152-174) and
// analysis::stat::p_distance_matrix (stat.rs:138-152) — count the unequal bytes of two rows.
// No DP: these kernels share nothing with the strip, finish and split code.
//
//   bg_dist_pairs_kernel    mismatches + transitions of independent pairs, one workgroup per
//                           BG_DIST_SEG-byte segment of a pair (memory-bound, 2 B per position)
//   bg_dist_rowpairs_kernel the same segment count for entry (i, j) of a matrix whose rows have
//                           different lengths (zip: min(len_i, len_j)), uint32 counts
//   bg_dist_tile_kernel     counts[i][j] of two equal-length row sets, 64 x 64 tiles from LDS
//                           (VALU-bound: xor, packed non-zero-byte test, popcount-accumulate)
#include <hip/hip_runtime.h>

#include "bg_dist.h"

namespace {

// 0x80 in every byte of x that is not zero (exact: the low seven bits carry into bit 7, bit 7
// itself is or-ed in)
__device__ __forceinline__ uint32_t nz_bytes(uint32_t x) {
  return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}
// 0x80 in every byte of x that equals the byte repeated in k4
__device__ __forceinline__ uint32_t eq_bytes(uint32_t x, uint32_t k4) {
  return nz_bytes(x ^ k4) ^ 0x80808080u;
}
// 0x80 in every byte position holding a transition (seq.rs:164-170): exactly (C,T), (T,C),
// (A,G), (G,A).  The xor alone does not decide it ('@' ^ 'W' == 'C' ^ 'T'), so a is tested too;
// with a ^ b fixed, b follows from a.
__device__ __forceinline__ uint32_t ts_bytes(uint32_t a, uint32_t x) {
  const uint32_t ct = eq_bytes(x, 0x17171717u) & (eq_bytes(a, 0x43434343u) | eq_bytes(a, 0x54545454u));
  const uint32_t ag = eq_bytes(x, 0x06060606u) & (eq_bytes(a, 0x41414141u) | eq_bytes(a, 0x47474747u));
  return ct | ag;
}
__device__ __forceinline__ bool ts_byte(uint8_t a, uint8_t b) {
  return (a == 'C' && b == 'T') || (a == 'T' && b == 'C') || (a == 'A' && b == 'G') ||
         (a == 'G' && b == 'A');
}

// 16 bytes from any address (the staged ranges sit back to back): the compiler emits one
// global_load_dwordx4, which gfx950 serves at any alignment
__device__ __forceinline__ uint4 load16(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// This thread's share of the unequal bytes (and transitions) of p1[0, n) against p2[0, n),
// n <= BG_DIST_SEG: 16-byte vectors strided over the workgroup, the last n % 16 bytes one per thread.
template <bool TS>
__device__ __forceinline__ void seg_count(const uint8_t* p1, const uint8_t* p2, uint32_t n, uint32_t& mis,
                                          uint32_t& ts) {
  const uint32_t nvec = n / 16;
  for (uint32_t v = threadIdx.x; v < nvec; v += BG_DIST_THREADS) {
    const uint4 a = load16(p1 + (size_t)v * 16), b = load16(p2 + (size_t)v * 16);
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t x = aw[w] ^ bw[w];
      mis += __popc(nz_bytes(x));
      if (TS) ts += __popc(ts_bytes(aw[w], x));
    }
  }
  const uint32_t at = nvec * 16 + threadIdx.x;
  if (at < n) {
    const uint8_t a = p1[at], b = p2[at];
    mis += a != b;
    if (TS) ts += ts_byte(a, b);
  }
}

// Sum over the workgroup, valid in thread 0: xor-shuffles inside each wave, then the four waves'
// sums through LDS.
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  uint32_t s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < BG_DIST_THREADS / 64; ++w) s += red[w];
  __syncthreads();
  return s;
}

}  // namespace

template <bool TS>
__global__ __launch_bounds__(BG_DIST_THREADS) void bg_dist_pairs_kernel(BgDistPairsArgs A) {
  __shared__ uint32_t red[BG_DIST_THREADS / 64];
  // the pair owning this segment: the last p with segBase[p] <= blockIdx.x (uniform search)
  uint32_t lo = 0, hi = A.npairs;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (A.segBase[mid] <= blockIdx.x) lo = mid; else hi = mid;
  }
  const BgDistPair P = A.pairs[lo];
  const uint32_t start = (blockIdx.x - A.segBase[lo]) * (uint32_t)BG_DIST_SEG;
  if (start >= P.n) return;                      // (never: segBase counts ceil(n / SEG) per pair)
  const uint32_t n = min(P.n - start, (uint32_t)BG_DIST_SEG);
  uint32_t mis = 0, ts = 0;
  seg_count<TS>(A.bytes + P.off1 + start, A.bytes + P.off2 + start, n, mis, ts);
  mis = block_sum(mis, red);
  if (TS) ts = block_sum(ts, red);
  // integer sums: the order the segments arrive in cannot change the result
  if (threadIdx.x == 0) {
    if (mis) atomicAdd(&A.counts[2 * (size_t)lo], (unsigned long long)mis);
    if (TS && ts) atomicAdd(&A.counts[2 * (size_t)lo + 1], (unsigned long long)ts);
  }
}

// grid: x = segment + segs * j, y = i - row0
__global__ __launch_bounds__(BG_DIST_THREADS) void bg_dist_rowpairs_kernel(BgDistRowsArgs A) {
  __shared__ uint32_t red[BG_DIST_THREADS / 64];
  const uint32_t j = blockIdx.x / A.segs, seg = blockIdx.x % A.segs;
  const uint32_t i = A.row0 + blockIdx.y;
  if (i >= A.na || j >= A.nb) return;
  const uint32_t len = min(A.alen[i], A.blen[j]);
  const uint64_t start = (uint64_t)seg * BG_DIST_SEG;
  if (start >= len) return;
  const uint32_t n = (uint32_t)min((uint64_t)len - start, (uint64_t)BG_DIST_SEG);
  uint32_t mis = 0, ts = 0;
  seg_count<false>(A.bytes + A.aoff[i] + start, A.bytes + A.boff[j] + start, n, mis, ts);
  mis = block_sum(mis, red);
  if (threadIdx.x == 0 && mis) atomicAdd(&A.counts[(size_t)i * A.nb + j], mis);
}

// ---- tiled matrix kernel.  A 256-thread workgroup owns a 64 x 64 tile of counts; thread
// (ty, tx) = (tid / 16, tid % 16) keeps rows 4 ty .. 4 ty + 3 against columns 4 tx .. 4 tx + 3 in
// sixteen uint32 accumulators.  The columns are walked in slabs of BG_DIST_SLAB bytes.  A slab is
// staged transposed: word k of the 64 A rows lies in 64 consecutive dwords (the same for B), so
// one ds_read_b128 gives a thread word k of its four rows and a second one word k of its four
// columns: 8 LDS words for 16 word comparisons.
//
// Bank rule (LDS table of the microarchitecture guide): ds_read_b128 is served in four groups of
// 16 lanes, bank = (address / 4) mod 64, equal addresses broadcast.  Within a wave every lane reads
// the same k.  The A read's address depends on ty only: a 16-lane group holds two values of ty,
// that is two 16-byte slots on disjoint banks, the rest broadcast.  The B read's address is
// 16 tx: each 16-lane group (lanes {0-3, 12-15, 20-27} and so on) holds all sixteen values of tx
// once, sixteen slots covering the 64 banks once.  Both reads are conflict-free.  The word rows are
// padded to 68 dwords (a multiple of 4, so the reads stay 16-byte aligned): the staging stores
// (ds_write_b32, bank = dword mod 32, two 32-lane groups) of the four lanes that share a row then
// land on banks 16 apart, a 2-way conflict, which a ds_write_b32 hides.
namespace {
// acc += unequal bytes of the words a and b, in the five VALU instructions of the tile kernel's
// inner step.  Left to itself hipcc (ROCm 7) folds (a ^ b) & 0x7f7f7f7f into a v_bitop3_b32 beside
// the v_xor_b32 it still needs, and sums popcounts in pairs through v_add3_u32: 5.5 instructions
// per word, three of them three-operand forms that occupy the SIMD about twice as long as a
// v_xor / v_and / v_add (profiles/r01/micro_valu_rates.txt).  The empty statement keeps the xor's
// result opaque, so the and stays a two-operand v_and_b32; the second one is v_bcnt_u32_b32's
// accumulating form (D = popcount(S0) + S1).  Both are plain register-to-register VALU.
__device__ __forceinline__ void count_nz(uint32_t& acc, uint32_t a, uint32_t b) {
  uint32_t x = a ^ b;
  asm("" : "+v"(x));
  const uint32_t t = nz_bytes(x);
  asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(t));
}
constexpr int kTile = BG_DIST_TILE;            // 64 rows / columns per tile
constexpr int kSlabW = BG_DIST_SLAB / 4;        // words per row and slab (16)
constexpr int kRowW = kTile + 4;                // padded dwords per word row
}  // namespace

// rows: na x stride bytes; stride % 16 == 0; columns L .. stride - 1 are zero in both sets
__global__ __launch_bounds__(BG_DIST_THREADS) void bg_dist_tile_kernel(BgDistTileArgs A) {
  __shared__ __attribute__((aligned(16))) uint32_t sA[kSlabW * kRowW];
  __shared__ __attribute__((aligned(16))) uint32_t sB[kSlabW * kRowW];
  const int tid = threadIdx.x;
  uint32_t ti, tj;
  if (A.symmetric) {
    // tiles tj >= ti only, row ti of the upper triangle starting at ti T - ti (ti - 1) / 2
    const uint32_t T = A.tilesB, b = blockIdx.x;
    const float f = 2.f * T + 1.f;
    int t = (int)((f - sqrtf(fmaxf(f * f - 8.f * b, 0.f))) * 0.5f);
    t = max(0, min(t, (int)T - 1));
    auto first = [T](uint32_t r) { return r * T - r * (r - 1) / 2; };
    while (t > 0 && first(t) > b) --t;
    while (t + 1 < (int)T && first(t + 1) <= b) ++t;
    ti = t;
    tj = ti + (b - first(ti));
  } else {
    ti = blockIdx.x / A.tilesB;
    tj = blockIdx.x % A.tilesB;
  }
  const uint32_t i0 = ti * kTile, j0 = tj * kTile;
  // staging: thread -> (row tid / 4, 16-byte piece tid % 4 of the slab).  Rows past the set's end
  // are never read: such a thread loads the set's last row, whose counts are not stored.
  const uint32_t srow = tid >> 2, spiece = tid & 3;
  const uint8_t* ga = A.a + (size_t)min(i0 + srow, A.na - 1) * A.stride;
  const uint8_t* gb = A.b + (size_t)min(j0 + srow, A.nb - 1) * A.stride;
  const int ty = tid >> 4, tx = tid & 15;
  uint32_t acc[4][4] = {};
  const uint32_t nslab = (A.stride + BG_DIST_SLAB - 1) / BG_DIST_SLAB;
  // The last slab may end before 64 bytes: a piece at or past the stride counts as zeros in both
  // sets.  Its load is not skipped but aimed at the row's last piece (stride >= 16), so that every
  // load stays one unconditional global_load_dwordx4 inside the row.
  auto piece = [&](const uint8_t* row, uint32_t col) {
    uint4 v = *reinterpret_cast<const uint4*>(row + min(col, A.stride - 16));
    if (col >= A.stride) v = make_uint4(0, 0, 0, 0);
    return v;
  };
  uint4 ra = piece(ga, spiece * 16), rb = piece(gb, spiece * 16);
  for (uint32_t s = 0; s < nslab; ++s) {
    __syncthreads();                              // the previous slab's reads are done
    {
      uint32_t* wa = sA + (spiece * 4) * kRowW + srow;
      uint32_t* wb = sB + (spiece * 4) * kRowW + srow;
      wa[0] = ra.x; wa[kRowW] = ra.y; wa[2 * kRowW] = ra.z; wa[3 * kRowW] = ra.w;
      wb[0] = rb.x; wb[kRowW] = rb.y; wb[2 * kRowW] = rb.z; wb[3 * kRowW] = rb.w;
    }
    __syncthreads();
    // the next slab's global loads fly during this slab's compares
    ra = piece(ga, (s + 1) * BG_DIST_SLAB + spiece * 16);
    rb = piece(gb, (s + 1) * BG_DIST_SLAB + spiece * 16);
#pragma unroll
    for (int k = 0; k < kSlabW; ++k) {
      const uint4 a = *reinterpret_cast<const uint4*>(sA + k * kRowW + ty * 4);
      const uint4 b = *reinterpret_cast<const uint4*>(sB + k * kRowW + tx * 4);
      const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) count_nz(acc[r][c], aw[r], bw[c]);
    }
  }
  const uint32_t ncols = A.nb;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t i = i0 + ty * 4 + r;
    if (i >= A.na) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t j = j0 + tx * 4 + c;
      if (j >= A.nb) continue;
      // B is A: the diagonal is 0 by definition (stat.rs:144), the tile below the diagonal is
      // this one transposed
      const uint32_t v = (A.symmetric && i == j) ? 0u : acc[r][c];
      A.counts[(size_t)i * ncols + j] = v;
      if (A.symmetric && ti != tj) A.counts[(size_t)j * ncols + i] = v;
    }
  }
}

extern "C" void* bg_dist_pairs_kernel_ptr(int transitions) {
  return transitions ? (void*)bg_dist_pairs_kernel<true> : (void*)bg_dist_pairs_kernel<false>;
}
extern "C" void* bg_dist_rowpairs_kernel_ptr(void) { return (void*)bg_dist_rowpairs_kernel; }
extern "C" void* bg_dist_tile_kernel_ptr(void) { return (void*)bg_dist_tile_kernel; }
