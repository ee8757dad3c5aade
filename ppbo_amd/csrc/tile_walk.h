// Workgroup id -> output tile: the two walks whose order is a tuning knob, as pure integer / double arithmetic shared
// by the kernels (predict.hip: quadform_kernel, gram.hip: gram_mfma_kernel) and by the host program that checks,
// exhaustively, that each is a bijection (tests/c/tile_walk_check.cpp).  Nothing here touches memory.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PPBO_WALK_FN __host__ __device__ __forceinline__
#else
#define PPBO_WALK_FN inline
#endif

// The XCD remap of launch_quadform: bit 0 of PPBO_QF_ORDER reaches the kernel only when the grid has at least 64
// workgroups (eight per XCD); the other bits pass unchanged.
PPBO_WALK_FN int ppbo_qf_swizzle(int order, int grid) { return (grid >= 64 ? (order & 1) : 0) | (order & ~1); }

// quadform_kernel: workgroup `id` of `grid` = ntm * ntn -> row tile mt, candidate tile nt.
// swizzle: bit 0 XCD remap, bit 1 candidate tile fastest, >> 2 the chunk width in candidate tiles (0: no chunks).
PPBO_WALK_FN void ppbo_qf_tile(int id, unsigned grid, int swizzle, int ntm, int ntn, int& mt, int& nt) {
  if (swizzle & 1) {                   // XCD-aware: consecutive logical ids share an XCD / L2 (workgroup b runs on XCD b % 8)
    const int per = grid >> 3, rem = grid & 7;
    const int xcd = id & 7, pos = id >> 3;            // a bijection for any grid size: XCDs [0, rem) hold per + 1 ids
    id = pos + (xcd < rem ? xcd * (per + 1) : rem * (per + 1) + (xcd - rem) * per);
  }
  if (swizzle & 2) {                   // candidate tile fastest: co-resident workgroups share one G row panel
    const int ch = swizzle >> 2;       // optional: candidate tiles in chunks of ch (K* chunk stays in the Infinity Cache)
    if (ch > 0 && ch < ntn) {
      const int per_chunk = ntm * ch, full = ntn / ch;
      if (id < full * per_chunk) {
        const int c = id / per_chunk, r = id % per_chunk;
        mt = ntm - 1 - (r / ch); nt = c * ch + (r % ch);
      } else {                         // the last, narrower chunk
        const int cw = ntn - full * ch, r = id - full * per_chunk;
        mt = ntm - 1 - (r / cw); nt = full * ch + (r % cw);
      }
    } else {
      mt = ntm - 1 - (id / ntn); nt = id % ntn;
    }
  } else {                             // row tile fastest, heaviest (largest K range) first: share one K* panel
    mt = ntm - 1 - (id % ntm); nt = id / ntm;
  }
}

// gram_mfma_kernel: workgroup b of nt (nt + 1) / 2 -> tile (bi <= bj) of the nt x nt tile grid.
// Off-diagonal tiles first (row by row over the strict upper triangle), the nt diagonal tiles last: the
// diagonal tiles have no mirror image to write, and the last-dispatched workgroups are the ones that land as
// a third tile on an already busy CU (528 tiles on 256 CUs at N = 2048)
PPBO_WALK_FN void ppbo_gram_tile(unsigned b, int nt, int order, int& bi, int& bj) {
  const int n1 = nt - 1, n_off = n1 * (n1 + 1) / 2;
  if ((int)b >= n_off) {
    bi = bj = b - n_off;
  } else {
    const int t = b;
    const double q = 2.0 * n1 + 1.0;
    bi = (int)floor((q - sqrt(q * q - 8.0 * (double)t)) * 0.5);
    while (bi > 0 && t < bi * n1 - bi * (bi - 1) / 2) --bi;
    while (t >= (bi + 1) * n1 - (bi + 1) * bi / 2) ++bi;
    bj = bi + (t - (bi * n1 - bi * (bi - 1) / 2)) + 1;
    if (order == 1) {
      // diagonal-major: the same decomposition read as (distance k = bi + 1 from the diagonal, position r along
      // it).  Row-major order makes co-resident workgroups share ONE 512-byte column window for their mirror
      // stores (same bi, consecutive bj): with a power-of-two row pitch those all fall on the same memory
      // channels.  Along a diagonal both the direct and the mirror windows move with every workgroup.
      const int k = bi + 1, r = bj - bi - 1;
      bi = r;
      bj = r + k;
    }
  }
}
