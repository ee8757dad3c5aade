// Host check of ppbo_amd/csrc/tile_walk.h: the workgroup id -> tile maps of quadform_kernel and gram_mfma_kernel, the
// very functions the kernels call, are bijections -- every tile is hit exactly once, none out of range.
//   contraction: ntm 1..48 x ntn 1..600 x orders {0, 1, 2, 3, 14, 23, 258, 514, 515, 1026, 1027}, bit 0 of the order
//                applied as launch_quadform applies it (ppbo_qf_swizzle: only from 64 workgroups on);
//   Gram:        nt 1..160, both orders: bi <= bj < nt and every tile on or above the diagonal once.
// Built by tests/test_tile_walks_host.py with -fsanitize=address,undefined.  Prints "tile_walk_check ok" and exits 0,
// or prints the first ids that collide / leave the grid and exits 1.
#include <cstdio>
#include <vector>

#include "../../ppbo_amd/csrc/tile_walk.h"

static int failures = 0;

static void fail(const char* what, int a, int b, int c, int id, int x, int y) {
  if (++failures <= 20) std::printf("FAIL %s (%d, %d, order %d): id %d -> (%d, %d)\n", what, a, b, c, id, x, y);
}

int main() {
  const int orders[] = {0, 1, 2, 3, 14, 23, 258, 514, 515, 1026, 1027};
  long long walks = 0, tiles = 0;
  std::vector<unsigned char> hit;
  for (int ntm = 1; ntm <= 48; ++ntm)
    for (int ntn = 1; ntn <= 600; ++ntn)
      for (int order : orders) {
        const int grid = ntm * ntn;
        const int swz = ppbo_qf_swizzle(order, grid);
        hit.assign((size_t)grid, 0);
        for (int id = 0; id < grid; ++id) {
          int mt = -1, nt = -1;
          ppbo_qf_tile(id, (unsigned)grid, swz, ntm, ntn, mt, nt);
          if (mt < 0 || mt >= ntm || nt < 0 || nt >= ntn) {
            fail("quadform tile out of range", ntm, ntn, order, id, mt, nt);
            continue;
          }
          if (hit[(size_t)mt * ntn + nt]++) fail("quadform tile hit twice", ntm, ntn, order, id, mt, nt);
        }
        // grid ids, all in range, none twice: every tile exactly once
        ++walks;
        tiles += grid;
      }
  // the remap of bit 0 must be what launch_quadform decides, not the raw bit
  if (ppbo_qf_swizzle(23, 63) != 22 || ppbo_qf_swizzle(23, 64) != 23 || ppbo_qf_swizzle(1026, 4096) != 1026) {
    std::printf("FAIL ppbo_qf_swizzle\n");
    ++failures;
  }
  for (int nt = 1; nt <= 160; ++nt)
    for (int order = 0; order <= 1; ++order) {
      const int nblk = nt * (nt + 1) / 2;
      hit.assign((size_t)nt * nt, 0);
      for (int b = 0; b < nblk; ++b) {
        int bi = -1, bj = -1;
        ppbo_gram_tile((unsigned)b, nt, order, bi, bj);
        if (bi < 0 || bi > bj || bj >= nt) {
          fail("gram tile out of range", nt, nt, order, b, bi, bj);
          continue;
        }
        if (hit[(size_t)bi * nt + bj]++) fail("gram tile hit twice", nt, nt, order, b, bi, bj);
      }
      ++walks;
      tiles += nblk;
    }
  if (failures) {
    std::printf("tile_walk_check: %d failures\n", failures);
    return 1;
  }
  std::printf("tile_walk_check ok: %lld walks, %lld tiles\n", walks, tiles);
  return 0;
}
