// Stencil-mask layout on a box grid: are the masks implied by the geometry?  Host only, no HIP (tests/stencil_geom_check.cpp builds
// this header with a plain host compiler under the sanitizers).
//
// A 7-point stencil on an nx x ny x nz box, rows numbered x fastest, has the dictionary deltas (-P, -nx, -1, 0, +1, +nx, +P) with
// P = nx ny, and row r = x + nx (y + ny z) lacks exactly the entries that would leave the box.  Where every row's mask equals that
// rule, a kernel can derive the masks from the row number and need not stream them (k_spmv_stencil_marchg, ks_spmv_march.hpp).
// One row that differs -- an entry knocked out, a periodic wrap, a delta order that is not the one above -- and the masks stay
// what decides.
#pragma once

#include <cstddef>
#include <cstdint>

struct StencilGeom {
  bool box = false;         // the masks are the box rule of an nx x ny x nz grid
  int64_t nx = 0, ny = 0, nz = 0;
};

// the mask of row (x, y, z) under the box rule: bit k = slot k present, slots in the order (-P, -nx, -1, 0, +1, +nx, +P)
inline uint8_t stencil_box_mask(int64_t x, int64_t y, int64_t z, int64_t nx, int64_t ny, int64_t nz) {
  return (uint8_t)((z > 0 ? 0x01u : 0u) | (y > 0 ? 0x02u : 0u) | (x > 0 ? 0x04u : 0u) | 0x08u | (x < nx - 1 ? 0x10u : 0u) |
                   (y < ny - 1 ? 0x20u : 0u) | (z < nz - 1 ? 0x40u : 0u));
}

// delta[0 .. nslot): the dictionary's column offsets in slot order; mask8[0 .. n): one byte per row, bit k = slot k present
inline StencilGeom stencil_geometry(const int32_t* delta, int nslot, int64_t n, const uint8_t* mask8, size_t nmask) {
  StencilGeom g;
  if (nslot != 7 || n <= 0 || !delta || !mask8 || nmask != (size_t)n) return g;
  const int64_t nx = delta[5], P = delta[6];
  if (nx < 2 || P <= nx || P % nx != 0 || n % P != 0) return g;
  if (delta[0] != -P || delta[1] != -nx || delta[2] != -1 || delta[3] != 0 || delta[4] != 1) return g;
  const int64_t ny = P / nx, nz = n / P;
  int64_t r = 0;
  for (int64_t z = 0; z < nz; ++z)
    for (int64_t y = 0; y < ny; ++y)
      for (int64_t x = 0; x < nx; ++x, ++r)
        if (mask8[r] != stencil_box_mask(x, y, z, nx, ny, nz)) return g;
  g.box = true;
  g.nx = nx;
  g.ny = ny;
  g.nz = nz;
  return g;
}
