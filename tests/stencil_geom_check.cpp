// Stand-alone host check of csrc/ks_stencil_geom.hpp, built by tests/test_stencil_geom_cpu.py with the host compiler under
// -fsanitize=address,undefined: the decision "the masks of this stencil-mask layout are the box rule of an nx x ny x nz grid" on
// box masks written out here from the definition, and on every way of not being one (each array on the heap at its exact size, so
// a read past an end is reported).  Prints STENCIL_GEOM_CHECK_OK and exits 0 when everything holds.
#include <cstdio>
#include <utility>
#include <vector>

#include "../arnoldimethod.jl_amd/csrc/ks_stencil_geom.hpp"

namespace {

int failures = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);         \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

struct Box {
  int64_t nx, ny, nz, n;
  std::vector<int32_t> delta;
  std::vector<uint8_t> mask;
  Box(int64_t nx_, int64_t ny_, int64_t nz_) : nx(nx_), ny(ny_), nz(nz_), n(nx_ * ny_ * nz_) {
    const int32_t P = (int32_t)(nx * ny);
    delta = {-P, -(int32_t)nx, -1, 0, 1, (int32_t)nx, P};
    // the rule written out entry by entry: slot k is present iff column r + delta[k] is the neighbour inside the box
    for (int64_t z = 0; z < nz; ++z)
      for (int64_t y = 0; y < ny; ++y)
        for (int64_t x = 0; x < nx; ++x) {
          unsigned m = 1u << 3;
          if (z > 0) m |= 1u << 0;
          if (y > 0) m |= 1u << 1;
          if (x > 0) m |= 1u << 2;
          if (x + 1 < nx) m |= 1u << 4;
          if (y + 1 < ny) m |= 1u << 5;
          if (z + 1 < nz) m |= 1u << 6;
          mask.push_back((uint8_t)m);
        }
  }
  StencilGeom decide() const { return stencil_geometry(delta.data(), (int)delta.size(), n, mask.data(), mask.size()); }
  int64_t row(int64_t x, int64_t y, int64_t z) const { return x + nx * (y + ny * z); }
};

void boxes() {
  const int64_t dims[3][3] = {{4, 3, 5}, {7, 2, 2}, {2, 2, 2}};
  for (const auto& d : dims) {
    const Box b(d[0], d[1], d[2]);
    const StencilGeom g = b.decide();
    CHECK(g.box && g.nx == d[0] && g.ny == d[1] && g.nz == d[2]);
  }
}

void not_boxes() {
  {  // one cleared bit (a knocked-out entry), at an interior row, at the first and at the last row
    const int64_t rows[3] = {Box(4, 3, 5).row(1, 1, 2), 0, 4 * 3 * 5 - 1};
    const unsigned bits[3] = {4, 4, 2};
    for (int i = 0; i < 3; ++i) {
      Box b(4, 3, 5);
      CHECK((b.mask[(size_t)rows[i]] >> bits[i]) & 1u);
      b.mask[(size_t)rows[i]] = (uint8_t)(b.mask[(size_t)rows[i]] & ~(1u << bits[i]));
      CHECK(!b.decide().box);
    }
  }
  {  // the own entry missing
    Box b(4, 3, 5);
    b.mask[7] = (uint8_t)(b.mask[7] & ~(1u << 3));
    CHECK(!b.decide().box);
  }
  {  // one extra bit: row (3, 0, 0) with an entry at +1, the first row of the next grid line
    Box b(4, 3, 5);
    const size_t r = (size_t)b.row(3, 0, 0);
    CHECK(!((b.mask[r] >> 4) & 1u));
    b.mask[r] = (uint8_t)(b.mask[r] | (1u << 4));
    CHECK(!b.decide().box);
  }
  {  // an unused eighth bit set
    Box b(4, 3, 5);
    b.mask[11] = (uint8_t)(b.mask[11] | 0x80u);
    CHECK(!b.decide().box);
  }
  {  // a periodic wrap in z: the last plane's rows reach the first plane through a slot of their own (delta -(nz - 1) P in front)
    Box b(4, 3, 5);
    b.delta.insert(b.delta.begin(), -(int32_t)(4 * 12));
    for (auto& m : b.mask) m = (uint8_t)(m << 1);
    for (int64_t r = b.row(0, 0, 4); r < b.n; ++r) b.mask[(size_t)r] = (uint8_t)(b.mask[(size_t)r] | 1u);
    CHECK(!b.decide().box);
  }
  {  // a periodic wrap in x that reuses the +1 slot's neighbour: row (3, 1, 1) reads column r + 1 (an extra bit by the box rule)
    Box b(4, 3, 5);
    for (int64_t z = 0; z < 5; ++z)
      for (int64_t y = 0; y < 3; ++y) b.mask[(size_t)b.row(3, y, z)] = (uint8_t)(b.mask[(size_t)b.row(3, y, z)] | (1u << 4));
    CHECK(!b.decide().box);
  }
  {  // the same deltas in another order
    Box b(4, 3, 5);
    std::swap(b.delta[2], b.delta[4]);
    CHECK(!b.decide().box);
    Box c(4, 3, 5);
    std::swap(c.delta[0], c.delta[1]);
    CHECK(!c.decide().box);
  }
  {  // n is not a whole number of planes: the last plane is cut short
    Box b(4, 3, 5);
    b.mask.resize(b.mask.size() - 5);
    b.n -= 5;
    CHECK(!b.decide().box);
  }
  {  // P is not a whole number of grid lines
    Box b(4, 3, 5);
    b.delta[0] = -14;
    b.delta[6] = 14;
    CHECK(!b.decide().box);
  }
  {  // nx = 1: -1 and -nx would be the same column
    Box b(4, 3, 5);
    b.delta[1] = -1;
    b.delta[5] = 1;
    CHECK(!b.decide().box);
  }
  {  // a 5-point (2-D) dictionary
    const std::vector<int32_t> delta{-4, -1, 0, 1, 4};
    std::vector<uint8_t> mask;
    for (int y = 0; y < 3; ++y)
      for (int x = 0; x < 4; ++x) mask.push_back((uint8_t)((y > 0 ? 1u : 0u) | (x > 0 ? 2u : 0u) | 4u | (x < 3 ? 8u : 0u) | (y < 2 ? 16u : 0u)));
    CHECK(!stencil_geometry(delta.data(), 5, 12, mask.data(), mask.size()).box);
  }
  {  // a mask array of another length than n, no masks, no rows
    const Box b(4, 3, 5);
    CHECK(!stencil_geometry(b.delta.data(), 7, b.n, b.mask.data(), b.mask.size() - 1).box);
    CHECK(!stencil_geometry(b.delta.data(), 7, b.n, nullptr, 0).box);
    CHECK(!stencil_geometry(b.delta.data(), 7, 0, b.mask.data(), 0).box);
  }
}

}  // namespace

int main() {
  boxes();
  not_boxes();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("STENCIL_GEOM_CHECK_OK\n");
  return 0;
}
