// What the host-only code (ks_csr_layout.hpp, ks_halo_plan.hpp) shares with the device side: the launch-shape constants the CSR
// layouts are planned around, the neighbour limit of the peer-to-peer halo, the error type and the two small helpers.  No HIP header: a plain host compiler can build this.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <string>

#include "../../include/kschur.h"

namespace ksd {
constexpr int kBlock = 256;           // threads per workgroup (4 waves)
constexpr int kSpmvRows = 256;        // k_spmv_csr: rows per block at most
constexpr int kSpmvCapBytes = 32768;  // k_spmv_csr: LDS for the products of a block: NI * 256 * sizeof(T) <= 32 KiB
constexpr int kCbMaxBlocks = 8;       // k_spmv_csr_cb: column blocks of one launch (CbArgs)
constexpr int kStencilSlots = 32;     // k_spmv_stencil: dictionary slots (StencilDict)
constexpr int kP2pMaxNeigh = 16;      // peer-to-peer halo: neighbours of a rank (HaloArgs, ks_p2p.hpp)
}  // namespace ksd

namespace {

struct KsError {
  int code;
  std::string msg;
};

#define KS_REQUIRE(cond, code, text)           \
  do {                                         \
    if (!(cond)) throw KsError{(code), (text)}; \
  } while (0)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline int env_int(const char* name, int dflt) {
  const char* s = std::getenv(name);
  return s ? std::atoi(s) : dflt;
}

}  // namespace
