// Host side of the halo exchange of a distributed row block (ks_operator_csr_dist): everything that is decided from the caller's
// arrays alone -- which ghost slots lower ranks own, the interior rows that never read a ghost, the receive offsets, which send
// lists go out in place and which are packed -- and the arithmetic of the peer-to-peer table.  No HIP: a plain host compiler
// builds this header (tests/halo_plan_check.cpp); Halo<D>::upload (ks_halo.hpp) turns a plan into device arrays, and
// ks_host_halo_plan (include/kschur.h) reports it without a device.
#pragma once

#include <algorithm>
#include <vector>

#include "ks_host_defs.hpp"

namespace {

struct HaloPlan {
  int64_t nghost = 0;
  // ghost slots owned by lower ranks (they precede the local columns in the global order: column blocks keep the single-GPU
  // summation order); -1: a lower-ranked neighbour follows one that is not lower -> no column blocks
  int64_t nlow = 0;
  // rows that reference ghost columns all lie outside ONE interval [ghost_lo_end, ghost_hi_begin) -- the largest gap between
  // such rows (a slab of a structured grid: everything between its first and its last plane).  Workgroups whose rows fall
  // inside never wait for the exchange (fused halo, ks_p2p.hpp).
  int64_t ghost_lo_end = 0, ghost_hi_begin = 0;
  std::vector<int> neigh;
  std::vector<int64_t> send_ptr, recv_ptr;  // nneigh + 1 each; recv_ptr: neighbour p fills the ghost slots [recv_ptr[p], recv_ptr[p+1])
  std::vector<int64_t> send_first;  // >= 0: neighbour p's rows are the consecutive run starting here (sent in place, no packing)
  std::vector<int64_t> pack_ptr;    // offset of neighbour p's entries in `packed` (non-consecutive lists only)
  std::vector<int32_t> packed;      // the non-consecutive send lists, neighbour by neighbour
  int64_t nscatter = 0;             // == packed.size()
  std::vector<int32_t> send_all;    // every send entry (consecutive runs included), neighbour by neighbour: the peer-to-peer transport
  int nneigh() const { return (int)neigh.size(); }
};

// (rp, ci): the validated CSR arrays of the row block, columns local-extended (>= nrows_local: a ghost slot)
inline HaloPlan plan_halo(const std::vector<int64_t>& rp, const std::vector<int32_t>& ci, int64_t nrows_local, int64_t nghost, int rank,
                          int nneigh, const int32_t* neigh, const int64_t* send_ptr, const int32_t* send_idx, const int64_t* recv_cnt) {
  KS_REQUIRE(nneigh >= 0, KS_ERR_ARGUMENT, "negative neighbour count");
  KS_REQUIRE(nneigh == 0 || (neigh && send_ptr && recv_cnt), KS_ERR_ARGUMENT, "null halo plan array");
  HaloPlan P;
  P.nghost = nghost;
  P.neigh.assign(neigh, neigh + nneigh);
  bool above = false, ascending = true;
  P.recv_ptr.assign((size_t)nneigh + 1, 0);
  for (int p = 0; p < nneigh; ++p) {
    KS_REQUIRE(recv_cnt[p] >= 0, KS_ERR_ARGUMENT, "negative receive count");
    if (neigh[p] < rank) { if (above) ascending = false; P.nlow += recv_cnt[p]; }
    else above = true;
    P.recv_ptr[p + 1] = P.recv_ptr[p] + recv_cnt[p];
  }
  if (!ascending) P.nlow = -1;
  KS_REQUIRE(P.recv_ptr[nneigh] == nghost, KS_ERR_ARGUMENT, "recv counts do not add up to nghost");
  {
    int64_t best_a = 0, best_b = nrows_local, prev = -1, gap_best = -1;
    bool any = false;
    for (int64_t r = 0; r < nrows_local; ++r) {
      bool touches = false;
      for (int64_t q = rp[r]; q < rp[r + 1] && !touches; ++q) touches = ci[q] >= nrows_local;
      if (!touches) continue;
      any = true;
      if (r - prev - 1 > gap_best) { gap_best = r - prev - 1; best_a = prev + 1; best_b = r; }
      prev = r;
    }
    if (any && nrows_local - prev - 1 > gap_best) { best_a = prev + 1; best_b = nrows_local; }
    P.ghost_lo_end = any ? best_a : 0;
    P.ghost_hi_begin = any ? best_b : nrows_local;
  }
  // split the send lists into consecutive runs (sent in place) and the others (packed)
  P.send_ptr.assign((size_t)nneigh + 1, 0);
  P.send_first.assign(nneigh, -1);
  P.pack_ptr.assign((size_t)nneigh + 1, 0);
  KS_REQUIRE(nneigh == 0 || send_ptr[0] == 0, KS_ERR_ARGUMENT, "send pointer does not start at 0");
  for (int p = 0; p < nneigh; ++p) {
    const int64_t a = send_ptr[p], b = send_ptr[p + 1];
    KS_REQUIRE(b >= a, KS_ERR_ARGUMENT, "send pointer is not monotone");
    KS_REQUIRE(b == a || send_idx, KS_ERR_ARGUMENT, "null send index array");
    P.send_ptr[p + 1] = b;
    bool consecutive = b > a;
    for (int64_t q = a; q < b; ++q) {
      KS_REQUIRE(send_idx[q] >= 0 && send_idx[q] < nrows_local, KS_ERR_ARGUMENT, "send index out of range");
      if (q > a && send_idx[q] != send_idx[q - 1] + 1) consecutive = false;
    }
    if (consecutive) P.send_first[p] = send_idx[a];
    else if (b > a) P.packed.insert(P.packed.end(), send_idx + a, send_idx + b);
    P.pack_ptr[p + 1] = (int64_t)P.packed.size();
  }
  P.nscatter = (int64_t)P.packed.size();
  if (P.send_ptr[nneigh] > 0) P.send_all.assign(send_idx, send_idx + P.send_ptr[nneigh]);
  return P;
}

// ---- peer-to-peer transport: the ghost vector lives (double-buffered) in this rank's shared arena, the neighbours store into
// it directly.  One collective at upload time gathers a table with one row per rank; these three functions are its arithmetic
// (elem: sizeof of the element type).
struct P2pGhost {
  int64_t stride;  // elements between the two ghost slots
  size_t bytes;    // of the arena, both slots
};
inline P2pGhost p2p_ghost_size(const HaloPlan& P, size_t elem) {
  KS_REQUIRE(P.nneigh() <= ksd::kP2pMaxNeigh, KS_ERR_ARGUMENT, "peer-to-peer halo supports at most 16 neighbours per rank");
  const int64_t stride = round_up(std::max<int64_t>(P.nghost, 1), 32);
  return {stride, (size_t)round_up(2 * stride * (int64_t)elem, 256)};
}

// the row a rank publishes: {byte offset of its ghost vector in its region, stride, then per sender rank (recv_ptr, recv_cnt)}
inline std::vector<int64_t> p2p_table_row(const HaloPlan& P, int nranks, int64_t ghost_offset, int64_t ghost_stride) {
  std::vector<int64_t> row((size_t)2 + 2 * nranks, 0);
  row[0] = ghost_offset;
  row[1] = ghost_stride;
  for (int p = 0; p < P.nneigh(); ++p) {
    KS_REQUIRE(P.neigh[p] >= 0 && P.neigh[p] < nranks, KS_ERR_ARGUMENT, "bad neighbour rank");
    row[2 + 2 * P.neigh[p]] = P.recv_ptr[p];
    row[3 + 2 * P.neigh[p]] = P.recv_ptr[p + 1] - P.recv_ptr[p];
  }
  return row;
}

// what the gathered table (nranks rows of p2p_table_row) says about this rank's neighbours
struct P2pPeers {
  std::vector<int64_t> dst_offset;  // per neighbour: byte offset, in the peer's region, of where THIS rank's entries go (ghost slot 0)
  std::vector<int64_t> dst_stride;  // per neighbour: elements between the peer's two ghost slots
  std::vector<int> recv_from;       // the ranks this one receives entries from
};
inline P2pPeers p2p_read_table(const HaloPlan& P, int rank, int nranks, const std::vector<int64_t>& tab, size_t elem) {
  const size_t K = (size_t)2 + 2 * nranks;
  P2pPeers out;
  for (int p = 0; p < P.nneigh(); ++p) {
    const int q = P.neigh[p];
    const int64_t sc = P.send_ptr[p + 1] - P.send_ptr[p];
    const int64_t* tq = tab.data() + (size_t)q * K;
    KS_REQUIRE(tq[3 + 2 * rank] == sc, KS_ERR_ARGUMENT,
               "halo plans disagree: rank " + std::to_string(q) + " expects " + std::to_string(tq[3 + 2 * rank]) + " entries from rank " +
                   std::to_string(rank) + ", which sends " + std::to_string(sc));
    out.dst_offset.push_back(tq[0] + tq[2 + 2 * rank] * (int64_t)elem);
    out.dst_stride.push_back(tq[1]);
    if (P.recv_ptr[p + 1] > P.recv_ptr[p]) out.recv_from.push_back(q);
  }
  return out;
}

}  // namespace
