// Stand-alone host check of csrc/ks_halo_plan.hpp, built by tests/test_halo_plan_cpu.py with the host compiler under
// -fsanitize=address,undefined: plan_halo on a mixed plan and on the malformed inputs that used to be read out of bounds (every
// array lives on the heap at its exact size, so a read past an end is reported), and the arithmetic of the peer-to-peer table on
// hand-made two- and three-rank tables.  Prints HALO_PLAN_CHECK_OK and exits 0 when everything holds.
#include <cstdio>
#include <string>
#include <vector>

#include "../arnoldimethod.jl_amd/csrc/ks_halo_plan.hpp"

namespace {

int failures = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);         \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

using I64 = std::vector<int64_t>;
using I32 = std::vector<int32_t>;

template <class F> void expect_error(int line, F f, const std::string& msg) {
  try {
    f();
    std::printf("line %d: no error, expected \"%s\"\n", line, msg.c_str());
    ++failures;
  } catch (const KsError& e) {
    if (e.code != KS_ERR_ARGUMENT || e.msg != msg) {
      std::printf("line %d: error %d \"%s\", expected %d \"%s\"\n", line, e.code, e.msg.c_str(), (int)KS_ERR_ARGUMENT, msg.c_str());
      ++failures;
    }
  }
}
#define EXPECT_ERROR(msg, ...) expect_error(__LINE__, [&] { __VA_ARGS__; }, msg)

// 12 rows with their diagonal; rows 0 and 11 also read a ghost column
struct Block {
  int64_t n = 12, nghost = 6;
  I64 rp;
  I32 ci;
  Block() {
    rp.push_back(0);
    for (int32_t r = 0; r < n; ++r) {
      ci.push_back(r);
      if (r == 0) ci.push_back((int32_t)n);
      if (r == n - 1) ci.push_back((int32_t)(n + nghost - 1));
      rp.push_back((int64_t)ci.size());
    }
  }
};

// a plan with one neighbour `q` that sends `nsend` consecutive rows and receives `nrecv` entries
HaloPlan one_neighbour(int rank, int q, int64_t nsend, int64_t nrecv) {
  const I64 rp(13, 0);
  const I32 ci, neigh{q};
  const I64 sp{0, nsend}, rc{nrecv};
  I32 si;
  for (int64_t i = 0; i < nsend; ++i) si.push_back((int32_t)i);
  return plan_halo(rp, ci, 12, nrecv, rank, 1, neigh.data(), sp.data(), si.data(), rc.data());
}

void mixed_plan() {
  const Block B;
  // rank 1: a consecutive list to rank 0, a scattered one to rank 2, nothing sent to rank 3 (which still fills 3 ghost slots)
  const I32 neigh{0, 2, 3}, si{3, 4, 5, 1, 7, 8};
  const I64 sp{0, 3, 6, 6}, rc{2, 1, 3};
  const HaloPlan P = plan_halo(B.rp, B.ci, B.n, B.nghost, 1, 3, neigh.data(), sp.data(), si.data(), rc.data());
  CHECK(P.nghost == 6 && P.nlow == 2);
  CHECK(P.ghost_lo_end == 1 && P.ghost_hi_begin == 11);
  CHECK((P.neigh == std::vector<int>{0, 2, 3}));
  CHECK((P.send_ptr == I64{0, 3, 6, 6}));
  CHECK((P.recv_ptr == I64{0, 2, 3, 6}));
  CHECK((P.send_first == I64{3, -1, -1}));
  CHECK((P.pack_ptr == I64{0, 0, 3, 3}));
  CHECK((P.packed == I32{1, 7, 8}) && P.nscatter == 3);
  CHECK((P.send_all == si));
  // no neighbours at all: null arrays are fine, nothing is read
  const Block B0;
  I32 local(B0.ci);
  for (auto& c : local) c = std::min<int32_t>(c, 11);
  const HaloPlan Z = plan_halo(B0.rp, local, B0.n, 0, 0, 0, nullptr, nullptr, nullptr, nullptr);
  CHECK(Z.nlow == 0 && Z.ghost_lo_end == 0 && Z.ghost_hi_begin == 12 && Z.nscatter == 0);
  CHECK((Z.send_ptr == I64{0}) && (Z.recv_ptr == I64{0}) && Z.send_first.empty() && Z.send_all.empty());
  // a lower-ranked neighbour after a higher one
  const I32 neigh2{2, 0};
  const I64 sp2{0, 0, 0}, rc2{4, 2};
  CHECK(plan_halo(B.rp, B.ci, B.n, B.nghost, 1, 2, neigh2.data(), sp2.data(), nullptr, rc2.data()).nlow == -1);
}

void malformed_inputs() {
  const Block B;
  const I32 neigh{0, 2}, si{3, 4, 5, 1, 7, 8};
  const I64 sp{0, 3, 6}, rc{2, 4};
  auto plan = [&](int nneigh, const int32_t* ne, const int64_t* s, const int32_t* i, const int64_t* r) {
    plan_halo(B.rp, B.ci, B.n, B.nghost, 1, nneigh, ne, s, i, r);
  };
  plan(2, neigh.data(), sp.data(), si.data(), rc.data());  // the well-formed one
  EXPECT_ERROR("negative neighbour count", plan(-1, neigh.data(), sp.data(), si.data(), rc.data()));
  EXPECT_ERROR("null halo plan array", plan(2, nullptr, sp.data(), si.data(), rc.data()));
  EXPECT_ERROR("null halo plan array", plan(2, neigh.data(), nullptr, si.data(), rc.data()));
  EXPECT_ERROR("null halo plan array", plan(2, neigh.data(), sp.data(), si.data(), nullptr));
  EXPECT_ERROR("null send index array", plan(2, neigh.data(), sp.data(), nullptr, rc.data()));
  const I64 sp_off{2, 3, 6}, sp_back{0, 4, 3}, sp_neg{0, -1, 6};
  EXPECT_ERROR("send pointer does not start at 0", plan(2, neigh.data(), sp_off.data(), si.data(), rc.data()));
  EXPECT_ERROR("send pointer is not monotone", plan(2, neigh.data(), sp_back.data(), si.data(), rc.data()));
  EXPECT_ERROR("send pointer is not monotone", plan(2, neigh.data(), sp_neg.data(), si.data(), rc.data()));
  const I64 rc_neg{7, -1}, rc_short{2, 3};
  EXPECT_ERROR("negative receive count", plan(2, neigh.data(), sp.data(), si.data(), rc_neg.data()));
  EXPECT_ERROR("recv counts do not add up to nghost", plan(2, neigh.data(), sp.data(), si.data(), rc_short.data()));
  const I32 si_high{3, 4, 5, 1, 7, 12}, si_neg{3, 4, 5, -1, 7, 8};
  EXPECT_ERROR("send index out of range", plan(2, neigh.data(), sp.data(), si_high.data(), rc.data()));
  EXPECT_ERROR("send index out of range", plan(2, neigh.data(), sp.data(), si_neg.data(), rc.data()));
}

void peer_to_peer_tables() {
  // sizes: stride = round_up(max(nghost, 1), 32) elements, bytes = round_up(2 stride elem, 256)
  CHECK(p2p_ghost_size(one_neighbour(0, 1, 0, 0), 8).stride == 32 && p2p_ghost_size(one_neighbour(0, 1, 0, 0), 8).bytes == 512);
  CHECK(p2p_ghost_size(one_neighbour(0, 1, 0, 33), 8).stride == 64 && p2p_ghost_size(one_neighbour(0, 1, 0, 33), 16).bytes == 2048);
  {
    const I64 rp(13, 0), sp(18, 0), rc(17, 0);
    const I32 ci, neigh(17, 1);
    const HaloPlan wide = plan_halo(rp, ci, 12, 0, 0, 17, neigh.data(), sp.data(), nullptr, rc.data());  // fine on the collective transports
    EXPECT_ERROR("peer-to-peer halo supports at most 16 neighbours per rank", p2p_ghost_size(wide, 8));
  }
  // two ranks, 8-byte elements: rank 0 sends 3 and receives 2, rank 1 the reverse
  {
    const HaloPlan P0 = one_neighbour(0, 1, 3, 2), P1 = one_neighbour(1, 0, 2, 3);
    const I64 row0 = p2p_table_row(P0, 2, 4096, 32), row1 = p2p_table_row(P1, 2, 8704, 64);
    CHECK((row0 == I64{4096, 32, 0, 0, 0, 2}));
    CHECK((row1 == I64{8704, 64, 0, 3, 0, 0}));
    I64 tab(row0);
    tab.insert(tab.end(), row1.begin(), row1.end());
    const P2pPeers a = p2p_read_table(P0, 0, 2, tab, 8), b = p2p_read_table(P1, 1, 2, tab, 8);
    CHECK((a.dst_offset == I64{8704}) && (a.dst_stride == I64{64}) && (a.recv_from == std::vector<int>{1}));
    CHECK((b.dst_offset == I64{4096}) && (b.dst_stride == I64{32}) && (b.recv_from == std::vector<int>{0}));
    EXPECT_ERROR("bad neighbour rank", p2p_table_row(one_neighbour(0, 2, 3, 2), 2, 4096, 32));
    EXPECT_ERROR("bad neighbour rank", p2p_table_row(one_neighbour(0, -1, 3, 2), 2, 4096, 32));
    // rank 1 expects 3 entries from rank 0, which now sends 4
    EXPECT_ERROR("halo plans disagree: rank 1 expects 3 entries from rank 0, which sends 4", p2p_read_table(one_neighbour(0, 1, 4, 2), 0, 2, tab, 8));
  }
  // three ranks, 16-byte elements, seen from rank 1: 3 rows to rank 0 (which puts them behind 7 entries of rank 2's), 2 rows to
  // rank 2; 4 entries from rank 0, none from rank 2
  {
    const I64 rp(13, 0), sp{0, 3, 5}, rc{4, 0};
    const I32 ci, neigh{0, 2}, si{0, 1, 2, 10, 11};
    const HaloPlan P = plan_halo(rp, ci, 12, 4, 1, 2, neigh.data(), sp.data(), si.data(), rc.data());
    CHECK((p2p_table_row(P, 3, 1024, 32) == I64{1024, 32, 0, 4, 0, 0, 4, 0}));
    const I64 tab{/* rank 0 */ 4096, 32, 0, 0, 7, 3, 0, 7,
                  /* rank 1 */ 1024, 32, 0, 4, 0, 0, 4, 0,
                  /* rank 2 */ 512, 96, 2, 5, 0, 2, 0, 0};
    const P2pPeers a = p2p_read_table(P, 1, 3, tab, 16);
    CHECK((a.dst_offset == I64{4096 + 7 * 16, 512}) && (a.dst_stride == I64{32, 96}) && (a.recv_from == std::vector<int>{0}));
    I64 bad(tab);
    bad[16 + 5] = 5;
    EXPECT_ERROR("halo plans disagree: rank 2 expects 5 entries from rank 1, which sends 2", p2p_read_table(P, 1, 3, bad, 16));
  }
}

}  // namespace

int main() {
  mixed_plan();
  malformed_inputs();
  peer_to_peer_tables();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("HALO_PLAN_CHECK_OK\n");
  return 0;
}
