// Which device layout a stored sparse matrix gets, and the host arrays of that layout: pure host arithmetic on the int32 0-based
// CSR arrays (rp / ci / vv).  No HIP header and no hip* call -- make_csr (ks_operators.hpp) uploads the plan made here, and
// ks_host_csr_plan (include/kschur.h) reports it without a device.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "ks_host_defs.hpp"

namespace {

// whether the operator may be split into column blocks
enum class CbMode {
  None,                // not allowed
  Allowed,             // decided by plan_column_blocks
  IsColumnBlock,       // this IS a column block: plain CSR row blocks, nothing else is tried
  DistributedRowBlock  // allowed, row block of a distributed operator: columns >= nrows are ghost slots (nghost of them, the first
                       // nlow owned by lower ranks -- they precede the local columns in the global order)
};

// The environment switches of the layout choice, read once per upload (tests switch them inside one process).
struct FormatRequest {
  bool format_set = false;  // KS_SPMV_FORMAT = stencil | dvi | vi | sell | sellvi | csr pins a layout (default: the most compact
  std::string format;       // that applies); a value that is none of these only switches the dictionary-per-entry layouts off
  bool ptr64 = false;       // KS_SPMV_PTR64=1 forces 64-bit non-zero offsets (tests)
  int sell_sigma = 1;       // KS_SELL_SIGMA: window for sorting rows by length, rounded up to a multiple of 64 (1: no permutation)
  int dvi_rpt = 1;          // KS_DVI_RPT
  int colblocks = -1;       // KS_SPMV_COLBLOCKS = 0 off / k >= 2 force
  int cb_rpt = 0;           // KS_SPMV_CB_RPT = k forces the single-launch form with k sub-tiles per workgroup
  int cb_single = 1;        // KS_SPMV_CB_SINGLE = 0: never the single-launch form
  int ni = INT_MIN;         // KS_SPMV_NI (INT_MIN: from the matrix)
  int row_gather = -1;      // KS_SPMV_CSR_ROWGATHER = 0 / 1 forces

  static FormatRequest from_env() {
    FormatRequest q;
    const char* fmt = std::getenv("KS_SPMV_FORMAT");
    q.format_set = fmt != nullptr;
    q.format = fmt ? fmt : "";
    q.ptr64 = env_int("KS_SPMV_PTR64", 0) != 0;
    q.sell_sigma = std::max(1, env_int("KS_SELL_SIGMA", 1));
    if (q.sell_sigma > 1) q.sell_sigma = (int)round_up(q.sell_sigma, 64);
    q.dvi_rpt = env_int("KS_DVI_RPT", 1);
    q.colblocks = env_int("KS_SPMV_COLBLOCKS", -1);
    q.cb_rpt = env_int("KS_SPMV_CB_RPT", 0);
    q.cb_single = env_int("KS_SPMV_CB_SINGLE", 1);
    q.ni = env_int("KS_SPMV_NI", INT_MIN);
    q.row_gather = env_int("KS_SPMV_CSR_ROWGATHER", -1);
    return q;
  }
  FormatRequest for_column_block() const {  // plain CSR whatever the environment says
    FormatRequest q = *this;
    q.format_set = true;
    q.format = "csr";
    return q;
  }
  bool try_dvi() const { return !format_set || format == "dvi" || format == "stencil"; }  // build the (delta, value) dictionary
  bool try_stencil() const { return format != "dvi"; }       // ... =dvi keeps the byte-per-entry layout,
  bool insist_stencil() const { return format == "stencil"; }  // =stencil insists on the mask layout
  bool try_vi() const { return format != "csr" && format != "dvi" && format != "sell"; }
  bool force_sell() const { return format == "sell" || format == "sellvi"; }
  bool allow_sell() const { return force_sell() || format.empty(); }
  bool sell_keeps_dict() const { return format != "sell"; }
};

// the matrix being planned: int32 0-based CSR on the host
template <class D> struct CsrHost {
  int64_t nrows, nnz;
  const std::vector<int64_t>& rp;
  const std::vector<int32_t>& ci;
  const std::vector<D>& vv;
};

// The chosen layout: the scalars the operator keeps and the host arrays make_csr uploads.
template <class D> struct CsrPlan {
  int layout = -1;  // KS_LAYOUT_*
  bool ptr64 = false;
  double bytes_per_nnz = 0.0, aux_bytes = 0.0;
  // stencil mask (KS_LAYOUT_STENCIL): dictionary in slot order, one mask per row (bytes or words)
  int nstencil = 0, nstencil_local = 0, stencil_mask_bytes = 1;
  std::vector<int32_t> sdelta;
  std::vector<D> sval;
  std::vector<uint8_t> mask8;
  std::vector<uint32_t> mask32;
  // delta-value-indexed (KS_LAYOUT_DVI)
  int ndvi = 0, dvi_unroll = 8, dvi_rpt = 1;
  std::vector<uint8_t> codes;
  std::vector<int32_t> ddelta;
  std::vector<D> dval;
  // value-indexed (KS_LAYOUT_CSR_VI / SELL_VI): dictionary and (dictionary index << 24) | column
  int ndict = 0;
  std::vector<D> dict;
  std::vector<int32_t> packed;
  // sliced ELLPACK (KS_LAYOUT_SELL / SELL_VI)
  int nslices = 0, sell_un = 8;
  int64_t sell_entries = 0;
  std::vector<int64_t> sliceptr;
  std::vector<int32_t> sell_col, sell_perm;
  std::vector<D> sell_val;
  // column blocks (KS_LAYOUT_CSR_CB): block b holds the entries with key in [cb_bounds[b], cb_bounds[b+1]); each is a plan of its
  // own over its sub-matrix (sub_*: filled in a column block only)
  std::vector<CsrPlan<D>> cblocks;
  std::vector<char> cb_from_ghost;
  std::vector<int64_t> cb_bounds;
  int cb_rpt = 0, cb_ni = 0;
  std::vector<int64_t> sub_rp;
  std::vector<int32_t> sub_ci;
  std::vector<D> sub_vv;
  // CSR row blocks (KS_LAYOUT_CSR / CSR_VI)
  int ni = 7, nblk = 0, nlong = 0;
  bool row_gather = false;
  std::vector<int64_t> blkptr;
  std::vector<int32_t> blkrow, blkpart, lrow, lfirst;
};

// Dictionary of the distinct (column - row, value) pairs, at most 256 of them, and one byte per non-zero into it.
template <class D> struct DviDict {
  bool ok = true;  // at most 256 entries
  std::vector<uint8_t> codes;
  std::vector<int32_t> delta;
  std::vector<D> val;
  int64_t max_row = 0;
  std::vector<uint8_t> local_used = std::vector<uint8_t>(256, 0);  // entry used by at least one LOCAL column (ghost-only entries: the split product)
};

template <class D> DviDict<D> build_dvi_dict(const CsrHost<D>& A) {
  struct Key {
    uint64_t a, b;
    int64_t d;
    bool operator==(const Key& o) const { return a == o.a && b == o.b && d == o.d; }
  };
  struct KeyHash {
    size_t operator()(const Key& k) const {
      return std::hash<uint64_t>()((k.a * 0x9E3779B97F4A7C15ull ^ k.b) + (uint64_t)k.d * 0xC2B2AE3D27D4EB4Full);
    }
  };
  DviDict<D> t;
  std::unordered_map<Key, int, KeyHash> index;
  t.codes.resize((size_t)A.nnz);
  Key ckey[8];
  int cid[8], ncache = 0, cnext = 0;
  for (int64_t r = 0; r < A.nrows && t.ok; ++r) {
    t.max_row = std::max(t.max_row, A.rp[r + 1] - A.rp[r]);
    for (int64_t p = A.rp[r]; p < A.rp[r + 1]; ++p) {
      Key k{0, 0, (int64_t)A.ci[p] - r};
      std::memcpy(&k, &A.vv[p], sizeof(D));
      // stencils cycle through a handful of keys: a tiny recent-key cache in front of the hash map
      // (n = 1e8 rows / 7e8 non-zeros convert in seconds instead of half a minute)
      bool hit = false;
      for (int q = 0; q < ncache; ++q)
        if (ckey[q] == k) { t.codes[p] = (uint8_t)cid[q]; hit = true; break; }
      if (hit) { if (A.ci[p] < A.nrows) t.local_used[t.codes[p]] = 1; continue; }
      auto it = index.find(k);
      int id;
      if (it == index.end()) {
        if (t.delta.size() == 256) { t.ok = false; break; }
        id = (int)t.delta.size();
        index.emplace(k, id);
        t.delta.push_back((int32_t)k.d);
        t.val.push_back(A.vv[p]);
      } else {
        id = it->second;
      }
      t.codes[p] = (uint8_t)id;
      if (A.ci[p] < A.nrows) t.local_used[id] = 1;
      ckey[cnext] = k;
      cid[cnext] = id;
      cnext = (cnext + 1) & 7;
      if (ncache < 8) ++ncache;
    }
  }
  return t;
}

// Stencil-mask layout (k_spmv_stencil): <= 32 dictionary entries and every row a sub-sequence of ONE ordering of them (a
// topological order of "entry a precedes entry b in some row"): one bit per slot and row.  false: no such order.
template <class D> bool plan_stencil(const CsrHost<D>& A, const DviDict<D>& t, CsrPlan<D>& P) {
  const int ns = (int)t.delta.size();
  std::vector<uint32_t> succ((size_t)ns, 0u);  // succ[a] bit b: a directly precedes b in some row
  for (int64_t r = 0; r < A.nrows; ++r)
    for (int64_t p = A.rp[r] + 1; p < A.rp[r + 1]; ++p) succ[t.codes[p - 1]] |= 1u << t.codes[p];
  // Kahn's algorithm on <= 32 nodes; ties broken by dictionary id (first appearance) -> deterministic
  std::vector<int> indeg((size_t)ns, 0), order;
  for (int a = 0; a < ns; ++a)
    for (int b = 0; b < ns; ++b)
      if (succ[a] >> b & 1u) indeg[b]++;
  std::vector<char> done((size_t)ns, 0);
  for (int it = 0; it < ns; ++it) {
    int pick = -1;
    for (int a = 0; a < ns; ++a)
      if (!done[a] && indeg[a] == 0) { pick = a; break; }
    if (pick < 0) return false;  // a cycle: no common order
    done[pick] = 1;
    order.push_back(pick);
    for (int b = 0; b < ns; ++b)
      if (succ[pick] >> b & 1u) indeg[b]--;
  }
  std::vector<int> slot((size_t)ns, 0);
  for (int k = 0; k < ns; ++k) slot[order[k]] = k;
  const int mbytes = ns <= 8 ? 1 : 4;
  std::vector<uint8_t> m8;
  std::vector<uint32_t> m32;
  if (mbytes == 1) m8.assign((size_t)A.nrows, 0); else m32.assign((size_t)A.nrows, 0u);
  for (int64_t r = 0; r < A.nrows; ++r) {
    uint32_t m = 0;
    int last = -1;
    for (int64_t p = A.rp[r]; p < A.rp[r + 1]; ++p) {
      const int k = slot[t.codes[p]];
      if (k <= last) return false;  // (a repeated entry in one row: not a sub-sequence)
      last = k;
      m |= 1u << k;
    }
    if (mbytes == 1) m8[r] = (uint8_t)m; else m32[r] = m;
  }
  P.nstencil = ns;
  // (trailing slots that only ever name ghost columns -- one stride per neighbour of a slab: rows using them are boundary rows)
  P.nstencil_local = ns;
  for (int k = ns - 1; k >= 0 && !t.local_used[order[k]]; --k) P.nstencil_local = k;
  P.stencil_mask_bytes = mbytes;
  for (int k = 0; k < ns; ++k) {
    P.sdelta.push_back(t.delta[order[k]]);
    P.sval.push_back(t.val[order[k]]);
  }
  P.mask8 = std::move(m8);
  P.mask32 = std::move(m32);
  P.layout = KS_LAYOUT_STENCIL;
  P.bytes_per_nnz = (double)mbytes * (double)A.nrows / (double)A.nnz;
  P.aux_bytes = 0.0;
  return true;
}

// Delta-value-indexed layout (k_spmv_dvi): one byte per non-zero.
template <class D> void plan_dvi(const CsrHost<D>& A, DviDict<D>&& t, const FormatRequest& req, CsrPlan<D>& P) {
  P.ndvi = (int)t.delta.size();
  P.dvi_unroll = t.max_row <= 4 ? 4 : 8;
  // rows per thread (KS_DVI_RPT = 1, 2 or 4).  Measured on the 216^3 Laplacian: 77.8 / 78.7 / 117 us for
  // 1 / 2 / 4 -- the kernel is bound by instruction issue (byte decode, two dictionary reads and one gather per
  // entry), not by memory latency, so more rows per thread only cost occupancy.
  P.dvi_rpt = req.dvi_rpt;
  P.codes = std::move(t.codes);
  P.ddelta = std::move(t.delta);
  P.dval = std::move(t.val);
  P.layout = KS_LAYOUT_DVI;
  P.bytes_per_nnz = 1.0;
  P.aux_bytes = (P.ptr64 ? 8.0 : 4.0) * (double)(A.nrows + 1);
}

// Value-indexed layout (k_spmv_csr<.., VI>): at most 256 distinct stored values (compared bit for bit, so
// -0.0 and NaN payloads survive) and every column index below 2^24.  Fills P.dict / P.packed, or leaves them empty.
template <class D> void build_vi_dict(const CsrHost<D>& A, CsrPlan<D>& P) {
  struct Key {
    uint64_t a, b;
    bool operator==(const Key& o) const { return a == o.a && b == o.b; }
  };
  struct KeyHash {
    size_t operator()(const Key& k) const { return std::hash<uint64_t>()(k.a * 0x9E3779B97F4A7C15ull ^ k.b); }
  };
  std::unordered_map<Key, int, KeyHash> index;
  Key last_key{0, 0};
  int last_id = 0;
  bool ok = true;
  std::vector<D> dict;
  std::vector<int32_t> packed((size_t)A.nnz);
  for (int64_t p = 0; p < A.nnz && ok; ++p) {
    Key k{0, 0};
    std::memcpy(&k, &A.vv[p], sizeof(D));
    int id;
    if (p > 0 && k == last_key) {  // runs of equal values are the common case
      id = last_id;
    } else {
      auto it = index.find(k);
      if (it == index.end()) {
        if (dict.size() == 256) { ok = false; break; }
        id = (int)dict.size();
        index.emplace(k, id);
        dict.push_back(A.vv[p]);
      } else {
        id = it->second;
      }
      last_key = k;
      last_id = id;
    }
    if (A.ci[p] >= (1 << 24)) { ok = false; break; }
    packed[p] = (int32_t)(((uint32_t)id << 24) | (uint32_t)A.ci[p]);
  }
  if (!ok) return;
  P.dict = std::move(dict);
  P.packed = std::move(packed);
  P.ndict = (int)P.dict.size();
}

// Sliced ELLPACK (k_spmv_sell, lane = row: coalesced index / value loads and, for banded matrices, coalesced gathers) when slicing
// the rows 64 at a time pads the matrix by at most 15 % -- uniform row lengths: stencils with variable coefficients, structured
// finite-element meshes, banded matrices; otherwise (ragged rows, where a lane per row would idle and the gathers are scattered
// anyway) false: the non-zero-parallel CSR blocks of k_spmv_csr.  KS_SPMV_FORMAT=sell / sellvi force it.
template <class D> bool plan_sell(const CsrHost<D>& A, const FormatRequest& req, CsrPlan<D>& P) {
  const std::vector<int64_t>& rp = A.rp;
  const int64_t nrows = A.nrows;
  const int sigma = req.sell_sigma;
  // slice position -> row (identity unless sigma > 1: stable sort by descending length inside each window)
  std::vector<int32_t> perm;
  if (sigma > 1) {
    perm.resize((size_t)nrows);
    for (int64_t i = 0; i < nrows; ++i) perm[i] = (int32_t)i;
    for (int64_t w0 = 0; w0 < nrows; w0 += sigma) {
      const int64_t w1 = std::min<int64_t>(nrows, w0 + sigma);
      std::stable_sort(perm.begin() + w0, perm.begin() + w1,
                       [&](int32_t x_, int32_t y_) { return rp[x_ + 1] - rp[x_] > rp[y_ + 1] - rp[y_]; });
    }
  }
  auto row_at = [&](int64_t pos) { return sigma > 1 ? (int64_t)perm[pos] : pos; };
  const int64_t nsl = (nrows + 63) / 64;
  std::vector<int64_t> sp((size_t)nsl + 1, 0);
  int64_t wmax = 0;
  for (int64_t sl = 0; sl < nsl; ++sl) {
    int64_t w = 0;
    for (int64_t pos = sl * 64; pos < std::min<int64_t>(nrows, sl * 64 + 64); ++pos) {
      const int64_t r = row_at(pos);
      w = std::max(w, rp[r + 1] - rp[r]);
    }
    wmax = std::max(wmax, w);
    sp[sl + 1] = sp[sl] + 64 * w;
  }
  const int64_t padded = sp[nsl];
  if (!(req.force_sell() || (double)padded <= 1.15 * (double)A.nnz + 64.0)) return false;
  KS_REQUIRE(padded < ((int64_t)1 << 40), KS_ERR_ARGUMENT, "sliced-ELLPACK padding explodes: use KS_SPMV_FORMAT=csr");
  if (padded >= (int64_t)2147483647) P.ptr64 = true;
  const bool vi = P.ndict > 0;
  P.sell_col.assign((size_t)padded, -1);
  P.sell_val.resize(vi ? 0 : (size_t)padded);
  for (int64_t sl = 0; sl < nsl; ++sl)
    for (int64_t pos = sl * 64; pos < std::min<int64_t>(nrows, sl * 64 + 64); ++pos) {
      const int64_t r = row_at(pos);
      const int64_t lane = pos - sl * 64;
      for (int64_t p = rp[r], k = 0; p < rp[r + 1]; ++p, ++k) {
        const int64_t q = sp[sl] + k * 64 + lane;
        P.sell_col[q] = vi ? P.packed[p] : A.ci[p];
        if (!vi) P.sell_val[q] = A.vv[p];
      }
    }
  P.nslices = (int)nsl;
  P.sell_un = wmax <= 4 ? 4 : 8;
  P.sell_entries = padded;
  P.sliceptr = std::move(sp);
  P.sell_perm = std::move(perm);
  P.layout = vi ? KS_LAYOUT_SELL_VI : KS_LAYOUT_SELL;
  P.bytes_per_nnz = (vi ? 4.0 : 4.0 + sizeof(D)) * (double)padded / (double)A.nnz;
  P.aux_bytes = (P.ptr64 ? 8.0 : 4.0) * (double)(nsl + 1) + (sigma > 1 ? 4.0 * (double)nrows : 0.0);
  return true;
}

// Row blocks of k_spmv_csr.  A block holds at most ni * 256 products in LDS (<= 32 KiB; KS_SPMV_NI overrides), so
// regular matrices get full 256-row blocks and the LDS footprint (occupancy) follows the matrix.  Greedy pass over the
// rows: close the block at 256 rows or when the next row would overflow it; a row longer than the capacity becomes a
// block of its own (handled by all 256 threads).
template <class D> void plan_row_blocks(const CsrHost<D>& A, const FormatRequest& req, CsrPlan<D>& P) {
  const std::vector<int64_t>& rp = A.rp;
  const int64_t nrows = A.nrows;
  constexpr int kBlock = ksd::kBlock;
  const int nimax = (int)(ksd::kSpmvCapBytes / (kBlock * sizeof(D)));  // 16 (Float64) / 8 (ComplexF64)
  // depth from the 90th percentile of the non-zeros of fixed 256-row tiles: a regular matrix gets exactly what its
  // tiles need (7-point stencil: 1792 -> 7; 12 measured 14 % slower than 7 or 8 there: LDS footprint), the heavy tail
  // of a skewed one gets shorter blocks instead of inflating everybody's LDS
  std::vector<int64_t> tile_nnz;
  for (int64_t r0 = 0; r0 < nrows; r0 += ksd::kSpmvRows) tile_nnz.push_back(rp[std::min<int64_t>(nrows, r0 + ksd::kSpmvRows)] - rp[r0]);
  int64_t t90 = 0;
  if (!tile_nnz.empty()) {
    const size_t k = (tile_nnz.size() - 1) * 9 / 10;
    std::nth_element(tile_nnz.begin(), tile_nnz.begin() + k, tile_nnz.end());
    t90 = tile_nnz[k];
  }
  const int need = (int)((t90 + kBlock - 1) / kBlock);
  int ni = need <= 4 ? 4 : need <= 7 ? 7 : need <= 8 ? 8 : need <= 12 ? 12 : 16;
  if (req.ni != INT_MIN) ni = req.ni;
  if (ni != 4 && ni != 7 && ni != 8 && ni != 12 && ni != 16) ni = 16;
  ni = std::min(ni, nimax);
  P.ni = ni;
  {
    // ROW-GATHER or NON-ZERO-PARALLEL gathers (k_spmv_csr): with lane = row the gathers of one instruction are coalesced
    // when neighbouring rows reference neighbouring columns (banded / stencil / FEM matrices: 212 -> 204 us on the 216^3
    // Laplacian, 0.62 -> 0.64 of the HBM spec), and a chain of dependent LDS reads and scattered loads when they do not
    // (hashed columns: 46.5 -> 49.5 us, heavy-tailed rows 109 -> 125 us).  Decided once from the matrix: the share of
    // consecutive row pairs whose first stored columns are at most 16 apart.  KS_SPMV_CSR_ROWGATHER=0/1 forces.
    int64_t pairs = 0, close = 0;
    const int64_t stride = std::max<int64_t>(1, nrows / 65536);
    for (int64_t r = 0; r + 1 < nrows; r += stride) {
      if (rp[r + 1] == rp[r] || rp[r + 2] == rp[r + 1]) continue;
      ++pairs;
      const int64_t d = (int64_t)A.ci[rp[r + 1]] - (int64_t)A.ci[rp[r]];
      if (d >= -16 && d <= 16) ++close;
    }
    P.row_gather = req.row_gather >= 0 ? req.row_gather != 0 : (pairs > 0 && 2 * close >= pairs);
  }
  const int64_t cap = (int64_t)ni * kBlock;
  std::vector<int64_t>& bp = P.blkptr;
  std::vector<int32_t>&br = P.blkrow, &part = P.blkpart, &lrow = P.lrow, &lfirst = P.lfirst;
  bp = {0};
  br = {0};
  lfirst = {0};
  int64_t r = 0;
  while (r < nrows) {
    const int64_t first = rp[r + 1] - rp[r];
    if (first > cap) {  // long row: chunk blocks of <= cap entries, all with row range [r, r+1)
      for (int64_t q = rp[r]; q < rp[r + 1]; q += cap) {
        part.push_back((int32_t)lfirst.back() + (int32_t)((q - rp[r]) / cap));
        br.push_back((int32_t)(r + 1));
        bp.push_back(std::min(q + cap, rp[r + 1]));
        if (q + cap < rp[r + 1]) br.back() = (int32_t)r;  // the next chunk starts at the same row
      }
      lrow.push_back((int32_t)r);
      lfirst.push_back(lfirst.back() + (int32_t)((first + cap - 1) / cap));
      P.nlong++;
      r += 1;
      continue;
    }
    int64_t e = r + 1;
    while (e < nrows && e - r < ksd::kSpmvRows && rp[e + 1] - rp[r] <= cap && rp[e + 1] - rp[e] <= cap) ++e;
    part.push_back(-1);
    br.push_back((int32_t)e);
    bp.push_back(rp[e]);
    r = e;
  }
  KS_REQUIRE((int64_t)br.size() - 1 < (int64_t)2147483647, KS_ERR_ARGUMENT, "too many row blocks");
  P.nblk = (int)br.size() - 1;
  P.layout = P.ndict > 0 ? KS_LAYOUT_CSR_VI : KS_LAYOUT_CSR;
  P.bytes_per_nnz = P.ndict > 0 ? 4.0 : 4.0 + sizeof(D);
  P.aux_bytes = (P.ptr64 ? 8.0 : 4.0) * (double)(nrows + 1 + 2 * ((int64_t)P.nblk + 1));
}

template <class D> CsrPlan<D> plan_csr(const CsrHost<D>& A, const FormatRequest& req, CbMode mode, int64_t nghost, int64_t nlow, int num_cu);

// The referenced columns in GLOBAL order are [ghosts of lower ranks | local columns | ghosts of higher ranks] (one GPU: the local
// columns alone); key(c) is the position of local-extended column c in that order.
struct CbKeys {
  int64_t nrows, nlow, next;  // next = nrows + nghost
  int64_t key(int64_t c) const { return c < nrows ? nlow + c : (c - nrows < nlow ? c - nrows : c); }
  int64_t seg_lo(int g) const { return g == 0 ? 0 : g == 1 ? nlow : nlow + nrows; }
  int64_t seg_hi(int g) const { return g == 0 ? nlow : g == 1 ? nlow + nrows : next; }
};

// How many column blocks (0: none).  Auto: plain CSR row blocks would be used, single GPU, x between 6 and 160 MiB, rows sorted by
// column and short, and at least half of the entries further than n/16 from the diagonal -> blocks of ~4 MiB of x, at most 8.
template <class D> int cb_count(const CsrHost<D>& A, const FormatRequest& req, const CbKeys& K) {
  if (req.colblocks == 0) return 0;
  bool sorted = true;
  int64_t far = 0, maxrow = 0;
  const int64_t fardist = std::max<int64_t>(1, K.next / 16);
  for (int64_t r = 0; r < A.nrows && sorted; ++r) {
    maxrow = std::max(maxrow, A.rp[r + 1] - A.rp[r]);
    for (int64_t q = A.rp[r]; q < A.rp[r + 1]; ++q) {
      if (q > A.rp[r] && K.key(A.ci[q]) < K.key(A.ci[q - 1])) { sorted = false; break; }
      far += std::llabs(K.key(A.ci[q]) - (K.nlow + r)) > fardist;
    }
  }
  const double xmb = (double)K.next * sizeof(D) / (1 << 20);
  if (!(sorted && maxrow <= 4 * ksd::kBlock)) return 0;
  if (req.colblocks >= 2) return req.colblocks;
  // block width ~ 4 MiB of x (measured optimum at n = 1e6: 2 blocks, 2e6: 4 blocks); beyond 8 blocks the y that is
  // written and read back between the launches (16 n bytes each) eats the gain (n = 1e7: 8 blocks -11 %, 16: +35 %)
  if (xmb >= 6.0 && xmb <= 160.0 && 2 * far >= A.nnz) return std::min(8, std::max(2, (int)std::lround(xmb / 4.0)));
  return 0;
}

// Block boundaries in key space: nbk blocks shared out over the non-empty segments in proportion to their width (one segment -- a
// single GPU --: b n / nbk), none straddling a segment.  bseg[b]: the segment of block b.
inline std::vector<int64_t> cb_bounds(int nbk, const CbKeys& K, std::vector<int>& bseg) {
  std::vector<int64_t> bounds{0};
  int nseg = 0;
  for (int g = 0; g < 3; ++g) nseg += K.seg_hi(g) > K.seg_lo(g);
  nbk = std::max(nbk, nseg);
  int cnt[3] = {0, 0, 0}, used = 0;
  auto width = [&](int g) { return K.seg_hi(g) - K.seg_lo(g); };
  for (int g = 0; g < 3; ++g)
    if (width(g) > 0) { cnt[g] = std::max(1, (int)((double)nbk * (double)width(g) / (double)K.next)); used += cnt[g]; }
  while (used > std::min(nbk, ksd::kCbMaxBlocks)) {  // (rounding up the narrow segments): take from the segment with the most blocks
    int g = 0;
    for (int h = 1; h < 3; ++h) if (cnt[h] > cnt[g]) g = h;
    if (cnt[g] <= 1) break;
    --cnt[g]; --used;
  }
  while (used < nbk) {  // give the rest to the segment with the widest blocks
    int g = -1;
    for (int h = 0; h < 3; ++h)
      if (cnt[h] > 0 && (g < 0 || (double)width(h) / cnt[h] > (double)width(g) / cnt[g])) g = h;
    ++cnt[g]; ++used;
  }
  KS_REQUIRE(used <= ksd::kCbMaxBlocks, KS_ERR_INTERNAL, "column blocks: more segments than blocks");
  for (int g = 0; g < 3; ++g)
    for (int b = 0; b < cnt[g]; ++b) {
      bounds.push_back(b + 1 == cnt[g] ? K.seg_hi(g) : K.seg_lo(g) + (int64_t)(b + 1) * width(g) / cnt[g]);
      bseg.push_back(g);
    }
  return bounds;
}

// COLUMN BLOCKS (KS_LAYOUT_CSR_CB).  A matrix with scattered columns whose x is larger than one XCD's L2 (4 MiB) runs at
// the device's random-gather rate (config 3: 59 us at n = 1e6, 5.1x its algorithmic traffic through the fabric).  Split
// into column blocks -- block b holds the entries with column in [b n/NB, (b+1) n/NB) -- each launch gathers from an
// x block that stays L2 resident, and because the entries of a row are sorted by column the row sums are simply
// continued from launch to launch (k_spmv_csr's yacc): same additions in the same order, bit-identical y.  Measured
// (tools/colblock_probe.py, n = 1e6): 59.5 us whole, 2 blocks 23 + 23 us, 4 blocks 4 x 13 us (launch floor), 8: 8 x 9.
// Distributed operators (CbMode::DistributedRowBlock): blocks are ranges of keys that do not straddle a segment, so every block
// gathers either from x or from the ghost vector, and a row stored in global column order (what a row block of a sorted CSR
// matrix is) is summed in the same order as on one GPU.  false: no column blocks (the row blocks of plain CSR follow).
template <class D>
bool plan_column_blocks(const CsrHost<D>& A, const FormatRequest& req, CbMode mode, int64_t nghost, int64_t nlow, int num_cu, CsrPlan<D>& P) {
  constexpr int kBlock = ksd::kBlock;
  const int64_t nrows = A.nrows;
  const CbKeys K{nrows, nlow, nrows + nghost};
  int nbk = cb_count(A, req, K);
  if (nbk < 2) return false;
  std::vector<int> bseg;
  std::vector<int64_t> bounds = cb_bounds(std::min(nbk, ksd::kCbMaxBlocks), K, bseg);
  nbk = (int)bseg.size();
  // single-launch form (k_spmv_csr_cb): largest segment (entries of a tile of 256 * RPT rows inside one column block)
  // for every candidate RPT
  constexpr int kRptCand[5] = {1, 2, 4, 8, 16};
  int64_t maxseg[5] = {0, 0, 0, 0, 0};
  bool small_ptrs = true;
  std::vector<CsrPlan<D>> blocks;
  std::vector<char> from_ghost_of;
  for (int b = 0; b < nbk; ++b) {
    const int64_t lo = bounds[b], hi = (b + 1 == nbk) ? (int64_t)1 << 40 : bounds[b + 1];
    const bool from_ghost = bseg[b] != 1;
    std::vector<int64_t> rpb((size_t)nrows + 1, 0);
    std::vector<int32_t> cib;
    std::vector<D> vvb;
    for (int64_t r = 0; r < nrows; ++r) {
      for (int64_t q = A.rp[r]; q < A.rp[r + 1]; ++q) {
        const int64_t kq = K.key(A.ci[q]);
        if (kq >= lo && kq < hi) { cib.push_back(from_ghost ? (int32_t)(A.ci[q] - nrows) : A.ci[q]); vvb.push_back(A.vv[q]); }
      }
      rpb[r + 1] = (int64_t)cib.size();
    }
    for (int k = 0; k < 5; ++k) {
      const int64_t tr = (int64_t)kBlock * kRptCand[k];
      for (int64_t r0 = 0; r0 < nrows; r0 += tr) maxseg[k] = std::max(maxseg[k], rpb[std::min(nrows, r0 + tr)] - rpb[r0]);
    }
    blocks.push_back(plan_csr<D>(CsrHost<D>{nrows, (int64_t)cib.size(), rpb, cib, vvb}, req.for_column_block(), CbMode::IsColumnBlock, 0, 0, num_cu));
    blocks.back().sub_rp = std::move(rpb);
    blocks.back().sub_ci = std::move(cib);
    blocks.back().sub_vv = std::move(vvb);
    from_ghost_of.push_back(from_ghost ? 1 : 0);
    small_ptrs = small_ptrs && !blocks.back().ptr64;
  }
  // Measured (tools/cb_single_ab.py, profiles/r03_column_blocks.txt): the single launch wins where the y round trips of
  // many blocks hurt (n = 1e7, 8 blocks: 858 -> 823 us) and loses a little where two to four launches were already close
  // to what bounds this product -- the rate at which an XCD's L2 hands out randomly addressed lines, 5e6 of them for
  // 1e6 rows: 46 us either way at n = 1e6, 100 vs 107 us at 2e6.  So: single launch from 5 blocks on
  // (KS_SPMV_CB_SINGLE=0 never, KS_SPMV_CB_RPT=k forces it with k sub-tiles per workgroup).  A distributed operator
  // always takes the single launch (the per-block launches have one x; the kernel takes a base per block).
  int cb_rpt = 0, cb_ni = 0;
  if (small_ptrs && (mode == CbMode::DistributedRowBlock || (req.cb_single && (nbk > 4 || req.cb_rpt > 0)))) {
    // all tiles resident at once (one round of workgroups keeps them in step on the same column block): the smallest RPT
    // whose tile count fits, among those whose segments fit the LDS depth (8 x 256 products, 16 x 256 for Float64)
    const int nimax = (int)(ksd::kSpmvCapBytes / (kBlock * sizeof(D)));  // 16 (Float64) / 8 (ComplexF64)
    int best = -1;
    for (int k = 0; k < 5; ++k) {
      const int ni = maxseg[k] <= 8 * kBlock ? 8 : (maxseg[k] <= 16 * kBlock && nimax >= 16 ? 16 : 0);
      if (!ni) break;  // (segments only grow with RPT)
      best = k;
      const int64_t ntiles = (nrows + (int64_t)kBlock * kRptCand[k] - 1) / ((int64_t)kBlock * kRptCand[k]);
      if (req.cb_rpt ? kRptCand[k] >= req.cb_rpt : ntiles <= (int64_t)num_cu * (ni == 8 ? 8 : 4)) break;
    }
    if (best >= 0) {
      cb_rpt = kRptCand[best];
      cb_ni = maxseg[best] <= 8 * kBlock ? 8 : 16;
    }
  }
  if (mode == CbMode::DistributedRowBlock && !cb_rpt) return false;  // (no single-launch shape fits)
  P.cblocks = std::move(blocks);
  P.cb_from_ghost = std::move(from_ghost_of);
  P.cb_bounds = std::move(bounds);
  P.cb_rpt = cb_rpt;
  P.cb_ni = cb_ni;
  P.layout = KS_LAYOUT_CSR_CB;
  P.bytes_per_nnz = 4.0 + sizeof(D);
  P.aux_bytes = 0.0;
  for (const auto& cbk : P.cblocks) P.aux_bytes += cbk.aux_bytes;
  if (!cb_rpt) P.aux_bytes += (double)(nbk - 1) * 2.0 * sizeof(D) * (double)nrows;  // y written and read back between the blocks
  return true;
}

// The cascade: the most compact layout that applies, unless KS_SPMV_FORMAT pins one.  num_cu: compute units of the device (the
// rows-per-workgroup choice of the single-launch column blocks).
template <class D> CsrPlan<D> plan_csr(const CsrHost<D>& A, const FormatRequest& req, CbMode mode, int64_t nghost, int64_t nlow, int num_cu) {
  CsrPlan<D> P;
  // int64-nnz CSR: offsets need 64 bits from 2^31 stored entries on
  P.ptr64 = A.nnz >= (int64_t)2147483647 || req.ptr64;
  if (A.nnz > 0 && req.try_dvi()) {
    DviDict<D> t = build_dvi_dict(A);
    if (t.ok && t.delta.size() <= (size_t)ksd::kStencilSlots && req.try_stencil()) {
      if (plan_stencil(A, t, P)) return P;
      KS_REQUIRE(!req.insist_stencil(), KS_ERR_ARGUMENT, "KS_SPMV_FORMAT=stencil: the rows are not sub-sequences of one entry order");
    }
    if (t.ok) { plan_dvi(A, std::move(t), req, P); return P; }
  }
  if (A.nnz > 0 && req.try_vi()) build_vi_dict(A, P);
  if (!req.sell_keeps_dict()) { P.dict.clear(); P.packed.clear(); P.ndict = 0; }
  if (req.allow_sell() && A.nrows > 0 && A.nnz > 0 && plan_sell(A, req, P)) return P;
  if ((mode == CbMode::Allowed || mode == CbMode::DistributedRowBlock) && P.ndict == 0 && A.nnz > 0 &&
      plan_column_blocks(A, req, mode, nghost, nlow, num_cu, P))
    return P;
  plan_row_blocks(A, req, P);
  return P;
}

}  // namespace
