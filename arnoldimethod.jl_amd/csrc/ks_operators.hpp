// operators: anything with mul!(y, A, x) (src/run.jl:21-22) -- stored sparse matrices in their device layouts, dense matrices, host / device callbacks
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip, in this order --
//     ks_context.hpp -> ks_operators.hpp -> ks_workspace.hpp -> ks_backend.hpp -> (C ABI in ks_hip.hip)
// -- and not meant to be included on its own (needs ks_context.hpp, ks_csr_layout.hpp and ks_halo.hpp).
#pragma once
// ------------------------------------------------------------------------------------------------
// operators
// ------------------------------------------------------------------------------------------------
struct ks_operator {
  ks_ctx* ctx = nullptr;
  int64_t n_local = 0, nnz = 0;
  int dtype = KS_F64;
  bool async_capable = true;  // may be enqueued ahead without host involvement
  double bytes_per_nnz = 0.0;  // what the SpMV streams per stored non-zero (0: not a stored-matrix operator)
  double aux_bytes = 0.0;      // index structures next to the non-zeros (row pointers, slice offsets, permutation)
  int layout = -1;             // KS_LAYOUT_* of include/kschur.h (-1: not a stored sparse matrix)
  // Inside an expansion the newest basis column is stored unnormalised (x = beta * v up to a correction in span(V)); the
  // library's own operators are linear and do not care, a HOST callback is handed the vector scaled to unit norm and its
  // result is scaled back (a user's inner solver may use absolute tolerances).  Set by the expansion before apply().
  double in_scale = 1.0;
  // Newton products of a LONG block (s-step expansion, ks_block.hpp): the product is stored cacheably instead of streaming --
  // the next product of the chain gathers exactly this vector (49 instead of 59 us at n = 1e7), and the dirty lines cost the
  // ONE inner-product pass that follows a block of 20 less (+45 us) than the twenty products gain (headline 4 332 -> 4 501
  // iterations/s; blocks of 10 with the ring form of pass 1: 3 836 -> 3 923).  With the register form of pass 1 and blocks of
  // 5-8 it was the other way round (products 61 -> 51 us, pass 1 415 -> 510 us), so shorter blocks keep streaming stores.
  // KS_SHIFT_PLAIN = 0 / 1 forces.
  bool shift_store_cacheable = false;
  virtual ~ks_operator() = default;
  // y = A x on device pointers, enqueued on ctx->stream; `st` lets the kernels of a batch skip work
  // after a breakdown.
  virtual void apply(const void* x, void* y, const DevState* st) = 0;
  // y = sigma (A x - theta x): one step of the Newton basis of the s-step expansion (ks_block.hpp).  Default: the product
  // followed by a streaming pass (24 n bytes); layouts with a fused form override it.  theta = (re, im).
  virtual void apply_shifted(const void* x, void* y, double theta_re, double theta_im, double sigma, int64_t ld, const DevState* st);
  // y = sigma (A x - theta x) - w + gamma x0, evaluated as ((t - w) + gamma x0) with t the Newton step: one Clenshaw step of a
  // Chebyshev series (ks_cheb.hpp).  y is distinct from x, w and x0; a null w / x0 drops that term.  Default: the product followed
  // by ONE streaming pass (k_clenshaw_tail: 40 n bytes in Float64); the grid operators do it in the product's own store.
  // shift_store_cacheable picks the store, as for apply_shifted.  Every step an operator runs is counted by the path it took.
  virtual void apply_clenshaw(const void* x, void* y, double theta_re, double theta_im, double sigma, const void* w, double gamma,
                              const void* x0, int64_t ld, const DevState* st);
  int64_t clenshaw_fused = 0, clenshaw_generic = 0;   // steps since creation: in the product's launch / product + streaming pass
};

namespace {

template <class D> struct CsrOp : ks_operator {
  void* rowptr = nullptr;   // int32[n+1], or int64[n+1] when ptr64 (nnz >= 2^31: int64-nnz CSR)
  bool ptr64 = false;
  int32_t* colidx = nullptr;
  D* val = nullptr;
  // row blocks of k_spmv_csr (CSR-adaptive tiling): rows [blkrow[b], blkrow[b+1]), non-zeros [blkptr[b], blkptr[b+1])
  void* blkptr = nullptr;   // same integer type as rowptr
  int32_t* blkrow = nullptr;
  int nblk = 0;
  // column-blocked layout: the matrix split into column blocks, each a CSR-row-block sub-operator of its own; apply() runs
  // them in order, each continuing the row sums of the previous one (k_spmv_csr's yacc)
  std::vector<std::unique_ptr<CsrOp<D>>> cblocks;
  std::vector<char> cb_from_ghost;  // per column block: gathers from the ghost vector (row block of a distributed operator)
  int cb_rpt = 0, cb_ni = 0;  // single-launch form of the column-blocked layout (k_spmv_csr_cb): 256-row sub-tiles per workgroup, LDS depth; 0: one launch per block
  int ni = 7;               // non-zeros per thread and block: a block holds at most ni * 256 entries in LDS
  bool row_gather = false;  // k_spmv_csr: one thread per row gathers x itself (banded matrices) instead of the non-zero-parallel gathers
  int nlong = 0;            // rows longer than that: cut into chunk blocks, partial sums added by k_spmv_longfix
  int32_t* blkpart = nullptr;  // per block: -1, or the index of the chunk's partial sum
  D* lpart = nullptr;
  int32_t* lrow = nullptr;
  int32_t* lfirst = nullptr;
  // stencil-mask layout (k_spmv_stencil): one bit per dictionary slot and row, the dictionary in the kernel arguments
  int nstencil = 0;          // slots (0: layout not in use)
  int stencil_mask_bytes = 1;
  void* smask = nullptr;
  void* smask2 = nullptr;    // == smask (the array is padded to an even number of rows): masks of rows 2t, 2t+1 in one word
  ksd::StencilDict<D> sdict{};
  int nstencil_local = 0;            // leading slots of the stencil dictionary; the rest name ghost columns only
  StencilGeom geom;                  // Float64, no ghosts: are the masks the box rule of a grid (ks_stencil_geom.hpp)
  mutable bool split_said = false;   // (KS_DIST_SPLIT_DEBUG: one line per operator)
  // sliced-ELLPACK layout (k_spmv_sell): slices of 64 rows, column-major, padded to the slice's longest row
  void* sliceptr = nullptr;  // entry offsets of the slices, same integer type as rowptr
  int32_t* sperm = nullptr;  // slice position -> row (sigma > 1 only)
  int nslices = 0;
  int sell_un = 8;
  int64_t sell_entries = 0;  // stored entries including padding
  int ndict = 0;      // > 0: value-indexed layout (k_spmv_csr<.., VI>): colidx = (dict index << 24) | column, val = dictionary
  // delta-value-indexed layout (k_spmv_dvi): one byte per non-zero into a dictionary of (column - row, value)
  int ndvi = 0;
  uint8_t* codes = nullptr;
  int32_t* ddelta = nullptr;
  int dvi_unroll = 8;
  int dvi_rpt = 1;          // rows per thread of k_spmv_dvi
  // ghost vector and exchange of a distributed row block (ks_halo.hpp; one GPU: empty)
  Halo<D> halo;

  ~CsrOp() override {
    (void)hipFree(rowptr); (void)hipFree(colidx); (void)hipFree(val); (void)hipFree(blkptr); (void)hipFree(blkrow); (void)hipFree(smask); (void)hipFree(sliceptr); (void)hipFree(sperm); (void)hipFree(blkpart); (void)hipFree(lpart); (void)hipFree(lrow); (void)hipFree(lfirst);
    (void)hipFree(codes); (void)hipFree(ddelta);
  }
  // the CSR-row-block kernel of THIS operator's arrays on x -> y, continuing the row sums in `yacc` (column-blocked
  // layout: plain CSR, single GPU, no long rows -- make_csr only builds column blocks under those conditions)
  void launch_csr_blocks(const D* x, D* y, const DevState* st, const D* yacc, int plain_store, ksd::ShiftArg<D> shift = ksd::ShiftArg<D>{}) {
    hipStream_t s = ctx->stream;
    auto go = [&](auto ip_tag) {
      using IP = decltype(ip_tag);
      auto launch = [&](auto ni_tag) {
        constexpr int NI = decltype(ni_tag)::value;
        if constexpr ((size_t)NI * kBlock * sizeof(D) <= (size_t)ksd::kSpmvCapBytes)
          ksd::k_spmv_csr<D, IP, false, NI><<<nblk, kBlock, 0, s>>>(static_cast<const IP*>(blkptr), blkrow, static_cast<const IP*>(rowptr), colidx, val, x,
                                                                    nullptr, y, n_local, nblk, st, nullptr, 0, 0, nullptr, nullptr, yacc, plain_store,
                                                                    ksd::HaloFused{}, ksd::HaloArgs{}, ksd::P2pDev{}, env_int("KS_SPMV_CSR_NT", 1) != 0, row_gather,
                                                                    plain_store ? ksd::ShiftArg<D>{} : shift);
        else
          throw KsError{KS_ERR_INTERNAL, "CSR row blocks of " + std::to_string(NI) + " x 256 entries exceed the LDS budget of this element type"};
      };
      switch (ni) {
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 7: launch(std::integral_constant<int, 7>{}); break;
        case 8: launch(std::integral_constant<int, 8>{}); break;
        case 12: launch(std::integral_constant<int, 12>{}); break;
        default: launch(std::integral_constant<int, 16>{}); break;
      }
    };
    if (ptr64) go(int64_t{});
    else go(int32_t{});
  }
  // fused Newton-basis step (s-step expansion): the paired stencil kernel applies y = sigma (A x - theta x) itself
  bool shift_on = false;
  D shift_theta{};
  double shift_sigma = 1.0;
  bool shift_plain() const {
    static const int env = env_int("KS_SHIFT_PLAIN", -1);
    return env >= 0 ? env != 0 : shift_store_cacheable;
  }
  // ---- marching form of the paired stencil kernel (ks_spmv_march.hpp; Float64, one GPU, at most 8 slots) ----
  static bool march_on() {
    return env_int("KS_STENCIL_MARCH", 1) != 0;   // (read per launch: the tests switch the forms inside one process)
  }
  // Workgroups per XCD (= tiles of 512 rows an XCD takes per round).  With a far stride P (the xy-plane of a 3-D grid) a round
  // that covers a WHOLE NUMBER OF PLANES keeps the z - 1 / z + 1 taps of a round in step with the rows other rounds own.  How much
  // that buys depends on where x comes from (tools/spmv_slab.hip, profiles/r06_spmv_sweep.txt, r06_spmv_columns.txt, 216^3):
  //   x and y ping-pong between two buffers that stay in the 256-MB Infinity Cache:   34.0 us at 92 (one plane), 40 at 184-192
  //     (two planes), 41-45 in between and beyond (k_spmv_stencil2: 43-44);
  //   the solver's chain (column i -> column i + 1 of a basis that does not fit the cache):   48.7 at 192, 50.5 at 92, 49-55 for
  //     k_spmv_stencil2 -- a plain copy of the same columns takes 29-31 there, the same kernel with ONE slot 36.
  // The solver lives in the second regime: two planes per round (5-6 workgroups per CU), a multiple of one plane in general.
  int march_slots(int ntiles) const {
    const int env = env_int("KS_MARCH_S", 0);
    int S = 192;
    if (env > 0) S = env;
    else {
      int64_t P = 0;
      for (int k = 0; k < nstencil; ++k) P = std::max<int64_t>(P, std::llabs((long long)sdict.delta[k]));
      const int64_t per = P / 512 + 1;                         // tiles of one far stride, rounded up
      if (per >= 16 && per <= 224) S = (int)(per * ((160 + per - 1) / per)) <= 224 ? (int)(per * ((160 + per - 1) / per)) : (int)per;
    }
    S = std::min(S, std::max(1, (ntiles + 7) / 8));
    return S;
  }
  void launch_march(const D* x, D* y, int nt, const DevState* st, hipStream_t s) const {
    if constexpr (std::is_same<D, double>::value) {
      const int sh = shift_on ? (1 | (shift_plain() ? 2 : 0)) : 0;
      const uint16_t* m2 = static_cast<const uint16_t*>(smask2);
      const int G = 8 * march_slots(nt);
      int kown = -1;
      for (int k = 0; k < nstencil; ++k)
        if (sdict.delta[k] == 0) kown = k;
      auto go = [&](auto ns_tag, auto ko_tag) {
        ksd::k_spmv_stencil_march<decltype(ns_tag)::value, decltype(ko_tag)::value><<<G, kBlock, 0, s>>>(m2, sdict, x, y, n_local, nt, st, sh, shift_theta, shift_sigma);
      };
      // the 3-D 7-point shape (far, near, near, own, near, near, far with the near taps within 256 rows): the window form -- the five
      // near taps of a tile from one copy of its rows in LDS (ks_spmv_march.hpp; 47 against 49 us in the solver's chain,
      // profiles/r06_spmv_columns.txt).  KS_MARCH_WINDOW=0: the register form for every shape.
      const int window = env_int("KS_MARCH_WINDOW", 1);
      if (window && nstencil == 7 && kown == 3) {
        bool shape = std::llabs((long long)sdict.delta[0]) > 256 && std::llabs((long long)sdict.delta[6]) > 256;
        unsigned odd = 0;
        for (int k = 1; k <= 5; ++k) {
          shape = shape && std::llabs((long long)sdict.delta[k]) <= 256;
          if (sdict.delta[k] & 1) odd |= 1u << k;
        }
        // ... and where the planes are large enough to give every XCD a dozen in-plane tiles, the Z-MARCHING form: a workgroup
        // keeps its tile and walks up the planes, the far taps come from registers / the next plane's window (41-42 us against
        // 46-47 for the window form and 50-56 for k_spmv_stencil2 in the solver's chain, profiles/r06_spmv_columns.txt).
        // KS_MARCH_Z=0 switches it off, KS_MARCH_ZR sets the number of z-ranges.
        const int zmarch = env_int("KS_MARCH_Z", 1), zr_env = env_int("KS_MARCH_ZR", 0);
        const int64_t Pz = sdict.delta[6];
        if (shape && zmarch && sdict.delta[0] == -Pz && (Pz & 1) == 0 && Pz >= 8 * 8 * 512) {
          // ... and where the masks are the box rule of the grid (ks_stencil_geom.hpp), the form that derives them from the row
          // number instead of streaming them and takes the +P tap one step late (k_spmv_stencil_marchg): 33.1-33.8 us against
          // 37.8-38.7 in the solver's chain (profiles/stencil_geom.txt).  Tiles of 1 024 in-plane offsets on 512 threads (of the
          // widths 512 / 1 024 / 2 048 the one that measured fastest; four workgroups per CU by their window buffers); z-ranges so
          // that the resident workgroup slots of an XCD (32 CUs) are filled twice, at least four planes each.
          // KS_MARCH_GEOM=0 selects the form that reads the masks.
          if (geom.box && n_local / Pz >= 8 && env_int("KS_MARCH_GEOM", 1) != 0) {
            constexpr int kTileG = 1024, kThreadsG = 512, kSlotsG = 2 * 32 * 4;
            const int nzp = (int)(n_local / Pz), cmax = (int)(((Pz + kTileG - 1) / kTileG + 7) / 8);
            int nzr = zr_env > 0 ? zr_env : std::max(1, (kSlotsG + cmax / 2) / cmax);
            nzr = std::max(1, std::min(nzr, nzp / 4));
            auto gg = [&](auto odd_tag) {
              ksd::k_spmv_stencil_marchg<decltype(odd_tag)::value, kTileG, kThreadsG><<<8 * cmax * nzr, kThreadsG, 0, s>>>(m2, sdict, x, y, n_local, nzr, st, sh, shift_theta, shift_sigma);
            };
            if (odd == 0x14u) gg(std::integral_constant<unsigned, 0x14u>{});   // (a box grid: +-1 odd, +-nx odd with nx)
            else gg(std::integral_constant<unsigned, 0x36u>{});
            return;
          }
          const int nzp = (int)((n_local + Pz - 1) / Pz), cmax = (int)(((Pz + 511) / 512 + 7) / 8);
          int nzr = zr_env > 0 ? zr_env : std::max(1, (288 + cmax / 2) / cmax);
          nzr = std::max(1, std::min(nzr, nzp / 4));
          if (nzp >= 8) {
            auto gz = [&](auto odd_tag) {
              ksd::k_spmv_stencil_marchz<7, 0x3eu, decltype(odd_tag)::value, 3, 0, 6><<<8 * cmax * nzr, kBlock, 0, s>>>(m2, sdict, x, y, n_local, nzr, st, sh, shift_theta, shift_sigma);
            };
            if (odd == 0x14u) gz(std::integral_constant<unsigned, 0x14u>{});
            else if (odd == 0x36u) gz(std::integral_constant<unsigned, 0x36u>{});
            else gz(std::integral_constant<unsigned, 0x3eu>{});
            return;
          }
        }
        if (shape) {
          auto gw = [&](auto odd_tag) {
            ksd::k_spmv_stencil_marchw<7, 0x3eu, decltype(odd_tag)::value, 3><<<G, kBlock, 0, s>>>(m2, sdict, x, y, n_local, nt, st, sh, shift_theta, shift_sigma);
          };
          if (odd == 0x14u) gw(std::integral_constant<unsigned, 0x14u>{});        // nx even: only +-1 are odd
          else if (odd == 0x36u) gw(std::integral_constant<unsigned, 0x36u>{});   // nx odd
          else gw(std::integral_constant<unsigned, 0x3eu>{});                     // anything else: every near tap as two 8-byte reads
          return;
        }
      }
      using M1 = std::integral_constant<int, -1>;
      // the slot of the rows' own entry is a compile-time constant for the common stencils (3-, 5-, 7-point); otherwise one more load
      if (nstencil == 7 && kown == 3) go(std::integral_constant<int, 7>{}, std::integral_constant<int, 3>{});
      else if (nstencil == 5 && kown == 2) go(std::integral_constant<int, 5>{}, std::integral_constant<int, 2>{});
      else if (nstencil == 3 && kown == 1) go(std::integral_constant<int, 3>{}, std::integral_constant<int, 1>{});
      else switch (nstencil) {
        case 1: go(std::integral_constant<int, 1>{}, M1{}); break;
        case 2: go(std::integral_constant<int, 2>{}, M1{}); break;
        case 3: go(std::integral_constant<int, 3>{}, M1{}); break;
        case 4: go(std::integral_constant<int, 4>{}, M1{}); break;
        case 5: go(std::integral_constant<int, 5>{}, M1{}); break;
        case 6: go(std::integral_constant<int, 6>{}, M1{}); break;
        case 7: go(std::integral_constant<int, 7>{}, M1{}); break;
        default: go(std::integral_constant<int, 8>{}, M1{}); break;
      }
    }
  }
  ksd::ShiftArg<D> shift_arg() const {
    ksd::ShiftArg<D> a;
    a.on = shift_on ? 1 : 0;
    a.theta = shift_theta;
    a.sigma = shift_sigma;
    return a;
  }
  void apply_shifted(const void* xv, void* yv, double tre, double tim, double sigma, int64_t ld, const DevState* st) override {
    const int fuse = env_int("KS_SHIFT_FUSED", 1);   // (read per product, like the forms of the stencil kernels: the tests switch it inside one process)
    // (every stored-matrix layout stores y = sigma (A x - theta x) itself -- the row's own x entry is one more cached load
    // -- except rows cut into chunks, whose sums are finished by a second kernel)
    const bool fused = fuse && n_local > 0 && nlong == 0;
    if (!fused) { ks_operator::apply_shifted(xv, yv, tre, tim, sigma, ld, st); return; }
    shift_on = true;
    if constexpr (sizeof(D) == 8) shift_theta = tre; else shift_theta = D{tre, tim};
    shift_sigma = sigma;
    try { apply(xv, yv, st); } catch (...) { shift_on = false; throw; }
    shift_on = false;
  }
  void apply(const void* xv, void* yv, const DevState* st) override {
    const D* x = static_cast<const D*>(xv);
    D* y = static_cast<D*>(yv);
    hipStream_t s = ctx->stream;
    // the stencil and the CSR-row-block kernels take the exchange of the peer-to-peer transport into their own launch (hf)
    const typename Halo<D>::Begun begun = halo.begin(x, st, n_local > 0 && cblocks.empty() && ndvi == 0 && nslices == 0);
    const ksd::HaloFused& hf = begun.hf;
    const D* xg = begun.xg;
    if (n_local > 0 && !cblocks.empty()) {
      // column-blocked CSR: one launch per column block; block b > 0 reads the partial row sums block b-1 left in y
      ProfScope ps(ctx, KSP_SPMV, (double)nnz * bytes_per_nnz + aux_bytes + 2.0 * sizeof(D) * n_local);
      if (cb_rpt) {
        // ONE launch: a workgroup keeps the sums of its rows in registers while it walks the column blocks (k_spmv_csr_cb)
        ksd::CbArgs<D> a{};
        a.nb = (int)cblocks.size();
        for (int b = 0; b < a.nb; ++b) {
          a.rowptr[b] = static_cast<const int32_t*>(cblocks[b]->rowptr);
          a.colidx[b] = cblocks[b]->colidx;
          a.val[b] = cblocks[b]->val;
          a.xb[b] = (!cb_from_ghost.empty() && cb_from_ghost[b]) ? xg : nullptr;
        }
        const int nt = (int)((n_local + (int64_t)kBlock * cb_rpt - 1) / ((int64_t)kBlock * cb_rpt));
        auto go = [&](auto ni_tag, auto rpt_tag) {
          constexpr int NI = decltype(ni_tag)::value, RPT = decltype(rpt_tag)::value;
          if constexpr ((size_t)NI * kBlock * sizeof(D) <= (size_t)ksd::kSpmvCapBytes)
            ksd::k_spmv_csr_cb<D, NI, RPT><<<nt, kBlock, 0, s>>>(a, x, y, n_local, nt, st, shift_arg());
          else
            throw KsError{KS_ERR_INTERNAL, "column-blocked CSR: LDS depth exceeds the budget of this element type"};
        };
        auto by_rpt = [&](auto ni_tag) {
          switch (cb_rpt) {
            case 1: go(ni_tag, std::integral_constant<int, 1>{}); break;
            case 2: go(ni_tag, std::integral_constant<int, 2>{}); break;
            case 4: go(ni_tag, std::integral_constant<int, 4>{}); break;
            case 8: go(ni_tag, std::integral_constant<int, 8>{}); break;
            default: go(ni_tag, std::integral_constant<int, 16>{}); break;
          }
        };
        if (cb_ni == 8) by_rpt(std::integral_constant<int, 8>{});
        else by_rpt(std::integral_constant<int, 16>{});
        KS_HIP(hipGetLastError());
        return;
      }
      for (size_t b = 0; b < cblocks.size(); ++b) cblocks[b]->launch_csr_blocks(x, y, st, b > 0 ? y : nullptr, b + 1 < cblocks.size() ? 1 : 0, shift_arg());
      KS_HIP(hipGetLastError());
      return;
    }
    if (n_local > 0) {
      // algorithmic bytes: 12 nnz + 4 (n+1) + 16 n   (8 -> 16 for complex); 4 nnz in the
      // value-indexed layout, 1 nnz in the delta-value-indexed one
      ProfScope ps(ctx, KSP_SPMV, (double)nnz * bytes_per_nnz + aux_bytes + 2.0 * sizeof(D) * n_local);
      const uint32_t* hseq = nullptr;  // (the host picked the ghost slot: xg)
      auto with_ip = [&](auto f) {
        if (ptr64) f(int64_t{});
        else f(int32_t{});
      };
      if (nstencil > 0 && halo.plan.nghost == 0 && smask2 && n_local >= 2 && env_int("KS_STENCIL_PAIRS", 1)) {
        // two rows per lane, 16-byte gathers (no ghost columns: single GPU)
        const int nt = (int)(((n_local + 1) / 2 + kBlock - 1) / kBlock);
        if constexpr (std::is_same<D, double>::value) {
          // Float64, at most 8 slots: the persistent software-pipelined form (ks_spmv_march.hpp)
          if (stencil_mask_bytes == 1 && nstencil <= 8 && march_on()) {
            launch_march(x, y, nt, st, s);
            KS_HIP(hipGetLastError());
            return;
          }
        }
        if (stencil_mask_bytes == 1)
          ksd::k_spmv_stencil2<D, uint16_t><<<nt, kBlock, 0, s>>>(static_cast<const uint16_t*>(smask2), sdict, nstencil, x, y, n_local, nt, st, shift_on ? (1 | (shift_plain() ? 2 : 0)) : 0, shift_theta, shift_sigma);
        else
          ksd::k_spmv_stencil2<D, uint64_t><<<nt, kBlock, 0, s>>>(static_cast<const uint64_t*>(smask2), sdict, nstencil, x, y, n_local, nt, st, shift_on ? (1 | (shift_plain() ? 2 : 0)) : 0, shift_theta, shift_sigma);
        KS_HIP(hipGetLastError());
        return;
      }
      if (nstencil > 0 && halo.plan.nghost > 0 && !halo.p2p && smask2 && (stencil_mask_bytes == 1 || stencil_mask_bytes == 4) && n_local >= 2 * kBlock) {
        // SPLIT PRODUCT of a rank on the collective transports (round 6c).  The ghost-aware kernel below is the one-row-per-lane
        // form (8-byte gathers: 16.2 us at the 8-way share of 216^3, 1.26e6 rows) where the paired kernel of the single-GPU path
        // takes 7.7 us.  Only the rows outside [ghost_lo_end, ghost_hi_begin) -- a slab's first and last plane -- reference ghost
        // columns: the paired kernel runs over ALL local rows (a ghost column is clamped to a local row there: the boundary rows
        // come out wrong), then the ghost-aware kernel rewrites the boundary tiles.  Same products in the same order as either
        // kernel alone (both add the slots in dictionary order).  A slab with two neighbours has NINE dictionary slots (seven of the
        // stencil, one ghost stride per neighbour): with all nine the paired kernel issues two groups of eight pair loads per lane and
        // the split is SLOWER (0.0491 against 0.0471 ms per iteration at the 8-way share of 216^3); with the slots that local
        // columns use only (nstencil_local: the ghost strides come last, only boundary rows carry their bits) it is one group:
        // 0.0444 against 0.0475 (profiles/r06c_ab.txt).  KS_DIST_SPLIT=0: the ghost-aware kernel for every row.
        if constexpr (std::is_same<D, double>::value) {
          static const int split_env = env_int("KS_DIST_SPLIT", 1);
          const int nt1 = (int)((n_local + kBlock - 1) / kBlock);
          const int nlow = (int)((halo.plan.ghost_lo_end + kBlock - 1) / kBlock), first_high = (int)(halo.plan.ghost_hi_begin / kBlock);
          const int nhigh = nt1 - first_high;
          if (split_env && env_int("KS_STENCIL_PAIRS", 1) && nlow <= first_high && 4 * (nlow + nhigh) <= nt1 && nlow + nhigh > 0) {
            const int nt2 = (int)(((n_local + 1) / 2 + kBlock - 1) / kBlock);
            static const int split_dbg = env_int("KS_DIST_SPLIT_DEBUG", 0);
            if (split_dbg && !split_said) {
              split_said = true;
              std::fprintf(stderr, "[split] rows %lld: paired kernel on all of them (%d of %d slots), ghost-aware kernel on %d + %d boundary tiles of %d\n", (long long)n_local, nstencil_local, nstencil, nlow, nhigh, nt1);
            }
            // (a slab in the middle of the partition has NINE slots -- the seven of the stencil and one ghost stride per neighbour --,
            // hence 4-byte masks: the paired kernel takes them as 64-bit words of two rows)
            const int shf = shift_on ? (1 | (shift_plain() ? 2 : 0)) : 0;
            ksd::HaloFused h0{};
            // (the paired kernel only takes the slots that local columns use: the ghost strides come last in the dictionary, only
            // boundary rows have their bits, and those rows are rewritten below -- one group of eight pair loads instead of two)
            const int nsl = nstencil_local >= 1 ? nstencil_local : nstencil;
            if (stencil_mask_bytes == 1) {
              ksd::k_spmv_stencil2<D, uint16_t><<<nt2, kBlock, 0, s>>>(static_cast<const uint16_t*>(smask2), sdict, nsl, x, y, n_local, nt2, st, shf, shift_theta, shift_sigma);
              ksd::k_spmv_stencil<D, uint8_t, 1><<<nlow + nhigh, kBlock, 0, s>>>(static_cast<const uint8_t*>(smask), sdict, nstencil, x, xg, y, n_local,
                                                                                std::max<int64_t>(halo.plan.nghost, 0), nlow + nhigh, st, h0, halo.hargs, ctx->p2p.dev, shift_on ? 1 : 0,
                                                                                shift_theta, shift_sigma, nlow, first_high - nlow);
            } else {
              ksd::k_spmv_stencil2<D, uint64_t><<<nt2, kBlock, 0, s>>>(static_cast<const uint64_t*>(smask2), sdict, nsl, x, y, n_local, nt2, st, shf, shift_theta, shift_sigma);
              ksd::k_spmv_stencil<D, uint32_t, 1><<<nlow + nhigh, kBlock, 0, s>>>(static_cast<const uint32_t*>(smask), sdict, nstencil, x, xg, y, n_local,
                                                                                 std::max<int64_t>(halo.plan.nghost, 0), nlow + nhigh, st, h0, halo.hargs, ctx->p2p.dev, shift_on ? 1 : 0,
                                                                                 shift_theta, shift_sigma, nlow, first_high - nlow);
            }
            KS_HIP(hipGetLastError());
            return;
          }
        }
      }
      if (nstencil > 0) {
        static const int rpt_env = env_int("KS_STENCIL_RPT", 1);
        auto go = [&](auto mt_tag, auto rpt_tag) {
          using MT = decltype(mt_tag);
          constexpr int RPT = decltype(rpt_tag)::value;
          const int nt = (int)((n_local + kBlock * RPT - 1) / (kBlock * RPT));
          ksd::HaloFused h = hf;
          h.npush = std::min(h.npush, nt);
          h.tile_shift = (h.enabled && halo.plan.ghost_lo_end < n_local) ? (int)((halo.plan.ghost_lo_end + kBlock * RPT - 1) / (kBlock * RPT)) % std::max(nt, 1) : 0;
          ksd::k_spmv_stencil<D, MT, RPT><<<nt, kBlock, 0, s>>>(static_cast<const MT*>(smask), sdict, nstencil, x, xg, y, n_local,
                                                                std::max<int64_t>(halo.plan.nghost, 0), nt, st, h, halo.hargs, ctx->p2p.dev, shift_on ? 1 : 0,
                                                                shift_theta, shift_sigma);
        };
        auto by_rpt = [&](auto mt_tag) {
          if (rpt_env <= 1) go(mt_tag, std::integral_constant<int, 1>{});
          else if (rpt_env == 2) go(mt_tag, std::integral_constant<int, 2>{});
          else go(mt_tag, std::integral_constant<int, 4>{});
        };
        if (stencil_mask_bytes == 1) by_rpt(uint8_t{});
        else by_rpt(uint32_t{});
        KS_HIP(hipGetLastError());
        return;
      }
      if (ndvi > 0) {
        with_ip([&](auto ip_tag) {
          using IP = decltype(ip_tag);
          const IP* rp = static_cast<const IP*>(rowptr);
          auto go = [&](auto un_tag, auto rpt_tag) {
            constexpr int UN = decltype(un_tag)::value, RPT = decltype(rpt_tag)::value;
            const int nt = (int)((n_local + kBlock * RPT - 1) / (kBlock * RPT));
            ksd::k_spmv_dvi<D, IP, UN, RPT><<<nt, kBlock, 0, s>>>(rp, codes, ddelta, val, x, xg, y, n_local, nt, ndvi, st, hseq, halo.ghost_stride, shift_arg());
          };
          using I = std::integral_constant<int, 0>;
          (void)sizeof(I);
          if (dvi_unroll == 4) {
            if (dvi_rpt == 1) go(std::integral_constant<int, 4>{}, std::integral_constant<int, 1>{});
            else if (dvi_rpt == 2) go(std::integral_constant<int, 4>{}, std::integral_constant<int, 2>{});
            else go(std::integral_constant<int, 4>{}, std::integral_constant<int, 4>{});
          } else {
            if (dvi_rpt == 1) go(std::integral_constant<int, 8>{}, std::integral_constant<int, 1>{});
            else if (dvi_rpt == 2) go(std::integral_constant<int, 8>{}, std::integral_constant<int, 2>{});
            else go(std::integral_constant<int, 8>{}, std::integral_constant<int, 4>{});
          }
        });
        KS_HIP(hipGetLastError());
        return;
      }
      if (nslices > 0) {
        with_ip([&](auto ip_tag) {
          using IP = decltype(ip_tag);
          const int ng = (nslices + 3) / 4;
          auto go = [&](auto vi_tag, auto un_tag) {
            constexpr bool VI = decltype(vi_tag)::value;
            constexpr int UN = decltype(un_tag)::value;
            static const int plain_loads = env_int("KS_SELL_PLAIN_LOADS", 0);  // experiment: default-policy loads of the matrix streams
            if (plain_loads)
              ksd::k_spmv_sell<D, IP, VI, UN, false><<<ng, kBlock, 0, s>>>(static_cast<const IP*>(sliceptr), colidx, val, sperm, x, xg, y,
                                                                           n_local, nslices, ng, st, hseq, halo.ghost_stride, ndict, shift_arg());
            else
              ksd::k_spmv_sell<D, IP, VI, UN, true><<<ng, kBlock, 0, s>>>(static_cast<const IP*>(sliceptr), colidx, val, sperm, x, xg, y,
                                                                          n_local, nslices, ng, st, hseq, halo.ghost_stride, ndict, shift_arg());
          };
          auto by_un = [&](auto vi_tag) {
            if (sell_un <= 4) go(vi_tag, std::integral_constant<int, 4>{});
            else go(vi_tag, std::integral_constant<int, 8>{});
          };
          if (ndict > 0) by_un(std::true_type{});
          else by_un(std::false_type{});
        });
        KS_HIP(hipGetLastError());
        return;
      }
      with_ip([&](auto ip_tag) {
        using IP = decltype(ip_tag);
        auto launch = [&](auto vi_tag, auto ni_tag) {
          constexpr bool VI = decltype(vi_tag)::value;
          constexpr int NI = decltype(ni_tag)::value;
          if constexpr ((size_t)NI * kBlock * sizeof(D) <= (size_t)ksd::kSpmvCapBytes)
          {
            static const int csr_nt = env_int("KS_SPMV_CSR_NT", 1);
            ksd::HaloFused h = hf;
            h.npush = std::min(h.npush, nblk);
            ksd::k_spmv_csr<D, IP, VI, NI><<<nblk, kBlock, 0, s>>>(static_cast<const IP*>(blkptr), blkrow, static_cast<const IP*>(rowptr), colidx,
                                                                   val, x, xg, y, n_local, nblk, st, hseq, halo.ghost_stride, ndict, blkpart, lpart,
                                                                   nullptr, 0, h, halo.hargs, ctx->p2p.dev, csr_nt != 0, row_gather, shift_arg());
          }
          else
            throw KsError{KS_ERR_INTERNAL, "CSR row blocks of " + std::to_string(NI) + " x 256 entries exceed the LDS budget of this element type"};
        };
        auto by_ni = [&](auto vi_tag) {
          switch (ni) {
            case 4: launch(vi_tag, std::integral_constant<int, 4>{}); break;
            case 7: launch(vi_tag, std::integral_constant<int, 7>{}); break;
            case 8: launch(vi_tag, std::integral_constant<int, 8>{}); break;
            case 12: launch(vi_tag, std::integral_constant<int, 12>{}); break;
            default: launch(vi_tag, std::integral_constant<int, 16>{}); break;
          }
        };
        if (ndict > 0) by_ni(std::true_type{});
        else by_ni(std::false_type{});
      });
      if (nlong > 0) ksd::k_spmv_longfix<D><<<(nlong + kBlock - 1) / kBlock, kBlock, 0, s>>>(lrow, lfirst, lpart, y, nlong, st);
    }
    KS_HIP(hipGetLastError());
  }
};

// dense matrix resident in HBM, row-major with padded rows
template <class D> struct DenseOp : ks_operator {
  D* A = nullptr;
  int64_t lda = 0;
  ~DenseOp() override { (void)hipFree(A); }
  void apply(const void* xv, void* yv, const DevState* st) override {
    ProfScope ps(ctx, KSP_SPMV, (double)n_local * n_local * sizeof(D) + 2.0 * sizeof(D) * n_local);
    const int64_t want = (n_local + 3) / 4;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->num_cu * 8));
    ksd::k_gemv_rows<D><<<nb, kBlock, 0, ctx->stream>>>(A, lda, n_local, n_local, static_cast<const D*>(xv), static_cast<D*>(yv), st);
    KS_HIP(hipGetLastError());
  }
};

struct HostCallbackOp : ks_operator {
  ks_host_apply_fn fn = nullptr;
  void* user = nullptr;
  void* xh = nullptr;
  void* yh = nullptr;
  ~HostCallbackOp() override { (void)hipHostFree(xh); (void)hipHostFree(yh); }
  void apply(const void* x, void* y, const DevState*) override {
    const size_t bytes = (size_t)n_local * (dtype == KS_F64 ? 8 : 16);
    KS_HIP(hipMemcpyAsync(xh, x, bytes, hipMemcpyDeviceToHost, ctx->stream));
    KS_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t nd = n_local * (dtype == KS_F64 ? 1 : 2);
    if (in_scale != 1.0) {
      double* xd = static_cast<double*>(xh);
      for (int64_t i = 0; i < nd; ++i) xd[i] *= in_scale;
    }
    const int rc = fn(user, xh, yh);
    KS_REQUIRE(rc == 0, KS_ERR_OPERATOR, "host operator callback returned " + std::to_string(rc));
    if (in_scale != 1.0) {
      const double back = 1.0 / in_scale;
      double* yd = static_cast<double*>(yh);
      for (int64_t i = 0; i < nd; ++i) yd[i] *= back;
    }
    KS_HIP(hipMemcpyAsync(y, yh, bytes, hipMemcpyHostToDevice, ctx->stream));
  }
};

struct DeviceCallbackOp : ks_operator {
  ks_device_apply_fn fn = nullptr;
  void* user = nullptr;
  void apply(const void* x, void* y, const DevState*) override {
    const int rc = fn(user, x, y, (void*)ctx->stream);
    KS_REQUIRE(rc == 0, KS_ERR_OPERATOR, "device operator callback returned " + std::to_string(rc));
  }
};

// Host conversion of whatever the caller has into int32 0-based CSR.
template <class I> inline int64_t idx_at(const void* p, int64_t i) { return (int64_t) static_cast<const I*>(p)[i]; }

template <class D>
void build_csr_host(int64_t nrows, int64_t ncols, int64_t nnz, const void* ptr, const void* idx, const void* val,
                    int layout, int base, int itype, std::vector<int64_t>& rp, std::vector<int32_t>& ci,
                    std::vector<D>& vv) {
  auto P = [&](int64_t i) { return (itype == KS_I32 ? idx_at<int32_t>(ptr, i) : idx_at<int64_t>(ptr, i)) - base; };
  auto J = [&](int64_t i) { return (itype == KS_I32 ? idx_at<int32_t>(idx, i) : idx_at<int64_t>(idx, i)) - base; };
  const D* v = static_cast<const D*>(val);
  // column indices are 32-bit on the device; the non-zero offsets (rowptr) switch to 64 bits when nnz >= 2^31
  KS_REQUIRE(nrows < (int64_t)2147483647 && ncols < (int64_t)2147483647, KS_ERR_ARGUMENT, "matrix order must fit int32");
  {
    // the pointer array must be monotone and stay inside [0, nnz]: a malformed one would index host (CSC
    // conversion) or device (SpMV) arrays out of bounds
    const int64_t np = (layout == KS_CSR ? nrows : ncols);
    int64_t prev = P(0);
    KS_REQUIRE(prev == 0, KS_ERR_ARGUMENT, layout == KS_CSR ? "row pointer does not match nnz" : "column pointer does not match nnz");
    for (int64_t i = 1; i <= np; ++i) {
      const int64_t cur = P(i);
      KS_REQUIRE(cur >= prev && cur <= nnz, KS_ERR_ARGUMENT, "pointer array is not monotone within [0, nnz]");
      prev = cur;
    }
    KS_REQUIRE(prev == nnz, KS_ERR_ARGUMENT, layout == KS_CSR ? "row pointer does not match nnz" : "column pointer does not match nnz");
  }
  rp.assign(nrows + 1, 0);
  ci.resize(nnz);
  vv.resize(nnz);
  if (layout == KS_CSR) {
    for (int64_t i = 0; i <= nrows; ++i) rp[i] = P(i);
    for (int64_t p = 0; p < nnz; ++p) {
      const int64_t c = J(p);
      KS_REQUIRE(c >= 0 && c < ncols, KS_ERR_ARGUMENT, "column index out of range");
      ci[p] = (int32_t)c;
      vv[p] = v[p];
    }
  } else {  // CSC (Julia SparseMatrixCSC: colptr, rowval, nzval) -> CSR by counting sort
    for (int64_t p = 0; p < nnz; ++p) {
      const int64_t r = J(p);
      KS_REQUIRE(r >= 0 && r < nrows, KS_ERR_ARGUMENT, "row index out of range");
      rp[r + 1]++;
    }
    for (int64_t i = 0; i < nrows; ++i) rp[i + 1] += rp[i];
    std::vector<int64_t> fill(rp.begin(), rp.end() - 1);
    for (int64_t c = 0; c < ncols; ++c)
      for (int64_t p = P(c); p < P(c + 1); ++p) {
        const int64_t r = J(p);
        const int64_t q = fill[r]++;
        ci[q] = (int32_t)c;
        vv[q] = v[p];
      }
  }
}

// ... and of a distributed row block (ks_operator_csr_dist: 0-based, local-extended columns nrows + ghost slot) into the same arrays
inline void build_csr_dist_host(int64_t nrows, int64_t nghost, int64_t nnz, const int64_t* rowptr, const int32_t* colidx,
                                std::vector<int64_t>& rp, std::vector<int32_t>& ci) {
  KS_REQUIRE(nrows < (int64_t)2147483647 && nghost < (int64_t)2147483647 - nrows, KS_ERR_ARGUMENT, "local-extended column range must fit int32");
  rp.resize(nrows + 1);
  KS_REQUIRE(rowptr[0] == 0 && rowptr[nrows] == nnz, KS_ERR_ARGUMENT, "row pointer does not match nnz");
  for (int64_t i = 0; i <= nrows; ++i) {
    KS_REQUIRE(i == 0 || (rowptr[i] >= rowptr[i - 1] && rowptr[i] <= nnz), KS_ERR_ARGUMENT, "pointer array is not monotone within [0, nnz]");
    rp[i] = rowptr[i];
  }
  ci.assign(colidx, colidx + nnz);
  for (int64_t p = 0; p < nnz; ++p)
    KS_REQUIRE(ci[p] >= 0 && ci[p] < nrows + nghost, KS_ERR_ARGUMENT, "local-extended column index out of range");
}

// device copy of the non-zero offsets in the width the kernels will use
inline void* upload_ptr(const std::vector<int64_t>& v, bool ptr64) {
  void* d = nullptr;
  const size_t cnt = v.size();
  if (ptr64) {
    KS_HIP(hipMalloc(&d, std::max<size_t>(cnt * 8, 16)));
    KS_HIP(hipMemcpy(d, v.data(), cnt * 8, hipMemcpyHostToDevice));
  } else {
    std::vector<int32_t> t(v.begin(), v.end());
    KS_HIP(hipMalloc(&d, std::max<size_t>(cnt * 4, 16)));
    KS_HIP(hipMemcpy(d, t.data(), cnt * 4, hipMemcpyHostToDevice));
  }
  return d;
}

// device copy of the first `cnt` elements of v with `pad` more elements behind them; `zero`: the padding is zero-filled (a kernel
// reads it), otherwise it is slack nothing interprets
template <class T> T* upload_vec(const T* v, size_t cnt, size_t pad, bool zero = false) {
  void* d = nullptr;
  KS_HIP(hipMalloc(&d, (cnt + pad) * sizeof(T)));
  if (zero) KS_HIP(hipMemset(d, 0, (cnt + pad) * sizeof(T)));
  if (cnt) KS_HIP(hipMemcpy(d, v, cnt * sizeof(T), hipMemcpyHostToDevice));
  return static_cast<T*>(d);
}
template <class T> T* upload_vec(const std::vector<T>& v, size_t pad, bool zero = false) { return upload_vec(v.data(), v.size(), pad, zero); }

// the device arrays of a plan (ks_csr_layout.hpp) over the matrix (rp, ci, vv) it was made for
template <class D>
CsrOp<D>* upload(ks_ctx* ctx, const CsrPlan<D>& P, int64_t nrows, int64_t nnz, const std::vector<int64_t>& rp, const std::vector<int32_t>& ci,
                 const std::vector<D>& vv) {
  auto op = std::make_unique<CsrOp<D>>();
  op->ctx = ctx;
  op->n_local = nrows;
  op->nnz = nnz;
  op->dtype = sizeof(D) == 8 ? KS_F64 : KS_C64;
  op->layout = P.layout;
  op->ptr64 = P.ptr64;
  op->bytes_per_nnz = P.bytes_per_nnz;
  op->aux_bytes = P.aux_bytes;
  op->ndict = P.ndict;
  constexpr size_t kPad16 = 16 / sizeof(D);  // 16 bytes of D
  switch (P.layout) {
    case KS_LAYOUT_STENCIL: {
      op->nstencil = P.nstencil;
      op->nstencil_local = P.nstencil_local;
      op->stencil_mask_bytes = P.stencil_mask_bytes;
      for (int k = 0; k < ksd::kStencilSlots; ++k) {
        op->sdict.delta[k] = k < P.nstencil ? P.sdelta[k] : 0;
        op->sdict.val[k] = k < P.nstencil ? P.sval[k] : D{};
      }
      // zeroed masks up to a multiple of 8 rows beyond nrows + 2: k_spmv_stencil2 and the marching kernels (ks_spmv_march.hpp) read
      // the masks of two rows in one word (smask2)
      const size_t pad = (size_t)(round_up(nrows + 2, 8) - nrows);
      if (P.stencil_mask_bytes == 1) op->smask = upload_vec(P.mask8, pad, true);
      else op->smask = upload_vec(P.mask32, pad, true);
      op->smask2 = op->smask;
      // (the masks stay uploaded: the clamped edge path and every other kernel read them)
      if (std::is_same<D, double>::value && P.stencil_mask_bytes == 1 && P.nstencil == P.nstencil_local)
        op->geom = stencil_geometry(P.sdelta.data(), P.nstencil, nrows, P.mask8.data(), P.mask8.size());
      break;
    }
    case KS_LAYOUT_DVI:
      op->ndvi = P.ndvi;
      op->dvi_unroll = P.dvi_unroll;
      op->dvi_rpt = P.dvi_rpt;
      op->rowptr = upload_ptr(rp, P.ptr64);
      op->codes = upload_vec(P.codes, 64, true);  // k_spmv_dvi stages the codes of a tile in 16-byte packs: 64 zero bytes behind them
      op->ddelta = upload_vec(P.ddelta, 256 - P.ddelta.size());  // (the dictionaries are allocated at their full 256 entries)
      op->val = upload_vec(P.dval, 256 - P.dval.size());
      break;
    case KS_LAYOUT_SELL:
    case KS_LAYOUT_SELL_VI:
      op->nslices = P.nslices;
      op->sell_un = P.sell_un;
      op->sell_entries = P.sell_entries;
      op->sliceptr = upload_ptr(P.sliceptr, P.ptr64);
      op->colidx = upload_vec(P.sell_col, 4);  // (16 bytes of slack behind indices and values; k_spmv_sell stays inside its slices)
      if (P.ndict > 0) op->val = upload_vec(P.dict, 256 - P.dict.size());
      else op->val = upload_vec(P.sell_val, kPad16);
      if (!P.sell_perm.empty()) op->sperm = upload_vec(P.sell_perm, 0);
      break;
    case KS_LAYOUT_CSR_CB:
      for (const CsrPlan<D>& cb : P.cblocks)
        op->cblocks.emplace_back(upload<D>(ctx, cb, nrows, (int64_t)cb.sub_ci.size(), cb.sub_rp, cb.sub_ci, cb.sub_vv));
      op->cb_from_ghost = P.cb_from_ghost;
      op->cb_rpt = P.cb_rpt;
      op->cb_ni = P.cb_ni;
      break;
    default: {  // KS_LAYOUT_CSR / KS_LAYOUT_CSR_VI: row blocks of k_spmv_csr
      op->ni = P.ni;
      op->row_gather = P.row_gather;
      op->nlong = P.nlong;
      op->nblk = P.nblk;
      op->blkptr = upload_ptr(P.blkptr, P.ptr64);
      op->blkrow = upload_vec(P.blkrow, P.blkrow.size() < 4 ? 4 - P.blkrow.size() : 0);  // (at least 16 bytes)
      if (P.nlong > 0) {
        op->blkpart = upload_vec(P.blkpart, 0);
        KS_HIP(hipMalloc(&op->lpart, (size_t)P.lfirst.back() * sizeof(D)));
        op->lrow = upload_vec(P.lrow, 0);
        op->lfirst = upload_vec(P.lfirst, 0);
      }
      op->rowptr = upload_ptr(rp, P.ptr64);
      // (two entries + 16 bytes of slack behind indices and values: k_spmv_csr and k_spmv_csr_cb guard every load by the block's
      // entry count, nothing reads it)
      if (P.ndict > 0) {
        op->colidx = upload_vec(P.packed, 2 + 4);
        op->val = upload_vec(P.dict, 256 - P.dict.size());
      } else {
        op->colidx = upload_vec(ci.data(), (size_t)nnz, 2 + 4);
        op->val = upload_vec(vv.data(), (size_t)nnz, 2 + kPad16);
      }
    }
  }
  return op.release();
}

// stored sparse matrix -> its device layout: planned on the host (ks_csr_layout.hpp), then uploaded
template <class D>
CsrOp<D>* make_csr(ks_ctx* ctx, int64_t nrows, int64_t nnz, const std::vector<int64_t>& rp, const std::vector<int32_t>& ci,
                   const std::vector<D>& vv, CbMode cb_mode = CbMode::None, int64_t nghost = 0, int64_t nlow = 0) {
  const CsrPlan<D> plan = plan_csr<D>(CsrHost<D>{nrows, nnz, rp, ci, vv}, FormatRequest::from_env(), cb_mode, nghost, nlow, ctx->num_cu);
  return upload<D>(ctx, plan, nrows, nnz, rp, ci, vv);
}

}  // namespace

// default of ks_operator::apply_shifted: product + one streaming pass
inline void ks_operator::apply_shifted(const void* x, void* y, double theta_re, double theta_im, double sigma, int64_t ld, const DevState* st) {
  apply(x, y, st);
  ProfScope ps(ctx, KSP_SCALE, 3.0 * (double)n_local * (dtype == KS_F64 ? 8.0 : 16.0));
  const int nbk = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)ctx->num_cu * 8, ld / (2 * kBlock) + 1));
  if (dtype == KS_F64) {
    ksd::k_shift_scale<double><<<nbk, kBlock, 0, ctx->stream>>>(static_cast<double*>(y), static_cast<const double*>(x), theta_re, sigma, ld, st);
  } else {
    ksd::k_shift_scale<cd><<<nbk, kBlock, 0, ctx->stream>>>(static_cast<cd*>(y), static_cast<const cd*>(x), cd{theta_re, theta_im}, sigma, ld, st);
  }
  KS_HIP(hipGetLastError());
}

// default of ks_operator::apply_clenshaw: product + one streaming pass over rows < n_local (shift, scale and tail together)
inline void ks_operator::apply_clenshaw(const void* x, void* y, double theta_re, double theta_im, double sigma, const void* w, double gamma,
                                        const void* x0, int64_t, const DevState* st) {
  KS_REQUIRE(y != x && y != w && y != x0, KS_ERR_ARGUMENT, "Clenshaw step: y must be distinct from x, w and x0");
  auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  KS_REQUIRE(aligned(x) && aligned(y) && aligned(w) && aligned(x0), KS_ERR_INTERNAL, "Clenshaw step: a vector is not 16-byte aligned");
  apply(x, y, st);
  ++clenshaw_generic;
  if (n_local <= 0) return;
  ProfScope ps(ctx, KSP_SCALE, (3.0 + (w ? 1.0 : 0.0) + (x0 ? 1.0 : 0.0)) * (double)n_local * (dtype == KS_F64 ? 8.0 : 16.0));
  const int nbk = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)ctx->num_cu * 8, n_local / (2 * kBlock) + 1));
  const int plain = shift_store_cacheable ? 1 : 0;
  if (dtype == KS_F64) {
    ksd::k_clenshaw_tail<double><<<nbk, kBlock, 0, ctx->stream>>>(static_cast<double*>(y), static_cast<const double*>(x), theta_re, sigma,
                                                                  static_cast<const double*>(w), gamma, static_cast<const double*>(x0), n_local, plain, st);
  } else {
    ksd::k_clenshaw_tail<cd><<<nbk, kBlock, 0, ctx->stream>>>(static_cast<cd*>(y), static_cast<const cd*>(x), cd{theta_re, theta_im}, sigma,
                                                              static_cast<const cd*>(w), gamma, static_cast<const cd*>(x0), n_local, plain, st);
  }
  KS_HIP(hipGetLastError());
}
