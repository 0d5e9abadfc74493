// Halo<D>: the device side of a halo plan (ks_halo_plan.hpp) -- the ghost vector of a distributed row block, the buffers of its
// transport, and the exchange that precedes every product.  One member of CsrOp<D> (ks_operators.hpp).
// Part of the ONE translation unit of libkschur_hip.so (needs ks_context.hpp and ks_halo_plan.hpp).
#pragma once

namespace {

template <class D> struct Halo {
  ks_ctx* ctx = nullptr;
  HaloPlan plan;  // (one GPU: no neighbours, no ghosts)
  D* ghost = nullptr;
  // collective transports (RCCL, host-staged): consecutive send lists go straight out of x, the others through the pack kernel
  D* sendbuf = nullptr;         // plan.nscatter packed values
  int32_t* send_idx = nullptr;  // plan.packed
  // host-staged halo (ks_ctx_create_hostcomm): pinned send / receive images of the plan
  D* hsend = nullptr;
  D* hrecv = nullptr;
  // peer-to-peer halo (ks_p2p.hpp): ghost lives (double-buffered) in this rank's shared arena, neighbours store into it directly
  bool p2p = false;
  int64_t ghost_stride = 0;         // elements between the two ghost slots
  size_t arena_lo = 0, arena_hi = 0;
  int32_t* send_idx_all = nullptr;  // plan.send_all
  ksd::HaloArgs hargs{};

  Halo() = default;
  Halo(const Halo&) = delete;
  Halo& operator=(const Halo&) = delete;
  ~Halo() {
    if (p2p) {
      if (ctx->p2p.arena_used == arena_hi) ctx->p2p.arena_used = arena_lo;  // stack discipline; otherwise kept until the context dies
    } else {
      (void)hipFree(ghost);
    }
    (void)hipHostFree(hsend); (void)hipHostFree(hrecv);
    (void)hipFree(sendbuf); (void)hipFree(send_idx); (void)hipFree(send_idx_all);
  }

  // COLLECTIVE in peer-to-peer mode (one all-gather of the ranks' table rows)
  void upload(ks_ctx* c, const HaloPlan& P) {
    ctx = c;
    plan = P;
    p2p = c->p2p.attached;
    if (!p2p) {
      KS_HIP(hipMalloc(&ghost, std::max<size_t>((size_t)P.nghost * sizeof(D), 16)));
      KS_HIP(hipMemset(ghost, 0, std::max<size_t>((size_t)P.nghost * sizeof(D), 16)));
    }
    KS_HIP(hipMalloc(&sendbuf, std::max<size_t>(P.packed.size() * sizeof(D), 16)));
    KS_HIP(hipMalloc(&send_idx, std::max<size_t>(P.packed.size() * 4, 16)));
    if (!P.packed.empty()) KS_HIP(hipMemcpy(send_idx, P.packed.data(), P.packed.size() * 4, hipMemcpyHostToDevice));
    KS_REQUIRE(P.neigh.empty() || c->distributed(), KS_ERR_ARGUMENT, "halo plan needs a distributed context");
    if (c->hc.exchange) {
      KS_HIP(hipHostMalloc(&hsend, std::max<size_t>((size_t)P.send_ptr.back() * sizeof(D), 16)));
      KS_HIP(hipHostMalloc(&hrecv, std::max<size_t>((size_t)P.nghost * sizeof(D), 16)));
    }
    if (!p2p) return;
    // every rank publishes where its ghost vector lives in its shared arena and, per sender, at which offset that sender's
    // entries go (and how many it expects)
    auto& R = c->p2p;
    const P2pGhost g = p2p_ghost_size(P, sizeof(D));
    ghost_stride = g.stride;
    KS_REQUIRE(R.arena_used + g.bytes <= R.arena_bytes, KS_ERR_ARGUMENT, "ghost vectors do not fit the shared arena (raise KS_P2P_ARENA_MB)");
    arena_lo = R.arena_used;
    arena_hi = R.arena_used + g.bytes;
    R.arena_used = arena_hi;
    ghost = reinterpret_cast<D*>(static_cast<char*>(R.region) + R.arena_off + arena_lo);
    KS_HIP(hipMemset(ghost, 0, g.bytes));
    KS_HIP(hipDeviceSynchronize());
    const std::vector<int64_t> tab = p2p_allgather_i64(c, p2p_table_row(P, c->nranks, (int64_t)(R.arena_off + arena_lo), ghost_stride));
    const P2pPeers peers = p2p_read_table(P, c->rank, c->nranks, tab, sizeof(D));
    hargs.nneigh = P.nneigh();
    hargs.nrecv = (int)peers.recv_from.size();
    std::copy(P.send_ptr.begin(), P.send_ptr.end(), hargs.send_ptr);
    std::copy(peers.recv_from.begin(), peers.recv_from.end(), hargs.recv_from);
    for (int p = 0; p < P.nneigh(); ++p) {
      const int q = P.neigh[p];
      hargs.dst[p] = static_cast<char*>(R.peer[q]) + peers.dst_offset[p];
      hargs.dst_stride[p] = peers.dst_stride[p];
      hargs.flag_dst[p] = static_cast<uint64_t*>(R.peer[q]) + ksd::p2p_ll_words(c->nranks, R.cap) + c->rank;
    }
    KS_HIP(hipMalloc(&send_idx_all, std::max<size_t>(P.send_all.size() * 4, 16)));
    if (!P.send_all.empty()) KS_HIP(hipMemcpy(send_idx_all, P.send_all.data(), P.send_all.size() * 4, hipMemcpyHostToDevice));
  }

  struct Begun {
    ksd::HaloFused hf;  // for a kernel that does the exchange itself (enabled == 0: nothing left to do)
    const D* xg;        // the ghost vector the product reads
  };
  // Starts the exchange of x's boundary entries on the context's stream.  `kernel_fuses`: the layout's SpMV kernel takes a
  // HaloFused (the stencil and the CSR-row-block kernels) -- in peer-to-peer mode it then does the exchange itself, every other
  // layout gets the push kernel in front.
  Begun begin(const D* x, const DevState* st, bool kernel_fuses) {
    const HaloPlan& P = plan;
    ksd::HaloFused hf{};
    const D* xg = ghost;
    if (P.neigh.empty()) return {hf, xg};  // (nothing to exchange; on one GPU no upload() has set ctx)
    hipStream_t s = ctx->stream;
    if (p2p) {
      // sequence number and ghost slot of this exchange (host counter, ks_p2p.hpp)
      uint32_t seq = ctx->p2p.hseq + 1u;
      if (seq == 0u) seq = 1u;
      ctx->p2p.hseq = seq;
      xg = ghost + (int64_t)(seq & 1u) * ghost_stride;
      static const int fuse_env = env_int("KS_HALO_FUSED", 1);
      const int64_t total = P.send_ptr.back();
      if (fuse_env && kernel_fuses) {
        hf.enabled = 1;
        hf.seq = seq;
        // pushers: ~8 entries per thread (two trips of four independent entries), at most 64 workgroups -- each pusher ends
        // with a system-scope release fence (an L2 write-back), which is what an SpMV launch can afford only a few of
        static const int npush_env = env_int("KS_HALO_NPUSH", 0);
        hf.npush = npush_env > 0 ? npush_env : (int)std::max<int64_t>(1, std::min<int64_t>((total + 2047) / 2048, 64));
        hf.send_idx = send_idx_all;
        hf.counter = ctx->p2p.hstate + 1;
        hf.ghost_lo_end = P.ghost_lo_end;
        hf.ghost_hi_begin = P.ghost_hi_begin;
      } else {
        const int gb = (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 512));
        ksd::k_halo_push<D><<<gb, 256, 0, s>>>(x, send_idx_all, hargs, ctx->p2p.dev, ctx->p2p.hstate, seq, st ? &st->breakdown : nullptr);
      }
      return {hf, xg};
    }
    if (P.nscatter > 0) {
      const int gb = (int)std::min<int64_t>((P.nscatter + kBlock - 1) / kBlock, 4096);
      ksd::k_gather<D><<<gb, kBlock, 0, s>>>(x, send_idx, sendbuf, P.nscatter, st);
    }
    if (ctx->hc.exchange) {
      // host-staged: the same plan (in-place runs, packed lists, consecutive ghost slots) through pinned memory
      const size_t np_ = P.neigh.size();
      std::vector<const void*> sp_(np_);
      std::vector<void*> rp_(np_);
      std::vector<int64_t> sb_(np_), rb_(np_);
      for (size_t p = 0; p < np_; ++p) {
        const int64_t sc = P.send_ptr[p + 1] - P.send_ptr[p], rc = P.recv_ptr[p + 1] - P.recv_ptr[p];
        if (sc > 0) {
          const D* src = P.send_first[p] >= 0 ? x + P.send_first[p] : sendbuf + P.pack_ptr[p];
          KS_HIP(hipMemcpyAsync(hsend + P.send_ptr[p], src, (size_t)sc * sizeof(D), hipMemcpyDeviceToHost, s));
        }
        sp_[p] = hsend + P.send_ptr[p]; sb_[p] = sc * (int64_t)sizeof(D);
        rp_[p] = hrecv + P.recv_ptr[p]; rb_[p] = rc * (int64_t)sizeof(D);
      }
      KS_HIP(hipStreamSynchronize(s));
      const int rc = ctx->hc.exchange(ctx->hc.user, (int)np_, P.neigh.data(), sp_.data(), sb_.data(), rp_.data(), rb_.data());
      KS_REQUIRE(rc == 0, KS_ERR_COMM, "host exchange callback returned " + std::to_string(rc));
      if (P.nghost > 0) KS_HIP(hipMemcpyAsync(ghost, hrecv, (size_t)P.nghost * sizeof(D), hipMemcpyHostToDevice, s));
    } else {
      constexpr int dpe = sizeof(D) / 8;  // doubles per element
      KS_NCCL(ncclGroupStart());
      for (size_t p = 0; p < P.neigh.size(); ++p) {
        const int64_t sc = P.send_ptr[p + 1] - P.send_ptr[p], rc = P.recv_ptr[p + 1] - P.recv_ptr[p];
        if (sc > 0) {
          const D* src = P.send_first[p] >= 0 ? x + P.send_first[p] : sendbuf + P.pack_ptr[p];
          KS_NCCL(ncclSend(src, (size_t)sc * dpe, ncclDouble, P.neigh[p], ctx->comm, s));
        }
        if (rc > 0) KS_NCCL(ncclRecv(ghost + P.recv_ptr[p], (size_t)rc * dpe, ncclDouble, P.neigh[p], ctx->comm, s));
      }
      KS_NCCL(ncclGroupEnd());
    }
    return {hf, xg};
  }
};

}  // namespace
