// Product of operators  y = ops[0] ops[1] ... ops[k-1] x  (ks_operator_product, include/kschur.h): what the reference's recipes for
// generalized problems compose out of LinearMaps -- x -> (A - sigma B)^-1 (B x), docs/src/index.md:273-287, and x -> L^-1 A L^-* x,
// docs/src/index.md:325-336 -- with every intermediate vector resident in HBM.
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip after ks_tridiag.hpp.
//
// The factors are BORROWED (the caller keeps them alive; the same one may appear more than once) and run right to left on
// ctx->stream with the DevState of the batch, so a breakdown skips them all.  Between two factors the vector lives in one of at most
// two ping-pong vectors the product owns: x is a basis column and comes back untouched, y is only written by ops[0].  An
// intermediate is allocated like a basis column -- a multiple of 64 elements, zero-filled once: the stored-matrix kernels may read
// the pad rows of their input, and every factor writes rows < n_local only, so the pad stays zero.
#pragma once

namespace {

struct ProductOp : ks_operator {
  std::vector<ks_operator*> ops;          // mathematical order: ops.back() is applied first
  void* tmp[2] = {nullptr, nullptr};
  ~ProductOp() override { (void)hipFree(tmp[0]); (void)hipFree(tmp[1]); }
  // (no ProfScope: the factors book their own time and bytes)
  void apply(const void* x, void* y, const DevState* st) override {
    const int k = (int)ops.size();
    const void* in = x;
    for (int i = k - 1; i >= 0; --i) {
      void* out = i == 0 ? y : tmp[(k - 1 - i) & 1];
      ops[i]->in_scale = in_scale;  // a host-callback factor scales its input and unscales its result: linear, the product does not depend on it
      ops[i]->apply(in, out, st);
      in = out;
    }
  }
};

inline ks_operator* make_product(ks_ctx* ctx, int nops, ks_operator* const* ops) {
  auto op = std::make_unique<ProductOp>();
  op->ctx = ctx;
  for (int i = 0; i < nops; ++i) {
    const ks_operator* f = ops[i];
    const std::string who = "ks_operator_product: factor " + std::to_string(i);
    KS_REQUIRE(f, KS_ERR_ARGUMENT, who + " is null");
    KS_REQUIRE(f->ctx == ctx, KS_ERR_ARGUMENT, who + " lives on another context");
    KS_REQUIRE(f->n_local == ops[0]->n_local, KS_ERR_ARGUMENT,
               who + " has " + std::to_string(f->n_local) + " rows, factor 0 has " + std::to_string(ops[0]->n_local));
    KS_REQUIRE(f->dtype == ops[0]->dtype, KS_ERR_ARGUMENT, who + " does not have the element type of factor 0");
    op->async_capable = op->async_capable && f->async_capable;
    op->nnz += f->nnz;
    op->ops.push_back(ops[i]);
  }
  op->n_local = ops[0]->n_local;
  op->dtype = ops[0]->dtype;
  const size_t bytes = (size_t)std::max<int64_t>(round_up(op->n_local, 64), 64) * (op->dtype == KS_F64 ? 8 : 16);
  for (int t = 0; t < (nops > 2 ? 2 : 1); ++t) {
    KS_HIP(hipMalloc(&op->tmp[t], bytes));
    KS_HIP(hipMemset(op->tmp[t], 0, bytes));
  }
  return op.release();
}

}  // namespace
