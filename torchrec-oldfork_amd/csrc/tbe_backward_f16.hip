// TBE backward + fused optimizer, FP16 tables: the tbe_backward_*_f16w entry points (kernels:
// tbe_backward_impl.hpp).  The gradient-independent phase (linearize + sort) never touches the
// tables, so the fused entry runs the shared tbe_backward_prepare and then its own apply phase.
#include "tbe_backward_impl.hpp"

using namespace tbe;

static int apply_f16(
    const char* who, const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window, int32_t rounding, uint64_t seed,
    void* stream, bool fused, bool ex = false, const tbe_optimizer_ext* ext = nullptr) {
  TBE_REQUIRE(rounding == TBE_ROUND_NEAREST_EVEN || rounding == TBE_ROUND_STOCHASTIC, "%s: rounding %d", who, rounding);
  if (opt.optimizer == TBE_OPT_DENSE_GRAD) {
    set_error("%s: TBE_OPT_DENSE_GRAD is not supported with FP16 tables (dense parameters are float)", who);
    return TBE_ERR_UNSUPPORTED;
  }
  if (fused && per_sample_weights != nullptr) flags |= TBE_FLAG_WEIGHTED;
  BwdArgs a;
  BwdWorkspace w;
  bool wide = false, done = false;
  const int rc = bwd_setup(who, feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base, feat_state0, feat_state1,
                           F, B, max_D, key_bits, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling,
                           grad_out, grad_row_stride, opt, flags, workspace, workspace_bytes, bounds_errors, feat_window,
                           kPhaseApply, &a, &w, &wide, &done, ex, ext);
  if (rc != TBE_OK || done) return rc;
  a.rounding = rounding;
  a.round_hash = call_hash(seed, opt.iteration);
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfileSpan total_span(TBE_PROFILE_BWD_TOTAL, st);
  if (fused) {
    const int prc = tbe_backward_prepare(feat_rows, feat_row_base, F, B, max_D, key_bits, indices, N, offsets,
                                         pooling_mode, flags, workspace, workspace_bytes, bounds_errors, feat_window,
                                         stream);
    if (prc != TBE_OK) return prc;
  }
  if (key_bits > 32)
    return wide ? run_apply<_Float16, uint64_t, uint64_t>(a, max_D, st) : run_apply<_Float16, uint64_t, uint32_t>(a, max_D, st);
  return wide ? run_apply<_Float16, uint32_t, uint64_t>(a, max_D, st) : run_apply<_Float16, uint32_t, uint32_t>(a, max_D, st);
}

extern "C" int tbe_backward_fused_f16w(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window, int32_t rounding, uint64_t seed,
    void* stream) {
  return apply_f16("tbe_backward_fused_f16w", feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base,
                   feat_state0, feat_state1, F, B, max_D, key_bits, indices, N, offsets, per_sample_weights, pooling_mode,
                   feat_pooling, grad_out, grad_row_stride, opt, flags, workspace, workspace_bytes, bounds_errors,
                   feat_window, rounding, seed, stream, true);
}

extern "C" int tbe_backward_apply_f16w(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, int32_t rounding, uint64_t seed, void* stream) {
  return apply_f16("tbe_backward_apply_f16w", feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base,
                   feat_state0, feat_state1, F, B, max_D, key_bits, indices, N, offsets, per_sample_weights, pooling_mode,
                   feat_pooling, grad_out, grad_row_stride, opt, flags, workspace, workspace_bytes, nullptr, nullptr,
                   rounding, seed, stream, false);
}

// The twins that also take the row-norm optimizer family and gradient clipping (include/tbe_hip.h).
extern "C" int tbe_backward_fused_ex_f16w(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window, int32_t rounding, uint64_t seed,
    const tbe_optimizer_ext* ext, void* stream) {
  return apply_f16("tbe_backward_fused_ex_f16w", feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base,
                   feat_state0, feat_state1, F, B, max_D, key_bits, indices, N, offsets, per_sample_weights, pooling_mode,
                   feat_pooling, grad_out, grad_row_stride, opt, flags, workspace, workspace_bytes, bounds_errors,
                   feat_window, rounding, seed, stream, true, true, ext);
}

extern "C" int tbe_backward_apply_ex_f16w(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, int32_t rounding, uint64_t seed, const tbe_optimizer_ext* ext, void* stream) {
  return apply_f16("tbe_backward_apply_ex_f16w", feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base,
                   feat_state0, feat_state1, F, B, max_D, key_bits, indices, N, offsets, per_sample_weights, pooling_mode,
                   feat_pooling, grad_out, grad_row_stride, opt, flags, workspace, workspace_bytes, nullptr, nullptr,
                   rounding, seed, stream, false, true, ext);
}
