// TBE backward + fused optimizer, FP16 tables: the tbe_backward_*_f16w entry points, backward_entry<_Float16> of
// tbe_backward_impl.hpp in a translation unit of its own.
#include "tbe_backward_impl.hpp"

using namespace tbe;

extern "C" int tbe_backward_fused_f16w(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window, int32_t rounding, uint64_t seed,
    void* stream) {
  BwdCall c{feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base, feat_state0, feat_state1, F, B, max_D,
            key_bits, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling, grad_out, grad_row_stride,
            opt, flags, workspace, workspace_bytes};
  c.stream = stream;
  c.who = "tbe_backward_fused_f16w";
  c.phase = kPhasePrepare | kPhaseApply;
  c.rounding = rounding;
  c.seed = seed;
  c.bounds_errors = bounds_errors;
  c.feat_window = feat_window;
  return backward_entry<_Float16>(c);
}

extern "C" int tbe_backward_apply_f16w(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, int32_t rounding, uint64_t seed, void* stream) {
  BwdCall c{feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base, feat_state0, feat_state1, F, B, max_D,
            key_bits, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling, grad_out, grad_row_stride,
            opt, flags, workspace, workspace_bytes};
  c.stream = stream;
  c.who = "tbe_backward_apply_f16w";
  c.phase = kPhaseApply;
  c.rounding = rounding;
  c.seed = seed;
  return backward_entry<_Float16>(c);
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
  BwdCall c{feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base, feat_state0, feat_state1, F, B, max_D,
            key_bits, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling, grad_out, grad_row_stride,
            opt, flags, workspace, workspace_bytes};
  c.stream = stream;
  c.who = "tbe_backward_fused_ex_f16w";
  c.phase = kPhasePrepare | kPhaseApply;
  c.rounding = rounding;
  c.seed = seed;
  c.bounds_errors = bounds_errors;
  c.feat_window = feat_window;
  c.ex = true;
  c.ext = ext;
  return backward_entry<_Float16>(c);
}

extern "C" int tbe_backward_apply_ex_f16w(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, int32_t rounding, uint64_t seed, const tbe_optimizer_ext* ext, void* stream) {
  BwdCall c{feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base, feat_state0, feat_state1, F, B, max_D,
            key_bits, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling, grad_out, grad_row_stride,
            opt, flags, workspace, workspace_bytes};
  c.stream = stream;
  c.who = "tbe_backward_apply_ex_f16w";
  c.phase = kPhaseApply;
  c.rounding = rounding;
  c.seed = seed;
  c.ex = true;
  c.ext = ext;
  return backward_entry<_Float16>(c);
}
