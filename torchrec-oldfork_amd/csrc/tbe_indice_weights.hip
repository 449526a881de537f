// Per-sample-weight gradient of the pooled TBE lookup: the tbe_backward_indice_weights_* entry
// points for FP32 and FP16 tables (kernels: tbe_indice_weights_impl.hpp).
#include "tbe_indice_weights_impl.hpp"

using namespace tbe;

extern "C" int tbe_backward_indice_weights_f32(const uint64_t* feat_weights, const int32_t* feat_D,
                                               const int64_t* feat_out_offset, const int64_t* feat_rows,
                                               int32_t F, int32_t B, int32_t max_D,
                                               const int64_t* indices, int64_t N, const int64_t* offsets,
                                               int32_t pooling_mode, const int32_t* feat_pooling,
                                               const float* grad_out, int64_t grad_row_stride,
                                               const int32_t* feat_requires_grad, float* grad_indice_weights,
                                               const int64_t* feat_window, void* stream) {
  return backward_indice_weights<float>("tbe_backward_indice_weights_f32", feat_weights, feat_D, feat_out_offset,
                                        feat_rows, F, B, max_D, indices, N, offsets, pooling_mode, feat_pooling,
                                        grad_out, grad_row_stride, feat_requires_grad, grad_indice_weights,
                                        feat_window, stream);
}

extern "C" int tbe_backward_indice_weights_f16w(const uint64_t* feat_weights, const int32_t* feat_D,
                                                const int64_t* feat_out_offset, const int64_t* feat_rows,
                                                int32_t F, int32_t B, int32_t max_D,
                                                const int64_t* indices, int64_t N, const int64_t* offsets,
                                                int32_t pooling_mode, const int32_t* feat_pooling,
                                                const float* grad_out, int64_t grad_row_stride,
                                                const int32_t* feat_requires_grad, float* grad_indice_weights,
                                                const int64_t* feat_window, void* stream) {
  return backward_indice_weights<_Float16>("tbe_backward_indice_weights_f16w", feat_weights, feat_D, feat_out_offset,
                                           feat_rows, F, B, max_D, indices, N, offsets, pooling_mode, feat_pooling,
                                           grad_out, grad_row_stride, feat_requires_grad, grad_indice_weights,
                                           feat_window, stream);
}
