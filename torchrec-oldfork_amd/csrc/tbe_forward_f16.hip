// TBE forward, FP16 tables: the tbe_forward_*_f16w entry points (kernels: tbe_forward_impl.hpp).
// Rows are _Float16, read as 8 B per lane; accumulation and the pooled output stay FP32.
#include "tbe_forward_impl.hpp"

using namespace tbe;

extern "C" int tbe_forward_pooled_f16w(const uint64_t* feat_weights, const int32_t* feat_D,
                                       const int64_t* feat_out_offset, const int64_t* feat_rows,
                                       int32_t F, int32_t B, int32_t max_D,
                                       const int64_t* indices, int64_t N, const int64_t* offsets,
                                       const float* per_sample_weights, int32_t pooling_mode,
                                       const int32_t* feat_pooling, float* out, int64_t out_row_stride,
                                       int32_t* bounds_errors, const int64_t* feat_window, void* stream) {
  return forward_pooled<_Float16>("tbe_forward_pooled_f16w", feat_weights, feat_D, feat_out_offset, feat_rows, F, B,
                                  max_D, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling, out,
                                  out_row_stride, bounds_errors, feat_window, stream);
}

extern "C" int tbe_forward_nobag_f16w(const uint64_t* feat_weights, const int64_t* feat_rows,
                                      int32_t F, int32_t B, int32_t D, const int64_t* indices,
                                      int64_t N, const int64_t* offsets, float* out,
                                      int32_t* bounds_errors, void* stream) {
  return forward_nobag<_Float16>("tbe_forward_nobag_f16w", feat_weights, feat_rows, F, B, D, indices, N, offsets, out,
                                 bounds_errors, stream);
}
