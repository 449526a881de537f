// permute_pooled_embs: reorders the column segments of a pooled-embedding matrix [B, D_total].
//
// The reference calls the fbgemm op of this name from one place, the column-wise sharding's output-dist callback
// (torchrec/distributed/sharding/cw_sharding.py:221-231, through fbgemm_gpu.permute_pooled_embedding_modules): after the
// pooled all-to-all the column shards of a table arrive grouped by rank, and the permutation puts them back next to each
// other.  Segment i of the OUTPUT is segment permute[i] of the input:
//   out[:, inv_offset[i]:inv_offset[i+1]] = in[:, offset[permute[i]]:offset[permute[i]+1]]
// The backward is the same kernel with (inv_offset, inv_permute, offset) in the three roles.  A pure copy in one launch,
// shaped like pooled_exchange_kernel: the three lists sit in LDS, every element finds its output segment by binary search.
#include <algorithm>

#include "common.hpp"

namespace tbe {

template <int VEC>
__global__ __launch_bounds__(256) void permute_pooled_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            const int64_t* __restrict__ offset,
                                                            const int64_t* __restrict__ permute,
                                                            const int64_t* __restrict__ inv_offset, int32_t T,
                                                            int32_t B, int32_t D_total) {
  extern __shared__ int32_t lds[];
  int32_t* s_inv = lds;          // [T+1] first output column of every output segment
  int32_t* s_src = s_inv + T + 1;  // [T] first input column of the segment that lands there
  for (int i = threadIdx.x; i <= T; i += blockDim.x) s_inv[i] = static_cast<int32_t>(inv_offset[i]);
  for (int i = threadIdx.x; i < T; i += blockDim.x) {
    const int64_t p = permute[i];
    // a list that is no permutation reads nothing out of bounds: the segment is skipped below
    s_src[i] = (p >= 0 && p < T) ? static_cast<int32_t>(offset[p]) : -1;
  }
  __syncthreads();
  const int cols = D_total / VEC;
  const int64_t total = static_cast<int64_t>(B) * cols;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t b = i / cols;
    const int d = static_cast<int>(i - b * cols) * VEC;
    int lo = 0, hi = T;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_inv[mid] <= d) lo = mid; else hi = mid;
    }
    const int src = s_src[lo] + (d - s_inv[lo]);
    if (s_src[lo] < 0 || d < s_inv[lo] || src + VEC > D_total) continue;  // inconsistent lists: never read outside the row
    const int64_t row = b * D_total;
    if (VEC == 4) st4(out + row + d, ld4(in + row + src));
    else out[row + d] = in[row + src];
  }
}

}  // namespace tbe

using namespace tbe;

extern "C" int tbe_permute_pooled_embs_f32(const float* in, float* out, const int64_t* offset_dim_list,
                                           const int64_t* permute_list, const int64_t* inv_offset_dim_list, int32_t T,
                                           int32_t B, int32_t D_total, int32_t all_multiple_of_4, void* stream) {
  TBE_REQUIRE(T > 0 && B >= 0 && D_total >= 0, "tbe_permute_pooled_embs_f32: bad sizes");
  if (static_cast<int64_t>(B) * D_total == 0) return TBE_OK;
  TBE_REQUIRE(in && out && offset_dim_list && permute_list && inv_offset_dim_list,
              "tbe_permute_pooled_embs_f32: null pointer");
  TBE_REQUIRE(in != out, "tbe_permute_pooled_embs_f32: in-place permutation is not supported");
  const size_t lds = (static_cast<size_t>(T) * 2 + 1) * sizeof(int32_t);
  if (lds > 60000) {
    set_error("tbe_permute_pooled_embs_f32: too many segments (%d)", T);
    return TBE_ERR_UNSUPPORTED;
  }
  const bool vec = all_multiple_of_4 && (D_total % 4 == 0) && ((reinterpret_cast<uintptr_t>(in) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  const int64_t total = static_cast<int64_t>(B) * (D_total / (vec ? 4 : 1));
  int64_t g = (total + 255) / 256;
  g = std::max<int64_t>(1, std::min<int64_t>(g, 256 * 32));
  const dim3 grid(static_cast<unsigned>(g));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec) {
    hipLaunchKernelGGL((permute_pooled_kernel<4>), grid, dim3(256), lds, st, in, out, offset_dim_list, permute_list,
                       inv_offset_dim_list, T, B, D_total);
  } else {
    hipLaunchKernelGGL((permute_pooled_kernel<1>), grid, dim3(256), lds, st, in, out, offset_dim_list, permute_list,
                       inv_offset_dim_list, T, B, D_total);
  }
  TBE_CHECK_LAUNCH("permute pooled embs");
  return TBE_OK;
}
