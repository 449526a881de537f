// Column sums of a [B, N] float32 matrix in the pass that does an entry's element-wise work, in a fixed order (no float
// atomics; the order depends on B and N only and is pinned by tests/test_colsum_order_gpu.py):
//   first stage   a workgroup of 256 threads = TY rows x TX float4 columns owns rows_per_block(N) rows.  Thread row ty starts
//                 from 0.0f and adds the rows ty, ty + TY, ... of its block; the block's sum of a column is red[0] + red[1]
//                 + ... + red[TY - 1], left to right, and goes to partial[row block][N].  A kernel with two sums per
//                 column (the head backward, mlp_epilogue.hip) keeps both in this order: partial[row block][2][N].
//   second stage  colsum_partials_kernel (mlp_epilogue.hip): wave w of 4 adds the blocks w, w + 4, ...; the result is
//                 ((a0 + a1) + a2) + a3.  A captured backward, and an eager one that defers (modules/mlp.py _EagerFinish),
//                 finish all their layers with one multi_chunk_sum instead, which keeps this order (TBE_CHUNKS_WAVE_ORDER).
// The kernels that keep a whole row in registers (rowreg.hpp: row sums, a first stage of their own) use this second stage.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.hpp"

namespace tbe {

// rows per workgroup of the first stage: wide layers have the column tiles to fill the chip with 256-row blocks (4x fewer partials)
__host__ __device__ inline int rows_per_block(int N) { return N >= 512 ? 256 : 64; }
inline int64_t colsum_row_blocks(int64_t B, int N) { return (B + rows_per_block(N) - 1) / rows_per_block(N); }
inline size_t colsum_workspace_bytes(int64_t B, int N) {
  if (B <= 0 || N <= 0) return 256;
  return align_up(static_cast<size_t>(colsum_row_blocks(B, N)) * N * sizeof(float), 256);
}

__device__ __forceinline__ void add4(float4& a, const float4 b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// First stage of a kernel with grid = (column tiles, row blocks) that keeps NS sums per column, each in the order above:
// body(row, row * N + column, sum) does one float4 of one row and adds its addends to sum[0 .. NS).  It captures the kernel's
// own __restrict__ parameters, which let the four unrolled rows' loads go first.  The row block's sums go to
// partial[row block][NS][N]: one second stage over NS * N columns finishes all of them.  LDS: NS * 4 KB.
template <int TX, int NS, typename RowBody>
__device__ __forceinline__ void colsum_row_block_n(float* __restrict__ partial, int64_t B, int N, RowBody body) {
  constexpr int TY = 256 / TX;
  __shared__ float4 red[NS][TY][TX];
  const int tx = threadIdx.x % TX;
  const int ty = threadIdx.x / TX;
  const int col = (blockIdx.x * TX + tx) * 4;
  const int64_t row0 = static_cast<int64_t>(blockIdx.y) * rows_per_block(N);
  const int64_t row1 = min(B, row0 + rows_per_block(N));
  float4 sum[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) sum[s] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col < N) {
#pragma unroll 4
    for (int64_t r = row0 + ty; r < row1; r += TY) body(r, r * N + col, sum);
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) red[s][ty][tx] = sum[s];
  __syncthreads();
  if (ty == 0 && col < N) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      float4 a = red[s][0][tx];
#pragma unroll
      for (int y = 1; y < TY; ++y) add4(a, red[s][y][tx]);
      st4(partial + (static_cast<int64_t>(blockIdx.y) * NS + s) * N + col, a);
    }
  }
}

// The one-sum form: body(row, row * N + column, float4& sum).
template <int TX, typename RowBody>
__device__ __forceinline__ void colsum_row_block(float* __restrict__ partial, int64_t B, int N, RowBody body) {
  colsum_row_block_n<TX, 1>(partial, B, N, [&](int64_t r, int64_t o, float4(&sum)[1]) { body(r, o, sum[0]); });
}

// launch(std::integral_constant<int, TX>, grid) for the TX of N: 64, 32 or 16 float4 columns per workgroup
template <typename Launch>
void colsum_dispatch(int N, int64_t row_blocks, Launch launch) {
  const int vecs = N / 4;
  const auto grid = [&](int tx) { return dim3((vecs + tx - 1) / tx, static_cast<unsigned>(row_blocks)); };
  if (vecs >= 64) return launch(std::integral_constant<int, 64>{}, grid(64));
  if (vecs >= 32) return launch(std::integral_constant<int, 32>{}, grid(32));
  launch(std::integral_constant<int, 16>{}, grid(16));
}

// Validates the arguments of entry `name` and launches its first stage through `launch` (see colsum_dispatch); *row_blocks
// = rows of `partial` written.  `tensors`: the [B, N] arrays, which like `partial` move as float4.  A one-pass entry (the
// finish follows) takes an empty batch (*row_blocks = 0, nothing launched) and a workspace of colsum_workspace_bytes; a
// first stage alone needs B > 0 and its [row blocks, N] floats.
template <typename Launch>
int colsum_first_stage(const char* name, bool one_pass, int64_t B, int N, std::initializer_list<const void*> tensors,
                       void* partial, size_t partial_bytes, int64_t* row_blocks, Launch launch) {
  TBE_REQUIRE(B >= (one_pass ? 0 : 1) && N > 0 && (N & 3) == 0, "%s: B=%lld must be %s and N=%d a positive multiple of 4", name,
              (long long)B, one_pass ? ">= 0" : "> 0", N);
  *row_blocks = 0;
  if (B == 0) return TBE_OK;
  int rc = check_pointers(name, {partial});
  if (rc == TBE_OK) rc = check_pointers(name, tensors);
  if (rc != TBE_OK) return rc;
  const int64_t nrb = colsum_row_blocks(B, N);
  TBE_REQUIRE(nrb <= 65535, "%s: B=%lld too large (more than 65535 row blocks)", name, (long long)B);
  const size_t need = one_pass ? colsum_workspace_bytes(B, N) : static_cast<size_t>(nrb) * N * sizeof(float);
  TBE_REQUIRE(partial_bytes >= need, "%s: workspace of the row-block sums too small (%zu bytes, %zu needed)", name,
              partial_bytes, need);
  colsum_dispatch(N, nrb, launch);
  TBE_CHECK_LAUNCH(name);
  *row_blocks = nrb;
  return TBE_OK;
}

// The second stage (mlp_epilogue.hip): out[c] = sum over the `row_blocks` rows of partial[row_blocks][N]; zeros for no rows.
int launch_colsum_partials(const char* name, const float* partial, int64_t row_blocks, int N, float* out, hipStream_t st);

}  // namespace tbe
