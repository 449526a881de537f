// SwishLayerNorm on gfx950:  out = y * sigmoid(LayerNorm(y))  over the last N elements of every row, one pass each way.
//
// Reference: torchrec/modules/activation.py:18-55 — `input * Sequential(LayerNorm, Sigmoid)(input)` — trained through
// autograd.  As torch runs it the forward is three HBM-bound kernels (layer norm, sigmoid, multiply) and the backward a chain
// of six or more, with sigmoid(...) kept as a second [B, N] tensor.  Here the row lives in registers: the forward reads y and
// writes out, the backward reads grad_out and y and writes grad_y; two floats per row (mean, rstd) are kept in between.
//
// Per row b, float32, each product and add rounded on its own (the Makefile builds with -ffp-contract=off; no fmaf here):
//   forward   mean = (sum_c y[c]) / N;   var = (sum_c (y[c] - mean)^2) / N   (two-pass: never E[y^2] - mean^2)
//             rstd = 1 / sqrtf(var + eps)
//             n = (y - mean) * rstd;  z = n * gamma + beta;  s = 1 / (1 + expf(-z));  out = y * s
//   backward  n, z, s recomputed from y, mean, rstd in the forward's operation order;  g = grad_out
//             dz = ((g * y) * s) * (1 - s);   dn = dz * gamma
//             c1 = (sum_c dn) / N;            c2 = (sum_c dn * n) / N
//             grad_y = g * s + rstd * ((dn - c1) - n * c2)
//             grad_gamma = sum_b dz * n;      grad_beta = sum_b dz
// A constant row has var = 0, n = 0, rstd = 1 / sqrtf(eps); |z| beyond expf's range gives s = exactly 0 or 1 (1 / inf = 0,
// 1 / (1 + 0) = 1) and no inf * 0 anywhere, since s itself is finite.
//
// Threads per row (TPR) by N — thread `lane` of a row holds the float4 columns lane, lane + TPR, ... (at most kSlnK = 4):
//   N <= 64           TPR = 16:  16 rows of the workgroup in flight, one float4 slot per thread, 128 rows per workgroup
//   64 < N <= 1024    TPR = 64:  a wave per row, four rows in flight, 1 ... 4 slots,             32 rows per workgroup
//   1024 < N <= 4096  TPR = 256: the workgroup per row, 2 ... 4 slots,                           16 rows per workgroup
// Row sums: every thread adds its own elements from 0.0f in slot order (x, y, z, w inside a float4), then row_sum<TPR>
// (colsum.hpp): xor butterfly, then wave order through LDS.  Column sums (the parameter gradients): thread (sub, lane) adds
// the rows sub, sub + 256 / TPR, ... of its row block from 0.0f; the block's sum is that of sub = 0, 1, ... left to right
// (LDS); partial[row block][2][N] (gamma row, beta row) is finished by ONE colsum_partials launch over 2 N columns
// (colsum.hpp, second stage).  No float atomics; every order depends on (B, N) only, so two runs are bit-identical.
#include <cmath>

#include "colsum.hpp"

namespace tbe {

constexpr int kSlnMaxN = 4096;
constexpr int kSlnK = 4;  // float4 slots per thread

__host__ __device__ constexpr int sln_rows_per_block(int tpr) { return tpr == 16 ? 128 : tpr == 64 ? 32 : 16; }
static int sln_tpr(int N) { return N <= 16 * 4 ? 16 : N <= 64 * kSlnK * 4 ? 64 : 256; }
static int64_t sln_row_blocks(int64_t B, int N) {
  const int rpb = sln_rows_per_block(sln_tpr(N));
  return (B + rpb - 1) / rpb;
}

__device__ __forceinline__ float sum4(const float4 a, float acc) {
  acc += a.x;
  acc += a.y;
  acc += a.z;
  acc += a.w;
  return acc;
}

__device__ __forceinline__ float sigmoid1(const float z) { return 1.f / (1.f + expf(-z)); }

// n = (y - mean) * rstd;  s = sigmoid(n * gamma + beta)
__device__ __forceinline__ void norm_sigmoid(const float4 y, const float mean, const float rstd, const float4 ga,
                                             const float4 be, float4& n, float4& s) {
  n = make_float4((y.x - mean) * rstd, (y.y - mean) * rstd, (y.z - mean) * rstd, (y.w - mean) * rstd);
  s = make_float4(sigmoid1(n.x * ga.x + be.x), sigmoid1(n.y * ga.y + be.y), sigmoid1(n.z * ga.z + be.z),
                  sigmoid1(n.w * ga.w + be.w));
}

// grid = row blocks of sln_rows_per_block(TPR) rows.  stats: [2, B] — mean, then rstd.
template <int TPR>
__global__ __launch_bounds__(256) void swish_layernorm_fwd_kernel(const float* __restrict__ yg, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float eps,
                                                                  float* __restrict__ out, float* __restrict__ stats,
                                                                  int64_t B, int N) {
  __shared__ float red[2][4];
  int phase = 0;
  constexpr int RP = 256 / TPR;  // rows in flight per block
  const int lane = threadIdx.x % TPR;
  const int sub = threadIdx.x / TPR;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * sln_rows_per_block(TPR);
  const int64_t row1 = min(B, row0 + sln_rows_per_block(TPR));
  const float fn = static_cast<float>(N);
  float4 ga[kSlnK], be[kSlnK];
#pragma unroll
  for (int k = 0; k < kSlnK; ++k) {
    const int col = (k * TPR + lane) * 4;
    ga[k] = col < N ? ld4(gamma + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    be[k] = col < N ? ld4(beta + col) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // the trip count is the same for every thread that meets at a barrier (TPR = 256: sub = 0 everywhere; else no barrier)
  for (int64_t r = row0 + sub; r < row1; r += RP) {
    float4 y[kSlnK];
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < kSlnK; ++k) {
      const int col = (k * TPR + lane) * 4;
      y[k] = col < N ? ld4(yg + r * N + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      part = sum4(y[k], part);  // columns beyond N hold zeros
    }
    const float mean = row_sum<TPR>(part, red, phase) / fn;
    part = 0.f;
#pragma unroll
    for (int k = 0; k < kSlnK; ++k) {
      const int col = (k * TPR + lane) * 4;
      if (col < N) {
        const float4 d = make_float4(y[k].x - mean, y[k].y - mean, y[k].z - mean, y[k].w - mean);
        part = sum4(make_float4(d.x * d.x, d.y * d.y, d.z * d.z, d.w * d.w), part);
      }
    }
    const float var = row_sum<TPR>(part, red, phase) / fn;
    const float rstd = 1.f / sqrtf(var + eps);
    if (lane == 0) {
      stats[r] = mean;
      stats[B + r] = rstd;
    }
#pragma unroll
    for (int k = 0; k < kSlnK; ++k) {
      const int col = (k * TPR + lane) * 4;
      if (col < N) {
        float4 n, s;
        norm_sigmoid(y[k], mean, rstd, ga[k], be[k], n, s);
        st4(out + r * N + col, make_float4(y[k].x * s.x, y[k].y * s.y, y[k].z * s.z, y[k].w * s.w));
      }
    }
  }
}

// partial: [row blocks][2][N] — row 0 the gamma gradient, row 1 the beta gradient of the row block.
template <int TPR>
__global__ __launch_bounds__(256) void swish_layernorm_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ yg,
                                                                  const float* __restrict__ stats,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float* __restrict__ gin,
                                                                  float* __restrict__ partial, int64_t B, int N) {
  __shared__ float red[2][4];
  __shared__ float4 fin[256];  // [RP][TPR]
  int phase = 0;
  constexpr int RP = 256 / TPR;
  const int lane = threadIdx.x % TPR;
  const int sub = threadIdx.x / TPR;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * sln_rows_per_block(TPR);
  const int64_t row1 = min(B, row0 + sln_rows_per_block(TPR));
  const float fn = static_cast<float>(N);
  float4 ga[kSlnK], be[kSlnK], sum_g[kSlnK], sum_b[kSlnK];
#pragma unroll
  for (int k = 0; k < kSlnK; ++k) {
    const int col = (k * TPR + lane) * 4;
    ga[k] = col < N ? ld4(gamma + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    be[k] = col < N ? ld4(beta + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    sum_g[k] = sum_b[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int64_t r = row0 + sub; r < row1; r += RP) {
    const float mean = stats[r];
    const float rstd = stats[B + r];
    float4 n[kSlnK], dn[kSlnK], gs[kSlnK];
    float p1 = 0.f, p2 = 0.f;
#pragma unroll
    for (int k = 0; k < kSlnK; ++k) {
      const int col = (k * TPR + lane) * 4;
      n[k] = dn[k] = gs[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (col < N) {
        const float4 y = ld4(yg + r * N + col);
        const float4 g = ld4(gout + r * N + col);
        float4 s;
        norm_sigmoid(y, mean, rstd, ga[k], be[k], n[k], s);
        const float4 dz = make_float4(((g.x * y.x) * s.x) * (1.f - s.x), ((g.y * y.y) * s.y) * (1.f - s.y),
                                      ((g.z * y.z) * s.z) * (1.f - s.z), ((g.w * y.w) * s.w) * (1.f - s.w));
        gs[k] = make_float4(g.x * s.x, g.y * s.y, g.z * s.z, g.w * s.w);
        dn[k] = make_float4(dz.x * ga[k].x, dz.y * ga[k].y, dz.z * ga[k].z, dz.w * ga[k].w);
        add4(sum_g[k], make_float4(dz.x * n[k].x, dz.y * n[k].y, dz.z * n[k].z, dz.w * n[k].w));
        add4(sum_b[k], dz);
      }
      p1 = sum4(dn[k], p1);  // columns beyond N hold zeros
      p2 = sum4(make_float4(dn[k].x * n[k].x, dn[k].y * n[k].y, dn[k].z * n[k].z, dn[k].w * n[k].w), p2);
    }
    const float c1 = row_sum<TPR>(p1, red, phase) / fn;
    const float c2 = row_sum<TPR>(p2, red, phase) / fn;
#pragma unroll
    for (int k = 0; k < kSlnK; ++k) {
      const int col = (k * TPR + lane) * 4;
      if (col < N) {
        const float4 d = dn[k], nn = n[k];
        st4(gin + r * N + col,
            make_float4(gs[k].x + rstd * ((d.x - c1) - nn.x * c2), gs[k].y + rstd * ((d.y - c1) - nn.y * c2),
                        gs[k].z + rstd * ((d.z - c1) - nn.z * c2), gs[k].w + rstd * ((d.w - c1) - nn.w * c2)));
      }
    }
  }
  // the row block's column sums: TPR = 256 — every thread owns its columns alone; else the RP thread groups hold the sums of
  // the rows sub, sub + RP, ... and are added in `sub` order through LDS
  float* pb = partial + static_cast<int64_t>(blockIdx.x) * 2 * N;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int k = 0; k < kSlnK; ++k) {
      const int col = (k * TPR + lane) * 4;
      float4 v = half == 0 ? sum_g[k] : sum_b[k];
      float* dst = pb + static_cast<int64_t>(half) * N + col;
      if constexpr (TPR == 256) {
        if (col < N) st4(dst, v);
      } else {
        if (k * TPR * 4 < N) {  // block-uniform: some lane of this slot holds a column
          __syncthreads();      // the previous round's reads of `fin` are done
          fin[sub * TPR + lane] = v;
          __syncthreads();
          if (sub == 0 && col < N) {
            v = fin[lane];
#pragma unroll
            for (int j = 1; j < RP; ++j) add4(v, fin[j * TPR + lane]);
            st4(dst, v);
          }
        }
      }
    }
  }
}

// Limits shared by the two entries; *nrb = row blocks (grid size).
static int sln_limits(const char* name, int64_t B, int N, int64_t* nrb) {
  TBE_REQUIRE(B >= 0 && N > 0 && (N & 3) == 0, "%s: B=%lld must be >= 0 and N=%d a positive multiple of 4", name, (long long)B, N);
  TBE_REQUIRE(N <= kSlnMaxN, "%s: N=%d beyond the limit N <= %d", name, N, kSlnMaxN);
  *nrb = sln_row_blocks(B, N);
  TBE_REQUIRE(*nrb < (1ll << 31), "%s: B=%lld too large (more than 2^31 - 1 row blocks)", name, (long long)B);
  return TBE_OK;
}

static bool all_aligned(std::initializer_list<const void*> ptrs, uintptr_t mask) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & mask) == 0;
}

}  // namespace tbe

using namespace tbe;

extern "C" size_t tbe_swish_layernorm_backward_workspace_bytes(int64_t B, int32_t N) {
  if (B <= 0 || N <= 0) return 256;
  return align_up(static_cast<size_t>(sln_row_blocks(B, N)) * 2 * N * sizeof(float), 256);
}

extern "C" int tbe_swish_layernorm_forward_f32(const float* y, const float* gamma, const float* beta, float eps, int64_t B,
                                               int32_t N, float* out, float* stats, void* stream) {
  const char* name = "tbe_swish_layernorm_forward_f32";
  int64_t nrb;
  const int rc = sln_limits(name, B, N, &nrb);
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(std::isfinite(eps) && eps >= 0.f, "%s: eps=%g must be finite and >= 0", name, static_cast<double>(eps));
  if (B == 0) return TBE_OK;
  TBE_REQUIRE(y && gamma && beta && out && stats, "%s: null pointer", name);
  TBE_REQUIRE(all_aligned({y, gamma, beta, out}, 15) && all_aligned({stats}, 3), "%s: tensors must be 16-B aligned (stats: 4 B)", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(nrb));
  switch (sln_tpr(N)) {
    case 16:
      hipLaunchKernelGGL(swish_layernorm_fwd_kernel<16>, grid, dim3(256), 0, st, y, gamma, beta, eps, out, stats, B, N);
      break;
    case 64:
      hipLaunchKernelGGL(swish_layernorm_fwd_kernel<64>, grid, dim3(256), 0, st, y, gamma, beta, eps, out, stats, B, N);
      break;
    default:
      hipLaunchKernelGGL(swish_layernorm_fwd_kernel<256>, grid, dim3(256), 0, st, y, gamma, beta, eps, out, stats, B, N);
  }
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}

extern "C" int tbe_swish_layernorm_backward_f32(const float* grad_out, const float* y, const float* stats, const float* gamma,
                                                const float* beta, int64_t B, int32_t N, float* grad_y, float* grad_params,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "tbe_swish_layernorm_backward_f32";
  int64_t nrb;
  const int rc = sln_limits(name, B, N, &nrb);
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(grad_params != nullptr && all_aligned({grad_params}, 3), "%s: null or misaligned grad_params", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (B == 0) return hipMemsetAsync(grad_params, 0, sizeof(float) * 2 * N, st) == hipSuccess ? TBE_OK : TBE_ERR_LAUNCH;
  TBE_REQUIRE(grad_out && y && stats && gamma && beta && grad_y && workspace, "%s: null pointer", name);
  TBE_REQUIRE(all_aligned({grad_out, y, gamma, beta, grad_y, workspace}, 15) && all_aligned({stats}, 3),
              "%s: tensors must be 16-B aligned (stats, grad_params: 4 B)", name);
  const size_t need = tbe_swish_layernorm_backward_workspace_bytes(B, N);
  TBE_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu bytes, %zu needed)", name, workspace_bytes, need);
  float* partial = static_cast<float*>(workspace);
  const dim3 grid(static_cast<unsigned>(nrb));
  switch (sln_tpr(N)) {
    case 16:
      hipLaunchKernelGGL(swish_layernorm_bwd_kernel<16>, grid, dim3(256), 0, st, grad_out, y, stats, gamma, beta, grad_y,
                         partial, B, N);
      break;
    case 64:
      hipLaunchKernelGGL(swish_layernorm_bwd_kernel<64>, grid, dim3(256), 0, st, grad_out, y, stats, gamma, beta, grad_y,
                         partial, B, N);
      break;
    default:
      hipLaunchKernelGGL(swish_layernorm_bwd_kernel<256>, grid, dim3(256), 0, st, grad_out, y, stats, gamma, beta, grad_y,
                         partial, B, N);
  }
  TBE_CHECK_LAUNCH(name);
  return launch_colsum_partials(name, partial, nrb, 2 * N, grad_params, st);
}
