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
// The row-in-registers scheme of rowreg.hpp (geometry, slot addressing, row sums, the finish of the column sums, the host side
// of an entry); this file holds the arithmetic and the rule of N.  Threads per row (TPR) and rows per workgroup by N:
//   N <= 64           TPR = 16:  16 rows of the workgroup in flight, one float4 slot per thread, 128 rows per workgroup
//   64 < N <= 1024    TPR = 64:  a wave per row, four rows in flight, 1 ... 4 slots,             32 rows per workgroup
//   1024 < N <= 4096  TPR = 256: the workgroup per row, 2 ... 4 slots,                           16 rows per workgroup
// The column sums (the parameter gradients) go to partial[row block][2][N]: gamma row, beta row.  Every order depends on
// (B, N) only and is pinned (tests/test_rowreg_order_gpu.py), so two runs are bit-identical.
#include <cmath>

#include "rowreg.hpp"

namespace tbe {

__host__ __device__ constexpr int sln_rows_per_block(int tpr) { return tpr == 16 ? 128 : tpr == 64 ? 32 : 16; }
static int sln_tpr(int N) { return N <= 16 * 4 ? 16 : N <= 64 * kRowSlots * 4 ? 64 : 256; }
template <int TPR>
using SlnTile = RowTile<TPR, sln_rows_per_block(TPR)>;

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

// stats: [2, B] — mean, then rstd.
template <int TPR>
__global__ __launch_bounds__(256) void swish_layernorm_fwd_kernel(const float* __restrict__ yg, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float eps,
                                                                  float* __restrict__ out, float* __restrict__ stats,
                                                                  int64_t B, int N) {
  SlnTile<TPR> t(B, N);
  const float fn = static_cast<float>(N);
  float4 ga[kRowSlots], be[kRowSlots];
  t.load(gamma, ga);
  t.load(beta, be);
  t.for_rows([&](int64_t r) {
    float4 y[kRowSlots];
    t.load(yg + r * N, y);
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < kRowSlots; ++k) part = sum4(y[k], part);  // columns beyond N hold zeros
    const float mean = t.sum(part) / fn;
    part = 0.f;
    t.for_slots([&](int k, int) {
      const float4 d = make_float4(y[k].x - mean, y[k].y - mean, y[k].z - mean, y[k].w - mean);
      part = sum4(make_float4(d.x * d.x, d.y * d.y, d.z * d.z, d.w * d.w), part);
    });
    const float var = t.sum(part) / fn;
    const float rstd = 1.f / sqrtf(var + eps);
    if (t.lane == 0) {
      stats[r] = mean;
      stats[B + r] = rstd;
    }
    t.for_slots([=, &y, &ga, &be](int k, int col) {
      float4 n, s;
      norm_sigmoid(y[k], mean, rstd, ga[k], be[k], n, s);
      st4(out + r * N + col, make_float4(y[k].x * s.x, y[k].y * s.y, y[k].z * s.z, y[k].w * s.w));
    });
  });
}

// partial: [row blocks][2][N] — row 0 the gamma gradient, row 1 the beta gradient of the row block.
template <int TPR>
__global__ __launch_bounds__(256) void swish_layernorm_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ yg,
                                                                  const float* __restrict__ stats,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float* __restrict__ gin,
                                                                  float* __restrict__ partial, int64_t B, int N) {
  SlnTile<TPR> t(B, N);
  const float fn = static_cast<float>(N);
  float4 ga[kRowSlots], be[kRowSlots], sums[2][kRowSlots];  // sums: of dz * n (gamma), of dz (beta)
  t.load(gamma, ga);
  t.load(beta, be);
#pragma unroll
  for (int k = 0; k < kRowSlots; ++k) sums[0][k] = sums[1][k] = make_float4(0.f, 0.f, 0.f, 0.f);
  t.for_rows([&](int64_t r) {
    const float mean = stats[r];
    const float rstd = stats[B + r];
    float4 n[kRowSlots], dn[kRowSlots], gs[kRowSlots];
    float p1 = 0.f, p2 = 0.f;
    // a plain loop over the slots, not t.for_slots: with these statements in a lambda the compiler schedules the body otherwise
    // and the TPR = 256 kernel measured 5 ... 8 % slower (N = 2048, 4096)
#pragma unroll
    for (int k = 0; k < kRowSlots; ++k) {
      n[k] = dn[k] = gs[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t.has(k)) {
        const float4 y = ld4(yg + r * N + t.col(k));
        const float4 g = ld4(gout + r * N + t.col(k));
        float4 s;
        norm_sigmoid(y, mean, rstd, ga[k], be[k], n[k], s);
        const float4 dz = make_float4(((g.x * y.x) * s.x) * (1.f - s.x), ((g.y * y.y) * s.y) * (1.f - s.y),
                                      ((g.z * y.z) * s.z) * (1.f - s.z), ((g.w * y.w) * s.w) * (1.f - s.w));
        gs[k] = make_float4(g.x * s.x, g.y * s.y, g.z * s.z, g.w * s.w);
        dn[k] = make_float4(dz.x * ga[k].x, dz.y * ga[k].y, dz.z * ga[k].z, dz.w * ga[k].w);
        add4(sums[0][k], make_float4(dz.x * n[k].x, dz.y * n[k].y, dz.z * n[k].z, dz.w * n[k].w));
        add4(sums[1][k], dz);
      }
      p1 = sum4(dn[k], p1);  // columns beyond N hold zeros
      p2 = sum4(make_float4(dn[k].x * n[k].x, dn[k].y * n[k].y, dn[k].z * n[k].z, dn[k].w * n[k].w), p2);
    }
    const float c1 = t.sum(p1) / fn;
    const float c2 = t.sum(p2) / fn;
    t.for_slots([=, &n, &dn, &gs](int k, int col) {
      const float4 d = dn[k], nn = n[k];
      st4(gin + r * N + col,
          make_float4(gs[k].x + rstd * ((d.x - c1) - nn.x * c2), gs[k].y + rstd * ((d.y - c1) - nn.y * c2),
                      gs[k].z + rstd * ((d.z - c1) - nn.z * c2), gs[k].w + rstd * ((d.w - c1) - nn.w * c2)));
    });
  });
  t.finish(sums, partial);
}

// The limits shared by the two entries; *tpr = threads per row, *nrb = row blocks (grid size).
static int sln_limits(const char* name, int64_t B, int N, int* tpr, int64_t* nrb) {
  *tpr = sln_tpr(N);
  return rowreg_limits(name, B, N, sln_rows_per_block(*tpr), nrb);
}

}  // namespace tbe

using namespace tbe;

extern "C" size_t tbe_swish_layernorm_backward_workspace_bytes(int64_t B, int32_t N) {
  if (B <= 0) return rowreg_workspace_bytes(0, 2, N);
  const int rpb = sln_rows_per_block(sln_tpr(N));
  return rowreg_workspace_bytes((B + rpb - 1) / rpb, 2, N);
}

extern "C" int tbe_swish_layernorm_forward_f32(const float* y, const float* gamma, const float* beta, float eps, int64_t B,
                                               int32_t N, float* out, float* stats, void* stream) {
  const char* name = "tbe_swish_layernorm_forward_f32";
  int tpr;
  int64_t nrb;
  const int rc = sln_limits(name, B, N, &tpr, &nrb);
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(std::isfinite(eps) && eps >= 0.f, "%s: eps=%g must be finite and >= 0", name, static_cast<double>(eps));
  hipStream_t st = static_cast<hipStream_t>(stream);
  return rowreg_run(name, B, N, nrb, {y, gamma, beta, out}, {stats}, nullptr, st, [&](dim3 grid) {
    dispatch_value<16, 64, 256>(tpr, [&](auto t) {
      hipLaunchKernelGGL(swish_layernorm_fwd_kernel<decltype(t)::value>, grid, dim3(256), 0, st, y, gamma, beta, eps, out, stats,
                         B, N);
    });
  });
}

extern "C" int tbe_swish_layernorm_backward_f32(const float* grad_out, const float* y, const float* stats, const float* gamma,
                                                const float* beta, int64_t B, int32_t N, float* grad_y, float* grad_params,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "tbe_swish_layernorm_backward_f32";
  int tpr;
  int64_t nrb;
  const int rc = sln_limits(name, B, N, &tpr, &nrb);
  if (rc != TBE_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RowColSums cs{2, grad_params, workspace, workspace_bytes};
  return rowreg_run(name, B, N, nrb, {grad_out, y, gamma, beta, grad_y}, {stats}, &cs, st, [&](dim3 grid) {
    dispatch_value<16, 64, 256>(tpr, [&](auto t) {
      hipLaunchKernelGGL(swish_layernorm_bwd_kernel<decltype(t)::value>, grid, dim3(256), 0, st, grad_out, y, stats, gamma, beta,
                         grad_y, static_cast<float*>(workspace), B, N);
    });
  });
}
