// The passes of BERT4Rec's TransformerBlock between its GEMMs and its attention kernel, on gfx950: residual add, the
// dropouts and the pre-norm LayerNorm of the NEXT sublayer in one launch, and relu + dropout of the feed-forward.
//
// Reference: examples/bert4rec/models/bert4rec.py:174-320 — SublayerConnection `x + dropout(sublayer(norm(x)))`, the
// feed-forward `w_2(dropout(relu(w_1(x))))` and the block's final dropout.  As torch runs them a block is about ten
// launch-bound passes over [R, N] forward and more backward, each dropout keeps a mask and each LayerNorm its input.  Here:
//   forward   y = drop_out(x + drop_in(s));   n = (y - mean) * rstd * gamma + beta;   stats[r] = (mean, rstd)
//             the row lives in registers (rowreg.hpp): x and s are read once, y and n written once, two floats per row kept.
//   backward  xhat = (y - mean) * rstd;  d = g_n * gamma;  c1 = mean_row(d);  c2 = mean_row(d * xhat)
//             g = g_y + rstd * ((d - c1) - xhat * c2);   g_x = drop_out'(g);   g_s = drop_in'(g_x)
//             grad_gamma = sum_r g_n * xhat;   grad_beta = sum_r g_n   (partial[row block][2][N], one finishing launch)
//             the keep decisions are drawn again from (seed, call, site, row, column): no mask is stored.
//   relu_dropout   h = dropout(relu(a)) over a flat array;  g_a = h > 0 ? g_h * scale : 0 — the backward needs h alone.
// mean = (sum_c y[c]) / N;  var = (sum_c (y[c] - mean)^2) / N from the registers (two-pass);  rstd = 1 / sqrtf(var + eps).
// Each product and add is rounded on its own (-ffp-contract=off).  Threads per row and rows per workgroup by N are those of
// swish_layernorm.hip (16 | 64 | 256 threads, 128 | 32 | 16 rows); every sum runs in an order fixed by (R, N).
//
// The draw (include/tbe_hip.h) is rln_draw.hpp's.
#include <cmath>

#include "rowreg.hpp"

#include "rln_draw.hpp"

namespace tbe {

__host__ __device__ constexpr int rln_rows_per_block(int tpr) { return tpr == 16 ? 128 : tpr == 64 ? 32 : 16; }
static int rln_tpr(int N) { return N <= 16 * 4 ? 16 : N <= 64 * kRowSlots * 4 ? 64 : 256; }
template <int TPR>
using RlnTile = RowTile<TPR, rln_rows_per_block(TPR)>;

// colsum.hpp and tbe_row.hpp both have an add4, ambiguous where both are seen
__device__ __forceinline__ void rln_add4(float4& a, const float4 b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

__device__ __forceinline__ float rln_sum4(const float4 a, float acc) {
  acc += a.x;
  acc += a.y;
  acc += a.z;
  acc += a.w;
  return acc;
}

struct RlnFwdArgs {
  const float *x, *s, *gamma, *beta;  // s may be null; gamma, beta read when n is wanted
  float eps;
  float *y, *n, *stats;  // y may be null (not written); n, stats may be null together (no LayerNorm); stats [R, 2]
  int64_t R;
  int32_t N;
  RlnDrop din, dout;
};

struct RlnBwdArgs {
  const float *gy, *gn, *y, *stats, *gamma;  // gy may be null (zero); gn may be null (no LayerNorm: y, stats, gamma unread)
  float *gx, *gs, *partial;                  // gs may be null; partial [row blocks][2][N] when PG
  int64_t R;
  int32_t N;
  RlnDrop din, dout;
};

// DROP: some dropout of the launch is active (the p = 0 launches carry no hash code).
template <int TPR, bool DROP>
__global__ __launch_bounds__(256) void residual_layernorm_fwd_kernel(const RlnFwdArgs a) {
  RlnTile<TPR> t(a.R, a.N);
  const float* __restrict__ xg = a.x;
  const float* __restrict__ sg = a.s;
  float* __restrict__ yg = a.y;
  float* __restrict__ ng = a.n;
  float* __restrict__ stats = a.stats;
  const int N = a.N;
  const float fn = static_cast<float>(N);
  const bool drop_in = DROP && a.din.on && sg != nullptr, drop_out = DROP && a.dout.on;
  float4 ga[kRowSlots], be[kRowSlots];
#pragma unroll
  for (int k = 0; k < kRowSlots; ++k) ga[k] = be[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ng != nullptr) {
    t.load(a.gamma, ga);
    t.load(a.beta, be);
  }
  t.for_rows([&](int64_t r) {
    float4 v[kRowSlots];
    t.load(xg + r * N, v);  // columns beyond N hold zeros, and keep them through every step below
    if (sg != nullptr) {
      const uint32_t w2 = drop_in ? rln_row_word(a.din, static_cast<uint32_t>(r)) : 0u;
#pragma unroll
      for (int k = 0; k < kRowSlots; ++k) {
        if (t.has(k)) {
          float4 sv = ld4(sg + r * N + t.col(k));
          if (drop_in) sv = rln_keep4(sv, w2, a.din, static_cast<uint32_t>(t.col(k)));
          rln_add4(v[k], sv);
        }
      }
    }
    if (drop_out) {
      const uint32_t w2 = rln_row_word(a.dout, static_cast<uint32_t>(r));
#pragma unroll
      for (int k = 0; k < kRowSlots; ++k) {
        if (t.has(k)) v[k] = rln_keep4(v[k], w2, a.dout, static_cast<uint32_t>(t.col(k)));
      }
    }
    if (yg != nullptr) t.store(yg + r * N, v);
    if (ng != nullptr) {  // uniform over the workgroup: the barriers of t.sum (TPR = 256) are met by every thread
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < kRowSlots; ++k) part = rln_sum4(v[k], part);
      const float mean = t.sum(part) / fn;
      part = 0.f;
      t.for_slots([&](int k, int) {
        const float4 d = make_float4(v[k].x - mean, v[k].y - mean, v[k].z - mean, v[k].w - mean);
        part = rln_sum4(make_float4(d.x * d.x, d.y * d.y, d.z * d.z, d.w * d.w), part);
      });
      const float var = t.sum(part) / fn;
      const float rstd = 1.f / sqrtf(var + a.eps);
      if (t.lane == 0) {
        stats[2 * r] = mean;
        stats[2 * r + 1] = rstd;
      }
      t.for_slots([=, &v, &ga, &be](int k, int col) {
        st4(ng + r * N + col, make_float4(((v[k].x - mean) * rstd) * ga[k].x + be[k].x, ((v[k].y - mean) * rstd) * ga[k].y + be[k].y,
                                          ((v[k].z - mean) * rstd) * ga[k].z + be[k].z, ((v[k].w - mean) * rstd) * ga[k].w + be[k].w));
      });
    }
  });
}

// PG: the parameter gradients are wanted (sums[0] the gamma row, sums[1] the beta row of the row block).
template <int TPR, bool DROP, bool PG>
__global__ __launch_bounds__(256) void residual_layernorm_bwd_kernel(const RlnBwdArgs a) {
  RlnTile<TPR> t(a.R, a.N);
  const float* __restrict__ gyg = a.gy;
  const float* __restrict__ gng = a.gn;
  const float* __restrict__ yg = a.y;
  const float* __restrict__ stats = a.stats;
  float* __restrict__ gxg = a.gx;
  float* __restrict__ gsg = a.gs;
  const int N = a.N;
  const float fn = static_cast<float>(N);
  const bool drop_in = DROP && a.din.on, drop_out = DROP && a.dout.on;
  float4 ga[kRowSlots], sums[2][kRowSlots];
#pragma unroll
  for (int k = 0; k < kRowSlots; ++k) ga[k] = sums[0][k] = sums[1][k] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (gng != nullptr) t.load(a.gamma, ga);
  t.for_rows([&](int64_t r) {
    float4 g[kRowSlots];
    if (gyg != nullptr) {
      t.load(gyg + r * N, g);
    } else {
#pragma unroll
      for (int k = 0; k < kRowSlots; ++k) g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (gng != nullptr) {  // uniform over the workgroup (the barriers of t.sum)
      const float mean = stats[2 * r];
      const float rstd = stats[2 * r + 1];
      float4 xh[kRowSlots], d[kRowSlots];
      float p1 = 0.f, p2 = 0.f;
#pragma unroll
      for (int k = 0; k < kRowSlots; ++k) {
        xh[k] = d[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t.has(k)) {
          const float4 y = ld4(yg + r * N + t.col(k));
          const float4 q = ld4(gng + r * N + t.col(k));
          xh[k] = make_float4((y.x - mean) * rstd, (y.y - mean) * rstd, (y.z - mean) * rstd, (y.w - mean) * rstd);
          d[k] = make_float4(q.x * ga[k].x, q.y * ga[k].y, q.z * ga[k].z, q.w * ga[k].w);
          if constexpr (PG) {
            rln_add4(sums[0][k], make_float4(q.x * xh[k].x, q.y * xh[k].y, q.z * xh[k].z, q.w * xh[k].w));
            rln_add4(sums[1][k], q);
          }
        }
        p1 = rln_sum4(d[k], p1);  // columns beyond N hold zeros
        p2 = rln_sum4(make_float4(d[k].x * xh[k].x, d[k].y * xh[k].y, d[k].z * xh[k].z, d[k].w * xh[k].w), p2);
      }
      const float c1 = t.sum(p1) / fn;
      const float c2 = t.sum(p2) / fn;
#pragma unroll
      for (int k = 0; k < kRowSlots; ++k) {
        if (t.has(k)) {
          rln_add4(g[k], make_float4(rstd * ((d[k].x - c1) - xh[k].x * c2), rstd * ((d[k].y - c1) - xh[k].y * c2),
                                 rstd * ((d[k].z - c1) - xh[k].z * c2), rstd * ((d[k].w - c1) - xh[k].w * c2)));
        }
      }
    }
    if (drop_out) {
      const uint32_t w2 = rln_row_word(a.dout, static_cast<uint32_t>(r));
#pragma unroll
      for (int k = 0; k < kRowSlots; ++k) {
        if (t.has(k)) g[k] = rln_keep4(g[k], w2, a.dout, static_cast<uint32_t>(t.col(k)));
      }
    }
    t.store(gxg + r * N, g);
    if (gsg != nullptr) {
      if (drop_in) {
        const uint32_t w2 = rln_row_word(a.din, static_cast<uint32_t>(r));
#pragma unroll
        for (int k = 0; k < kRowSlots; ++k) {
          if (t.has(k)) g[k] = rln_keep4(g[k], w2, a.din, static_cast<uint32_t>(t.col(k)));
        }
      }
      t.store(gsg + r * N, g);
    }
  });
  if constexpr (PG) t.finish(sums, a.partial);
}

// ---- relu + dropout over a flat array of n4 float4 groups.  Element i draws with (row, col) = (hi32(i), lo32(i)).
constexpr int64_t kReluDropCap = 256 * 8;  // workgroups of 256 threads = 1024 floats each; the kernel strides over the rest

__global__ __launch_bounds__(256) void relu_dropout_fwd_kernel(const float* __restrict__ a, float* __restrict__ h, int64_t n4,
                                                               const RlnDrop d) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n4; i += static_cast<int64_t>(gridDim.x) * 256) {
    float4 v = ld4(a + 4 * i);
    v = make_float4(v.x <= 0.f ? 0.f : v.x, v.y <= 0.f ? 0.f : v.y, v.z <= 0.f ? 0.f : v.z, v.w <= 0.f ? 0.f : v.w);
    if (d.on) {
      const uint64_t e = static_cast<uint64_t>(i) * 4;
      v = rln_keep4(v, rln_row_word(d, static_cast<uint32_t>(e >> 32)), d, static_cast<uint32_t>(e));
    }
    st4(h + 4 * i, v);
  }
}

__global__ __launch_bounds__(256) void relu_dropout_bwd_kernel(const float* __restrict__ gh, const float* __restrict__ h,
                                                               float* __restrict__ ga, int64_t n4, float scale, bool on) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n4; i += static_cast<int64_t>(gridDim.x) * 256) {
    const float4 hv = ld4(h + 4 * i);
    float4 g = ld4(gh + 4 * i);
    if (on) g = scaled(g, scale);
    st4(ga + 4 * i, make_float4(hv.x > 0.f ? g.x : 0.f, hv.y > 0.f ? g.y : 0.f, hv.z > 0.f ? g.z : 0.f, hv.w > 0.f ? g.w : 0.f));
  }
}

// ---- host side
// The limits the row entries share; *tpr = threads per row, *nrb = row blocks (grid size).
static int rln_limits(const char* name, int64_t R, int N, float p_in, float p_out, int* tpr, int64_t* nrb) {
  TBE_REQUIRE(N >= 4, "%s: R=%lld must be >= 0 and N=%d a positive multiple of 4", name, static_cast<long long>(R), N);
  *tpr = rln_tpr(N);
  const int rc = rowreg_limits(name, R, N, rln_rows_per_block(*tpr), nrb);
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(R < (1ll << 31), "%s: R=%lld too large (2^31 rows or more)", name, static_cast<long long>(R));
  TBE_REQUIRE(rln_p_ok(p_in) && rln_p_ok(p_out), "%s: dropout p_in=%g / p_out=%g outside [0, 1)", name,
              static_cast<double>(p_in), static_cast<double>(p_out));
  return TBE_OK;
}

static int relu_dropout_check(const char* name, int64_t n, float p, std::initializer_list<const void*> ptrs) {
  TBE_REQUIRE(n >= 0 && (n & 3) == 0, "%s: n=%lld must be >= 0 and a multiple of 4", name, static_cast<long long>(n));
  TBE_REQUIRE(rln_p_ok(p), "%s: dropout p=%g outside [0, 1)", name, static_cast<double>(p));
  return check_pointers(name, ptrs);
}

}  // namespace tbe

using namespace tbe;

extern "C" size_t tbe_residual_layernorm_backward_workspace_bytes(int64_t R, int32_t N) {
  if (R <= 0) return rowreg_workspace_bytes(0, 2, N);
  const int rpb = rln_rows_per_block(rln_tpr(N));
  return rowreg_workspace_bytes((R + rpb - 1) / rpb, 2, N);
}

extern "C" int tbe_residual_layernorm_forward_f32(const float* x, const float* s, const float* gamma, const float* beta,
                                                  float eps, int64_t R, int32_t N, float p_in, uint32_t site_in, float p_out,
                                                  uint32_t site_out, uint64_t seed, int64_t call, float* y, float* n,
                                                  float* stats, void* stream) {
  const char* name = "tbe_residual_layernorm_forward_f32";
  int tpr;
  int64_t nrb;
  int rc = rln_limits(name, R, N, p_in, p_out, &tpr, &nrb);
  if (rc != TBE_OK) return rc;
  const bool drop = (s != nullptr && p_in > 0.f) || p_out > 0.f;
  TBE_REQUIRE(y != nullptr || n != nullptr, "%s: null pointer: neither y nor n is wanted", name);
  TBE_REQUIRE(y != nullptr || !drop, "%s: null pointer: y is needed when a dropout is active", name);
  if (n != nullptr) {
    TBE_REQUIRE(std::isfinite(eps) && eps >= 0.f, "%s: eps=%g must be finite and >= 0", name, static_cast<double>(eps));
    rc = check_pointers(name, {gamma, beta}, {stats});
    if (rc != TBE_OK) return rc;
  }
  rc = check_pointers(name, {x});
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(all_aligned({s, y, n}, 15), "%s: tensors must be 16-B aligned", name);
  RlnFwdArgs a{x, s, gamma, beta, eps, y, n, stats, R, N, rln_drop(seed, call, p_in, site_in), rln_drop(seed, call, p_out, site_out)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return rowreg_run(name, R, N, nrb, {x}, {}, nullptr, st, [&](dim3 grid) {
    dispatch_value<16, 64, 256>(tpr, [&](auto t) {
      dispatch_value<0, 1>(drop, [&](auto d) {
        hipLaunchKernelGGL((residual_layernorm_fwd_kernel<decltype(t)::value, decltype(d)::value != 0>), grid, dim3(256), 0, st, a);
      });
    });
  });
}

extern "C" int tbe_residual_layernorm_backward_f32(const float* g_y, const float* g_n, const float* y, const float* stats,
                                                   const float* gamma, int64_t R, int32_t N, float p_in, uint32_t site_in,
                                                   float p_out, uint32_t site_out, uint64_t seed, int64_t call, float* g_x,
                                                   float* g_s, float* grad_params, void* workspace, size_t workspace_bytes,
                                                   void* stream) {
  const char* name = "tbe_residual_layernorm_backward_f32";
  int tpr;
  int64_t nrb;
  int rc = rln_limits(name, R, N, p_in, p_out, &tpr, &nrb);
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(g_y != nullptr || g_n != nullptr, "%s: null pointer: neither g_y nor g_n is given", name);
  TBE_REQUIRE(grad_params == nullptr || g_n != nullptr, "%s: null pointer: parameter gradients need g_n", name);
  if (g_s == g_x) {
    TBE_REQUIRE(!(p_in > 0.f), "%s: g_s may alias g_x only with p_in = 0", name);
    g_s = nullptr;  // the same values at the same place: written once
  }
  rc = check_pointers(name, {g_x});
  if (rc == TBE_OK && g_n != nullptr) rc = check_pointers(name, {y, gamma}, {stats});
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(all_aligned({g_y, g_n, g_s}, 15), "%s: tensors must be 16-B aligned", name);
  const bool drop = (g_s != nullptr && p_in > 0.f) || p_out > 0.f;
  RlnBwdArgs a{g_y, g_n, y, stats, gamma, g_x, g_s, static_cast<float*>(workspace), R, N, rln_drop(seed, call, p_in, site_in),
               rln_drop(seed, call, p_out, site_out)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RowColSums cs{2, grad_params, workspace, workspace_bytes};
  return rowreg_run(name, R, N, nrb, {g_x}, {}, grad_params != nullptr ? &cs : nullptr, st, [&](dim3 grid) {
    dispatch_value<16, 64, 256>(tpr, [&](auto t) {
      dispatch_value<0, 1>(drop, [&](auto d) {
        dispatch_value<0, 1>(grad_params != nullptr, [&](auto pg) {
          hipLaunchKernelGGL((residual_layernorm_bwd_kernel<decltype(t)::value, decltype(d)::value != 0, decltype(pg)::value != 0>),
                             grid, dim3(256), 0, st, a);
        });
      });
    });
  });
}

extern "C" int tbe_relu_dropout_forward_f32(const float* a, int64_t n, float p, uint32_t site, uint64_t seed, int64_t call,
                                            float* h, void* stream) {
  const char* name = "tbe_relu_dropout_forward_f32";
  const int rc = relu_dropout_check(name, n, p, {a, h});
  if (rc != TBE_OK || n == 0) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(relu_dropout_fwd_kernel, dim3(grid_blocks(n / 4, kReluDropCap)), dim3(256), 0, st, a, h, n / 4,
                     rln_drop(seed, call, p, site));
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}

extern "C" int tbe_relu_dropout_backward_f32(const float* grad_h, const float* h, int64_t n, float p, float* grad_a,
                                             void* stream) {
  const char* name = "tbe_relu_dropout_backward_f32";
  const int rc = relu_dropout_check(name, n, p, {grad_h, h, grad_a});
  if (rc != TBE_OK || n == 0) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(relu_dropout_bwd_kernel, dim3(grid_blocks(n / 4, kReluDropCap)), dim3(256), 0, st, grad_h, h, grad_a, n / 4,
                     1.f / (1.f - p), p > 0.f);
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}
