// Cross networks (DCN / DCN-v2) on gfx950: the element-wise work between the library GEMMs, and all of VectorCrossNet.
//
// Reference: torchrec/modules/crossnet.py — CrossNet :19-89, LowRankCrossNet :92-188, VectorCrossNet :191-268 — trained
// through autograd.  A layer of the two GEMM-based nets is  x_{l+1} = x_0 * t + x_l,  t = y + b,  y = x_l K^T  or
// (x_l V^T) W^T.
//
// The FORWARD of the GEMM-based nets needs no kernel of this file: the bias rides in the GEMM (torch.addmm with
// bias.view(N)) and x_0 * t + x_l is one torch.addcmul; t is what the backward saves.
//
// Their BACKWARD through autograd is, per layer, a chain of HBM-bound kernels over [B, N]: mul (G * x_0), mul (G * t),
// AccumulateGrad add into x_0's gradient, a column sum for the bias.  cross_bwd_kernel does all of it in one pass: it
// reads G, x_0, t (and acc, unless `first`), writes g_y = G * x_0 and acc (+)= G * t and leaves the column sums of g_y per
// row block, which a fixed-order second stage adds (deterministic, no float atomics) — the scheme of colsum.hpp.
//
// VectorCrossNet is element-wise work plus row dots only:  s_l[b] = x_l[b, :] . w_l,  x_{l+1} = x_0 * s_l + b_l + x_l.
// One forward kernel runs all L layers with the row in registers; one backward kernel recomputes every x_l from x_0, s and
// the biases in the forward's own operation order (so bit for bit the forward's x_l) and produces the input gradient and
// the row-block partial sums of all 2 L parameter gradients, which ONE second-stage launch over 2 L N columns finishes.
// Geometry, slot addressing, the row sums, the finish of the column sums and the host side of the two entries are the
// row-in-registers scheme of rowreg.hpp (orders pinned by tests/test_rowreg_order_gpu.py); the mixture gate takes its
// row_sum<64> from there.
//
// LowRankMixtureCrossNet (:271-446) is LowRankCrossNet's layer of rank K r once its K experts are folded (include/tbe_hip.h);
// what it adds is one narrow pass over [B, K r] between the GEMMs each way: mixture_gate_fwd_kernel / _bwd_kernel below.
//
// Every product and every add is rounded on its own (the Makefile builds with -ffp-contract=off; no fmaf here), so a float32
// restatement in numpy reproduces the element-wise results bit for bit.
#include <algorithm>

#include "rowreg.hpp"

namespace tbe {

// block = 256 threads = TY rows x TX float4-columns; grid = (column tiles, row blocks): colsum.hpp
template <int TX>
__global__ __launch_bounds__(256) void cross_bwd_kernel(const float* __restrict__ G, const float* __restrict__ x0,
                                                        const float* __restrict__ t, float* __restrict__ gy,
                                                        float* __restrict__ acc, float* __restrict__ partial, int64_t B,
                                                        int N, int first) {
  colsum_row_block<TX>(partial, B, N, [=](int64_t, int64_t o, float4& sum) {
    const float4 g = ld4(G + o);
    const float4 x = ld4(x0 + o);
    const float4 tt = ld4(t + o);
    const float4 y = make_float4(g.x * x.x, g.y * x.y, g.z * x.z, g.w * x.w);
    float4 a = make_float4(g.x * tt.x, g.y * tt.y, g.z * tt.z, g.w * tt.w);
    if (!first) {
      const float4 p = ld4(acc + o);
      a.x = p.x + a.x;
      a.y = p.y + a.y;
      a.z = p.z + a.z;
      a.w = p.w + a.w;
    }
    st4(gy + o, y);
    st4(acc + o, a);
    add4(sum, y);
  });
}

// ---- VectorCrossNet: the row-in-registers scheme of rowreg.hpp; the arithmetic and the rule of N are here -----------------------
constexpr int kVecMaxL = 8;
constexpr int kVecRowsPerBlock = 128;  // rows per workgroup = rows per partial sum
// threads per row: 64 — one wave per row, four rows of the block in flight; 256 — the block per row
static int vec_tpr(int N) { return N <= 64 * kRowSlots * 4 ? 64 : 256; }
template <int TPR>
using VecTile = RowTile<TPR, kVecRowsPerBlock>;

__device__ __forceinline__ float dot4(const float4 a, const float4 b, float acc) {
  acc += a.x * b.x;
  acc += a.y * b.y;
  acc += a.z * b.z;
  acc += a.w * b.w;
  return acc;
}

// x <- (x0 * s + b) + x: the reference's order (torchrec/modules/crossnet.py:266), each operation rounded
__device__ __forceinline__ float4 cross_step(const float4 x0, const float s, const float4 b, const float4 x) {
  return make_float4((x0.x * s + b.x) + x.x, (x0.y * s + b.y) + x.y, (x0.z * s + b.z) + x.z, (x0.w * s + b.w) + x.w);
}

template <int TPR>
__global__ __launch_bounds__(256) void vector_cross_fwd_kernel(const float* __restrict__ x0g, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ out,
                                                               float* __restrict__ s_out, int64_t B, int N, int L) {
  VecTile<TPR> t(B, N);
  t.for_rows([&](int64_t r) {
    float4 x0[kRowSlots], x[kRowSlots];
    t.load(x0g + r * N, x0);
#pragma unroll
    for (int k = 0; k < kRowSlots; ++k) x[k] = x0[k];
    for (int l = 0; l < L; ++l) {
      float part = 0.f;
      t.for_slots([=, &part, &x](int k, int col) { part = dot4(x[k], ld4(w + l * N + col), part); });
      const float s = t.sum(part);
      if (t.lane == 0) s_out[static_cast<int64_t>(l) * B + r] = s;
      t.for_slots([=, &x, &x0](int k, int col) { x[k] = cross_step(x0[k], s, ld4(bias + l * N + col), x[k]); });
    }
    t.store(out + r * N, x);
  });
}

// L is a template parameter, so that the 2 * L * kRowSlots float4 column sums of a thread stay in registers.
// partial: [row blocks][2 L][N] — rows 0 .. L-1 the bias gradients, L .. 2L-1 the weight gradients of the row block.
template <int TPR, int L>
__global__ __launch_bounds__(256) void vector_cross_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ x0g,
                                                               const float* __restrict__ sg, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ gin,
                                                               float* __restrict__ partial, int64_t B, int N) {
  VecTile<TPR> t(B, N);
  float4 sums[2 * L][kRowSlots];  // [l]: of G_l (bias), [L + l]: of d_l * x_l (weight)
#pragma unroll
  for (int i = 0; i < 2 * L; ++i) {
#pragma unroll
    for (int k = 0; k < kRowSlots; ++k) sums[i][k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  t.for_rows([&](int64_t r) {
    float4 x0[kRowSlots], g[kRowSlots], acc[kRowSlots];
    t.load(x0g + r * N, x0);
    t.load(gout + r * N, g);
#pragma unroll
    for (int k = 0; k < kRowSlots; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    float s[L];
#pragma unroll
    for (int l = 0; l < L; ++l) s[l] = sg[static_cast<int64_t>(l) * B + r];
#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
      // x_l, recomputed in the forward's order
      float4 x[kRowSlots];
#pragma unroll
      for (int k = 0; k < kRowSlots; ++k) x[k] = x0[k];
#pragma unroll
      for (int j = 0; j < l; ++j) {
        t.for_slots([=, &x, &x0, &s](int k, int col) { x[k] = cross_step(x0[k], s[j], ld4(bias + j * N + col), x[k]); });
      }
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < kRowSlots; ++k) part = dot4(g[k], x0[k], part);  // columns beyond N hold zeros
      const float d = t.sum(part);
      t.for_slots([=, &g, &s, &acc, &sums, &x](int k, int col) {
        const float4 gk = g[k];
        const float sl = s[l];
        add4(acc[k], make_float4(gk.x * sl, gk.y * sl, gk.z * sl, gk.w * sl));
        add4(sums[l][k], gk);
        add4(sums[L + l][k], make_float4(d * x[k].x, d * x[k].y, d * x[k].z, d * x[k].w));
        const float4 wl = ld4(w + l * N + col);
        add4(g[k], make_float4(d * wl.x, d * wl.y, d * wl.z, d * wl.w));
      });
    }
    t.for_slots([&](int k, int) { add4(g[k], acc[k]); });
    t.store(gin + r * N, g);
  });
  t.finish(sums, partial);
}

// The limits shared by the two entries; *nrb = row blocks (grid size).
static int vec_limits(const char* name, int64_t B, int N, int L, int64_t* nrb) {
  TBE_REQUIRE(L >= 1 && L <= kVecMaxL, "%s: L=%d must be in [1, %d] (the limits: N <= %d, L <= %d)", name, L, kVecMaxL, kRowMaxN,
              kVecMaxL);
  static_assert(kVecMaxL == 8, "the message below names it");
  return rowreg_limits(name, B, N, kVecRowsPerBlock, nrb, ", L <= 8");
}

// ---- LowRankMixtureCrossNet: the narrow pass between the folded GEMMs -----------------------------------------------------
// a2, grad_a2 [K, B, r] (what the batched GEMM over experts writes / reads); m, grad_m [B, K r] (what the Ucat GEMMs read /
// write); logits, p, grad_logits [B, K].  Per row b, with relu(a) = a > 0 ? a : +0:
//   forward    mx = max_k logits[b, k];  e_k = expf(logits[b, k] - mx);  s = ((e_0 + e_1) + ...) + e_{K-1};
//              p[b, k] = e_k / s;  m[b, k r + j] = p[b, k] * relu(a2[k, b, j])                      (one product)
//   backward   d_k = sum_j grad_m[b, k r + j] * relu(a2[k, b, j]);  t = ((p_0 d_0 + p_1 d_1) + ...) + p_{K-1} d_{K-1};
//              grad_logits[b, k] = p_k * (d_k - t);  grad_a2[k, b, j] = a2[k, b, j] > 0 ? p_k * grad_m[b, k r + j] : 0
// One wave per row, four rows per workgroup; lane k holds p_k (and d_k).  d_k: lane i adds the columns 4 (i + 64 n) + c,
// n = 0, 1, ..., c = 0 .. 3, in that order from 0.0f, then the xor butterfly of row_sum — an order that depends on r only
// and is the same whether the columns move as float4 or as scalars.
constexpr int kMixMaxK = 16;
constexpr int kMixRowsPerBlock = 4;

__device__ __forceinline__ float relu1(const float a) { return a > 0.f ? a : 0.f; }

// p[b, lane] for lane < K (0 in the other lanes); all 64 lanes of the row's wave call it
__device__ __forceinline__ float mix_softmax(const float* __restrict__ logits_row, const int K, const int lane) {
  const float lg = lane < K ? logits_row[lane] : 0.f;
  float mx = __shfl(lg, 0, kWave);
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, __shfl(lg, k, kWave));
  const float e = lane < K ? expf(lg - mx) : 0.f;
  float s = __shfl(e, 0, kWave);
  for (int k = 1; k < K; ++k) s += __shfl(e, k, kWave);
  return e / s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void mixture_gate_fwd_kernel(const float* __restrict__ a2, const float* __restrict__ logits,
                                                               float* __restrict__ m, float* __restrict__ p, int64_t B, int K,
                                                               int r) {
  const int lane = threadIdx.x & 63;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kMixRowsPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;  // the whole wave
  const float p_mine = mix_softmax(logits + b * K, K, lane);
  if (lane < K) p[b * K + lane] = p_mine;
  const int W = K * r;
  float* __restrict__ mrow = m + b * W;
  constexpr int E = VEC ? 4 : 1;  // elements per lane and round
  // the trip count is the wave's: every lane takes part in the shuffle
  for (int base = 0; base < W; base += 64 * E) {
    const int i = base + lane * E;
    const bool in = i < W;
    const int k = in ? i / r : 0;  // VEC: r % 4 == 0, the four columns are one expert's
    const float pk = __shfl(p_mine, k, kWave);
    if (in) {
      const float* src = a2 + (static_cast<int64_t>(k) * B + b) * r + (i - k * r);
      if constexpr (VEC) {
        const float4 a = ld4(src);
        st4(mrow + i, make_float4(pk * relu1(a.x), pk * relu1(a.y), pk * relu1(a.z), pk * relu1(a.w)));
      } else {
        mrow[i] = pk * relu1(*src);
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void mixture_gate_bwd_kernel(const float* __restrict__ gm, const float* __restrict__ a2,
                                                               const float* __restrict__ p, float* __restrict__ ga2,
                                                               float* __restrict__ gl, int64_t B, int K, int r) {
  const int lane = threadIdx.x & 63;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kMixRowsPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;  // the whole wave
  const float p_mine = lane < K ? p[b * K + lane] : 0.f;
  float d_mine = 0.f;
  for (int k = 0; k < K; ++k) {
    const float pk = __shfl(p_mine, k, kWave);
    const float* __restrict__ g = gm + (b * K + k) * r;
    const int64_t o = (static_cast<int64_t>(k) * B + b) * r;
    float part = 0.f;
    for (int j = lane * 4; j < r; j += 256) {
      if constexpr (VEC) {
        const float4 gv = ld4(g + j);
        const float4 av = ld4(a2 + o + j);
        st4(ga2 + o + j, make_float4(av.x > 0.f ? pk * gv.x : 0.f, av.y > 0.f ? pk * gv.y : 0.f,
                                     av.z > 0.f ? pk * gv.z : 0.f, av.w > 0.f ? pk * gv.w : 0.f));
        part = dot4(gv, make_float4(relu1(av.x), relu1(av.y), relu1(av.z), relu1(av.w)), part);
      } else {
        const int end = min(j + 4, r);
        for (int c = j; c < end; ++c) {
          const float gv = g[c];
          const float av = a2[o + c];
          ga2[o + c] = av > 0.f ? pk * gv : 0.f;
          part += gv * relu1(av);
        }
      }
    }
    const float d = row_sum<64>(part);
    if (lane == k) d_mine = d;
  }
  float t = __shfl(p_mine, 0, kWave) * __shfl(d_mine, 0, kWave);
  for (int k = 1; k < K; ++k) t += __shfl(p_mine, k, kWave) * __shfl(d_mine, k, kWave);
  if (lane < K) gl[b * K + lane] = p_mine * (d_mine - t);
}

// The checks of both gate entries; *launch = false for an empty batch.  *vec: the data moves as float4.
static int mix_gate_args(const char* name, std::initializer_list<const void*> tensors, int64_t B, int K, int r, bool* launch,
                         bool* vec) {
  *launch = false;
  TBE_REQUIRE(K >= 2 && K <= kMixMaxK, "%s: K=%d beyond the limits 2 <= K <= %d", name, K, kMixMaxK);
  TBE_REQUIRE(r >= 1 && r <= (1 << 26), "%s: r=%d must be in [1, 2^26]", name, r);
  TBE_REQUIRE(B >= 0, "%s: B=%lld must be >= 0", name, (long long)B);
  if (B == 0) return TBE_OK;
  const int rc = check_pointers(name, {}, tensors);
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE((B + kMixRowsPerBlock - 1) / kMixRowsPerBlock < (1ll << 31), "%s: B=%lld too large", name, (long long)B);
  *vec = (r & 3) == 0 && all_aligned(tensors, 15);
  *launch = true;
  return TBE_OK;
}

}  // namespace tbe

using namespace tbe;

extern "C" size_t tbe_cross_backward_workspace_bytes(int64_t B, int32_t N) { return colsum_workspace_bytes(B, N); }

extern "C" int tbe_cross_backward_f32(const float* grad_out, const float* x0, const float* t, int64_t B, int32_t N,
                                      int32_t first, float* grad_y, float* acc, float* bias_grad, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  const char* name = "tbe_cross_backward_f32";
  TBE_REQUIRE(bias_grad != nullptr, "%s: null bias_grad", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  const int f = first != 0;
  int64_t nrb;
  const int rc = colsum_first_stage(name, true, B, N, {grad_out, x0, t, grad_y, acc}, partial, workspace_bytes, &nrb,
                                    [&](auto tx, dim3 grid) {
                                      hipLaunchKernelGGL(cross_bwd_kernel<decltype(tx)::value>, grid, dim3(256), 0, st, grad_out,
                                                         x0, t, grad_y, acc, partial, B, N, f);
                                    });
  return rc != TBE_OK ? rc : launch_colsum_partials(name, partial, nrb, N, bias_grad, st);
}

extern "C" size_t tbe_vector_cross_backward_workspace_bytes(int64_t B, int32_t N, int32_t L) {
  return rowreg_workspace_bytes(B <= 0 ? 0 : (B + kVecRowsPerBlock - 1) / kVecRowsPerBlock, 2 * L, N);
}

extern "C" int tbe_vector_cross_forward_f32(const float* x0, const float* weights, const float* bias, int64_t B, int32_t N,
                                            int32_t L, float* out, float* s, void* stream) {
  const char* name = "tbe_vector_cross_forward_f32";
  int64_t nrb;
  const int rc = vec_limits(name, B, N, L, &nrb);
  if (rc != TBE_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return rowreg_run(name, B, N, nrb, {x0, weights, bias, out}, {s}, nullptr, st, [&](dim3 grid) {
    dispatch_value<64, 256>(vec_tpr(N), [&](auto t) {
      hipLaunchKernelGGL(vector_cross_fwd_kernel<decltype(t)::value>, grid, dim3(256), 0, st, x0, weights, bias, out, s, B, N, L);
    });
  });
}

extern "C" int tbe_vector_cross_backward_f32(const float* grad_out, const float* x0, const float* s, const float* weights,
                                             const float* bias, int64_t B, int32_t N, int32_t L, float* grad_in,
                                             float* grad_params, void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "tbe_vector_cross_backward_f32";
  int64_t nrb;
  const int rc = vec_limits(name, B, N, L, &nrb);
  if (rc != TBE_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RowColSums cs{2 * L, grad_params, workspace, workspace_bytes};
  return rowreg_run(name, B, N, nrb, {grad_out, x0, weights, bias, grad_in}, {s}, &cs, st, [&](dim3 grid) {
    dispatch_value<64, 256>(vec_tpr(N), [&](auto t) {
      dispatch_value<1, 2, 3, 4, 5, 6, 7, 8>(L, [&](auto l) {  // 1 ... kVecMaxL
        hipLaunchKernelGGL((vector_cross_bwd_kernel<decltype(t)::value, decltype(l)::value>), grid, dim3(256), 0, st, grad_out, x0,
                           s, weights, bias, grad_in, static_cast<float*>(workspace), B, N);
      });
    });
  });
}

extern "C" int tbe_mixture_gate_forward_f32(const float* a2, const float* logits, int64_t B, int32_t K, int32_t r, float* m,
                                            float* p, void* stream) {
  const char* name = "tbe_mixture_gate_forward_f32";
  bool launch, vec;
  const int rc = mix_gate_args(name, {a2, logits, m, p}, B, K, r, &launch, &vec);
  if (rc != TBE_OK || !launch) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((B + kMixRowsPerBlock - 1) / kMixRowsPerBlock));
  if (vec)
    hipLaunchKernelGGL(mixture_gate_fwd_kernel<true>, grid, dim3(256), 0, st, a2, logits, m, p, B, K, r);
  else
    hipLaunchKernelGGL(mixture_gate_fwd_kernel<false>, grid, dim3(256), 0, st, a2, logits, m, p, B, K, r);
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}

extern "C" int tbe_mixture_gate_backward_f32(const float* grad_m, const float* a2, const float* p, int64_t B, int32_t K,
                                             int32_t r, float* grad_a2, float* grad_logits, void* stream) {
  const char* name = "tbe_mixture_gate_backward_f32";
  bool launch, vec;
  const int rc = mix_gate_args(name, {grad_m, a2, p, grad_a2, grad_logits}, B, K, r, &launch, &vec);
  if (rc != TBE_OK || !launch) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((B + kMixRowsPerBlock - 1) / kMixRowsPerBlock));
  if (vec)
    hipLaunchKernelGGL(mixture_gate_bwd_kernel<true>, grid, dim3(256), 0, st, grad_m, a2, p, grad_a2, grad_logits, B, K, r);
  else
    hipLaunchKernelGGL(mixture_gate_bwd_kernel<false>, grid, dim3(256), 0, st, grad_m, a2, p, grad_a2, grad_logits, B, K, r);
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}
