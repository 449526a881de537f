// Gradient of the pooled TBE lookup with respect to per_sample_weights (fbgemm's
// grad_indice_weights): giw[i] = s * <grad_out block of the bag of i, table row of indices[i]>.
// Templates over the table element type WT (float or _Float16); tbe_indice_weights.hip
// instantiates both.  Products and sums are FP32.
//
// Reference call site: torchrec/modules/feature_processor.py:29-74 (PositionWeightedModule) in
// front of a weighted EmbeddingBagCollection (torchrec/modules/embedding_modules.py:165-193),
// which trains the position weights through nn.EmbeddingBag's per_sample_weights gradient.
//
// Design: the forward's gather with the roles of the output block swapped (tbe_forward_impl.hpp).
//  * the same wave -> bags mapping, (G, NV) row geometry, U = 4 rows in flight per group and
//    short/long split, so the row reads coalesce exactly as in the forward;
//  * a group loads its bag's gradient block into registers ONCE (16 B per lane, the forward's
//    output store turned into a load) and reuses it for every id of the bag;
//  * each lane multiplies its columns, then the G lane partials of the U rows in flight are
//    combined by one fixed-order butterfly that folds the U values into each other on its first
//    two steps (3 + log2(G/4) shuffles for 4 rows instead of 4 * log2(G));
//  * no atomics, no LDS: every row's dot is finished inside its group, every summation order
//    is a function of the launch shape only.
// giw is zeroed by a memset node first (4 B per id, ~5 us next to a 258 us gather at the Criteo
// shape; a fill kernel of our own measured the same), so positions that lie in no well-formed
// bag, and the features masked by feat_requires_grad, need no pass of their own.
#pragma once
#include "tbe_forward_impl.hpp"

namespace tbe {

struct IwgArgs {
  const uint64_t* feat_weights;
  const int32_t* feat_D;
  const int64_t* feat_out_offset;
  const int64_t* feat_rows;
  const int64_t* feat_window;         // [2F] or nullptr, as FwdArgs
  const int32_t* feat_pooling;        // [F] or nullptr, as FwdArgs
  const int32_t* feat_requires_grad;  // [F] or nullptr = every feature
  const int64_t* indices;
  const int64_t* offsets;
  const float* grad_out;
  float* giw;
  int64_t grad_stride;
  int64_t N;
  int32_t F;
  int32_t B;
  int32_t bags_per_wave;
};

// Lane partial of <g, x> over the lane's 4 columns (fixed order; -ffp-contract=off keeps it).
__device__ __forceinline__ float dot4(const float4& g, const float4& x, float acc) {
  acc = fmaf(g.x, x.x, acc);
  acc = fmaf(g.y, x.y, acc);
  acc = fmaf(g.z, x.z, acc);
  acc = fmaf(g.w, x.w, acc);
  return acc;
}

// Sums 4 per-lane values over the G lanes of a group.  Lane gl of the group ends with the group
// total of value iwg_slot(gl): steps xor 1 and xor 2 each halve the number of live values, the
// remaining steps are a plain butterfly.  The order of additions depends on G only.
__device__ __forceinline__ int iwg_slot(int gl) { return ((gl & 1) << 1) | ((gl >> 1) & 1); }
template <int G>
__device__ __forceinline__ float reduce4(const float (&p)[4], int gl) {
  static_assert(G >= 4, "reduce4 folds over the 4 low lanes of a group");
  const bool hi1 = gl & 1;
  const float k0 = hi1 ? p[2] : p[0], k1 = hi1 ? p[3] : p[1];
  const float s0 = hi1 ? p[0] : p[2], s1 = hi1 ? p[1] : p[3];
  const float r0 = k0 + __shfl_xor(s0, 1, kWave);
  const float r1 = k1 + __shfl_xor(s1, 1, kWave);
  const bool hi2 = gl & 2;
  float r = (hi2 ? r1 : r0) + __shfl_xor(hi2 ? r0 : r1, 2, kWave);
#pragma unroll
  for (int m = 4; m < G; m <<= 1) r += __shfl_xor(r, m, kWave);
  return r;
}

template <typename WT>
__device__ __forceinline__ bool iwg_vec(const IwgArgs& a, const WT* W, int D, int64_t Doff) {
  return ((D & 3) == 0) && ((Doff & 3) == 0) && ((a.grad_stride & 3) == 0) &&
         ((reinterpret_cast<uintptr_t>(W) & kRowAlignMask<WT>) == 0) &&
         ((reinterpret_cast<uintptr_t>(a.grad_out) & 15) == 0);
}

template <typename WT, int G, int NV, bool MEAN>
__global__ __launch_bounds__(256) void tbe_iwg_short_kernel(IwgArgs a) {
  constexpr int NG = kWave / G;
  constexpr int U = 4;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int f = blockIdx.x % a.F;
  const int tile = blockIdx.x / a.F;
  const int bpw = a.bags_per_wave;
  const int bag0 = (tile * 4 + wave) * bpw;
  if (bag0 >= a.B) return;                                                   // wave-uniform
  if (a.feat_requires_grad != nullptr && a.feat_requires_grad[f] == 0) return;  // block-uniform: stays 0

  const WT* __restrict__ W = reinterpret_cast<const WT*>(a.feat_weights[f]);
  const int D = a.feat_D[f];
  const int64_t Doff = a.feat_out_offset[f];
  const RowWindow win = load_window(a.feat_rows, a.feat_window, f);
  const bool mean_f = MEAN && (a.feat_pooling == nullptr || a.feat_pooling[f] == TBE_POOL_MEAN);
  const bool vec = iwg_vec(a, W, D, Doff);

  // Coalesced metadata: lane l owns bag (f, bag0 + l).
  const int64_t* __restrict__ offs = a.offsets + static_cast<int64_t>(f) * a.B;
  const int b_l = bag0 + lane;
  int64_t s_l = 0, e_l = 0;
  if (b_l < a.B && lane < bpw) {
    s_l = offs[b_l];
    e_l = offs[b_l + 1];
    if (s_l < 0 || e_l > a.N || s_l > e_l) s_l = e_l = 0;  // malformed offsets: no position of this bag is touched
  }
  const int len_l = static_cast<int>(e_l - s_l);
  int64_t idx0_l = 0;
  if (len_l > 0) idx0_l = a.indices[s_l];

  const int g = lane / G;
  const int gl = lane % G;
  const int slot = iwg_slot(gl);

#pragma unroll 1
  for (int p = 0; p < bpw; p += NG * U) {
    if (bag0 + p >= a.B) break;  // wave-uniform tail
    int64_t s[U];
    int len[U];
    int64_t idx[U];
    float4 go[U][NV];
    int maxlen = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = p + u * NG + g;  // < 64: p + U*NG <= bpw when the loop runs
      s[u] = shfl64(s_l, j);
      len[u] = __shfl(len_l, j, kWave);
      idx[u] = shfl64(idx0_l, j);
      maxlen = max(maxlen, len[u]);
      // len > 0 implies a bag inside the batch (lanes past B or bpw hold len 0)
      const float* grow = a.grad_out + static_cast<int64_t>(bag0 + j) * a.grad_stride + Doff;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int d = (v * G + gl) * 4;
        go[u][v] = (len[u] > 0 && d < D) ? load_cols(grow, d, D, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    // my_*: the bag whose total this lane holds after reduce4 (lanes gl < 4 store it)
    const int64_t my_s = slot == 0 ? s[0] : slot == 1 ? s[1] : slot == 2 ? s[2] : s[3];
    const int my_len = slot == 0 ? len[0] : slot == 1 ? len[1] : slot == 2 ? len[2] : len[3];
    for (int i = 0; i < maxlen; ++i) {
      float part[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool in = i < len[u];
        int64_t ix = idx[u];  // element 0 is already in registers
        if (in && i > 0) ix = a.indices[s[u] + i];
        int64_t lix = 0;
        const bool ok = in && classify_id(win, ix, lix) == kIdLocal;
        const WT* row = W + lix * D;
        part[u] = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const int d = (v * G + gl) * 4;
          const float4 x = (ok && d < D) ? load_cols(row, d, D, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
          if (ok) part[u] = dot4(go[u][v], x, part[u]);  // a skipped id is 0 whatever grad_out holds
        }
      }
      float r = reduce4<G>(part, gl);
      if (gl < U && i < my_len) {
        if (mean_f) r = r / static_cast<float>(my_len);
        a.giw[my_s + i] = r;
      }
    }
  }
}

// Long-bag variant: one wave per bag, the wave's NG groups take alternate rows of the bag, 4 rows
// in flight per group.  Every row's dot is finished inside its group: no LDS combine.
template <typename WT, int G, int NV, bool MEAN>
__global__ __launch_bounds__(256) void tbe_iwg_long_kernel(IwgArgs a) {
  constexpr int NG = kWave / G;
  constexpr int U = 4;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t bag = static_cast<int64_t>(blockIdx.x) * 4 + wave;  // f*B + b
  const int64_t nbags = static_cast<int64_t>(a.F) * a.B;
  if (bag >= nbags) return;
  const int f = static_cast<int>(bag / a.B);
  const int b = static_cast<int>(bag % a.B);
  if (a.feat_requires_grad != nullptr && a.feat_requires_grad[f] == 0) return;  // wave-uniform: stays 0
  const WT* __restrict__ W = reinterpret_cast<const WT*>(a.feat_weights[f]);
  const int D = a.feat_D[f];
  const int64_t Doff = a.feat_out_offset[f];
  const RowWindow win = load_window(a.feat_rows, a.feat_window, f);
  const bool mean_f = MEAN && (a.feat_pooling == nullptr || a.feat_pooling[f] == TBE_POOL_MEAN);
  const bool vec = iwg_vec(a, W, D, Doff);
  const int64_t s = a.offsets[bag];
  const int64_t e = a.offsets[bag + 1];
  if (s < 0 || e > a.N || s > e || s == e) return;  // malformed or empty (wave-uniform): nothing to write
  const int len = static_cast<int>(e - s);
  const int g = lane / G;
  const int gl = lane % G;
  const int slot = iwg_slot(gl);

  float4 go[NV];
  const float* grow = a.grad_out + static_cast<int64_t>(b) * a.grad_stride + Doff;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int d = (v * G + gl) * 4;
    go[v] = d < D ? load_cols(grow, d, D, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
  }

  // The wave walks the bag in chunks of 64 indices; lane l holds index s + c + l.
  for (int c = 0; c < len; c += kWave) {
    const int n = min(kWave, len - c);
    int64_t ix_l = 0;
    if (lane < n) ix_l = a.indices[s + c + lane];
    // group g takes elements g, g+NG, g+2NG, ... of the chunk (fixed assignment).
    for (int k = 0; k < n; k += NG * U) {
      float part[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = k + u * NG + g;
        const int64_t ix = shfl64(ix_l, j & 63);
        int64_t lix = 0;
        const bool ok = j < n && classify_id(win, ix, lix) == kIdLocal;
        const WT* row = W + lix * D;
        part[u] = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const int d = (v * G + gl) * 4;
          const float4 x = (ok && d < D) ? load_cols(row, d, D, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
          if (ok) part[u] = dot4(go[v], x, part[u]);
        }
      }
      float r = reduce4<G>(part, gl);
      const int my_j = k + slot * NG + g;
      if (gl < U && my_j < n) {
        if (mean_f) r = r / static_cast<float>(len);
        a.giw[s + c + my_j] = r;
      }
    }
  }
}

template <typename WT, int G, int NV>
static int launch_iwg(const char* who, const IwgArgs& a, bool mean, bool long_bags, hipStream_t st) {
  if (long_bags) {
    const int64_t nbags = static_cast<int64_t>(a.F) * a.B;
    const unsigned grid = static_cast<unsigned>((nbags + 3) / 4);
    if (mean) hipLaunchKernelGGL((tbe_iwg_long_kernel<WT, G, NV, true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((tbe_iwg_long_kernel<WT, G, NV, false>), dim3(grid), dim3(256), 0, st, a);
  } else {
    const unsigned tiles = (a.B + 4 * a.bags_per_wave - 1) / (4 * a.bags_per_wave);
    const unsigned grid = tiles * a.F;
    if (mean) hipLaunchKernelGGL((tbe_iwg_short_kernel<WT, G, NV, true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((tbe_iwg_short_kernel<WT, G, NV, false>), dim3(grid), dim3(256), 0, st, a);
  }
  TBE_CHECK_LAUNCH(who);
  return TBE_OK;
}

// The body of tbe_backward_indice_weights_f32 / _f16w (`who` names the entry point in error messages).
template <typename WT>
static int backward_indice_weights(const char* who, const uint64_t* feat_weights, const int32_t* feat_D,
                                   const int64_t* feat_out_offset, const int64_t* feat_rows,
                                   int32_t F, int32_t B, int32_t max_D,
                                   const int64_t* indices, int64_t N, const int64_t* offsets,
                                   int32_t pooling_mode, const int32_t* feat_pooling,
                                   const float* grad_out, int64_t grad_row_stride,
                                   const int32_t* feat_requires_grad, float* grad_indice_weights,
                                   const int64_t* feat_window, void* stream) {
  TBE_REQUIRE(F > 0 && B >= 0 && N >= 0, "%s: bad sizes F=%d B=%d N=%lld", who, F, B, (long long)N);
  if (pooling_mode == TBE_POOL_NONE) {
    set_error("%s: PoolingMode.NONE takes no per_sample_weights", who);
    return TBE_ERR_UNSUPPORTED;
  }
  TBE_REQUIRE(pooling_mode == TBE_POOL_SUM || pooling_mode == TBE_POOL_MEAN,
              "%s: pooling_mode %d is not pooled", who, pooling_mode);
  TBE_REQUIRE(max_D > 0 && max_D <= 2048, "%s: max_D=%d outside (0, 2048]", who, max_D);
  TBE_REQUIRE(grad_row_stride > 0, "%s: grad_row_stride <= 0", who);
  if (N == 0) return TBE_OK;
  TBE_REQUIRE(grad_indice_weights != nullptr, "%s: null grad_indice_weights", who);
  TBE_REQUIRE(B == 0 || (feat_weights && feat_D && feat_out_offset && feat_rows && offsets && grad_out && indices),
              "%s: null pointer", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // every element is written: positions in no well-formed bag and masked features keep this 0
  if (hipMemsetAsync(grad_indice_weights, 0, static_cast<size_t>(N) * sizeof(float), st) != hipSuccess) {
    set_error("%s: memset of grad_indice_weights failed: %s", who, hipGetErrorString(hipGetLastError()));
    return TBE_ERR_LAUNCH;
  }
  if (B == 0) return TBE_OK;
  IwgArgs a{feat_weights, feat_D, feat_out_offset, feat_rows, feat_window, feat_pooling, feat_requires_grad,
            indices, offsets, grad_out, grad_indice_weights, grad_row_stride, N, F, B, 64};
  // the forward's launch rules (forward_pooled)
  if (static_cast<int64_t>(F) * B < (static_cast<int64_t>(1) << 19)) a.bags_per_wave = 16;
  const bool mean = pooling_mode == TBE_POOL_MEAN;
  const double avg_len = static_cast<double>(N) / (static_cast<double>(F) * B);
  const bool long_bags = avg_len >= 3.5;
  if (max_D <= 64) return launch_iwg<WT, 16, 1>(who, a, mean, long_bags, st);
  if (max_D <= 128) return launch_iwg<WT, 32, 1>(who, a, mean, long_bags, st);
  if (max_D <= 256) return launch_iwg<WT, 64, 1>(who, a, mean, long_bags, st);
  if (max_D <= 512) return launch_iwg<WT, 64, 2>(who, a, mean, long_bags, st);
  if (max_D <= 1024) return launch_iwg<WT, 64, 4>(who, a, mean, long_bags, st);
  return launch_iwg<WT, 64, 8>(who, a, mean, long_bags, st);
}

}  // namespace tbe
