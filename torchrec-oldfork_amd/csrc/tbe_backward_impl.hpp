// TBE backward + fused "exact" optimizer for gfx950: the update and fix-up kernels, templates over
// the table element type WT (float or _Float16).  tbe_backward.hip (FP32 tables, plus the
// weight-independent linearize + sort phase) and tbe_backward_f16.hip instantiate them; the pipeline
// is described at the top of tbe_backward.hip.  All arithmetic is FP32 on float(w); only the final
// store of a row converts to WT.
#pragma once
#include <cstdlib>
#include <cstring>

#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "radix_sort.hpp"

namespace tbe {

struct BwdArgs {
  const uint64_t* feat_weights;
  const int32_t* feat_D;
  const int64_t* feat_out_offset;
  const int64_t* feat_rows;
  const int64_t* feat_row_base;
  const int64_t* feat_window;
  const int32_t* feat_pooling;  // per-feature SUM / MEAN under pooling_mode MEAN, or nullptr = uniform
  const uint64_t* feat_state0;
  const uint64_t* feat_state1;
  const int64_t* indices;
  const int64_t* offsets;
  const float* psw;
  const float* grad_out;
  int64_t grad_stride;
  int64_t N;
  int32_t F;
  int32_t B;
  int32_t pooling_mode;
  int32_t key_bits;
  int32_t C;  // contributions per chunk
  tbe_optimizer_args opt;
  float bias1;  // ADAM, PARTIAL_ROWWISE_ADAM: 1 - beta1^t
  float bias2;  // ADAM, PARTIAL_ROWWISE_ADAM: 1 - beta2^t
  float momentum;      // LARS_SGD (tbe_optimizer_ext)
  float eta;           // LARS_SGD
  float max_gradient;  // gradient clipping bound; < 0 = no clipping
  // workspace
  void* keys_sorted;
  const void* payload_sorted;  // uint32 bag numbers, or uint64 (bag << 32) | position
  float* partial_first;  // [nchunks][max_D_pad]
  float* partial_last;   // [nchunks][max_D_pad]
  int32_t* origin_list;  // [nchunks] chunks whose last run continues (compacted, any order)
  int32_t* origin_count; // [1]
  int32_t max_D_pad;
  int32_t fast_D;  // uniform feature dim when TBE_FLAG_UNIFORM_ALIGNED, else 0
  int32_t* bounds_errors;
  unsigned long long* unique_rows;  // optional profiling counter: table rows updated
  // _Float16 tables only: how the FP32 result of a row update becomes a half (TBE_ROUND_*)
  int32_t rounding;
  uint32_t round_hash;  // call_hash(seed, opt.iteration)
  // host side only (launch_update picks the kernel by it): leave the single contributions to the caller, who has
  // applied them already (tbe_backward_apply_skip_single_f32)
  int32_t skip_single;
};

// The ONE rule for "contribution k (sorted position) is the only contribution of the call to its row": a valid key
// (below the sentinel) that neither sorted neighbour shares.  `has_prev` / `has_next`: the position is not the first /
// last of the sorted array.  tbe_backward_single_flags publishes it per contribution and the gather backward applies
// SGD to exactly those rows; bwd_update_kernel<..., SKIP> leaves exactly those out.  A single's run has length one, so
// it never crosses a chunk boundary: partials, origin list and fix-up never see it.
template <typename KeyT>
__device__ __forceinline__ bool key_is_single(KeyT key, KeyT prev, bool has_prev, KeyT next, bool has_next, KeyT sentinel) {
  return key < sentinel && !(has_prev && prev == key) && !(has_next && next == key);
}

template <typename PayT>
__device__ __forceinline__ PayT make_payload(uint32_t bag, uint32_t pos) {
  if constexpr (sizeof(PayT) == 4) return bag;
  else return (static_cast<uint64_t>(bag) << 32) | pos;
}
template <typename PayT>
__device__ __forceinline__ uint32_t payload_bag(PayT p) {
  if constexpr (sizeof(PayT) == 4) return p;
  else return static_cast<uint32_t>(p >> 32);
}
template <typename PayT>
__device__ __forceinline__ uint32_t payload_pos(PayT p) {
  if constexpr (sizeof(PayT) == 4) return 0u;  // never used: no per-sample weights, pooled
  else return static_cast<uint32_t>(p);
}

__device__ __forceinline__ float4 ldc(const float* row, int d, int D, bool vec) {
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    x = ld4(row + d);
  } else {
    if (d + 0 < D) x.x = row[d + 0];
    if (d + 1 < D) x.y = row[d + 1];
    if (d + 2 < D) x.z = row[d + 2];
    if (d + 3 < D) x.w = row[d + 3];
  }
  return x;
}
__device__ __forceinline__ void stc(float* row, int d, int D, bool vec, float4 x) {
  if (vec) {
    st4(row + d, x);
  } else {
    if (d + 0 < D) row[d + 0] = x.x;
    if (d + 1 < D) row[d + 1] = x.y;
    if (d + 2 < D) row[d + 2] = x.z;
    if (d + 3 < D) row[d + 3] = x.w;
  }
}

__device__ __forceinline__ float4 ldc(const _Float16* row, int d, int D, bool vec) {
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    const half4 h = ldh4(row + d);
    x = make_float4(static_cast<float>(h.x), static_cast<float>(h.y), static_cast<float>(h.z), static_cast<float>(h.w));
  } else {
    if (d + 0 < D) x.x = static_cast<float>(row[d + 0]);
    if (d + 1 < D) x.y = static_cast<float>(row[d + 1]);
    if (d + 2 < D) x.z = static_cast<float>(row[d + 2]);
    if (d + 3 < D) x.w = static_cast<float>(row[d + 3]);
  }
  return x;
}

// Stochastic rounding of a finite FP32 value x to one of its two FP16 neighbours lo <= x <= hi:
// P(hi) = (x - lo) / (hi - lo) in steps of 2^-13, from 13 random bits.  A representable x is kept.
//  * |x| >= 2^-14 (normal halves): the 13 float mantissa bits a half drops are the position of x
//    between its neighbours; adding the random bits to them and clearing them rounds the magnitude
//    up exactly when random >= 2^13 - dropped.  A carry out of the mantissa moves to the next
//    binade, beyond 65504 to infinity (as the nearest-even conversion does from 65520).
//  * |x| < 2^-14: halves are spaced 2^-24 there; the same draw is made in fixed point on
//    trunc(|x| * 2^37) (< 2^23, 13 fraction bits below the half's unit).
// The value handed to the cast is representable, so the cast is exact in every rounding mode.
__device__ __forceinline__ _Float16 round_stochastic(float x, uint32_t r13) {
  const uint32_t bits = __float_as_uint(x);
  const uint32_t mag = bits & 0x7fffffffu;
  if (mag >= 0x7f800000u) return static_cast<_Float16>(x);  // inf / nan
  const float big = __uint_as_float((bits + r13) & ~0x1fffu);
  const uint32_t units = (static_cast<uint32_t>(fminf(__uint_as_float(mag) * 137438953472.f, 8388608.f)) + r13) >> 13;  // of 2^-24
  const float small = copysignf(static_cast<float>(units) * (1.f / 16777216.f), x);
  return static_cast<_Float16>(mag >= 0x38800000u ? big : small);  // 2^-14
}

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {  // the murmur3 finalizer: full avalanche
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// The random bits of one row update: a counter-based hash of (seed, iteration, global row key, column) and
// nothing else, so the stored table does not depend on chunking, geometry or which kernel finished the row.
// call_hash (host, once per call) covers (seed, iteration); row_hash adds the key; columns [d, d+4) (d a
// multiple of 4) draw 13 bits each from two words hashed from the row's word and d / 4.
inline uint32_t call_hash(uint64_t seed, int64_t iteration) {
  uint32_t h = fmix32(static_cast<uint32_t>(seed) ^ 0x9e3779b9u);
  h = fmix32(h ^ static_cast<uint32_t>(seed >> 32));
  h = fmix32(h ^ static_cast<uint32_t>(iteration));
  return fmix32(h ^ static_cast<uint32_t>(static_cast<uint64_t>(iteration) >> 32));
}
__device__ __forceinline__ uint32_t row_hash(uint32_t call, uint64_t key) {
  return fmix32((call ^ static_cast<uint32_t>(key)) + static_cast<uint32_t>(key >> 32) * 0x9e3779b1u);
}

// Stores the FP32 result columns [d, d+4) of a row.  float rows: as they are.
struct RowRounding {
  int32_t mode;
  uint32_t rowh;
};
__device__ __forceinline__ void stw(float* row, int d, int D, bool vec, float4 x, const RowRounding&) {
  stc(row, d, D, vec, x);
}
// _Float16 rows: nearest-even is the IEEE conversion (a plain cast); one 8-B store on the vector path.
__device__ __forceinline__ void stw(_Float16* row, int d, int D, bool vec, float4 x, const RowRounding& rr) {
  half4 h;
  if (rr.mode == TBE_ROUND_STOCHASTIC) {
    const uint32_t c = static_cast<uint32_t>(d) >> 2;
    const uint32_t r0 = fmix32(rr.rowh ^ (2u * c + 1u) * 0x9e3779b1u);
    const uint32_t r1 = fmix32(rr.rowh ^ (2u * c + 2u) * 0x9e3779b1u);
    h.x = round_stochastic(x.x, r0 & 0x1fffu);
    h.y = round_stochastic(x.y, (r0 >> 16) & 0x1fffu);
    h.z = round_stochastic(x.z, r1 & 0x1fffu);
    h.w = round_stochastic(x.w, (r1 >> 16) & 0x1fffu);
  } else {
    h.x = static_cast<_Float16>(x.x);
    h.y = static_cast<_Float16>(x.y);
    h.z = static_cast<_Float16>(x.z);
    h.w = static_cast<_Float16>(x.w);
  }
  if (vec) {
    sth4(row + d, h);
  } else {
    if (d + 0 < D) row[d + 0] = h.x;
    if (d + 1 < D) row[d + 1] = h.y;
    if (d + 2 < D) row[d + 2] = h.z;
    if (d + 3 < D) row[d + 3] = h.w;
  }
}
// The hash of a row's key, where the table type and the rounding mode need one (0 otherwise): the update kernel
// computes it next to the key it loaded, the fix-up kernel from the key of the run.
template <typename WT>
__device__ __forceinline__ uint32_t row_hash_if_needed(const BwdArgs& a, uint64_t key) {
  if constexpr (sizeof(WT) == 2) {
    if (a.rounding == TBE_ROUND_STOCHASTIC) return row_hash(a.round_hash, key);
  }
  return 0u;
}

// Sum over the G lanes of a group (G consecutive lanes), fixed butterfly order.
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// OPTC of the row-norm family (LAMB, PARTIAL_ROWWISE_ADAM, PARTIAL_ROWWISE_LAMB, LARS_SGD; chosen at run time inside
// it): its own instantiations, so that the generic ones (OPTC = -1) keep their register footprint.
constexpr int kOptNormFamily = -2;
__host__ __device__ __forceinline__ bool is_norm_family(int optimizer) {
  return optimizer >= TBE_OPT_LAMB && optimizer <= TBE_OPT_LARS_SGD;
}

// x . x added to s in column order; columns beyond D must be zero in x.
__device__ __forceinline__ float sumsq4(float4 x, float s) {
  s = fmaf(x.x, x.x, s);
  s = fmaf(x.y, x.y, s);
  s = fmaf(x.z, x.z, s);
  return fmaf(x.w, x.w, s);
}
// Zeroes the columns of x (columns [d, d+4)) that lie beyond D: values computed from zero-filled loads need not be zero.
__device__ __forceinline__ float4 mask_tail(float4 x, int d, int D) {
  if (d + 1 >= D) x.y = 0.f;
  if (d + 2 >= D) x.z = 0.f;
  if (d + 3 >= D) x.w = 0.f;
  return x;
}

// The row-norm family (formulas: include/tbe_hip.h, tbe_backward_*_ex_*).  Two passes over register-resident data: the
// first updates the element-wise state (loaded and stored once, never held), leaves the update direction u in g's
// registers and sums the norms; the second writes the row.  Live across the norm: w and g only, as for ADAM.
template <typename WT, int G, int NV>
__device__ __forceinline__ void apply_row_norm(const BwdArgs& a, int f, int64_t local_row, int D, bool vec, int gl,
                                               WT* wrow, float4 (&w)[NV], float4 (&g)[NV], const RowRounding& rr) {
  const int optimizer = a.opt.optimizer;
  const float lr = a.opt.learning_rate, wd = a.opt.weight_decay;
  float* m1row = reinterpret_cast<float*>(a.feat_state0[f]) + local_row * D;
  const bool m1vec = vec && ((reinterpret_cast<uintptr_t>(m1row) & 15) == 0);
  // columns beyond D are zero in w and g (never loaded)
  float ww = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v)
    if ((v * G + gl) * 4 < D) ww = sumsq4(w[v], ww);
  if (optimizer == TBE_OPT_LARS_SGD) {
    float gg = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if ((v * G + gl) * 4 < D) gg = sumsq4(g[v], gg);
    const float wn = sqrtf(group_sum<G>(ww)), gn = sqrtf(group_sum<G>(gg));
    const float alr = (wn > 0.f && gn > 0.f) ? lr * a.eta * wn / (gn + wd * wn) : lr;
    const float mom = a.momentum;
#define TBE_LARS1(c)                                        \
  m.c = fmaf(mom, m.c, alr * fmaf(wd, w[v].c, g[v].c));     \
  r.c = w[v].c - m.c;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) {
        float4 m = ldc(m1row, d, D, m1vec);
        float4 r;
        TBE_LARS1(x) TBE_LARS1(y) TBE_LARS1(z) TBE_LARS1(w)
        stc(m1row, d, D, m1vec, m);
        stw(wrow, d, D, vec, r, rr);
      }
    }
#undef TBE_LARS1
    return;
  }
  const float b1 = a.opt.beta1, b2 = a.opt.beta2, eps = a.opt.eps;
  const bool lamb = optimizer == TBE_OPT_LAMB;
  const bool adam = optimizer == TBE_OPT_PARTIAL_ROWWISE_ADAM;
  float den_row = 1.f;  // PARTIAL_ROWWISE_*: the row's denominator
  float* m2row = nullptr;
  bool m2vec = false;
  if (lamb) {
    m2row = reinterpret_cast<float*>(a.feat_state1[f]) + local_row * D;
    m2vec = vec && ((reinterpret_cast<uintptr_t>(m2row) & 15) == 0);
  } else {
    float ss = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if ((v * G + gl) * 4 < D) ss = sumsq4(g[v], ss);
    ss = group_sum<G>(ss);
    float* vp = reinterpret_cast<float*>(a.feat_state1[f]) + local_row;
    const float v_new = fmaf(b2, *vp, (1.f - b2) * (ss / static_cast<float>(D)));
    if (gl == 0) *vp = v_new;
    den_row = adam ? sqrtf(v_new / a.bias2) + eps : sqrtf(v_new) + eps;
  }
  const float m1div = adam ? a.bias1 : 1.f;
  float uu = 0.f;
#define TBE_NORM_M1(c) m1.c = fmaf(b1, m1.c, (1.f - b1) * g[v].c);
#define TBE_NORM_M2(c)                                   \
  m2.c = fmaf(b2, m2.c, (1.f - b2) * g[v].c * g[v].c);   \
  den.c = sqrtf(m2.c) + eps;
#define TBE_NORM_U(c) u.c = (m1.c / m1div) / den.c + wd * w[v].c;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int d = (v * G + gl) * 4;
    if (d < D) {
      float4 m1 = ldc(m1row, d, D, m1vec);
      TBE_NORM_M1(x) TBE_NORM_M1(y) TBE_NORM_M1(z) TBE_NORM_M1(w)
      stc(m1row, d, D, m1vec, m1);
      float4 den = make_float4(den_row, den_row, den_row, den_row);
      if (lamb) {
        float4 m2 = ldc(m2row, d, D, m2vec);
        TBE_NORM_M2(x) TBE_NORM_M2(y) TBE_NORM_M2(z) TBE_NORM_M2(w)
        stc(m2row, d, D, m2vec, m2);
      }
      float4 u;
      TBE_NORM_U(x) TBE_NORM_U(y) TBE_NORM_U(z) TBE_NORM_U(w)
      g[v] = mask_tail(u, d, D);
      uu = sumsq4(g[v], uu);
    }
  }
#undef TBE_NORM_M1
#undef TBE_NORM_M2
#undef TBE_NORM_U
  float step = lr;
  if (!adam) {  // the trust ratio |w| / |u|, 1 when either norm is zero
    const float wn = sqrtf(group_sum<G>(ww)), un = sqrtf(group_sum<G>(uu));
    if (wn > 0.f && un > 0.f) step = lr * (wn / un);
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int d = (v * G + gl) * 4;
    if (d < D) {
      float4 r;
      r.x = fmaf(-step, g[v].x, w[v].x);
      r.y = fmaf(-step, g[v].y, w[v].y);
      r.z = fmaf(-step, g[v].z, w[v].z);
      r.w = fmaf(-step, g[v].w, w[v].w);
      stw(wrow, d, D, vec, r, rr);
    }
  }
}

// Applies the optimizer to one table row.  `g` = coalesced gradient columns held by this lane,
// `w` = current weight columns (pre-loaded).  Group-uniform control flow.
// OPTC >= 0 fixes the optimizer at compile time (smaller live state => more waves per SIMD).
template <typename WT, int G, int NV, int OPTC = -1>
__device__ __forceinline__ void apply_row(const BwdArgs& a, int f, int64_t local_row, int D,
                                          bool vec, int gl, WT* wrow, float4 (&w)[NV],
                                          float4 (&g)[NV], uint32_t rowh) {
  const RowRounding rr{sizeof(WT) == 2 ? a.rounding : TBE_ROUND_NEAREST_EVEN, rowh};
  if constexpr (OPTC == kOptNormFamily) {
    apply_row_norm<WT, G, NV>(a, f, local_row, D, vec, gl, wrow, w, g, rr);
    return;
  }
  const int optimizer = OPTC >= 0 ? OPTC : a.opt.optimizer;
  const float lr = a.opt.learning_rate;
  if (optimizer == TBE_OPT_EXACT_SGD) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) {
        float4 r;
        r.x = fmaf(-lr, g[v].x, w[v].x);
        r.y = fmaf(-lr, g[v].y, w[v].y);
        r.z = fmaf(-lr, g[v].z, w[v].z);
        r.w = fmaf(-lr, g[v].w, w[v].w);
        stw(wrow, d, D, vec, r, rr);
      }
    }
  } else if (optimizer == TBE_OPT_EXACT_ROWWISE_ADAGRAD) {
    const float wd = a.opt.weight_decay;
    float ss = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) {
        if (wd != 0.f) {
          g[v].x = fmaf(wd, w[v].x, g[v].x);
          g[v].y = fmaf(wd, w[v].y, g[v].y);
          g[v].z = fmaf(wd, w[v].z, g[v].z);
          g[v].w = fmaf(wd, w[v].w, g[v].w);
        }
        // columns beyond D are zero in g (never loaded), so the vector form is safe
        ss = fmaf(g[v].x, g[v].x, ss);
        ss = fmaf(g[v].y, g[v].y, ss);
        ss = fmaf(g[v].z, g[v].z, ss);
        ss = fmaf(g[v].w, g[v].w, ss);
      }
    }
    ss = group_sum<G>(ss);
    float* m = reinterpret_cast<float*>(a.feat_state0[f]) + local_row;
    const float m_new = *m + ss / static_cast<float>(D);
    const float mult = lr / (sqrtf(m_new) + a.opt.eps);
    if (gl == 0) *m = m_new;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) {
        float4 r;
        r.x = fmaf(-mult, g[v].x, w[v].x);
        r.y = fmaf(-mult, g[v].y, w[v].y);
        r.z = fmaf(-mult, g[v].z, w[v].z);
        r.w = fmaf(-mult, g[v].w, w[v].w);
        stw(wrow, d, D, vec, r, rr);
      }
    }
  } else if (optimizer == TBE_OPT_DENSE_GRAD) {
    float* grow = reinterpret_cast<float*>(a.feat_state0[f]) + local_row * D;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) stc(grow, d, D, vec && ((reinterpret_cast<uintptr_t>(grow) & 15) == 0), g[v]);
    }
  } else if (optimizer == TBE_OPT_EXACT_ADAGRAD) {
    float* mrow = reinterpret_cast<float*>(a.feat_state0[f]) + local_row * D;
    const bool mvec = vec && ((reinterpret_cast<uintptr_t>(mrow) & 15) == 0);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) {
        float4 m = ldc(mrow, d, D, mvec);
        m.x = fmaf(g[v].x, g[v].x, m.x);
        m.y = fmaf(g[v].y, g[v].y, m.y);
        m.z = fmaf(g[v].z, g[v].z, m.z);
        m.w = fmaf(g[v].w, g[v].w, m.w);
        stc(mrow, d, D, mvec, m);
        float4 r;
        r.x = w[v].x - lr * g[v].x / (sqrtf(m.x) + a.opt.eps);
        r.y = w[v].y - lr * g[v].y / (sqrtf(m.y) + a.opt.eps);
        r.z = w[v].z - lr * g[v].z / (sqrtf(m.z) + a.opt.eps);
        r.w = w[v].w - lr * g[v].w / (sqrtf(m.w) + a.opt.eps);
        stw(wrow, d, D, vec, r, rr);
      }
    }
  } else if (optimizer == TBE_OPT_ADAM) {
    float* m1row = reinterpret_cast<float*>(a.feat_state0[f]) + local_row * D;
    float* m2row = reinterpret_cast<float*>(a.feat_state1[f]) + local_row * D;
    const bool mvec = vec && ((reinterpret_cast<uintptr_t>(m1row) & 15) == 0) &&
                      ((reinterpret_cast<uintptr_t>(m2row) & 15) == 0);
    const float b1 = a.opt.beta1, b2 = a.opt.beta2, eps = a.opt.eps, wd = a.opt.weight_decay;
#define TBE_ADAM1(c)                                                     \
  m1.c = fmaf(b1, m1.c, (1.f - b1) * g[v].c);                            \
  m2.c = fmaf(b2, m2.c, (1.f - b2) * g[v].c * g[v].c);                   \
  r.c = w[v].c - lr * ((m1.c / a.bias1) / (sqrtf(m2.c / a.bias2) + eps) + wd * w[v].c);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) {
        float4 m1 = ldc(m1row, d, D, mvec);
        float4 m2 = ldc(m2row, d, D, mvec);
        float4 r;
        TBE_ADAM1(x) TBE_ADAM1(y) TBE_ADAM1(z) TBE_ADAM1(w)
        stc(m1row, d, D, mvec, m1);
        stc(m2row, d, D, mvec, m2);
        stw(wrow, d, D, vec, r, rr);
      }
    }
#undef TBE_ADAM1
  }
}

template <int NV>
struct BwdUnroll {
  static constexpr int U = NV == 1 ? 4 : (NV == 2 ? 2 : 1);
};

// FAST: every feature has dim a.fast_D (multiple of 4), SUM pooling, no per-sample weights, every
// row base 16-B aligned (TBE_FLAG_UNIFORM_ALIGNED from the host) — the Criteo configuration.
// SKIP: single contributions (key_is_single) were applied by the caller: no gradient-row load, no weight-row load, no
// apply_row for them; they still count as updated rows.
template <typename WT, typename KeyT, typename PayT, int G, int NV, int OPTC, bool FAST, int U, int MINW, bool SKIP = false>
__global__ __launch_bounds__(256, MINW) void bwd_update_kernel(BwdArgs a) {
  constexpr int NG = kWave / G;
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int gl = lane % G;
  const int gbase = g * G;  // first lane of this group
  const int64_t nchunks = (a.N + a.C - 1) / a.C;
  const int64_t chunk = (static_cast<int64_t>(blockIdx.x) * (blockDim.x / kWave) + (threadIdx.x >> 6)) * NG + g;
  // Whole wave out of range -> exit; a partially filled wave keeps its idle groups alive
  // (they execute the shuffles with in-range flags false).
  const int64_t chunk_w0 = chunk - g;
  if (chunk_w0 >= nchunks) return;
  const bool active = chunk < nchunks;

  const KeyT* __restrict__ skey = static_cast<const KeyT*>(a.keys_sorted);
  const PayT* __restrict__ spay = static_cast<const PayT*>(a.payload_sorted);
  const KeyT sentinel = static_cast<KeyT>((a.key_bits >= 64) ? ~0ull : ((1ull << a.key_bits) - 1ull));
  const bool nobag = a.pooling_mode == TBE_POOL_NONE;
  const bool mean = a.pooling_mode == TBE_POOL_MEAN;

  const int64_t i0 = active ? chunk * a.C : 0;
  const int64_t i1 = active ? min(a.N, i0 + static_cast<int64_t>(a.C)) : 0;
  bool started_here = true;
  if (active && i0 > 0) started_here = skey[i0 - 1] != skey[i0];
  bool tail_open = false;  // last processed contribution did not end its run
  int nrows = 0;           // table rows this group finished (profiling counter)

  float4 acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);

  // The loop trip count must be wave-uniform for the shuffles: use the max span over groups.
  const int span = static_cast<int>(i1 - i0);
  int max_span = span;
#pragma unroll
  for (int o = 32; o >= G; o >>= 1) max_span = max(max_span, __shfl_xor(max_span, o, kWave));

  for (int sb = 0; sb < max_span; sb += G) {
    const int64_t kk = i0 + sb + gl;
    const bool in = active && kk < i1;
    KeyT key_k = sentinel;
    KeyT keyn_k = sentinel;
    PayT pay_k = 0;
    if (in) {
      key_k = skey[kk];
      pay_k = spay[kk];
      if (kk + 1 < a.N) keyn_k = skey[kk + 1];
    }
    bool single_k = false;
    if constexpr (SKIP) {
      if (in) single_k = key_is_single<KeyT>(key_k, kk > 0 ? skey[kk - 1] : sentinel, kk > 0, keyn_k, kk + 1 < a.N, sentinel);
    }
    // sentinel = invalid id; anything above = never written; a skipped single is no work for this kernel
    const bool valid_k = in && key_k < sentinel && !single_k;
    const bool last_k = valid_k && (key_k != keyn_k || kk + 1 >= a.N);
    const uint32_t bag_k = payload_bag<PayT>(pay_k);
    const uint32_t pos_k = payload_pos<PayT>(pay_k);
    const int f_k = valid_k ? static_cast<int>(bag_k / static_cast<uint32_t>(a.B)) : 0;
    const int b_k = static_cast<int>(bag_k - static_cast<uint32_t>(f_k) * static_cast<uint32_t>(a.B));
    const int D_k = FAST ? a.fast_D : a.feat_D[f_k];
    float w_k = 1.f;
    const float* gptr_k = a.grad_out;
    const WT* wptr_k = nullptr;
    int64_t lrow_k = 0;
    if (valid_k) {
      if (!FAST) {
        if (a.psw != nullptr) w_k = a.psw[pos_k];
        if (mean && (a.feat_pooling == nullptr || a.feat_pooling[f_k] == TBE_POOL_MEAN)) {
          const int64_t len = a.offsets[bag_k + 1] - a.offsets[bag_k];
          w_k = w_k / static_cast<float>(len);
        }
      }
      gptr_k = (!FAST && nobag) ? a.grad_out + static_cast<int64_t>(pos_k) * a.grad_stride
                     : a.grad_out + static_cast<int64_t>(b_k) * a.grad_stride + a.feat_out_offset[f_k];
      lrow_k = static_cast<int64_t>(key_k) - a.feat_row_base[f_k];
      wptr_k = reinterpret_cast<const WT*>(a.feat_weights[f_k]) + lrow_k * D_k;
    }
    const uint32_t rowh_k = row_hash_if_needed<WT>(a, static_cast<uint64_t>(key_k));
    const int n = active ? static_cast<int>(min<int64_t>(G, i1 - (i0 + sb))) : 0;
    int max_n = n;
#pragma unroll
    for (int o = 32; o >= G; o >>= 1) max_n = max(max_n, __shfl_xor(max_n, o, kWave));

    for (int j = 0; j < max_n; j += U) {
      float4 x[U][NV];
      float4 wr[U][NV];
      float wt[U];
      bool val[U], lst[U];
      const WT* wp[U];
      int Du[U], fu[U];
      int64_t lrow[U];
      bool vecu[U];
      uint32_t rowh[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int src = gbase + ((j + u) & (G - 1));
        const bool inb = (j + u) < n;
        // (a skipped single still takes its trip of this loop: walking only the lanes with work — tried, the set bits
        // of a ballot — made the kernel 5 % slower, not faster)
        if constexpr (SKIP) nrows += (inb && __shfl(static_cast<int>(single_k), src, kWave) != 0) ? 1 : 0;
        val[u] = inb && (__shfl(static_cast<int>(valid_k), src, kWave) != 0);
        lst[u] = inb && (__shfl(static_cast<int>(last_k), src, kWave) != 0);
        wt[u] = FAST ? 1.f : __shfl(w_k, src, kWave);
        const float* gp = reinterpret_cast<const float*>(shflu64(reinterpret_cast<uint64_t>(gptr_k), src));
        wp[u] = reinterpret_cast<const WT*>(shflu64(reinterpret_cast<uint64_t>(wptr_k), src));
        Du[u] = FAST ? a.fast_D : __shfl(D_k, src, kWave);
        fu[u] = __shfl(f_k, src, kWave);
        lrow[u] = shfl64(lrow_k, src);
        rowh[u] = sizeof(WT) == 2 ? static_cast<uint32_t>(__shfl(static_cast<int>(rowh_k), src, kWave)) : 0u;
        const bool gvec = FAST || (((Du[u] & 3) == 0) && ((reinterpret_cast<uintptr_t>(gp) & 15) == 0));
        vecu[u] = FAST || (((Du[u] & 3) == 0) && ((reinterpret_cast<uintptr_t>(wp[u]) & kRowAlignMask<WT>) == 0));
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const int d = (v * G + gl) * 4;
          x[u][v] = (val[u] && d < Du[u]) ? ldc(gp, d, Du[u], gvec) : make_float4(0.f, 0.f, 0.f, 0.f);
          // the current weight row (not needed when the coalesced gradient is only written out: DENSE_GRAD)
          wr[u][v] = (OPTC != TBE_OPT_DENSE_GRAD && lst[u] && d < Du[u]) ? ldc(wp[u], d, Du[u], vecu[u])
                                                                          : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (val[u]) {
          if (!FAST && a.max_gradient >= 0.f) {  // gradient clipping: the loaded element, before weight and MEAN division
            const float mg = a.max_gradient;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
              x[u][v].x = fminf(fmaxf(x[u][v].x, -mg), mg);
              x[u][v].y = fminf(fmaxf(x[u][v].y, -mg), mg);
              x[u][v].z = fminf(fmaxf(x[u][v].z, -mg), mg);
              x[u][v].w = fminf(fmaxf(x[u][v].w, -mg), mg);
            }
          }
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            acc[v].x = fmaf(wt[u], x[u][v].x, acc[v].x);
            acc[v].y = fmaf(wt[u], x[u][v].y, acc[v].y);
            acc[v].z = fmaf(wt[u], x[u][v].z, acc[v].z);
            acc[v].w = fmaf(wt[u], x[u][v].w, acc[v].w);
          }
          tail_open = !lst[u];
          if (lst[u]) {
            if (started_here) {
              ++nrows;
              apply_row<WT, G, NV, OPTC>(a, fu[u], lrow[u], Du[u], vecu[u], gl, const_cast<WT*>(wp[u]), wr[u], acc, rowh[u]);
            } else {
              float* pf = a.partial_first + chunk * a.max_D_pad;
#pragma unroll
              for (int v = 0; v < NV; ++v) {
                const int d = (v * G + gl) * 4;
                if (d < Du[u]) st4(pf + d, acc[v]);
              }
            }
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
            started_here = true;
          }
        }
      }
    }
  }
  if (active) {
    int is_origin = 0;
    if (tail_open) {
      float* dst = started_here ? a.partial_last + chunk * a.max_D_pad : a.partial_first + chunk * a.max_D_pad;
      is_origin = started_here ? 1 : 0;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int d = (v * G + gl) * 4;
        if (d < a.max_D_pad) st4(dst + d, acc[v]);
      }
    }
    if (gl == 0 && is_origin) a.origin_list[atomicAdd(a.origin_count, 1)] = static_cast<int32_t>(chunk);
    nrows += is_origin;
  }
  if (a.unique_rows != nullptr) {  // profiling only: one add per WAVE, spread over kProfileRowSlots cache lines
    int wave_rows = (active && gl == 0) ? nrows : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wave_rows += __shfl_xor(wave_rows, o, kWave);
    if (lane == 0 && wave_rows > 0)
      atomicAdd(a.unique_rows + ((blockIdx.x * 4 + (threadIdx.x >> 6)) % kProfileRowSlots) * 16,
                static_cast<unsigned long long>(wave_rows));
  }
}

// Fix-up: every "origin" chunk owns a run that continues into the following chunks.  One wave
// per origin: the wave gallops over the following chunk heads (64 per step) to find the chain
// length, its NG groups sum contiguous halves of the chain's partial rows (4 loads in flight)
// and the halves are combined through LDS in fixed order.  Chains longer than kLongChain
// (rows of tiny tables that receive thousands of contributions) are summed by the whole
// workgroup: 4*NG groups, LDS-staged partials, fixed combine order => bitwise reproducible.
constexpr int kLongChain = 24;

template <typename KeyT, int G, int NV>
struct FixupRow {
  int f;
  int D;
  int64_t lrow;
  float* wrow;
  bool vec;
};

template <int G, int NV>
__device__ __forceinline__ void sum_partials(const float* __restrict__ base, int max_D_pad, int64_t first,
                                             int begin, int end, int D, int gl, float4 (&acc)[NV]) {
  constexpr int U = 4;
  for (int j = begin; j < end; j += U) {
    float4 x[U][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float* pf = base + (first + j + u) * max_D_pad;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int d = (v * G + gl) * 4;
        x[u][v] = (j + u < end && d < D) ? ld4(pf + d) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        acc[v].x += x[u][v].x;
        acc[v].y += x[u][v].y;
        acc[v].z += x[u][v].z;
        acc[v].w += x[u][v].w;
      }
  }
}

template <typename WT, typename KeyT, typename PayT, int G, int NV, int OPTC>
__global__ __launch_bounds__(256) void bwd_fixup_kernel(BwdArgs a) {
  constexpr int NG = kWave / G;
  constexpr int NGB = 4 * NG;
  __shared__ float4 part[NGB][NV][G];
  __shared__ int64_t long_chunk[4];
  __shared__ int long_len[4];
  __shared__ int n_long;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / G;
  const int gl = lane % G;
  const int q = wave * NG + g;  // group index inside the block
  const int64_t nchunks = (a.N + a.C - 1) / a.C;
  const KeyT* __restrict__ skey = static_cast<const KeyT*>(a.keys_sorted);
  const PayT* __restrict__ spay = static_cast<const PayT*>(a.payload_sorted);
  const int count = *a.origin_count;

  for (int base = blockIdx.x * 4; base < count; base += gridDim.x * 4) {  // block-uniform
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    const int oi = base + wave;
    if (oi < count) {  // wave-uniform
      const int64_t chunk = a.origin_list[oi];
      const KeyT key_run = skey[(chunk + 1) * a.C - 1];
      int len = 0;
      bool more = true;
      while (more) {
        const int64_t cc = chunk + 1 + len + lane;
        const bool ok = cc < nchunks && skey[cc * a.C] == key_run;
        const unsigned long long m = __ballot(ok);
        const int lead = (m == ~0ull) ? 64 : __builtin_ctzll(~m);
        len += lead;
        more = lead == 64;
      }
      if (len > kLongChain) {
        if (lane == 0) {
          const int s = atomicAdd(&n_long, 1);
          long_chunk[s] = chunk;
          long_len[s] = len;
        }
      } else {
        const PayT pay = spay[(chunk + 1) * a.C - 1];
        const int f = static_cast<int>(payload_bag<PayT>(pay) / static_cast<uint32_t>(a.B));
        const int D = a.feat_D[f];
        const int64_t lrow = static_cast<int64_t>(key_run) - a.feat_row_base[f];
        WT* wrow = reinterpret_cast<WT*>(a.feat_weights[f]) + lrow * D;
        const bool vec = ((D & 3) == 0) && ((reinterpret_cast<uintptr_t>(wrow) & kRowAlignMask<WT>) == 0);
        float4 acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int per = (len + NG - 1) / NG;
        sum_partials<G, NV>(a.partial_first, a.max_D_pad, chunk + 1, min(len, g * per), min(len, (g + 1) * per), D, gl, acc);
        if (NG > 1) {
#pragma unroll
          for (int v = 0; v < NV; ++v) part[q][v][gl] = acc[v];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (g == 0) {
          float4 tot[NV], w[NV];
          const float* pl = a.partial_last + chunk * a.max_D_pad;
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const int d = (v * G + gl) * 4;
            tot[v] = (d < D) ? ld4(pl + d) : make_float4(0.f, 0.f, 0.f, 0.f);
            w[v] = (d < D) ? ldc(wrow, d, D, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            tot[v].x += acc[v].x;
            tot[v].y += acc[v].y;
            tot[v].z += acc[v].z;
            tot[v].w += acc[v].w;
            for (int og = 1; og < NG; ++og) {
              const float4 o = part[wave * NG + og][v][gl];
              tot[v].x += o.x;
              tot[v].y += o.y;
              tot[v].z += o.z;
              tot[v].w += o.w;
            }
          }
          apply_row<WT, G, NV, OPTC>(a, f, lrow, D, vec, gl, wrow, w, tot,
                            row_hash_if_needed<WT>(a, static_cast<uint64_t>(key_run)));
        }
      }
    }
    __syncthreads();
    const int nl = n_long;
    for (int s = 0; s < nl; ++s) {  // block-uniform
      const int64_t chunk = long_chunk[s];
      const int len = long_len[s];
      const KeyT key_run = skey[(chunk + 1) * a.C - 1];
      const PayT pay = spay[(chunk + 1) * a.C - 1];
      const int f = static_cast<int>(payload_bag<PayT>(pay) / static_cast<uint32_t>(a.B));
      const int D = a.feat_D[f];
      const int64_t lrow = static_cast<int64_t>(key_run) - a.feat_row_base[f];
      WT* wrow = reinterpret_cast<WT*>(a.feat_weights[f]) + lrow * D;
      const bool vec = ((D & 3) == 0) && ((reinterpret_cast<uintptr_t>(wrow) & kRowAlignMask<WT>) == 0);
      float4 acc[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
      const int per = (len + NGB - 1) / NGB;
      sum_partials<G, NV>(a.partial_first, a.max_D_pad, chunk + 1, min(len, q * per), min(len, (q + 1) * per), D, gl, acc);
      __syncthreads();  // previous iteration's readers are done with `part`
#pragma unroll
      for (int v = 0; v < NV; ++v) part[q][v][gl] = acc[v];
      __syncthreads();
      if (q == 0) {
        float4 tot[NV], w[NV];
        const float* pl = a.partial_last + chunk * a.max_D_pad;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const int d = (v * G + gl) * 4;
          tot[v] = (d < D) ? ld4(pl + d) : make_float4(0.f, 0.f, 0.f, 0.f);
          w[v] = (d < D) ? ldc(wrow, d, D, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
          for (int oq = 0; oq < NGB; ++oq) {
            const float4 o = part[oq][v][gl];
            tot[v].x += o.x;
            tot[v].y += o.y;
            tot[v].z += o.z;
            tot[v].w += o.w;
          }
        }
        apply_row<WT, G, NV, OPTC>(a, f, lrow, D, vec, gl, wrow, w, tot,
                            row_hash_if_needed<WT>(a, static_cast<uint64_t>(key_run)));
      }
    }
    __syncthreads();
  }
}

static int pick_chunk(int64_t N) {
  int64_t c = (N + 16383) / 16384;
  c = (c + 31) / 32 * 32;
  if (c < 32) c = 32;
  if (c > 256) c = 256;
  return static_cast<int>(c);
}

struct BwdWorkspace {
  void* keys_in;
  void* keys_out;
  void* pay_in;   // uint32 or uint64 payloads (sized for uint64)
  void* pay_out;
  float* partial_first;
  float* partial_last;
  int32_t* origin_list;
  int32_t* origin_count;
  RadixWorkspace sort;
  size_t total;
};

static int carve(void* ws, int64_t N, int32_t max_D, int32_t key_bits, BwdWorkspace* out) {
  const bool k64 = key_bits > 32;
  const size_t ksz = k64 ? 8 : 4;
  const int C = pick_chunk(N);
  const int64_t nchunks = (N + C - 1) / C;
  const int max_D_pad = (max_D + 3) / 4 * 4;
  const size_t sort_bytes = radix_carve(nullptr, N, key_bits).bytes;
  Carver c(ws);
  out->keys_in = c.take_bytes(N * ksz);
  out->keys_out = c.take_bytes(N * ksz);
  out->pay_in = c.take_bytes(N * sizeof(uint64_t));
  out->pay_out = c.take_bytes(N * sizeof(uint64_t));
  out->partial_first = c.take<float>(nchunks * max_D_pad);
  out->partial_last = c.take<float>(nchunks * max_D_pad);
  out->origin_list = c.take<int32_t>(nchunks);
  out->sort = radix_carve(c.take_bytes(sort_bytes), N, key_bits);
  // zeroed together with the sort's tickets by the one memset radix_sort_pairs issues
  out->origin_count = out->sort.tickets ? reinterpret_cast<int32_t*>(out->sort.tickets + 8) : nullptr;
  out->total = c.total();
  return TBE_OK;
}

template <typename WT, typename KeyT, typename PayT, int G, int NV>
static int launch_update(const BwdArgs& a, hipStream_t st) {
  constexpr int NG = kWave / G;
  const int64_t nchunks = (a.N + a.C - 1) / a.C;
  const int64_t groups_per_block = 4 * NG;
  const unsigned grid = static_cast<unsigned>((nchunks + groups_per_block - 1) / groups_per_block);
  {
    ProfileSpan span(TBE_PROFILE_BWD_UPDATE_KERNEL, st);
    // (a launch with gradient clipping takes the generic kernel: the fast ones have no clamp)
    const bool fast = a.fast_D > 0 && a.pooling_mode == TBE_POOL_SUM && a.psw == nullptr && a.max_gradient < 0.f;
    const int oc = a.opt.optimizer;
#define TBE_UPD(OPTC, FAST_, UU, MW) \
  hipLaunchKernelGGL((bwd_update_kernel<WT, KeyT, PayT, G, NV, OPTC, FAST_, UU, MW>), dim3(grid), dim3(256), 0, st, a)
#define TBE_UPD_SKIP(OPTC, FAST_, UU, MW) \
  hipLaunchKernelGGL((bwd_update_kernel<WT, KeyT, PayT, G, NV, OPTC, FAST_, UU, MW, true>), dim3(grid), dim3(256), 0, st, a)
    if (a.skip_single) {
      // EXACT_SGD on float tables of dim <= 128 with bag payloads (backward_entry checks): the two kernels such a call takes
      if constexpr (std::is_same_v<WT, float> && sizeof(PayT) == 4 && NV == 1 && G <= 32) {
        if (G == 32 && fast) {
          if constexpr (G == 32) TBE_UPD_SKIP(TBE_OPT_EXACT_SGD, true, 4, 4);
        } else {
          TBE_UPD_SKIP(-1, false, BwdUnroll<NV>::U, 1);
        }
      } else {
        set_error("tbe_backward update: no kernel that skips single contributions for this configuration");
        return TBE_ERR_UNSUPPORTED;
      }
    } else if (is_norm_family(oc)) {
      TBE_UPD(kOptNormFamily, false, BwdUnroll<NV>::U, 1);
    } else if constexpr (G == 32 && NV == 1) {  // the fast kernels exist for the one (G, NV) pair that can reach them
      if (fast && oc == TBE_OPT_EXACT_SGD) {
        TBE_UPD(TBE_OPT_EXACT_SGD, true, 4, 4);
      } else if (fast && oc == TBE_OPT_EXACT_ROWWISE_ADAGRAD) {
        TBE_UPD(TBE_OPT_EXACT_ROWWISE_ADAGRAD, true, 4, 4);
      } else if (fast && oc == TBE_OPT_DENSE_GRAD && sizeof(WT) == 4) {
        // the replicated tiny tables of a sharded collection (dense gradient); FP32 tables only
        if constexpr (sizeof(WT) == 4) TBE_UPD(TBE_OPT_DENSE_GRAD, true, 4, 4);
      } else {
        TBE_UPD(-1, false, BwdUnroll<NV>::U, 1);
      }
    } else {
      TBE_UPD(-1, false, BwdUnroll<NV>::U, 1);
    }
#undef TBE_UPD
#undef TBE_UPD_SKIP
  }
  TBE_CHECK_LAUNCH("tbe_backward update");
  const unsigned fgrid = static_cast<unsigned>(std::min<int64_t>((nchunks + 3) / 4, 1024));
  if (is_norm_family(a.opt.optimizer))
    hipLaunchKernelGGL((bwd_fixup_kernel<WT, KeyT, PayT, G, NV, kOptNormFamily>), dim3(fgrid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((bwd_fixup_kernel<WT, KeyT, PayT, G, NV, -1>), dim3(fgrid), dim3(256), 0, st, a);
  TBE_CHECK_LAUNCH("tbe_backward fixup");
  return TBE_OK;
}

constexpr int kPhasePrepare = 1;  // gradient-independent: linearize + sort
constexpr int kPhaseApply = 2;    // update + fix-up

// Update + fix-up on the sorted pairs a prepare phase left in the workspace.
template <typename WT, typename KeyT, typename PayT>
static int run_apply(const BwdArgs& a, int32_t max_D, hipStream_t st) {
  if (max_D <= 64) return launch_update<WT, KeyT, PayT, 16, 1>(a, st);
  if (max_D <= 128) return launch_update<WT, KeyT, PayT, 32, 1>(a, st);
  if (max_D <= 256) return launch_update<WT, KeyT, PayT, 64, 1>(a, st);
  if (max_D <= 512) return launch_update<WT, KeyT, PayT, 64, 2>(a, st);
  if (max_D <= 1024) return launch_update<WT, KeyT, PayT, 64, 4>(a, st);
  return launch_update<WT, KeyT, PayT, 64, 8>(a, st);
}

// One backward call as the ABI passes it: the wrappers of include/tbe_hip.h fill this and hand it to backward_entry.
// They aggregate-initialise the common arguments only and assign everything after them by name.
struct BwdCall {
  // the arguments every apply / fused entry takes, in the ABI's order
  const uint64_t* feat_weights;
  const int32_t* feat_D;
  const int64_t* feat_out_offset;
  const int64_t* feat_rows;
  const int64_t* feat_row_base;
  const uint64_t* feat_state0;
  const uint64_t* feat_state1;
  int32_t F, B, max_D, key_bits;
  const int64_t* indices;
  int64_t N;
  const int64_t* offsets;
  const float* per_sample_weights;
  int32_t pooling_mode;
  const int32_t* feat_pooling;
  const float* grad_out;
  int64_t grad_row_stride;
  tbe_optimizer_args opt;
  int32_t flags;
  void* workspace;
  size_t workspace_bytes;
  // what only some entries take, in the order the ABI appends it
  int32_t* bounds_errors = nullptr;           // fused, prepare
  const int64_t* feat_window = nullptr;       // fused, prepare
  int32_t rounding = TBE_ROUND_NEAREST_EVEN;  // _f16w
  uint64_t seed = 0;                          // _f16w
  const tbe_optimizer_ext* ext = nullptr;     // _ex
  bool skip_single = false;                   // _skip_single
  void* stream = nullptr;
  // not arguments: which entry this is
  const char* who = nullptr;  // its name, for error messages
  int phase = 0;              // kPhasePrepare | kPhaseApply
  bool ex = false;            // a tbe_backward_*_ex_* entry, which alone accepts the row-norm family and `ext`
};

// Argument validation and workspace carving shared by every backward entry point.  Nothing is launched.  *done is set
// when the call has nothing to do.
static int bwd_setup(BwdCall c, BwdArgs* args, BwdWorkspace* ws, bool* wide_payload, bool* done) {
  const char* const who = c.who;
  *done = false;
  TBE_REQUIRE(c.F > 0 && c.B >= 0 && c.N >= 0, "%s: bad sizes", who);
  if (c.phase == kPhasePrepare) {  // gradient / optimizer arguments are not used by this phase
    c.grad_row_stride = 1;
    c.opt.optimizer = TBE_OPT_EXACT_SGD;
  }
  TBE_REQUIRE(c.max_D > 0 && c.max_D <= 2048, "%s: max_D=%d outside (0, 2048]", who, c.max_D);
  TBE_REQUIRE(c.key_bits >= 1 && c.key_bits <= 64, "%s: key_bits=%d", who, c.key_bits);
  TBE_REQUIRE(c.pooling_mode == TBE_POOL_SUM || c.pooling_mode == TBE_POOL_MEAN || c.pooling_mode == TBE_POOL_NONE,
              "%s: pooling_mode %d", who, c.pooling_mode);
  TBE_REQUIRE(static_cast<int64_t>(c.F) * c.B < (1ll << 32), "%s: F*B must be < 2^32", who);
  // the pair sort's histogram words hold {pass tag | count} with a 29-bit count (radix_sort.hpp)
  TBE_REQUIRE(c.N < kSortMaxPairs, "%s: N = %lld ids in one call; the limit is 2^29 - 1 (split the batch)", who,
              static_cast<long long>(c.N));
  TBE_REQUIRE(c.grad_row_stride > 0, "%s: grad_row_stride <= 0", who);
  if (c.phase == (kPhasePrepare | kPhaseApply) && c.per_sample_weights != nullptr) c.flags |= TBE_FLAG_WEIGHTED;
  TBE_REQUIRE(c.per_sample_weights == nullptr || (c.flags & TBE_FLAG_WEIGHTED) != 0,
              "%s: per_sample_weights given but TBE_FLAG_WEIGHTED not set (it must be set in "
              "both tbe_backward_prepare and the apply call)", who);
  const tbe_optimizer_args& opt = c.opt;
  switch (opt.optimizer) {
    case TBE_OPT_EXACT_SGD:
      break;
    case TBE_OPT_EXACT_ROWWISE_ADAGRAD:
    case TBE_OPT_EXACT_ADAGRAD:
    case TBE_OPT_DENSE_GRAD:
      TBE_REQUIRE(c.feat_state0 != nullptr, "%s: optimizer %d needs feat_state0", who, opt.optimizer);
      break;
    case TBE_OPT_ADAM:
      TBE_REQUIRE(c.feat_state0 != nullptr && c.feat_state1 != nullptr, "%s: ADAM needs two states", who);
      TBE_REQUIRE(opt.iteration >= 1, "%s: ADAM iteration must be >= 1", who);
      break;
    case TBE_OPT_LAMB:
    case TBE_OPT_PARTIAL_ROWWISE_ADAM:
    case TBE_OPT_PARTIAL_ROWWISE_LAMB:
    case TBE_OPT_LARS_SGD:
      if (c.ex) {
        TBE_REQUIRE(c.feat_state0 != nullptr, "%s: optimizer %d needs feat_state0", who, opt.optimizer);
        TBE_REQUIRE(opt.optimizer == TBE_OPT_LARS_SGD || c.feat_state1 != nullptr, "%s: optimizer %d needs feat_state1",
                    who, opt.optimizer);
        TBE_REQUIRE(opt.optimizer != TBE_OPT_PARTIAL_ROWWISE_ADAM || opt.iteration >= 1,
                    "%s: PARTIAL_ROWWISE_ADAM iteration must be >= 1", who);
        break;
      }
      [[fallthrough]];
    default:
      set_error("%s: unknown optimizer %d", who, opt.optimizer);
      return TBE_ERR_UNSUPPORTED;
  }
  if (c.skip_single) {
    // what makes sorted position <-> contribution (f, b) the mapping the caller's flags use, and the update the caller's
    TBE_REQUIRE(opt.optimizer == TBE_OPT_EXACT_SGD && c.ext == nullptr, "%s: EXACT_SGD without extensions only", who);
    TBE_REQUIRE(c.pooling_mode == TBE_POOL_SUM && c.per_sample_weights == nullptr && (c.flags & TBE_FLAG_WEIGHTED) == 0 &&
                    c.N == static_cast<int64_t>(c.F) * c.B,
                "%s: SUM pooling, no per-sample weights, exactly one id per bag (N == F * B)", who);
    TBE_REQUIRE(c.max_D <= 128, "%s: max_D=%d above 128", who, c.max_D);
  }
  const tbe_optimizer_ext* const ext = c.ext;
  const bool clip = ext != nullptr && ext->gradient_clipping != 0;
  if (clip)
    TBE_REQUIRE(ext->max_gradient >= 0.f && ext->max_gradient <= 3.402823466e38f,
                "%s: gradient clipping needs a finite max_gradient >= 0", who);
  if (c.N == 0 || c.B == 0) {
    *done = true;
    return TBE_OK;
  }
  TBE_REQUIRE(c.feat_rows && c.feat_row_base && c.indices && c.offsets && c.workspace, "%s: null pointer", who);
  if (c.phase & kPhaseApply)
    TBE_REQUIRE(c.feat_weights && c.feat_D && c.feat_out_offset && c.grad_out, "%s: null pointer", who);
  TBE_REQUIRE((reinterpret_cast<uintptr_t>(c.workspace) & 255) == 0, "%s: workspace must be 256-B aligned", who);
  BwdWorkspace& w = *ws;
  int rc = carve(c.workspace, c.N, c.max_D, c.key_bits, &w);
  if (rc != TBE_OK) return rc;
  if (w.total > c.workspace_bytes) {
    set_error("%s: workspace too small (%zu < %zu)", who, c.workspace_bytes, w.total);
    return TBE_ERR_WORKSPACE;
  }
  BwdArgs a{};
  a.feat_weights = c.feat_weights;
  a.feat_D = c.feat_D;
  a.feat_out_offset = c.feat_out_offset;
  a.feat_rows = c.feat_rows;
  a.feat_row_base = c.feat_row_base;
  a.feat_window = c.feat_window;
  a.feat_pooling = c.feat_pooling;
  a.feat_state0 = c.feat_state0;
  a.feat_state1 = c.feat_state1;
  a.indices = c.indices;
  a.offsets = c.offsets;
  a.psw = c.per_sample_weights;
  a.grad_out = c.grad_out;
  a.grad_stride = c.grad_row_stride;
  a.N = c.N;
  a.F = c.F;
  a.B = c.B;
  a.pooling_mode = c.pooling_mode;
  a.key_bits = c.key_bits;
  a.C = pick_chunk(c.N);
  a.opt = opt;
  a.bias1 = 1.f;
  a.bias2 = 1.f;
  if (opt.optimizer == TBE_OPT_ADAM || opt.optimizer == TBE_OPT_PARTIAL_ROWWISE_ADAM) {
    a.bias1 = 1.f - powf(opt.beta1, static_cast<float>(opt.iteration));
    a.bias2 = 1.f - powf(opt.beta2, static_cast<float>(opt.iteration));
  }
  a.momentum = ext != nullptr ? ext->momentum : 0.f;
  a.eta = ext != nullptr ? ext->eta : 0.f;
  a.max_gradient = clip ? ext->max_gradient : -1.f;
  a.partial_first = w.partial_first;
  a.partial_last = w.partial_last;
  a.origin_list = w.origin_list;
  a.origin_count = w.origin_count;
  a.max_D_pad = (c.max_D + 3) / 4 * 4;
  a.fast_D = ((c.flags & TBE_FLAG_UNIFORM_ALIGNED) && c.max_D % 4 == 0 && c.grad_row_stride % 4 == 0 &&
              (reinterpret_cast<uintptr_t>(c.grad_out) & 15) == 0) ? c.max_D : 0;
  a.bounds_errors = c.bounds_errors;
  a.unique_rows = (c.phase & kPhaseApply) ? profile_unique_rows_counter() : nullptr;
  a.rounding = TBE_ROUND_NEAREST_EVEN;
  a.round_hash = 0;
  a.skip_single = c.skip_single ? 1 : 0;
  // the sort ping-pongs between the two buffer pairs: an odd number of passes ends in the second
  const bool in_second = (radix_passes(c.key_bits) & 1) != 0;
  a.keys_sorted = in_second ? w.keys_out : w.keys_in;
  a.payload_sorted = in_second ? w.pay_out : w.pay_in;
  *args = a;
  // payload width: the bag number alone unless positions are needed (per-sample weights, unpooled rows)
  *wide_payload = c.pooling_mode == TBE_POOL_NONE || (c.flags & TBE_FLAG_WEIGHTED) != 0;
  return TBE_OK;
}

// The gradient-independent phase (fill + linearize + sort of the row keys into the workspace): never touches the tables,
// so it is defined once, in tbe_backward.hip.
int run_prepare(const BwdArgs& a, const BwdWorkspace& w, bool wide_payload, hipStream_t st);

// Every backward entry point: validate, carve once, sort if the phase mask says so, update + fix-up on tables of WT.
template <typename WT>
static int backward_entry(const BwdCall& c) {
  if constexpr (std::is_same_v<WT, _Float16>) {
    TBE_REQUIRE(c.rounding == TBE_ROUND_NEAREST_EVEN || c.rounding == TBE_ROUND_STOCHASTIC, "%s: rounding %d", c.who,
                c.rounding);
    if (c.opt.optimizer == TBE_OPT_DENSE_GRAD) {
      set_error("%s: TBE_OPT_DENSE_GRAD is not supported with FP16 tables (dense parameters are float)", c.who);
      return TBE_ERR_UNSUPPORTED;
    }
  }
  BwdArgs a;
  BwdWorkspace w;
  bool wide = false, done = false;
  const int rc = bwd_setup(c, &a, &w, &wide, &done);
  if (rc != TBE_OK || done) return rc;
  if constexpr (std::is_same_v<WT, _Float16>) {
    a.rounding = c.rounding;
    a.round_hash = call_hash(c.seed, c.opt.iteration);
  }
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  ProfileSpan total_span(c.phase == kPhasePrepare ? -1 : TBE_PROFILE_BWD_TOTAL, st);
  if (c.phase & kPhasePrepare) {
    const int prc = run_prepare(a, w, wide, st);
    if (prc != TBE_OK) return prc;
  }
  if (!(c.phase & kPhaseApply)) return TBE_OK;
  if (c.key_bits > 32)
    return wide ? run_apply<WT, uint64_t, uint64_t>(a, c.max_D, st) : run_apply<WT, uint64_t, uint32_t>(a, c.max_D, st);
  return wide ? run_apply<WT, uint32_t, uint64_t>(a, c.max_D, st) : run_apply<WT, uint32_t, uint32_t>(a, c.max_D, st);
}

}  // namespace tbe
