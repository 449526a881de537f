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

#include "radix_sort.hpp"
#include "tbe_row.hpp"

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
  store_cols(row, d, D, vec, x);
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
  store_cols(row, d, D, vec, h);
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

// The step every optimizer ends with: w - s * g to the table row, each lane its columns.
template <typename WT, int G, int NV>
__device__ __forceinline__ void store_step(WT* wrow, int D, bool vec, int gl, float s, const float4 (&w)[NV],
                                           const float4 (&g)[NV], const RowRounding& rr) {
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int d = (v * G + gl) * 4;
    if (d < D) stw(wrow, d, D, vec, fmaf4(-s, g[v], w[v]), rr);
  }
}

// Max of v over the groups of a wave, on every lane (v is group-uniform): a wave-uniform trip count for loops that shuffle.
template <int G>
__device__ __forceinline__ int wave_max_over_groups(int v) {
#pragma unroll
  for (int o = 32; o >= G; o >>= 1) v = max(v, __shfl_xor(v, o, kWave));
  return v;
}

// OPTC of the row-norm family (LAMB, PARTIAL_ROWWISE_ADAM, PARTIAL_ROWWISE_LAMB, LARS_SGD; chosen at run time inside
// it): its own instantiations, so that the generic ones (OPTC = -1) keep their register footprint.
constexpr int kOptNormFamily = -2;
__host__ __device__ __forceinline__ bool is_norm_family(int optimizer) {
  return optimizer >= TBE_OPT_LAMB && optimizer <= TBE_OPT_LARS_SGD;
}

// The exponential moving averages of g and g * g that ADAM and the row-norm family keep.
__device__ __forceinline__ float ema_moment1(float b1, float m1, float g) { return fmaf(b1, m1, (1.f - b1) * g); }
__device__ __forceinline__ float ema_moment2(float b2, float m2, float g) { return fmaf(b2, m2, (1.f - b2) * g * g); }

// The row-norm family (formulas: include/tbe_hip.h, tbe_backward_*_ex_*).  Two passes over register-resident data: the
// first updates the element-wise state (loaded and stored once, never held), leaves the update direction u in g's
// registers and sums the norms; the second writes the row.  Live across the norm: w and g only, as for ADAM.
template <typename WT, int G, int NV>
__device__ __forceinline__ void apply_row_norm(const BwdArgs& a, int f, int64_t local_row, int D, bool vec, int gl,
                                               WT* wrow, float4 (&w)[NV], float4 (&g)[NV], const RowRounding& rr) {
  const int optimizer = a.opt.optimizer;
  const float lr = a.opt.learning_rate, wd = a.opt.weight_decay;
  float* m1row = reinterpret_cast<float*>(a.feat_state0[f]) + local_row * D;
  const bool m1vec = vec && row_aligned(m1row);
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
    const auto lars = [=](float& m, float& r, float w, float g) {
      m = fmaf(mom, m, alr * fmaf(wd, w, g));
      r = w - m;
    };
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) {
        float4 m = load_cols(m1row, d, D, m1vec);
        float4 r;
        each4(lars, m, r, w[v], g[v]);
        store_cols(m1row, d, D, m1vec, m);
        stw(wrow, d, D, vec, r, rr);
      }
    }
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
    m2vec = vec && row_aligned(m2row);
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
  const auto moment1 = [=](float& m1, float g) { m1 = ema_moment1(b1, m1, g); };
  const auto moment2_den = [=](float& m2, float& den, float g) {
    m2 = ema_moment2(b2, m2, g);
    den = sqrtf(m2) + eps;
  };
  const auto direction = [=](float& u, float m1, float den, float w) { u = (m1 / m1div) / den + wd * w; };
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int d = (v * G + gl) * 4;
    if (d < D) {
      float4 m1 = load_cols(m1row, d, D, m1vec);
      each4(moment1, m1, g[v]);
      store_cols(m1row, d, D, m1vec, m1);
      float4 den = make_float4(den_row, den_row, den_row, den_row);
      if (lamb) {
        float4 m2 = load_cols(m2row, d, D, m2vec);
        each4(moment2_den, m2, den, g[v]);
        store_cols(m2row, d, D, m2vec, m2);
      }
      float4 u;
      each4(direction, u, m1, den, w[v]);
      g[v] = mask_tail(u, d, D);
      uu = sumsq4(g[v], uu);
    }
  }
  float step = lr;
  if (!adam) {  // the trust ratio |w| / |u|, 1 when either norm is zero
    const float wn = sqrtf(group_sum<G>(ww)), un = sqrtf(group_sum<G>(uu));
    if (wn > 0.f && un > 0.f) step = lr * (wn / un);
  }
  store_step<WT, G, NV>(wrow, D, vec, gl, step, w, g, rr);
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
    store_step<WT, G, NV>(wrow, D, vec, gl, lr, w, g, rr);
  } else if (optimizer == TBE_OPT_EXACT_ROWWISE_ADAGRAD) {
    const float wd = a.opt.weight_decay;
    float ss = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) {
        if (wd != 0.f) fma4(g[v], wd, w[v]);
        ss = sumsq4(g[v], ss);  // columns beyond D are zero in g (never loaded)
      }
    }
    ss = group_sum<G>(ss);
    float* m = reinterpret_cast<float*>(a.feat_state0[f]) + local_row;
    const float m_new = *m + ss / static_cast<float>(D);
    const float mult = lr / (sqrtf(m_new) + a.opt.eps);
    if (gl == 0) *m = m_new;
    store_step<WT, G, NV>(wrow, D, vec, gl, mult, w, g, rr);
  } else if (optimizer == TBE_OPT_DENSE_GRAD) {
    float* grow = reinterpret_cast<float*>(a.feat_state0[f]) + local_row * D;
    const bool gvec = vec && row_aligned(grow);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) store_cols(grow, d, D, gvec, g[v]);
    }
  } else if (optimizer == TBE_OPT_EXACT_ADAGRAD) {
    float* mrow = reinterpret_cast<float*>(a.feat_state0[f]) + local_row * D;
    const bool mvec = vec && row_aligned(mrow);
    const float eps = a.opt.eps;
    const auto accumulate = [](float& m, float g) { m = fmaf(g, g, m); };
    const auto step = [=](float& r, float m, float w, float g) { r = w - lr * g / (sqrtf(m) + eps); };
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) {
        float4 m = load_cols(mrow, d, D, mvec);
        each4(accumulate, m, g[v]);
        store_cols(mrow, d, D, mvec, m);
        float4 r;
        each4(step, r, m, w[v], g[v]);
        stw(wrow, d, D, vec, r, rr);
      }
    }
  } else if (optimizer == TBE_OPT_ADAM) {
    float* m1row = reinterpret_cast<float*>(a.feat_state0[f]) + local_row * D;
    float* m2row = reinterpret_cast<float*>(a.feat_state1[f]) + local_row * D;
    const bool mvec = vec && row_aligned(m1row) && row_aligned(m2row);
    const float b1 = a.opt.beta1, b2 = a.opt.beta2, eps = a.opt.eps, wd = a.opt.weight_decay;
    const float bias1 = a.bias1, bias2 = a.bias2;
    const auto adam = [=](float& m1, float& m2, float& r, float w, float g) {
      m1 = ema_moment1(b1, m1, g);
      m2 = ema_moment2(b2, m2, g);
      r = w - lr * ((m1 / bias1) / (sqrtf(m2 / bias2) + eps) + wd * w);
    };
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int d = (v * G + gl) * 4;
      if (d < D) {
        float4 m1 = load_cols(m1row, d, D, mvec);
        float4 m2 = load_cols(m2row, d, D, mvec);
        float4 r;
        each4(adam, m1, m2, r, w[v], g[v]);
        store_cols(m1row, d, D, mvec, m1);
        store_cols(m2row, d, D, mvec, m2);
        stw(wrow, d, D, vec, r, rr);
      }
    }
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
  const int max_span = wave_max_over_groups<G>(span);

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
    const int max_n = wave_max_over_groups<G>(n);

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
        const bool gvec = FAST || row_vec(Du[u], gp);
        vecu[u] = FAST || row_vec(Du[u], wp[u]);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const int d = (v * G + gl) * 4;
          x[u][v] = (val[u] && d < Du[u]) ? load_cols(gp, d, Du[u], gvec) : make_float4(0.f, 0.f, 0.f, 0.f);
          // the current weight row (not needed when the coalesced gradient is only written out: DENSE_GRAD)
          wr[u][v] = (OPTC != TBE_OPT_DENSE_GRAD && lst[u] && d < Du[u]) ? load_cols(wp[u], d, Du[u], vecu[u])
                                                                          : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (val[u]) {
          if (!FAST && a.max_gradient >= 0.f) {  // gradient clipping: the loaded element, before weight and MEAN division
            const float mg = a.max_gradient;
#pragma unroll
            for (int v = 0; v < NV; ++v) x[u][v] = clamp4(x[u][v], -mg, mg);
          }
#pragma unroll
          for (int v = 0; v < NV; ++v) fma4(acc[v], wt[u], x[u][v]);
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
      for (int v = 0; v < NV; ++v) add4(acc[v], x[u][v]);
  }
}

// Finishes the run that origin `chunk` opened and the next `len` chunks continue (key_run: its row key) with N groups,
// of which the caller is group i: one wave's NG, or (BLOCK) the workgroup's 4 * NG, staging in set[0..N).  The row comes
// from the origin chunk's last contribution.  Every group sums its slice of the chain's partial_first rows and stages
// the sum; group 0 (always the finisher) then adds, per column, to partial_last the groups' sums in ascending group order
// (this order is the contract: the fixed combine order that makes the result bitwise reproducible) and applies the
// optimizer.  BLOCK also selects the barrier between staging and combining: __syncthreads, else the wave's fence.
template <typename WT, typename PayT, int G, int NV, int OPTC, bool BLOCK, typename KeyT>
__device__ __forceinline__ void finish_run(const BwdArgs& a, int64_t chunk, KeyT key_run, int len, int i, int gl,
                                           float4 (*set)[NV][G]) {
  constexpr int N = (BLOCK ? 4 : 1) * (kWave / G);
  const PayT pay = static_cast<const PayT*>(a.payload_sorted)[(chunk + 1) * a.C - 1];
  const int f = static_cast<int>(payload_bag<PayT>(pay) / static_cast<uint32_t>(a.B));
  const int D = a.feat_D[f];
  const int64_t lrow = static_cast<int64_t>(key_run) - a.feat_row_base[f];
  WT* wrow = reinterpret_cast<WT*>(a.feat_weights[f]) + lrow * D;
  const bool vec = row_vec(D, wrow);
  float4 acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int per = (len + N - 1) / N;
  sum_partials<G, NV>(a.partial_first, a.max_D_pad, chunk + 1, min(len, i * per), min(len, (i + 1) * per), D, gl, acc);
  if (N > 1) {
    if (BLOCK) __syncthreads();  // the previous run's group 0 is done with `set`
#pragma unroll
    for (int v = 0; v < NV; ++v) set[i][v][gl] = acc[v];
    if (BLOCK) {
      __syncthreads();
    } else {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  if (i != 0) return;
  float4 tot[NV], w[NV];
  const float* pl = a.partial_last + chunk * a.max_D_pad;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int d = (v * G + gl) * 4;
    tot[v] = (d < D) ? ld4(pl + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    w[v] = (d < D) ? load_cols(wrow, d, D, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    if (!BLOCK) add4(tot[v], acc[v]);  // group 0's own sum: a wave has it in registers, the workgroup reads set[0]
    for (int og = BLOCK ? 0 : 1; og < N; ++og) add4(tot[v], set[og][v][gl]);
  }
  apply_row<WT, G, NV, OPTC>(a, f, lrow, D, vec, gl, wrow, w, tot, row_hash_if_needed<WT>(a, static_cast<uint64_t>(key_run)));
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
        finish_run<WT, PayT, G, NV, OPTC, false>(a, chunk, key_run, len, g, gl, part + wave * NG);
      }
    }
    __syncthreads();
    const int nl = n_long;
    for (int s = 0; s < nl; ++s) {  // block-uniform
      const int64_t chunk = long_chunk[s];
      const int len = long_len[s];
      finish_run<WT, PayT, G, NV, OPTC, true>(a, chunk, skey[(chunk + 1) * a.C - 1], len, q, gl, part);
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

using BwdKernel = void (*)(BwdArgs);

// One launch of an update or fix-up kernel (256 threads), bracketed as `profile_slot` (-1: not bracketed).
static int launch_bwd(const char* what, int profile_slot, BwdKernel kernel, unsigned grid, const BwdArgs& a, hipStream_t st) {
  {
    ProfileSpan span(profile_slot, st);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, a);
  }
  TBE_CHECK_LAUNCH(what);
  return TBE_OK;
}

// The update kernel (OPTC, FAST, SKIP) of a (WT, KeyT, PayT, G, NV), or nullptr where none is built.  FAST kernels keep
// U = 4 rows in flight at 4 waves per SIMD and exist for the one (G, NV) pair that can reach them, DENSE_GRAD (the
// replicated tiny tables of a sharded collection) for FP32 tables only; the others take U from NV.  SKIP kernels exist
// for what a skip-single call can be: float tables of dim <= 128 with bag payloads (backward_entry checks).
template <typename WT, typename KeyT, typename PayT, int G, int NV, int OPTC, bool FAST, bool SKIP>
static BwdKernel update_kernel() {
  constexpr bool built = (!FAST || (G == 32 && NV == 1 && (OPTC != TBE_OPT_DENSE_GRAD || sizeof(WT) == 4))) &&
                         (!SKIP || (std::is_same_v<WT, float> && sizeof(PayT) == 4 && NV == 1 && G <= 32));
  if constexpr (built) {
    return bwd_update_kernel<WT, KeyT, PayT, G, NV, OPTC, FAST, FAST ? 4 : BwdUnroll<NV>::U, FAST ? 4 : 1, SKIP>;
  } else {
    return nullptr;
  }
}

template <typename WT, typename KeyT, typename PayT, int G, int NV>
static int launch_update(const BwdArgs& a, hipStream_t st) {
  constexpr int NG = kWave / G;
  const int64_t nchunks = (a.N + a.C - 1) / a.C;
  const int64_t groups_per_block = 4 * NG;
  const unsigned grid = static_cast<unsigned>((nchunks + groups_per_block - 1) / groups_per_block);
  // (a launch with gradient clipping takes the generic kernel: the fast ones have no clamp)
  const bool fast = a.fast_D > 0 && a.pooling_mode == TBE_POOL_SUM && a.psw == nullptr && a.max_gradient < 0.f;
  const int oc = a.opt.optimizer;
  const bool skip = a.skip_single != 0, norm = is_norm_family(oc);
  // The kernel of a call: the first row whose condition holds and whose kernel is built.
  const struct {
    bool when;
    BwdKernel kernel;
  } table[] = {
      {skip && fast, update_kernel<WT, KeyT, PayT, G, NV, TBE_OPT_EXACT_SGD, true, true>()},
      {skip, update_kernel<WT, KeyT, PayT, G, NV, -1, false, true>()},
      {!skip && norm, update_kernel<WT, KeyT, PayT, G, NV, kOptNormFamily, false, false>()},
      {!skip && fast && oc == TBE_OPT_EXACT_SGD, update_kernel<WT, KeyT, PayT, G, NV, TBE_OPT_EXACT_SGD, true, false>()},
      {!skip && fast && oc == TBE_OPT_EXACT_ROWWISE_ADAGRAD,
       update_kernel<WT, KeyT, PayT, G, NV, TBE_OPT_EXACT_ROWWISE_ADAGRAD, true, false>()},
      {!skip && fast && oc == TBE_OPT_DENSE_GRAD, update_kernel<WT, KeyT, PayT, G, NV, TBE_OPT_DENSE_GRAD, true, false>()},
      {!skip, update_kernel<WT, KeyT, PayT, G, NV, -1, false, false>()},
  };
  BwdKernel update = nullptr;
  for (const auto& row : table) {
    if (row.when && row.kernel != nullptr) {
      update = row.kernel;
      break;
    }
  }
  if (update == nullptr) {  // only a skip-single call can get here: the last row is built for every configuration
    set_error("tbe_backward update: no kernel that skips single contributions for this configuration");
    return TBE_ERR_UNSUPPORTED;
  }
  const int rc = launch_bwd("tbe_backward update", TBE_PROFILE_BWD_UPDATE_KERNEL, update, grid, a, st);
  if (rc != TBE_OK) return rc;
  const unsigned fgrid = static_cast<unsigned>(std::min<int64_t>((nchunks + 3) / 4, 1024));
  return launch_bwd("tbe_backward fixup", -1,
                    norm ? bwd_fixup_kernel<WT, KeyT, PayT, G, NV, kOptNormFamily> : bwd_fixup_kernel<WT, KeyT, PayT, G, NV, -1>,
                    fgrid, a, st);
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
