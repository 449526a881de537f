// Fused masked attention for BERT4Rec on gfx950, and JaggedTensor.to_padded_dense.
//
// Reference: examples/bert4rec/models/bert4rec.py:72-82 (Attention.forward) inside :152-170 (MultiHeadedAttention), trained
// through autograd.  Per (sample b, head h), float32:
//   S = Q K^T / sqrt(d);  S[:, j] = -1e9 where key j is not valid;  P = softmax_j(S);  P~ = dropout(P);  O = P~ V
// As torch runs it, scores, the masked copy, p_attn, the dropout mask and the dropped copy are [B, H, L, L] tensors in HBM and
// p_attn stays alive for the backward.  Here no [L, L] tensor reaches global memory: the forward keeps one float per row (the
// log-sum-exp) and the backward recomputes P from Q, K and that float.
//
// One workgroup of 8 waves per (b, h).  Two [L, d] matrices are staged in LDS (row stride d + 4 floats, so that the 16-byte
// reads of 16 consecutive rows fall on distinct banks); a wave owns kAttnTile = 16 rows at a time:
//   dots     16 x 16 tiles of v_mfma_f32_16x16x4_f32 (float32 in, float32 accumulate: a chain of fmaf, one rounding per
//            product).  Lane l = 16 g + r feeds owned row r and staged row 16 t + r, columns 16 s + 4 g .. + 3: one 16-byte
//            global read and, per tile, one 16-byte LDS read per four MFMAs (1024 multiply-adds each).  A dot product is
//            summed over c in the order (s, c mod 4, g); lane l ends with the owned rows 4 g .. 4 g + 3 (the accumulator's
//            four elements) against the staged rows 16 t + r
//   softmax  a row is spread over the 16 lanes of one g; row maximum and row sum are butterflies over them (every lane of
//            the row ends with the same bits)
//   sums     two owned rows at a time, their weights go through a per-wave LDS buffer; lane l holds the column quad l mod cw
//            (cw = d / 4 rounded up to a power of two) and the staged rows j = l / cw (mod 64 / cw); the 64 / cw partial
//            sums are combined by a butterfly
// forward    stages K, V; the row owner is the query i:            O_i = sum_j P~_ij V_j,  lse_i = m_i + log sum_j exp(S_ij - m_i)
// backward   phase A stages K, V; the row owner is the query i:    D_i = sum_j P~_ij (dO_i . V_j)  ( = dO_i . O_i ),
//                                                                  dQ_i = sum_j dS_ij K_j
//            phase B stages Q, dO; the row owner is the key j:     dV_j = sum_i P~_ij dO_i,  dK_j = sum_i dS_ij Q_i
//            with P_ij = exp(S_ij - lse_i),  dP_ij = keep_ij scale (dO_i . V_j),  dS_ij = P_ij (dP_ij - D_i) / sqrt(d), and
//            dS_ij = 0 at every masked key j.  S is computed twice (A and B) by the same operations in the same order, so both
//            phases see the same bits; the workgroup owns every row it writes: no atomics, no cross-block sums.
// A sample with no valid key has S = -1e9 everywhere; -1e9 + log L is not representable next to -1e9 in float32, so for such
// a sample both passes take P = 1 / L, which is what the forward's exp(0) / L gives, instead of exp(S - lse).
// Every sum runs in an order fixed by (L, d); the weighted sums use fmaf explicitly (the Makefile's -ffp-contract=off stays:
// nothing is contracted behind the source's back).  Two runs are bit-identical.
//
// MFMA for the dot products, vector FMA for the weighted sums: DESIGN.md (BERT4Rec) has the measurement behind the choice.
#include <atomic>
#include <cmath>

#include "common.hpp"
#include "tbe_backward_impl.hpp"  // fmix32, call_hash

namespace tbe {

constexpr int kAttnThreads = 512;
constexpr int kAttnWaves = kAttnThreads / kWave;
constexpr int kAttnTile = 16;         // rows a wave owns at a time, and staged rows per MFMA tile
constexpr int kAttnRows = 2;          // owned rows per weighted sum (they share every LDS read of the staged matrix)
constexpr int kAttnMaxKeys = 4;       // L <= 64 * kAttnMaxKeys (the kernels' template parameter T counts 64 staged rows)
using attn_f4 = float __attribute__((ext_vector_type(4)));  // one MFMA accumulator
constexpr int kAttnMaxL = kWave * kAttnMaxKeys;
constexpr int kAttnMaxD = 128;
constexpr size_t kAttnLdsBudget = 160 * 1024;  // the CU's LDS

__host__ __device__ constexpr int attn_ds(int d) { return d + 4; }
__host__ __device__ constexpr int attn_lp(int L) { return (L + 3) & ~3; }
// floats: two staged matrices, D [Lp], and per wave and owned row two weight buffers [Lp]
static size_t attn_lds_bytes(int L, int d) {
  const size_t lp = attn_lp(L);
  return sizeof(float) * (2 * static_cast<size_t>(L) * attn_ds(d) + lp + kAttnWaves * kAttnRows * 2 * lp);
}
static bool attn_supported(int64_t L, int64_t d) {
  return L >= 1 && L <= kAttnMaxL && d >= 4 && d <= kAttnMaxD && d % 4 == 0 &&
         attn_lds_bytes(static_cast<int>(L), static_cast<int>(d)) <= kAttnLdsBudget;
}

struct AttnArgs {
  const float *q, *k, *v;            // element (b, l, h, c) at base + b * bs + l * rs + h * d + c
  int64_t q_bs, q_rs, k_bs, k_rs, v_bs, v_rs;
  const uint8_t* key_valid;          // [B, L] or null
  const float* dout;                 // backward: [B, L, H * d]
  float* lse;                        // [B, H, L]: written by the forward, read by the backward
  float *out, *dq, *dk, *dv;         // [B, L, H * d]; forward: out; backward: dq / dk / dv, each may be null (not wanted)
  int32_t H, L, d;
  uint32_t callh, drop_thr;          // call_hash(seed, call); keep iff draw >= drop_thr
  float drop_scale;                  // 1 / (1 - p)
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// over the 16 lanes that share a row
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
  for (int o = kAttnTile / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = kAttnTile / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// The dropout draw of element (b, h, i, j): three words, each the murmur3 finalizer of the one before xor an index times an
// odd constant (include/tbe_hip.h states it for the tests).
__device__ __forceinline__ uint32_t attn_word_bh(uint32_t callh, uint32_t bh) { return fmix32(callh ^ (bh * 0x9e3779b1u)); }
__device__ __forceinline__ uint32_t attn_word_i(uint32_t wbh, uint32_t i) { return fmix32(wbh ^ (i * 0x85ebca6bu)); }
__device__ __forceinline__ uint32_t attn_draw(uint32_t wi, uint32_t j) { return fmix32(wi ^ (j * 0xc2b2ae35u)); }

// dst[r * ds + c] = src[r * rs + c] for r < L, c < d, by the whole workgroup
__device__ __forceinline__ void attn_stage(float* dst, const float* __restrict__ src, int64_t rs, int L, int d) {
  const int d4 = d >> 2, ds = attn_ds(d);
  for (int idx = threadIdx.x; idx < L * d4; idx += kAttnThreads) {
    const int r = idx / d4, c = (idx - r * d4) * 4;
    st4(dst + r * ds + c, ld4(src + r * rs + c));
  }
}

// acc[t][e] += sum_c own(row 4 g + e)[c] * Ms[16 t + r][c]   (and the same for the second pair when TWO).  `own` / `own2` are
// the lane's owned row r (clamped by the caller); columns beyond d feed zeros, which leave the accumulator as it is.  The
// tiles at or beyond L are skipped (wave-uniform), the staged row of a partial tile is clamped to L - 1.
template <int NT, bool TWO>
__device__ __forceinline__ void attn_dots(const float* Ms, const float* Ns, int d, int L, int r, int g, const float* own,
                                          const float* own2, attn_f4 (&acc)[NT], attn_f4 (&acc2)[NT]) {
  const int ds = attn_ds(d);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c0 = 0; c0 < d; c0 += 16) {
    const int c = c0 + 4 * g;
    const bool in = c < d;
    const float4 a = in ? ld4(own + c) : zero;
    float4 a2 = zero;
    if (TWO && in) a2 = ld4(own2 + c);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (kAttnTile * t < L) {
        const int row = min(kAttnTile * t + r, L - 1);
        const float4 m = in ? ld4(Ms + row * ds + c) : zero;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, m.x, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, m.y, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, m.z, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, m.w, acc[t], 0, 0, 0);
        if (TWO) {
          const float4 n = in ? ld4(Ns + row * ds + c) : zero;
          acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.x, n.x, acc2[t], 0, 0, 0);
          acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.y, n.y, acc2[t], 0, 0, 0);
          acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.z, n.z, acc2[t], 0, 0, 0);
          acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2.w, n.w, acc2[t], 0, 0, 0);
        }
      }
    }
  }
}

// out[r] = sum_j w[r * wstride + j] * Ms[j][4 cq .. 4 cq + 4), j over the lane's residue class ascending, then the classes
// combined by a butterfly: every lane of a column quad ends with the same bits.
struct AttnCols {
  int cw, shift, cq, g, ng;
  bool active;  // the lane that writes the quad
  __device__ AttnCols(int d, int lane) {
    const int d4 = d >> 2;
    shift = 0;
    while ((1 << shift) < d4) ++shift;
    cw = 1 << shift;
    cq = lane & (cw - 1);
    g = lane >> shift;
    ng = kWave >> shift;
    active = g == 0 && cq < d4;
    if (cq >= d4) cq = d4 - 1;  // reads stay inside the row; the result is not written
  }
};
__device__ __forceinline__ void attn_wsum(const float* Ms, int d, int L, const AttnCols& cl, const float* w, int wstride,
                                          float4 (&out)[kAttnRows]) {
  const int ds = attn_ds(d);
#pragma unroll
  for (int r = 0; r < kAttnRows; ++r) out[r] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = cl.g; j < L; j += cl.ng) {
    const float4 m = ld4(Ms + j * ds + 4 * cl.cq);
#pragma unroll
    for (int r = 0; r < kAttnRows; ++r) {
      const float x = w[r * wstride + j];
      out[r].x = fmaf(x, m.x, out[r].x);
      out[r].y = fmaf(x, m.y, out[r].y);
      out[r].z = fmaf(x, m.z, out[r].z);
      out[r].w = fmaf(x, m.w, out[r].w);
    }
  }
  for (int o = cl.cw; o < kWave; o <<= 1) {
#pragma unroll
    for (int r = 0; r < kAttnRows; ++r) {
      out[r].x += __shfl_xor(out[r].x, o, kWave);
      out[r].y += __shfl_xor(out[r].y, o, kWave);
      out[r].z += __shfl_xor(out[r].z, o, kWave);
      out[r].w += __shfl_xor(out[r].w, o, kWave);
    }
  }
}

// What every kernel starts with: who am I, where is the LDS image, which staged rows does the lane hold.
template <int T>
struct AttnWave {
  static constexpr int NT = 4 * T;  // MFMA tiles of 16 staged rows
  int lane, r, g, wave, b, h, bh, L, d, lp;
  float *Ms, *Ns, *Dsh, *wbuf;
  uint32_t vmask;      // bit t: key_valid of the staged row jt(t) (of its clamp beyond L: those are excluded by jt < L)
  int nvalid;          // valid keys of the sample
  float sqrt_d;
  uint32_t wbh;
  __device__ int jt(int t) const { return kAttnTile * t + r; }         // the lane's staged row of tile t
  __device__ int jc(int t) const { return min(jt(t), L - 1); }         // clamped for addressing
  __device__ bool valid(int t) const { return (vmask >> t) & 1u; }
  __device__ AttnWave(const AttnArgs& a, float* lds) {
    lane = threadIdx.x & (kWave - 1);
    r = lane & (kAttnTile - 1);
    g = lane >> 4;
    wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    bh = blockIdx.x;
    b = bh / a.H;
    h = bh - b * a.H;
    L = a.L;
    d = a.d;
    lp = attn_lp(L);
    Ms = lds;
    Ns = Ms + L * attn_ds(d);
    Dsh = Ns + L * attn_ds(d);
    wbuf = Dsh + lp + wave * (kAttnRows * 2 * lp);
    int n = 0;
    vmask = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const bool v = a.key_valid == nullptr || a.key_valid[static_cast<int64_t>(b) * L + jc(t)] != 0;
      vmask |= (v ? 1u : 0u) << t;
      n += (jt(t) < L && v) ? 1 : 0;
    }
#pragma unroll
    for (int o = kAttnTile / 2; o > 0; o >>= 1) n += __shfl_xor(n, o, kWave);  // the 16 lanes of one g hold every key
    nvalid = n;
    sqrt_d = sqrtf(static_cast<float>(d));
    wbh = attn_word_bh(a.callh, static_cast<uint32_t>(bh));
  }
  __device__ const float* row_of(const float* base, int64_t bs, int64_t rs, int l) const {
    return base + b * bs + l * rs + h * d;
  }
  __device__ int64_t dense_row(int l, int H) const { return (static_cast<int64_t>(b) * L + l) * H * d + h * d; }
};

template <int T>
__global__ __launch_bounds__(kAttnThreads) void attention_fwd_kernel(const AttnArgs a) {
  extern __shared__ float4 attn_lds[];
  AttnWave<T> w(a, reinterpret_cast<float*>(attn_lds));
  const int L = w.L, d = w.d;
  attn_stage(w.Ms, w.row_of(a.k, a.k_bs, a.k_rs, 0), a.k_rs, L, d);
  attn_stage(w.Ns, w.row_of(a.v, a.v_bs, a.v_rs, 0), a.v_rs, L, d);
  __syncthreads();
  const AttnCols cl(d, w.lane);
  const int wstride = 2 * w.lp;
  constexpr int NT = AttnWave<T>::NT;
  for (int i0 = w.wave * kAttnTile; i0 < L; i0 += kAttnWaves * kAttnTile) {
    attn_f4 acc[NT], unused[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = attn_f4{0.f, 0.f, 0.f, 0.f};
    const float* own = w.row_of(a.q, a.q_bs, a.q_rs, min(i0 + w.r, L - 1));
    attn_dots<NT, false>(w.Ms, nullptr, d, L, w.r, w.g, own, own, acc, unused);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = i0 + 4 * w.g + e;
      float s[NT], m = -INFINITY;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        s[t] = w.valid(t) ? acc[t][e] / w.sqrt_d : -1e9f;
        if (w.jt(t) < L) m = fmaxf(m, s[t]);
      }
      m = row_max(m);
      float sum = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        s[t] = w.jt(t) < L ? expf(s[t] - m) : 0.f;
        sum += s[t];
      }
      sum = row_sum(sum);
      if (w.r == 0 && i < L) a.lse[static_cast<int64_t>(w.bh) * L + i] = m + logf(sum);
      const uint32_t wi = attn_word_i(w.wbh, static_cast<uint32_t>(i));
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        float p = s[t] / sum;
        if (a.drop_thr != 0) p = attn_draw(wi, static_cast<uint32_t>(w.jt(t))) >= a.drop_thr ? p * a.drop_scale : 0.f;
        acc[t][e] = p;
      }
    }
    // O: two owned rows at a time, written to the weight buffer by the 16 lanes that hold them
    for (int q4 = 0; q4 < 4; ++q4) {
#pragma unroll
      for (int rp = 0; rp < 2; ++rp) {
        const int row0 = i0 + 4 * q4 + 2 * rp;
        if (row0 < L) {
          if (w.g == q4) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
              if (w.jt(t) < L) {
                w.wbuf[w.jt(t)] = acc[t][2 * rp];
                w.wbuf[wstride + w.jt(t)] = acc[t][2 * rp + 1];
              }
          }
          wave_sync();
          float4 o[kAttnRows];
          attn_wsum(w.Ns, d, L, cl, w.wbuf, wstride, o);
#pragma unroll
          for (int rr = 0; rr < kAttnRows; ++rr)
            if (cl.active && row0 + rr < L) st4(a.out + w.dense_row(row0 + rr, a.H) + 4 * cl.cq, o[rr]);
          wave_sync();
        }
      }
    }
  }
}

template <int T>
__global__ __launch_bounds__(kAttnThreads) void attention_bwd_kernel(const AttnArgs a) {
  extern __shared__ float4 attn_lds[];
  AttnWave<T> w(a, reinterpret_cast<float*>(attn_lds));
  const int L = w.L, d = w.d;
  const AttnCols cl(d, w.lane);
  const int wstride = 2 * w.lp;
  const float uniform_p = 1.f / static_cast<float>(L);  // the sample has no valid key
  const float* lse = a.lse + static_cast<int64_t>(w.bh) * L;

  // phase A: K, V staged; rows are queries, the lane's staged rows are keys
  attn_stage(w.Ms, w.row_of(a.k, a.k_bs, a.k_rs, 0), a.k_rs, L, d);
  attn_stage(w.Ns, w.row_of(a.v, a.v_bs, a.v_rs, 0), a.v_rs, L, d);
  __syncthreads();
  constexpr int NT = AttnWave<T>::NT;
  for (int i0 = w.wave * kAttnTile; i0 < L; i0 += kAttnWaves * kAttnTile) {
    attn_f4 acc[NT], acc2[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = acc2[t] = attn_f4{0.f, 0.f, 0.f, 0.f};
    {
      const int i = min(i0 + w.r, L - 1);
      attn_dots<NT, true>(w.Ms, w.Ns, d, L, w.r, w.g, w.row_of(a.q, a.q_bs, a.q_rs, i), a.dout + w.dense_row(i, a.H), acc,
                          acc2);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int irow = i0 + 4 * w.g + e, i = min(irow, L - 1);
      const float lse_i = lse[i];
      const uint32_t wi = attn_word_i(w.wbh, static_cast<uint32_t>(i));
      float part = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float s = w.valid(t) ? acc[t][e] / w.sqrt_d : -1e9f;
        const float p = w.jt(t) < L ? (w.nvalid == 0 ? uniform_p : expf(s - lse_i)) : 0.f;
        float dp = acc2[t][e];
        if (a.drop_thr != 0) dp = attn_draw(wi, static_cast<uint32_t>(w.jt(t))) >= a.drop_thr ? dp * a.drop_scale : 0.f;
        part += p * dp;
        acc[t][e] = p;
        acc2[t][e] = dp;
      }
      const float D = row_sum(part);
      if (w.r == 0 && irow < L) w.Dsh[i] = D;
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t][e] = w.valid(t) ? acc[t][e] * (acc2[t][e] - D) / w.sqrt_d : 0.f;  // dS
    }
    if (a.dq != nullptr) {
      for (int q4 = 0; q4 < 4; ++q4) {
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
          const int row0 = i0 + 4 * q4 + 2 * rp;
          if (row0 < L) {
            if (w.g == q4) {
#pragma unroll
              for (int t = 0; t < NT; ++t)
                if (w.jt(t) < L) {
                  w.wbuf[w.jt(t)] = acc[t][2 * rp];
                  w.wbuf[wstride + w.jt(t)] = acc[t][2 * rp + 1];
                }
            }
            wave_sync();
            float4 o[kAttnRows];
            attn_wsum(w.Ms, d, L, cl, w.wbuf, wstride, o);
#pragma unroll
            for (int rr = 0; rr < kAttnRows; ++rr)
              if (cl.active && row0 + rr < L) st4(a.dq + w.dense_row(row0 + rr, a.H) + 4 * cl.cq, o[rr]);
            wave_sync();
          }
        }
      }
    }
  }
  if (a.dk == nullptr && a.dv == nullptr) return;

  // phase B: Q, dO staged; rows are keys, the lane's staged rows are queries
  __syncthreads();
  attn_stage(w.Ms, w.row_of(a.q, a.q_bs, a.q_rs, 0), a.q_rs, L, d);
  attn_stage(w.Ns, a.dout + w.dense_row(0, a.H), static_cast<int64_t>(a.H) * d, L, d);
  __syncthreads();
  float lse_t[NT], D_t[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    lse_t[t] = lse[w.jc(t)];
    D_t[t] = w.Dsh[w.jc(t)];
  }
  for (int j0 = w.wave * kAttnTile; j0 < L; j0 += kAttnWaves * kAttnTile) {
    attn_f4 acc[NT], acc2[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = acc2[t] = attn_f4{0.f, 0.f, 0.f, 0.f};
    {
      const int j = min(j0 + w.r, L - 1);
      attn_dots<NT, true>(w.Ms, w.Ns, d, L, w.r, w.g, w.row_of(a.k, a.k_bs, a.k_rs, j), w.row_of(a.v, a.v_bs, a.v_rs, j),
                          acc, acc2);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = min(j0 + 4 * w.g + e, L - 1);
      const bool jvalid = a.key_valid == nullptr || a.key_valid[static_cast<int64_t>(w.b) * L + j] != 0;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float s = jvalid ? acc[t][e] / w.sqrt_d : -1e9f;
        const float p = w.nvalid == 0 ? uniform_p : expf(s - lse_t[t]);
        float pt = p, dp = acc2[t][e];
        if (a.drop_thr != 0) {
          const uint32_t wi = attn_word_i(w.wbh, static_cast<uint32_t>(w.jt(t)));
          const bool keep = attn_draw(wi, static_cast<uint32_t>(j)) >= a.drop_thr;
          pt = keep ? p * a.drop_scale : 0.f;
          dp = keep ? dp * a.drop_scale : 0.f;
        }
        acc[t][e] = pt;
        acc2[t][e] = jvalid ? p * (dp - D_t[t]) / w.sqrt_d : 0.f;  // dS
      }
    }
    for (int q4 = 0; q4 < 4; ++q4) {
#pragma unroll
      for (int rp = 0; rp < 2; ++rp) {
        const int row0 = j0 + 4 * q4 + 2 * rp;
        if (row0 < L) {
          if (w.g == q4) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
              if (w.jt(t) < L) {
                w.wbuf[w.jt(t)] = acc[t][2 * rp];
                w.wbuf[wstride + w.jt(t)] = acc[t][2 * rp + 1];
                w.wbuf[w.lp + w.jt(t)] = acc2[t][2 * rp];
                w.wbuf[wstride + w.lp + w.jt(t)] = acc2[t][2 * rp + 1];
              }
          }
          wave_sync();
          float4 o[kAttnRows];
          if (a.dv != nullptr) {
            attn_wsum(w.Ns, d, L, cl, w.wbuf, wstride, o);
#pragma unroll
            for (int rr = 0; rr < kAttnRows; ++rr)
              if (cl.active && row0 + rr < L) st4(a.dv + w.dense_row(row0 + rr, a.H) + 4 * cl.cq, o[rr]);
          }
          if (a.dk != nullptr) {
            attn_wsum(w.Ms, d, L, cl, w.wbuf + w.lp, wstride, o);
#pragma unroll
            for (int rr = 0; rr < kAttnRows; ++rr)
              if (cl.active && row0 + rr < L) st4(a.dk + w.dense_row(row0 + rr, a.H) + 4 * cl.cq, o[rr]);
          }
          wave_sync();
        }
      }
    }
  }
}

// The checks both entries share; fills the sizes and the dropout words of `a`.
static int attn_check(const char* name, AttnArgs& a, int64_t B, int32_t H, int32_t L, int32_t d, float p, uint64_t seed,
                      int64_t call) {
  TBE_REQUIRE(B >= 0 && H >= 1 && L >= 1 && d >= 1, "%s: bad sizes B=%lld H=%d L=%d d=%d", name, static_cast<long long>(B), H,
              L, d);
  TBE_REQUIRE(attn_supported(L, d), "%s: (L, d) = (%d, %d) is not supported (tbe_attention_supported)", name, L, d);
  TBE_REQUIRE(B * H <= INT32_MAX, "%s: B * H = %lld workgroups exceed the grid", name, static_cast<long long>(B * H));
  TBE_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout p=%g outside [0, 1)", name, static_cast<double>(p));
  const int64_t row = static_cast<int64_t>(H) * d;
  const int64_t strides[3][2] = {{a.q_bs, a.q_rs}, {a.k_bs, a.k_rs}, {a.v_bs, a.v_rs}};
  for (const auto& s : strides) {
    TBE_REQUIRE(s[1] >= row && s[1] % 4 == 0, "%s: row stride %lld below the row of %lld floats, or no multiple of 4", name,
                static_cast<long long>(s[1]), static_cast<long long>(row));
    TBE_REQUIRE(s[0] >= (L - 1) * s[1] + row && s[0] % 4 == 0,
                "%s: batch stride %lld below the sample's extent, or no multiple of 4", name, static_cast<long long>(s[0]));
  }
  a.H = H;
  a.L = L;
  a.d = d;
  a.callh = call_hash(seed, call);
  const double thr = std::floor(static_cast<double>(p) * 4294967296.0);
  a.drop_thr = thr >= 4294967295.0 ? 4294967295u : static_cast<uint32_t>(thr);
  a.drop_scale = 1.f / (1.f - p);
  return TBE_OK;
}

// An LDS image above 64 KiB has to be allowed per kernel; once per device and process, for all eight kernels, at the first
// call (so a later call inside a stream capture sets nothing).
static int attn_allow_lds(const char* name) {
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    set_error("%s: no current device", name);
    return TBE_ERR_LAUNCH;
  }
  const bool tracked = dev >= 0 && dev < 64;  // an ordinal the mask cannot hold has the attribute set at every call
  if (tracked && (done.load() & (1ull << dev))) return TBE_OK;
  for (const void* f : {reinterpret_cast<const void*>(attention_fwd_kernel<1>), reinterpret_cast<const void*>(attention_fwd_kernel<2>),
                        reinterpret_cast<const void*>(attention_fwd_kernel<3>), reinterpret_cast<const void*>(attention_fwd_kernel<4>),
                        reinterpret_cast<const void*>(attention_bwd_kernel<1>), reinterpret_cast<const void*>(attention_bwd_kernel<2>),
                        reinterpret_cast<const void*>(attention_bwd_kernel<3>), reinterpret_cast<const void*>(attention_bwd_kernel<4>)}) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kAttnLdsBudget));
    if (e != hipSuccess) {
      set_error("%s: %zu bytes of LDS refused: %s", name, kAttnLdsBudget, hipGetErrorString(e));
      return TBE_ERR_LAUNCH;
    }
  }
  if (tracked) done.fetch_or(1ull << dev);
  return TBE_OK;
}

template <typename K>
static int attn_launch(const char* name, K kernel, const AttnArgs& a, int64_t B, hipStream_t st) {
  const int rc = attn_allow_lds(name);
  if (rc != TBE_OK) return rc;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(B * a.H)), dim3(kAttnThreads), attn_lds_bytes(a.L, a.d), st, a);
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void jagged_to_padded_dense_kernel(const T* __restrict__ values,
                                                                     const int64_t* __restrict__ offsets, int64_t total, int N,
                                                                     float padding, bool pad_begin, bool chop_begin,
                                                                     float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / N;
  const int64_t n = idx - b * N;
  const int64_t lo = offsets[b], len = offsets[b + 1] - lo;
  int64_t src;  // position inside the bag, or -1: padding
  if (len <= N) {
    src = pad_begin ? n - (N - len) : (n < len ? n : -1);
  } else {
    src = chop_begin ? len - N + n : n;
  }
  out[idx] = src < 0 ? padding : static_cast<float>(values[lo + src]);
}

template <typename T>
static int jagged_to_padded_dense(const char* name, const T* values, const int64_t* offsets, int32_t B, int32_t N,
                                  float padding, int32_t pad_begin, int32_t chop_begin, float* out, void* stream) {
  TBE_REQUIRE(B >= 0 && N >= 0, "%s: bad sizes B=%d N=%d", name, B, N);
  const int64_t total = static_cast<int64_t>(B) * N;
  if (total == 0) return TBE_OK;
  TBE_REQUIRE(offsets != nullptr && out != nullptr, "%s: null pointer", name);
  const int64_t blocks = (total + 255) / 256;
  TBE_REQUIRE(blocks <= INT32_MAX, "%s: B * N = %lld exceeds the grid", name, static_cast<long long>(total));
  hipLaunchKernelGGL(jagged_to_padded_dense_kernel<T>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), values, offsets, total, N, padding, pad_begin != 0, chop_begin != 0, out);
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}

}  // namespace tbe

using namespace tbe;

extern "C" int tbe_attention_supported(int64_t L, int64_t d) { return attn_supported(L, d) ? 1 : 0; }

extern "C" int tbe_attention_forward_f32(const float* q, int64_t q_batch_stride, int64_t q_row_stride, const float* k,
                                         int64_t k_batch_stride, int64_t k_row_stride, const float* v, int64_t v_batch_stride,
                                         int64_t v_row_stride, const uint8_t* key_valid, int64_t B, int32_t H, int32_t L,
                                         int32_t d, float p, uint64_t seed, int64_t call, float* out, float* lse,
                                         void* stream) {
  const char* name = "tbe_attention_forward_f32";
  AttnArgs a{};
  a.q = q, a.k = k, a.v = v, a.key_valid = key_valid, a.out = out, a.lse = lse;
  a.q_bs = q_batch_stride, a.q_rs = q_row_stride, a.k_bs = k_batch_stride, a.k_rs = k_row_stride;
  a.v_bs = v_batch_stride, a.v_rs = v_row_stride;
  int rc = attn_check(name, a, B, H, L, d, p, seed, call);
  if (rc != TBE_OK) return rc;
  rc = check_pointers(name, {q, k, v, out}, {lse});
  if (rc != TBE_OK) return rc;
  if (B == 0) return TBE_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch ((L + kWave - 1) / kWave) {
    case 1: return attn_launch(name, attention_fwd_kernel<1>, a, B, st);
    case 2: return attn_launch(name, attention_fwd_kernel<2>, a, B, st);
    case 3: return attn_launch(name, attention_fwd_kernel<3>, a, B, st);
    default: return attn_launch(name, attention_fwd_kernel<4>, a, B, st);
  }
}

extern "C" int tbe_attention_backward_f32(const float* grad_out, const float* q, int64_t q_batch_stride, int64_t q_row_stride,
                                          const float* k, int64_t k_batch_stride, int64_t k_row_stride, const float* v,
                                          int64_t v_batch_stride, int64_t v_row_stride, const uint8_t* key_valid,
                                          const float* lse, int64_t B, int32_t H, int32_t L, int32_t d, float p, uint64_t seed,
                                          int64_t call, float* dq, float* dk, float* dv, void* stream) {
  const char* name = "tbe_attention_backward_f32";
  AttnArgs a{};
  a.q = q, a.k = k, a.v = v, a.key_valid = key_valid, a.dout = grad_out, a.lse = const_cast<float*>(lse);
  a.dq = dq, a.dk = dk, a.dv = dv;
  a.q_bs = q_batch_stride, a.q_rs = q_row_stride, a.k_bs = k_batch_stride, a.k_rs = k_row_stride;
  a.v_bs = v_batch_stride, a.v_rs = v_row_stride;
  int rc = attn_check(name, a, B, H, L, d, p, seed, call);
  if (rc != TBE_OK) return rc;
  rc = check_pointers(name, {q, k, v, grad_out}, {lse});
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(all_aligned({dq, dk, dv}, 15), "%s: tensors must be 16-B aligned", name);
  if (B == 0 || (dq == nullptr && dk == nullptr && dv == nullptr)) return TBE_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch ((L + kWave - 1) / kWave) {
    case 1: return attn_launch(name, attention_bwd_kernel<1>, a, B, st);
    case 2: return attn_launch(name, attention_bwd_kernel<2>, a, B, st);
    case 3: return attn_launch(name, attention_bwd_kernel<3>, a, B, st);
    default: return attn_launch(name, attention_bwd_kernel<4>, a, B, st);
  }
}

extern "C" int tbe_jagged_to_padded_dense_i64(const int64_t* values, const int64_t* offsets, int32_t B, int32_t N,
                                              float padding_value, int32_t pad_from_beginning, int32_t chop_from_beginning,
                                              float* out, void* stream) {
  return jagged_to_padded_dense("tbe_jagged_to_padded_dense_i64", values, offsets, B, N, padding_value, pad_from_beginning,
                                chop_from_beginning, out, stream);
}
extern "C" int tbe_jagged_to_padded_dense_i32(const int32_t* values, const int64_t* offsets, int32_t B, int32_t N,
                                              float padding_value, int32_t pad_from_beginning, int32_t chop_from_beginning,
                                              float* out, void* stream) {
  return jagged_to_padded_dense("tbe_jagged_to_padded_dense_i32", values, offsets, B, N, padding_value, pad_from_beginning,
                                chop_from_beginning, out, stream);
}
extern "C" int tbe_jagged_to_padded_dense_f32(const float* values, const int64_t* offsets, int32_t B, int32_t N,
                                              float padding_value, int32_t pad_from_beginning, int32_t chop_from_beginning,
                                              float* out, void* stream) {
  return jagged_to_padded_dense("tbe_jagged_to_padded_dense_f32", values, offsets, B, N, padding_value, pad_from_beginning,
                                chop_from_beginning, out, stream);
}
