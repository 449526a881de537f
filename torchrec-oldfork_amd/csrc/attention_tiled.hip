// Tiled masked attention for BERT4Rec on gfx950: the shapes the LDS-resident kernels of attention.hip cannot hold
// ((L, d) = (200, 128), every L above 256), with the semantics include/tbe_hip.h states for tbe_attention_forward_f32.
//
// Nothing of size L lives in LDS or in registers.  A workgroup of 4 waves owns 64 rows of one (b, h), 16 per wave, and the
// other side of the product streams through LDS in blocks of kTiledKB rows (row stride d + 4 floats, as in attention.hip):
//   operands  lane l = 16 g + r keeps its wave's owned row r, columns 16 s + 4 g .. + 3, in registers for the whole kernel
//             (d / 16 float4: the A operands of every dot product)
//   dots      16 x 16 tiles of v_mfma_f32_16x16x4_f32 against the staged rows 16 t + r: one 16-byte LDS read per four MFMAs,
//             a dot product summed over c in the order (s, c mod 4, g).  The lane ends with owned rows 4 g .. 4 g + 3 against
//             staged rows 16 t + r
//   weights   the block's 16 x kTiledKB weights (P~, dS or their transposes) go through a per-wave LDS tile [16][kTiledKB + 4]
//             and come back as A operands, one 16-byte read per four MFMAs: lane (r, g) reads the weights of owned row r at
//             staged rows 16 u + 4 g .. + 3, so the four k-slots of one MFMA are the staged rows 16 u + {0, 4, 8, 12} + n
//   sums      the B operands are the staged rows themselves: lane (r, g) reads columns 64 m + 4 r .. + 3 of staged row
//             16 u + 4 g + n (16 bytes) and feeds them to four accumulators, so accumulator 4 m + n' holds column
//             64 m + 4 r + n' of the owned rows 4 g .. 4 g + 3: a 16-byte store per row at the end.  4 * ceil(d / 64)
//             accumulators per product, whatever L is
// forward     owns queries, streams K, V: the online softmax keeps (m, l) per row and rescales O when m moves;
//             O = (sum_j keep_ij scale exp(S_ij - m_i) V_j) / l_i,  lse_i = m_i + log l_i
// backward 1  owns queries, streams K, V: D_i = dO_i . O_i from the forward's output (written to the workspace, always),
//             dQ_i = sum_j dS_ij K_j
// backward 2  owns keys, streams Q, dO with their lse and D: dV_j = sum_i P~_ij dO_i,  dK_j = sum_i dS_ij Q_i
// Every output row has one owner: no atomics, every sum in an order fixed by (L, d), two runs bit-identical.  A sample with no
// valid key: the running maximum is -1e9, every exp is 1 and the forward yields 1 / L by itself; the backward counts the
// sample's valid keys first (L bytes per wave) and takes P = 1 / L, because -1e9 + log L is -1e9 in float32.
// DESIGN.md 3o-2 has the choices, the compiler's register report and the measurements.
#include "attention_common.hpp"

namespace tbe {

constexpr int kTiledThreads = 256;
constexpr int kTiledWaves = kTiledThreads / kWave;
constexpr int kTiledRows = kTiledWaves * kAttnTile;  // owned rows per workgroup
constexpr int kTiledKB = 32;                         // streamed rows per block
constexpr int kTiledNT = kTiledKB / kAttnTile;
constexpr int kTiledPS = kTiledKB + 4;               // row stride of a weight tile
constexpr int kTiledMaxL = 4096;

static bool tiled_supported(int64_t L, int64_t d) { return L >= 1 && L <= kTiledMaxL && d >= 4 && d <= kAttnMaxD && d % 4 == 0; }
// floats: two staged blocks and `tiles` weight tiles per wave
static size_t tiled_lds_bytes(int d, int tiles) {
  return sizeof(float) * (2 * kTiledKB * attn_ds(d) + kTiledWaves * tiles * kAttnTile * kTiledPS);
}

struct TiledArgs {
  AttnArgs a;
  const float* fwd_out;  // backward: the forward's out [B, L, H * d]
  float* D;              // backward: [B, H, L], written by launch 1 and read by launch 2
  int32_t tiles;         // ceil(L / kTiledRows): workgroups per (b, h)
};

// dst[r * ds + c] = src[(row0 + r) * rs + c] for r < kTiledKB, c < d, zeros at and beyond row L, by the whole workgroup
__device__ __forceinline__ void tiled_stage(float* dst, const float* __restrict__ src, int64_t rs, int row0, int L, int d) {
  const int d4 = d >> 2, ds = attn_ds(d);
  for (int idx = threadIdx.x; idx < kTiledKB * d4; idx += kTiledThreads) {
    const int r = idx / d4, c = (idx - r * d4) * 4;
    st4(dst + r * ds + c, row0 + r < L ? ld4(src + static_cast<int64_t>(row0 + r) * rs + c) : make_float4(0.f, 0.f, 0.f, 0.f));
  }
}

// Who am I: the owned rows of the wave, the lane's place in a tile, the LDS image.
template <int NS>
struct TiledWave {
  static constexpr int NA = NS <= 4 ? 4 : 8;  // accumulators of a weighted sum: 4 per 64 columns
  int lane, r, g, wave, b, h, bh, L, d, ds, row0;
  bool active;   // the wave owns at least one row below L (wave-uniform)
  float *Ms, *Ns, *tile;
  float sqrt_d;
  uint32_t wbh;
  __device__ TiledWave(const TiledArgs& t, float* lds, int tiles_per_wave) {
    const AttnArgs& a = t.a;
    lane = threadIdx.x & (kWave - 1);
    r = lane & (kAttnTile - 1);
    g = lane >> 4;
    wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    bh = blockIdx.x / t.tiles;
    row0 = (blockIdx.x - bh * t.tiles) * kTiledRows + wave * kAttnTile;
    b = bh / a.H;
    h = bh - b * a.H;
    L = a.L;
    d = a.d;
    ds = attn_ds(d);
    active = row0 < L;
    Ms = lds;
    Ns = Ms + kTiledKB * ds;
    tile = Ns + kTiledKB * ds + wave * (tiles_per_wave * kAttnTile * kTiledPS);
    sqrt_d = sqrtf(static_cast<float>(d));
    wbh = attn_word_bh(a.callh, static_cast<uint32_t>(bh));
  }
  __device__ int own(int i) const { return min(row0 + i, L - 1); }  // owned row i of the wave, clamped for addressing
  __device__ const float* row_of(const float* base, int64_t bs, int64_t rs, int l) const {
    return base + b * bs + l * rs + h * d;
  }
  __device__ int64_t dense_row(int l, int H) const { return (static_cast<int64_t>(b) * L + l) * H * d + h * d; }
  __device__ bool key_ok(const uint8_t* kv, int j) const { return kv == nullptr || kv[static_cast<int64_t>(b) * L + j] != 0; }
  // the lane's slice of a row as A operands: columns 16 s + 4 g .. + 3, zeros beyond d
  __device__ void load_a(const float* row, float4 (&x)[NS]) const {
#pragma unroll
    for (int s = 0; s < NS; ++s) x[s] = 16 * s + 4 * g < d ? ld4(row + 16 * s + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // valid keys of the sample, the same in every lane
  __device__ int count_valid(const uint8_t* kv) const {
    if (kv == nullptr) return L;
    int n = 0;
    for (int j = lane; j < L; j += kWave) n += kv[static_cast<int64_t>(b) * L + j] != 0 ? 1 : 0;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) n += __shfl_xor(n, o, kWave);
    return n;
  }
  // acc[t][e] = sum_c x(row 4 g + e)[c] * Ms[16 t + r][c] for the first `live` tiles of the block
  __device__ void dots(const float4 (&x)[NS], const float* Xs, int live, attn_f4 (&acc)[kTiledNT]) const {
#pragma unroll
    for (int t = 0; t < kTiledNT; ++t) acc[t] = attn_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (16 * s < d) {
        const int c = 16 * s + 4 * g;
#pragma unroll
        for (int t = 0; t < kTiledNT; ++t) {
          if (t < live) {
            const float4 m = c < d ? ld4(Xs + (kAttnTile * t + r) * ds + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[s].x, m.x, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[s].y, m.y, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[s].z, m.z, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[s].w, m.w, acc[t], 0, 0, 0);
          }
        }
      }
    }
  }
  // acc[4 m + n'][e] += sum_j w[4 g + e][j] * Xs[j][64 m + 4 r + n'], j over the first `live` tiles of the block
  __device__ void wsum(const float* w, const float* Xs, int live, attn_f4 (&acc)[NA]) const {
#pragma unroll
    for (int u = 0; u < kTiledNT; ++u) {
      if (u < live) {
        const float4 wa = ld4(w + r * kTiledPS + kAttnTile * u + 4 * g);
        const float wk[4] = {wa.x, wa.y, wa.z, wa.w};
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const float* row = Xs + (kAttnTile * u + 4 * g + n) * ds;
#pragma unroll
          for (int m = 0; m < NA / 4; ++m) {
            const int c = 64 * m + 4 * r;
            const float4 x = c < d ? ld4(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            acc[4 * m + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[n], x.x, acc[4 * m + 0], 0, 0, 0);
            acc[4 * m + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[n], x.y, acc[4 * m + 1], 0, 0, 0);
            acc[4 * m + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[n], x.z, acc[4 * m + 2], 0, 0, 0);
            acc[4 * m + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[n], x.w, acc[4 * m + 3], 0, 0, 0);
          }
        }
      }
    }
  }
  // dst row (owned row 4 g + e)[64 m + 4 r .. + 3] = acc[4 m ..][e] * mul[e] for the owned rows below L
  __device__ void store(float* dst, int H, const attn_f4 (&acc)[NA], const float (&mul)[4]) const {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int l = row0 + 4 * g + e;
#pragma unroll
      for (int m = 0; m < NA / 4; ++m) {
        const int c = 64 * m + 4 * r;
        if (l < L && c < d)
          st4(dst + dense_row(l, H) + c, make_float4(acc[4 * m][e] * mul[e], acc[4 * m + 1][e] * mul[e],
                                                     acc[4 * m + 2][e] * mul[e], acc[4 * m + 3][e] * mul[e]));
      }
    }
  }
};

// tiles of 16 staged rows of the block at row j0 that hold a row below L
__device__ __forceinline__ int tiled_live(int j0, int L) { return min(kTiledNT, (L - j0 + kAttnTile - 1) / kAttnTile); }

template <int NS>
__global__ __launch_bounds__(kTiledThreads) void attention_tiled_fwd_kernel(const TiledArgs ta) {
  extern __shared__ float4 tiled_lds[];
  const AttnArgs& a = ta.a;
  TiledWave<NS> w(ta, reinterpret_cast<float*>(tiled_lds), 1);
  constexpr int NA = TiledWave<NS>::NA;
  const int L = w.L;
  float4 qa[NS];
  w.load_a(w.row_of(a.q, a.q_bs, a.q_rs, w.own(w.r)), qa);
  attn_f4 o[NA];
#pragma unroll
  for (int n = 0; n < NA; ++n) o[n] = attn_f4{0.f, 0.f, 0.f, 0.f};
  float m[4], l[4];
  uint32_t wi[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    m[e] = -INFINITY;
    l[e] = 0.f;
    wi[e] = attn_word_i(w.wbh, static_cast<uint32_t>(w.row0 + 4 * w.g + e));
  }
  for (int j0 = 0; j0 < L; j0 += kTiledKB) {
    __syncthreads();
    tiled_stage(w.Ms, w.row_of(a.k, a.k_bs, a.k_rs, 0), a.k_rs, j0, L, w.d);
    tiled_stage(w.Ns, w.row_of(a.v, a.v_bs, a.v_rs, 0), a.v_rs, j0, L, w.d);
    __syncthreads();
    if (!w.active) continue;
    const int live = tiled_live(j0, L);
    attn_f4 s[kTiledNT];
    w.dots(qa, w.Ms, live, s);
    bool in[kTiledNT];
#pragma unroll
    for (int t = 0; t < kTiledNT; ++t) {
      const int j = j0 + kAttnTile * t + w.r;
      in[t] = j < L;
      const bool ok = w.key_ok(a.key_valid, min(j, L - 1));
#pragma unroll
      for (int e = 0; e < 4; ++e) s[t][e] = ok ? s[t][e] / w.sqrt_d : -1e9f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float bm = -INFINITY;
#pragma unroll
      for (int t = 0; t < kTiledNT; ++t)
        if (in[t]) bm = fmaxf(bm, s[t][e]);
      const float mn = fmaxf(m[e], row_max(bm));  // finite: the block holds at least one key below L
      const float alpha = expf(m[e] - mn);        // 0 at the first block
      float sum = 0.f;
#pragma unroll
      for (int t = 0; t < kTiledNT; ++t) {
        float p = in[t] ? expf(s[t][e] - mn) : 0.f;
        sum += p;
        if (a.drop_thr != 0)
          p = attn_draw(wi[e], static_cast<uint32_t>(j0 + kAttnTile * t + w.r)) >= a.drop_thr ? p * a.drop_scale : 0.f;
        w.tile[(4 * w.g + e) * kTiledPS + kAttnTile * t + w.r] = p;
      }
      l[e] = l[e] * alpha + row_sum(sum);
      m[e] = mn;
#pragma unroll
      for (int n = 0; n < NA; ++n) o[n][e] *= alpha;
    }
    wave_sync();
    w.wsum(w.tile, w.Ns, live, o);
    wave_sync();
  }
  if (!w.active) return;
  float inv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = w.row0 + 4 * w.g + e;
    if (w.r == 0 && i < L) a.lse[static_cast<int64_t>(w.bh) * L + i] = m[e] + logf(l[e]);
    inv[e] = 1.f / l[e];
  }
  w.store(a.out, a.H, o, inv);
}

// backward, launch 1: the owned rows are queries
template <int NS>
__global__ __launch_bounds__(kTiledThreads) void attention_tiled_bwd_q_kernel(const TiledArgs ta) {
  extern __shared__ float4 tiled_lds[];
  const AttnArgs& a = ta.a;
  TiledWave<NS> w(ta, reinterpret_cast<float*>(tiled_lds), 1);
  constexpr int NA = TiledWave<NS>::NA;
  const int L = w.L;
  float4 qa[NS], ga[NS];
  w.load_a(w.row_of(a.q, a.q_bs, a.q_rs, w.own(w.r)), qa);
  w.load_a(a.dout + w.dense_row(w.own(w.r), a.H), ga);
  // dd[e] = dO(owned row 4 g + e) . O(owned row r), summed as dots() sums dO . V: D is the diagonal r == 4 g + e.  With one
  // valid key O_i is V_j bit for bit, so D_i has the bits of dP_ij and dS is exactly 0, as in the resident kernels.
  attn_f4 dd = {0.f, 0.f, 0.f, 0.f};
  {
    float4 oa[NS];
    w.load_a(ta.fwd_out + w.dense_row(w.own(w.r), a.H), oa);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (16 * s < w.d) {
        dd = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[s].x, oa[s].x, dd, 0, 0, 0);
        dd = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[s].y, oa[s].y, dd, 0, 0, 0);
        dd = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[s].z, oa[s].z, dd, 0, 0, 0);
        dd = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[s].w, oa[s].w, dd, 0, 0, 0);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (w.r == 4 * w.g + e && w.row0 + w.r < L) ta.D[static_cast<int64_t>(w.bh) * L + w.row0 + w.r] = dd[e];
  }
  if (a.dq == nullptr) return;
  const int nvalid = w.count_valid(a.key_valid);
  const float uniform_p = 1.f / static_cast<float>(L);
  float De[4], lse_e[4];
  uint32_t wi[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    De[e] = __shfl(dd[e], 20 * w.g + e, kWave);  // the lane (r, g) = (4 g + e, g) holds the diagonal element
    lse_e[e] = a.lse[static_cast<int64_t>(w.bh) * L + w.own(4 * w.g + e)];
    wi[e] = attn_word_i(w.wbh, static_cast<uint32_t>(w.row0 + 4 * w.g + e));
  }
  attn_f4 dq[NA];
#pragma unroll
  for (int n = 0; n < NA; ++n) dq[n] = attn_f4{0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < L; j0 += kTiledKB) {
    __syncthreads();
    tiled_stage(w.Ms, w.row_of(a.k, a.k_bs, a.k_rs, 0), a.k_rs, j0, L, w.d);
    tiled_stage(w.Ns, w.row_of(a.v, a.v_bs, a.v_rs, 0), a.v_rs, j0, L, w.d);
    __syncthreads();
    if (!w.active) continue;
    const int live = tiled_live(j0, L);
    attn_f4 s[kTiledNT], dp[kTiledNT];
    w.dots(qa, w.Ms, live, s);
    w.dots(ga, w.Ns, live, dp);
#pragma unroll
    for (int t = 0; t < kTiledNT; ++t) {
      const int j = j0 + kAttnTile * t + w.r;
      const bool ok = w.key_ok(a.key_valid, min(j, L - 1));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float sc = ok ? s[t][e] / w.sqrt_d : -1e9f;
        const float p = j < L ? (nvalid == 0 ? uniform_p : expf(sc - lse_e[e])) : 0.f;
        float x = dp[t][e];
        if (a.drop_thr != 0) x = attn_draw(wi[e], static_cast<uint32_t>(j)) >= a.drop_thr ? x * a.drop_scale : 0.f;
        w.tile[(4 * w.g + e) * kTiledPS + kAttnTile * t + w.r] = ok ? p * (x - De[e]) / w.sqrt_d : 0.f;  // dS
      }
    }
    wave_sync();
    w.wsum(w.tile, w.Ms, live, dq);
    wave_sync();
  }
  if (!w.active) return;
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  w.store(a.dq, a.H, dq, one);
}

// backward, launch 2: the owned rows are keys; Q and dO stream with their lse and D.  Two waves per SIMD asked for: left alone
// the compiler takes 277 registers at d = 128 (one wave per SIMD), bounded it takes 193 and still spills nothing.
template <int NS>
__global__ __launch_bounds__(kTiledThreads, 2) void attention_tiled_bwd_kv_kernel(const TiledArgs ta) {
  extern __shared__ float4 tiled_lds[];
  const AttnArgs& a = ta.a;
  TiledWave<NS> w(ta, reinterpret_cast<float*>(tiled_lds), 2);
  constexpr int NA = TiledWave<NS>::NA;
  const int L = w.L;
  float* tile_p = w.tile;                            // P~^T
  float* tile_s = w.tile + kAttnTile * kTiledPS;     // dS^T
  float4 ka[NS], va[NS];
  w.load_a(w.row_of(a.k, a.k_bs, a.k_rs, w.own(w.r)), ka);
  w.load_a(w.row_of(a.v, a.v_bs, a.v_rs, w.own(w.r)), va);
  const int nvalid = w.count_valid(a.key_valid);
  const float uniform_p = 1.f / static_cast<float>(L);
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) ok[e] = w.key_ok(a.key_valid, w.own(4 * w.g + e));
  attn_f4 dk[NA], dv[NA];
#pragma unroll
  for (int n = 0; n < NA; ++n) dk[n] = dv[n] = attn_f4{0.f, 0.f, 0.f, 0.f};
  const float* lse = a.lse + static_cast<int64_t>(w.bh) * L;
  const float* D = ta.D + static_cast<int64_t>(w.bh) * L;
  for (int i0 = 0; i0 < L; i0 += kTiledKB) {
    __syncthreads();
    tiled_stage(w.Ms, w.row_of(a.q, a.q_bs, a.q_rs, 0), a.q_rs, i0, L, w.d);
    tiled_stage(w.Ns, a.dout + w.dense_row(0, a.H), static_cast<int64_t>(a.H) * w.d, i0, L, w.d);
    __syncthreads();
    if (!w.active) continue;
    const int live = tiled_live(i0, L);
    attn_f4 s[kTiledNT], dp[kTiledNT];
    w.dots(ka, w.Ms, live, s);
    w.dots(va, w.Ns, live, dp);
#pragma unroll
    for (int t = 0; t < kTiledNT; ++t) {
      const int i = i0 + kAttnTile * t + w.r, ic = min(i, L - 1);
      const float lse_i = lse[ic], D_i = D[ic];
      const uint32_t wi = attn_word_i(w.wbh, static_cast<uint32_t>(i));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float sc = ok[e] ? s[t][e] / w.sqrt_d : -1e9f;
        const float p = i < L ? (nvalid == 0 ? uniform_p : expf(sc - lse_i)) : 0.f;
        float pt = p, x = dp[t][e];
        if (a.drop_thr != 0) {
          const bool keep = attn_draw(wi, static_cast<uint32_t>(w.row0 + 4 * w.g + e)) >= a.drop_thr;
          pt = keep ? p * a.drop_scale : 0.f;
          x = keep ? x * a.drop_scale : 0.f;
        }
        const int at = (4 * w.g + e) * kTiledPS + kAttnTile * t + w.r;
        tile_p[at] = pt;
        tile_s[at] = ok[e] ? p * (x - D_i) / w.sqrt_d : 0.f;
      }
    }
    wave_sync();
    if (a.dv != nullptr) w.wsum(tile_p, w.Ns, live, dv);
    if (a.dk != nullptr) w.wsum(tile_s, w.Ms, live, dk);
    wave_sync();
  }
  if (!w.active) return;
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  if (a.dv != nullptr) w.store(a.dv, a.H, dv, one);
  if (a.dk != nullptr) w.store(a.dk, a.H, dk, one);
}

// The checks both tiled entries share beyond attn_check: the grid of B * H * ceil(L / 64) workgroups.
static int tiled_check(const char* name, TiledArgs& t, int64_t B, int32_t H, int32_t L, int32_t d, float p, uint64_t seed,
                       int64_t call) {
  const int rc = attn_check(name, t.a, B, H, L, d, p, seed, call, tiled_supported(L, d), "tbe_attention_tiled_supported");
  if (rc != TBE_OK) return rc;
  t.tiles = (L + kTiledRows - 1) / kTiledRows;
  TBE_REQUIRE(B * H * t.tiles <= INT32_MAX, "%s: B * H * ceil(L / %d) = %lld workgroups exceed the grid", name, kTiledRows,
              static_cast<long long>(B * H * t.tiles));
  return TBE_OK;
}

// kernel<NS> for the NS of {1, 2, 4, 8} that covers d / 16
template <template <int> class Launch>
static int tiled_dispatch(const char* name, const TiledArgs& t, int64_t B, hipStream_t st) {
  const int ns = (t.a.d + 15) / 16;
  const dim3 grid(static_cast<unsigned>(B * t.a.H * t.tiles));
  if (ns <= 1) Launch<1>::run(t, grid, st);
  else if (ns <= 2) Launch<2>::run(t, grid, st);
  else if (ns <= 4) Launch<4>::run(t, grid, st);
  else Launch<8>::run(t, grid, st);
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}
template <int NS>
struct TiledFwd {
  static void run(const TiledArgs& t, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(attention_tiled_fwd_kernel<NS>, grid, dim3(kTiledThreads), tiled_lds_bytes(t.a.d, 1), st, t);
  }
};
template <int NS>
struct TiledBwdQ {
  static void run(const TiledArgs& t, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(attention_tiled_bwd_q_kernel<NS>, grid, dim3(kTiledThreads), tiled_lds_bytes(t.a.d, 1), st, t);
  }
};
template <int NS>
struct TiledBwdKV {
  static void run(const TiledArgs& t, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(attention_tiled_bwd_kv_kernel<NS>, grid, dim3(kTiledThreads), tiled_lds_bytes(t.a.d, 2), st, t);
  }
};

}  // namespace tbe

using namespace tbe;

extern "C" int tbe_attention_tiled_supported(int64_t L, int64_t d) { return tiled_supported(L, d) ? 1 : 0; }

extern "C" int tbe_attention_tiled_forward_f32(const float* q, int64_t q_batch_stride, int64_t q_row_stride, const float* k,
                                               int64_t k_batch_stride, int64_t k_row_stride, const float* v,
                                               int64_t v_batch_stride, int64_t v_row_stride, const uint8_t* key_valid,
                                               int64_t B, int32_t H, int32_t L, int32_t d, float p, uint64_t seed, int64_t call,
                                               float* out, float* lse, void* stream) {
  const char* name = "tbe_attention_tiled_forward_f32";
  TiledArgs t{};
  AttnArgs& a = t.a;
  a.q = q, a.k = k, a.v = v, a.key_valid = key_valid, a.out = out, a.lse = lse;
  a.q_bs = q_batch_stride, a.q_rs = q_row_stride, a.k_bs = k_batch_stride, a.k_rs = k_row_stride;
  a.v_bs = v_batch_stride, a.v_rs = v_row_stride;
  int rc = tiled_check(name, t, B, H, L, d, p, seed, call);
  if (rc != TBE_OK) return rc;
  rc = check_pointers(name, {q, k, v, out}, {lse});
  if (rc != TBE_OK) return rc;
  if (B == 0) return TBE_OK;
  return tiled_dispatch<TiledFwd>(name, t, B, static_cast<hipStream_t>(stream));
}

extern "C" int tbe_attention_tiled_backward_f32(const float* grad_out, const float* out, const float* q, int64_t q_batch_stride,
                                                int64_t q_row_stride, const float* k, int64_t k_batch_stride,
                                                int64_t k_row_stride, const float* v, int64_t v_batch_stride,
                                                int64_t v_row_stride, const uint8_t* key_valid, const float* lse, int64_t B,
                                                int32_t H, int32_t L, int32_t d, float p, uint64_t seed, int64_t call,
                                                float* D_ws, float* dq, float* dk, float* dv, void* stream) {
  const char* name = "tbe_attention_tiled_backward_f32";
  TiledArgs t{};
  AttnArgs& a = t.a;
  a.q = q, a.k = k, a.v = v, a.key_valid = key_valid, a.dout = grad_out, a.lse = const_cast<float*>(lse);
  a.dq = dq, a.dk = dk, a.dv = dv;
  a.q_bs = q_batch_stride, a.q_rs = q_row_stride, a.k_bs = k_batch_stride, a.k_rs = k_row_stride;
  a.v_bs = v_batch_stride, a.v_rs = v_row_stride;
  t.fwd_out = out, t.D = D_ws;
  int rc = tiled_check(name, t, B, H, L, d, p, seed, call);
  if (rc != TBE_OK) return rc;
  rc = check_pointers(name, {q, k, v, grad_out, out}, {lse, D_ws});
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(all_aligned({dq, dk, dv}, 15), "%s: tensors must be 16-B aligned", name);
  if (B == 0 || (dq == nullptr && dk == nullptr && dv == nullptr)) return TBE_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  rc = tiled_dispatch<TiledBwdQ>(name, t, B, st);
  if (rc != TBE_OK || (dk == nullptr && dv == nullptr)) return rc;
  return tiled_dispatch<TiledBwdKV>(name, t, B, st);
}
