// Quantized inference tables on gfx950: the row-wise INT8 / INT4 / INT2 quantizer and the pooled lookup that reads its rows.
//
// Reference call sites: torchrec/quant/embedding_modules.py:79 (torch.ops.fbgemm.FloatToFusedNBitRowwiseQuantizedSBHalf) and
// :168-184, :209-213 (IntNBitTableBatchedEmbeddingBagsCodegen construction and call).  fbgemm itself is absent from the
// reference tree, so the format below is fbgemm's as published and parity with it is unpinned.
//
// Format (include/tbe_hip.h "Quantized inference tables"): b = 8 / 4 / 2 bits, epb = 8 / b elements per byte, element j in
// byte j / epb at bit (j % epb) * b; a header of two halves (scale, bias).  Table layout: header in bytes 0..3, data from
// byte 4, row stride = (D / epb + 4) rounded up to 16, padding zero.  Compat layout: data first, header in the last 4 bytes.
//
// Quantizer (quantize_nbit_kernel<BITS, TPR>): a row of up to 4096 floats lives in the registers of its TPR threads, 16 columns
// a thread.  A thread's slot is 4 * epb consecutive columns = one packed dword, slot k of thread l is dword k * TPR + l (S = 4 /
// 2 / 1 slots for INT8 / INT4 / INT2).  min and max go through an xor butterfly over the row's lanes (TPR = 256: then the four
// waves in wave order through LDS).  The packed dwords, the header and the padding are assembled as the row's byte image in LDS
// at the global row's offset inside its 16-byte line, and leave as 16-byte stores line by line; what sticks out of the aligned
// lines at either end (compat rows only: they are 2-byte aligned) leaves as 2-byte stores.  One read of the input, one launch.
//   TPR by D:  D <= 256: 16 (16 rows of a workgroup in flight);  D <= 1024: 64 (a wave per row);  D <= 4096: 256.
//
// Lookup (nbit_fwd_kernel<IT, OT, LONG>: the short-bag and the long-bag body): HBM latency bound at pooling factor 1, where FP16 tables were
// not faster than FP32 ones (README "FP16 embedding tables"): what counts is the number of row reads in flight.
//  * a wave owns 64 (small launches: 16) consecutive bags of ONE feature: offsets, first ids and first weights are coalesced;
//  * a row is read by a group of G lanes, one aligned 16-byte chunk of the table-layout row per lane; G follows the row's BYTE
//    length, header included (the power of two >= (D / epb + 4) / 16 rounded up, at least 4): 16 lanes for INT8 at D = 128, 8 for INT4, 4 for INT2.  The header
//    arrives inside lane 0's chunk and is broadcast in the group: no second load;
//  * the wave has 64 / G groups and each keeps U = 4 row reads in flight: 16 / 32 / 64 independent reads per wave for INT8 /
//    INT4 / INT2 at D = 128 where the FP32 kernel has 8.  Only the 16-byte chunks are in flight; the FP32 sums of ONE bag at a
//    time live in registers (16 * epb columns a lane), so four chunks cost 16 registers, not four sets of sums;
//  * lane l's chunk holds data bytes 16 l - 4 ... 16 l + 11: columns from (16 l - 4) * epb on, a multiple of 4, so the
//    float4 / half4 output stores are aligned.  Lane 0's first dword is the header; its "columns" are negative, never stored;
//  * rows longer than 64 * 16 bytes loop: lane l also takes chunks l + 64, l + 128 (NV <= 3 / 2 / 1 for D <= 2048);
//  * bytes become floats with shifts, masks and integer-to-float conversions (v_cvt_f32_ubyteN / v_bfe_u32 in the ISA): no LDS;
//  * short kernel: the U first rows of a group's U bags are read together, then each bag is finished in turn (further ids one
//    at a time).  Long kernel (average bag >= 3.5 ids, the FP32 lookup's threshold; not re-measured here): a GROUP owns a bag,
//    reads G ids with one coalesced load and walks them with broadcasts, U rows in flight.  Either way a bag's sum runs in bag
//    order in one lane set: no LDS, no float atomics, the same bits every run.
// Arithmetic per bag (FP32):  acc_d = fmaf(w_i * scale_i, q_id, acc_d);  bacc = fmaf(w_i, bias_i, bacc);  out_d = acc_d + bacc;
// MEAN: out_d * (1.f / len).  A float16 output is that float rounded once, to nearest even.
#include <cmath>

#include "tbe_row.hpp"

namespace tbe {

constexpr int kQuantMaxD = 4096;

__device__ __forceinline__ float half_bits_to_float(uint32_t bits) {
  return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(bits & 0xffffu)));
}
__device__ __forceinline__ uint16_t float_to_half_bits(float v) {
  return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));  // round to nearest even
}

// ---- quantizer --------------------------------------------------------------------------------------------------------------
struct QuantArgs {
  const float* in;
  uint8_t* out;
  int64_t R, in_stride, out_stride;  // rows; input stride in floats; output stride in bytes
  int32_t D, data_off, hdr_off, row_len;  // row_len: bytes written per row (table: padding included)
};

// A 2-byte aligned store of 2 / 4 bytes into the LDS row image.
__device__ __forceinline__ void put16(uint8_t* p, uint32_t v) { *reinterpret_cast<uint16_t*>(p) = static_cast<uint16_t>(v); }
__device__ __forceinline__ void put32(uint8_t* p, uint32_t v) {
  if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = v;
  } else {
    put16(p, v);
    put16(p + 2, v >> 16);
  }
}

// min and max of the row over its TPR threads, in every one of them.
template <int TPR>
__device__ __forceinline__ void row_min_max(float& mn, float& mx, float (&red)[2][4]) {
  constexpr int W = TPR < kWave ? TPR : kWave;
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, o, kWave));
  }
  if constexpr (TPR == 256) {
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = mn;
      red[1][threadIdx.x >> 6] = mx;
    }
    __syncthreads();  // the image barriers of the row loop separate this use of `red` from the next row's
    mn = fminf(fminf(fminf(red[0][0], red[0][1]), red[0][2]), red[0][3]);
    mx = fmaxf(fmaxf(fmaxf(red[1][0], red[1][1]), red[1][2]), red[1][3]);
  }
}

template <int BITS, int TPR>
__global__ __launch_bounds__(256) void quantize_nbit_kernel(QuantArgs a) {
  constexpr int EPB = 8 / BITS;    // elements per byte
  constexpr int CPS = 4 * EPB;     // columns per slot = per packed dword
  constexpr int S = 16 / CPS;      // slots per thread
  constexpr int RP = 256 / TPR;    // rows in flight per workgroup
  constexpr int SLOT = TPR * 16 + 32;  // image bytes per row: the widest row of the class + header + the row's offset in its line
  constexpr float QMAX = static_cast<float>((1 << BITS) - 1);
  __shared__ __attribute__((aligned(16))) uint8_t image[RP][SLOT];
  __shared__ float red[2][4];
  const int lane = threadIdx.x % TPR;
  const int sub = threadIdx.x / TPR;
  const int D = a.D;
  const int nb = D / EPB;  // data bytes of a row
  const bool vec = (D & 3) == 0 && (a.in_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(a.in) & 15) == 0;
  const int64_t groups = (a.R + RP - 1) / RP;
  // the trip count is the same for every thread of the workgroup (barriers inside)
  for (int64_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    const int64_t r = rg * RP + sub;
    const bool live = r < a.R;
    const float* __restrict__ row = a.in + (live ? r : 0) * a.in_stride;
    float4 x[S][EPB];
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < S; ++k) {
#pragma unroll
      for (int e = 0; e < EPB; ++e) {
        const int d = (k * TPR + lane) * CPS + 4 * e;
        x[k][e] = (live && d < D) ? load_cols(row, d, D, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float el[4] = {x[k][e].x, x[k][e].y, x[k][e].z, x[k][e].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (live && d + i < D) {
            mn = fminf(mn, el[i]);
            mx = fmaxf(mx, el[i]);
          }
        }
      }
    }
    row_min_max<TPR>(mn, mx, red);
    // include/tbe_hip.h: every step FP32, no contraction
    const float minimum = half_bits_to_float(float_to_half_bits(mn));
    const float range = mx - minimum;
    float scale = half_bits_to_float(float_to_half_bits(range == 0.f ? 1.f : range / QMAX));
    if (scale == 0.f) scale = 1.f;
    float inv = 1.f / scale;
    if (isinf(inv)) {
      scale = 1.f;
      inv = 1.f;
    }
    uint8_t* grow = a.out + (live ? r : 0) * a.out_stride;
    const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(grow) & 15);
    uint8_t* img = image[sub] + mis;
    if (live) {
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const int o = 4 * (k * TPR + lane);  // data byte of this dword
        uint32_t dw = 0;
#pragma unroll
        for (int e = 0; e < EPB; ++e) {
          const int d = (k * TPR + lane) * CPS + 4 * e;
          const float el[4] = {x[k][e].x, x[k][e].y, x[k][e].z, x[k][e].w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float q = fminf(fmaxf(rintf((el[i] - minimum) * inv), 0.f), QMAX);
            if (d + i < D) dw |= static_cast<uint32_t>(q) << ((4 * e + i) * BITS);
          }
        }
        if (o + 4 <= nb) put32(img + a.data_off + o, dw);
        else if (o < nb) put16(img + a.data_off + o, dw);  // nb is even: the last dword of a row may be half a dword
      }
      if (lane == 0) {
        put16(img + a.hdr_off, float_to_half_bits(scale));
        put16(img + a.hdr_off + 2, float_to_half_bits(minimum));
      }
      // table layout: zero padding behind the data up to the row stride (fewer than 16 bytes)
      const int pad0 = max(a.data_off + nb, a.hdr_off + 4);
      if (lane < 8 && pad0 + 2 * lane < a.row_len) put16(img + pad0 + 2 * lane, 0);
    }
    __syncthreads();
    if (live) {
      // image -> global in the coordinates of the 16-byte line the row starts in: [mis, mis + row_len)
      const uint8_t* sbase = image[sub];
      uint8_t* gbase = grow - mis;
      const int end = mis + a.row_len;
      const int first_line = (mis + 15) & ~15, last_line = end & ~15;
      const int head_end = min(first_line, end);
      for (int o = mis + 2 * lane; o < head_end; o += 2 * TPR)
        *reinterpret_cast<uint16_t*>(gbase + o) = *reinterpret_cast<const uint16_t*>(sbase + o);
      for (int o = first_line + 16 * lane; o + 16 <= last_line; o += 16 * TPR)
        *reinterpret_cast<uint4*>(gbase + o) = *reinterpret_cast<const uint4*>(sbase + o);
      for (int o = max(last_line, head_end) + 2 * lane; o < end; o += 2 * TPR)
        *reinterpret_cast<uint16_t*>(gbase + o) = *reinterpret_cast<const uint16_t*>(sbase + o);
    }
    __syncthreads();  // the image is rewritten by the next row
  }
}

static int quant_tpr(int D) { return D <= 16 * 16 ? 16 : D <= 64 * 16 ? 64 : 256; }

// ---- lookup -----------------------------------------------------------------------------------------------------------------
template <typename IT>
struct NbitArgs {
  const uint64_t* feat_weights;
  const int32_t* feat_D;
  const int32_t* feat_bits;
  const int32_t* feat_row_bytes;
  const int64_t* feat_rows;
  const int64_t* feat_out_offset;
  const int32_t* feat_pooling;  // [F] TBE_POOL_SUM / TBE_POOL_MEAN (with pooling_mode MEAN), or nullptr = uniform
  const IT* indices;
  const IT* offsets;
  const float* psw;
  void* out;
  int32_t* bounds_errors;
  int64_t out_stride;
  int64_t N;
  int32_t F, B, bags_per_wave, mean;
};

// What a wave knows of its feature.
struct NbitFeat {
  const uint8_t* W;
  int64_t rows, Doff;
  int D, rb, nchunks, G;  // row bytes, their 16-byte chunks, lanes per row group
  bool mean, vec;
};

template <int BITS>
constexpr int kNbitNV = BITS == 8 ? 3 : BITS == 4 ? 2 : 1;  // chunks per lane that rows of D <= kNbitMaxD need
template <int BITS>
constexpr int kNbitCols = 128 / BITS;  // columns of one 16-byte chunk

// The chunks v * G + gl of row `id` (zeros for a row that does not count: its header is zero too, so it adds nothing).
template <int NV>
__device__ __forceinline__ void nbit_load(uint4 (&x)[NV], const NbitFeat& fr, int64_t id, bool ok, int gl) {
  const uint8_t* row = fr.W + id * fr.rb;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = v * fr.G + gl;
    x[v] = (ok && c < fr.nchunks) ? *reinterpret_cast<const uint4*>(row + 16 * c) : make_uint4(0u, 0u, 0u, 0u);
  }
}

// One row into the bag's sums.  Called by every lane of the wave (the header comes by shuffle from the group's lane 0).
template <int BITS>
__device__ __forceinline__ void nbit_accum(float (&acc)[kNbitNV<BITS>][kNbitCols<BITS>], float& bacc,
                                           const uint4 (&x)[kNbitNV<BITS>], float w, int hdr_lane, int nv) {
  constexpr int PD = 32 / BITS;  // values per dword
  constexpr uint32_t MASK = (1u << BITS) - 1u;
  const uint32_t h = static_cast<uint32_t>(__shfl(static_cast<int>(x[0].x), hdr_lane, kWave));
  const float ws = w * half_bits_to_float(h);
  bacc = fmaf(w, half_bits_to_float(h >> 16), bacc);
#pragma unroll
  for (int v = 0; v < kNbitNV<BITS>; ++v) {
    if (v < nv) {  // wave-uniform
      const uint32_t dw[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int e = 0; e < PD; ++e) {
          const float q = static_cast<float>((dw[j] >> (e * BITS)) & MASK);
          acc[v][j * PD + e] = fmaf(ws, q, acc[v][j * PD + e]);
        }
      }
    }
  }
}

template <typename OT>
__device__ __forceinline__ void nbit_store4(OT* orow, int d, int D, bool vec, float4 v) {
  if constexpr (std::is_same_v<OT, float>) {
    store_cols(orow, d, D, vec, v);
  } else {
    half4 h;
    h.x = static_cast<_Float16>(v.x);
    h.y = static_cast<_Float16>(v.y);
    h.z = static_cast<_Float16>(v.z);
    h.w = static_cast<_Float16>(v.w);
    store_cols(orow, d, D, vec, h);
  }
}

// The end of a bag: acc_d + bacc, times 1 / len under MEAN (an empty bag is +0), to the columns this lane's chunks cover.
template <int BITS, typename OT>
__device__ __forceinline__ void nbit_store(OT* orow, const NbitFeat& fr, int gl, int nv, int len,
                                           const float (&acc)[kNbitNV<BITS>][kNbitCols<BITS>], float bacc) {
  constexpr int EPB = 8 / BITS;
  float scale = 1.f;
  if (fr.mean) scale = len > 0 ? 1.f / static_cast<float>(len) : 0.f;
#pragma unroll
  for (int v = 0; v < kNbitNV<BITS>; ++v) {
    if (v < nv) {
      const int col0 = (16 * (v * fr.G + gl) - 4) * EPB;  // a chunk holds data bytes 16 c - 4 ... 16 c + 11
#pragma unroll
      for (int t = 0; t < kNbitCols<BITS> / 4; ++t) {
        const int col = col0 + 4 * t;
        if (col >= 0 && col < fr.D) {
          float4 o = make_float4(acc[v][4 * t] + bacc, acc[v][4 * t + 1] + bacc, acc[v][4 * t + 2] + bacc,
                                 acc[v][4 * t + 3] + bacc);
          if (fr.mean) o = scaled(o, scale);
          nbit_store4(orow, col, fr.D, fr.vec, o);
        }
      }
    }
  }
}

template <typename IT>
__device__ __forceinline__ bool nbit_row_ok(const NbitFeat& fr, int64_t id, bool in, int& nbad) {
  const bool inside = static_cast<uint64_t>(id) < static_cast<uint64_t>(fr.rows);
  if (in && !inside) ++nbad;
  return in && inside;
}

// Short bags: the U first rows of the group's U bags together, then each bag to its end.
template <int BITS, typename IT, typename OT>
__device__ __forceinline__ void nbit_short_body(const NbitArgs<IT>& a, const NbitFeat& fr, int lane, int bag0, int bpw,
                                                int64_t s_l, int len_l, int64_t idx0_l, float w0_l) {
  constexpr int U = 4, NV = kNbitNV<BITS>, C = kNbitCols<BITS>;
  const int G = fr.G, NG = kWave / G;
  const int g = lane / G, gl = lane & (G - 1), hdr_lane = lane - gl;
  const int nv = (fr.nchunks + G - 1) / G;
  const bool weighted = a.psw != nullptr;
  OT* out = static_cast<OT*>(a.out);
  int nbad = 0;
#pragma unroll 1
  for (int p = 0; p < bpw; p += NG * U) {  // NG * U <= 64: every j below is a lane
    if (bag0 + p >= a.B) break;            // wave-uniform tail
    int64_t s[U];
    int len[U];
    float w[U];
    uint4 x[U][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = p + u * NG + g;
      s[u] = shfl64(s_l, j);
      len[u] = __shfl(len_l, j, kWave);  // lanes from bpw on hold empty bags
      const int64_t id = shfl64(idx0_l, j);
      w[u] = __shfl(w0_l, j, kWave);
      nbit_load<NV>(x[u], fr, id, nbit_row_ok<IT>(fr, id, len[u] > 0, nbad), gl);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float acc[NV][C];
      float bacc = 0.f;
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int k = 0; k < C; ++k) acc[v][k] = 0.f;
      uint4 cur[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) cur[v] = x[u][v];
      float wc = w[u];
      for (int i = 1;; ++i) {
        nbit_accum<BITS>(acc, bacc, cur, wc, hdr_lane, nv);
        if (!__any(i < len[u])) break;  // wave-uniform: the shuffle above is met by all 64 lanes
        const bool in = i < len[u];
        int64_t id = 0;
        wc = 1.f;
        if (in) {
          id = static_cast<int64_t>(a.indices[s[u] + i]);
          if (weighted) wc = a.psw[s[u] + i];
        }
        nbit_load<NV>(cur, fr, id, nbit_row_ok<IT>(fr, id, in, nbad), gl);
      }
      const int j = p + u * NG + g;
      const int b = bag0 + j;
      if (b < a.B && j < bpw)
        nbit_store<BITS, OT>(out + static_cast<int64_t>(b) * a.out_stride + fr.Doff, fr, gl, nv, len[u], acc, bacc);
    }
  }
  if (a.bounds_errors != nullptr && nbad > 0 && gl == 0) atomicAdd(a.bounds_errors, nbad);
}

// Long bags: a group owns a bag, loads G ids at a time with one coalesced load and walks them with broadcasts.
template <int BITS, typename IT, typename OT>
__device__ __forceinline__ void nbit_long_body(const NbitArgs<IT>& a, const NbitFeat& fr, int lane, int bag0, int bpw,
                                               int64_t s_l, int len_l) {
  constexpr int U = 4, NV = kNbitNV<BITS>, C = kNbitCols<BITS>;
  const int G = fr.G, NG = kWave / G;
  const int g = lane / G, gl = lane & (G - 1), hdr_lane = lane - gl;
  const int nv = (fr.nchunks + G - 1) / G;
  const bool weighted = a.psw != nullptr;
  OT* out = static_cast<OT*>(a.out);
  int nbad = 0;
#pragma unroll 1
  for (int p = 0; p < bpw; p += NG) {  // bpw is a multiple of NG: every group makes every trip
    if (bag0 + p >= a.B) break;
    const int j = p + g;
    const int64_t s = shfl64(s_l, j);
    const int len = __shfl(len_l, j, kWave);
    float acc[NV][C];
    float bacc = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int k = 0; k < C; ++k) acc[v][k] = 0.f;
    for (int c = 0; __any(c < len); c += G) {
      const int n = min(G, max(len - c, 0));
      int64_t id_l = 0;
      float w_l = 1.f;
      if (gl < n) {
        id_l = static_cast<int64_t>(a.indices[s + c + gl]);
        if (weighted) w_l = a.psw[s + c + gl];
      }
      for (int k = 0; __any(k < n); k += U) {
        uint4 x[U][NV];
        float w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int src = hdr_lane + ((k + u) & (G - 1));
          const int64_t id = shfl64(id_l, src);
          w[u] = __shfl(w_l, src, kWave);
          nbit_load<NV>(x[u], fr, id, nbit_row_ok<IT>(fr, id, k + u < n, nbad), gl);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) nbit_accum<BITS>(acc, bacc, x[u], w[u], hdr_lane, nv);  // bag order
      }
    }
    const int b = bag0 + j;
    if (b < a.B) nbit_store<BITS, OT>(out + static_cast<int64_t>(b) * a.out_stride + fr.Doff, fr, gl, nv, len, acc, bacc);
  }
  if (a.bounds_errors != nullptr && nbad > 0 && gl == 0) atomicAdd(a.bounds_errors, nbad);
}

template <typename IT, typename OT, bool LONG>
__global__ __launch_bounds__(256) void nbit_fwd_kernel(NbitArgs<IT> a) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int f = blockIdx.x % a.F;
  const int tile = blockIdx.x / a.F;
  const int bpw = a.bags_per_wave;
  const int bag0 = (tile * 4 + wave) * bpw;
  if (bag0 >= a.B) return;  // wave-uniform

  NbitFeat fr;
  fr.W = reinterpret_cast<const uint8_t*>(a.feat_weights[f]);
  fr.rows = a.feat_rows[f];
  fr.Doff = a.feat_out_offset[f];
  fr.D = a.feat_D[f];
  fr.rb = a.feat_row_bytes[f];
  const int bits = a.feat_bits[f];
  // the chunks that hold the row (header + D * bits / 8 data bytes), never more than the stride has: a padded stride costs nothing
  fr.nchunks = min((4 + ((fr.D * (bits == 8 || bits == 4 ? bits : 2)) >> 3) + 15) >> 4, fr.rb >> 4);
  fr.G = 4;
  while (fr.G < fr.nchunks && fr.G < kWave) fr.G <<= 1;
  fr.mean = a.mean && (a.feat_pooling == nullptr || a.feat_pooling[f] == TBE_POOL_MEAN);
  fr.vec = (fr.D & 3) == 0 && (fr.Doff & 3) == 0 && (a.out_stride & 3) == 0 &&
           (reinterpret_cast<uintptr_t>(a.out) & (4 * sizeof(OT) - 1)) == 0;

  // Coalesced metadata: lane l owns bag (f, bag0 + l).
  const IT* __restrict__ offs = a.offsets + static_cast<int64_t>(f) * a.B;
  const int b_l = bag0 + lane;
  int64_t s_l = 0, e_l = 0;
  if (b_l < a.B && lane < bpw) {
    s_l = static_cast<int64_t>(offs[b_l]);
    e_l = static_cast<int64_t>(offs[b_l + 1]);
    if (s_l < 0 || e_l > a.N || s_l > e_l) {  // malformed offsets: empty bag, counted, never dereferenced
      s_l = e_l = 0;
      if (a.bounds_errors != nullptr) atomicAdd(a.bounds_errors, 1);
    }
  }
  const int len_l = static_cast<int>(e_l - s_l);
  if constexpr (LONG) {
    if (bits == 8) nbit_long_body<8, IT, OT>(a, fr, lane, bag0, bpw, s_l, len_l);
    else if (bits == 4) nbit_long_body<4, IT, OT>(a, fr, lane, bag0, bpw, s_l, len_l);
    else nbit_long_body<2, IT, OT>(a, fr, lane, bag0, bpw, s_l, len_l);
  } else {
    int64_t idx0_l = 0;
    float w0_l = 1.f;
    if (len_l > 0) {
      idx0_l = static_cast<int64_t>(a.indices[s_l]);
      if (a.psw != nullptr) w0_l = a.psw[s_l];
    }
    if (bits == 8) nbit_short_body<8, IT, OT>(a, fr, lane, bag0, bpw, s_l, len_l, idx0_l, w0_l);
    else if (bits == 4) nbit_short_body<4, IT, OT>(a, fr, lane, bag0, bpw, s_l, len_l, idx0_l, w0_l);
    else nbit_short_body<2, IT, OT>(a, fr, lane, bag0, bpw, s_l, len_l, idx0_l, w0_l);
  }
}

// The body of tbe_forward_nbit_i32 / _i64.
template <typename IT>
static int forward_nbit(const char* who, const uint64_t* feat_weights, const int32_t* feat_D, const int32_t* feat_bit_rate,
                        const int32_t* feat_row_bytes, const int64_t* feat_rows, const int64_t* feat_out_offset,
                        const int32_t* feat_pooling, int32_t F, int32_t B, const IT* indices, int64_t N, const IT* offsets,
                        const float* per_sample_weights, int32_t pooling_mode, void* out, int32_t out_f16,
                        int64_t out_row_stride, int32_t* bounds_errors, void* stream) {
  TBE_REQUIRE(F > 0 && B >= 0 && N >= 0, "%s: bad sizes F=%d B=%d N=%lld", who, F, B, (long long)N);
  TBE_REQUIRE(sizeof(IT) == 8 || N <= INT32_MAX, "%s: N=%lld ids do not fit int32 offsets", who, (long long)N);
  TBE_REQUIRE(pooling_mode == TBE_POOL_SUM || pooling_mode == TBE_POOL_MEAN, "%s: pooling_mode %d is not pooled", who,
              pooling_mode);
  TBE_REQUIRE(out_f16 == 0 || out_f16 == 1, "%s: out_f16=%d must be 0 or 1", who, out_f16);
  TBE_REQUIRE(out_row_stride > 0, "%s: out_row_stride <= 0", who);
  if (B == 0) return TBE_OK;
  TBE_REQUIRE(feat_weights && feat_D && feat_bit_rate && feat_row_bytes && feat_rows && feat_out_offset && offsets && out,
              "%s: null pointer", who);
  TBE_REQUIRE(N == 0 || indices != nullptr, "%s: null indices", who);
  TBE_REQUIRE(all_aligned({out}, out_f16 ? 1 : 3), "%s: out is not aligned to its element type", who);
  NbitArgs<IT> a{feat_weights, feat_D, feat_bit_rate, feat_row_bytes, feat_rows, feat_out_offset, feat_pooling, indices,
                 offsets, per_sample_weights, out, bounds_errors, out_row_stride, N, F, B, 64,
                 pooling_mode == TBE_POOL_MEAN ? 1 : 0};
  // small launches: 4x more waves (16 bags each) keep more row reads in flight per CU
  if (static_cast<int64_t>(F) * B < (static_cast<int64_t>(1) << 19)) a.bags_per_wave = 16;
  const int64_t tiles = (static_cast<int64_t>(B) + 4 * a.bags_per_wave - 1) / (4 * a.bags_per_wave);
  TBE_REQUIRE(tiles * F < (1ll << 31), "%s: F=%d B=%d: more than 2^31 - 1 workgroups", who, F, B);
  const dim3 grid(static_cast<unsigned>(tiles * F));
  const bool long_bags = static_cast<double>(N) / (static_cast<double>(F) * B) >= 3.5;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ProfileSpan span(TBE_PROFILE_FWD_KERNEL, st);
  dispatch_value<0, 1>(out_f16, [&](auto h) {
    using OT = std::conditional_t<decltype(h)::value == 1, _Float16, float>;
    if (long_bags) hipLaunchKernelGGL((nbit_fwd_kernel<IT, OT, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((nbit_fwd_kernel<IT, OT, false>), grid, dim3(256), 0, st, a);
  });
  TBE_CHECK_LAUNCH(who);
  return TBE_OK;
}

}  // namespace tbe

using namespace tbe;

extern "C" int tbe_quantize_nbit_f32(const float* in, int64_t R, int32_t D, int64_t in_row_stride, int32_t bit_rate,
                                     uint8_t* out, int64_t out_row_stride, int32_t data_offset, int32_t header_offset,
                                     void* stream) {
  const char* name = "tbe_quantize_nbit_f32";
  TBE_REQUIRE(bit_rate == 8 || bit_rate == 4 || bit_rate == 2, "%s: bit_rate=%d must be 8, 4 or 2", name, bit_rate);
  const int epb = 8 / bit_rate;
  TBE_REQUIRE(D > 0 && D % (2 * epb) == 0, "%s: D=%d must be a positive multiple of %d for bit_rate=%d", name, D, 2 * epb,
              bit_rate);
  TBE_REQUIRE(D <= kQuantMaxD, "%s: D=%d beyond the limit D <= %d", name, D, kQuantMaxD);
  const int nb = D / epb;
  const bool table = data_offset == 4 && header_offset == 0;
  const bool compat = data_offset == 0 && header_offset == nb;
  TBE_REQUIRE(table || compat, "%s: (data_offset, header_offset) = (%d, %d) is neither the table layout (4, 0) nor the compat "
              "layout (0, %d)", name, data_offset, header_offset, nb);
  const int row_len = table ? static_cast<int>(align_up(nb + 4, 16)) : nb + 4;
  TBE_REQUIRE(R >= 0 && in_row_stride >= D && out_row_stride >= row_len,
              "%s: R=%lld must be >= 0, in_row_stride=%lld >= D and out_row_stride=%lld >= %d", name, (long long)R,
              (long long)in_row_stride, (long long)out_row_stride, row_len);
  TBE_REQUIRE(R == 0 || (in_row_stride <= (INT64_MAX / 4) / R && out_row_stride <= INT64_MAX / R),
              "%s: R * stride beyond 2^63", name);
  if (R == 0) return TBE_OK;
  TBE_REQUIRE(in != nullptr && out != nullptr, "%s: null pointer", name);
  TBE_REQUIRE(all_aligned({in}, 3), "%s: in must be 4-B aligned", name);
  if (table) {
    TBE_REQUIRE(all_aligned({out}, 15) && out_row_stride % 16 == 0, "%s: table-layout rows must be 16-B aligned (out, out_row_stride)",
                name);
  } else {
    TBE_REQUIRE(all_aligned({out}, 1) && out_row_stride % 2 == 0, "%s: compat-layout rows must be 2-B aligned (out, out_row_stride)",
                name);
  }
  const QuantArgs a{in, out, R, in_row_stride, out_row_stride, D, data_offset, header_offset, row_len};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tpr = quant_tpr(D);
  const int64_t groups = (R + 256 / tpr - 1) / (256 / tpr);
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>(groups, 256 * 32)));
  dispatch_value<8, 4, 2>(bit_rate, [&](auto b) {
    dispatch_value<16, 64, 256>(tpr, [&](auto t) {
      hipLaunchKernelGGL((quantize_nbit_kernel<decltype(b)::value, decltype(t)::value>), grid, dim3(256), 0, st, a);
    });
  });
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}

extern "C" int tbe_forward_nbit_i32(const uint64_t* feat_weights, const int32_t* feat_D, const int32_t* feat_bit_rate,
                                    const int32_t* feat_row_bytes, const int64_t* feat_rows, const int64_t* feat_out_offset,
                                    const int32_t* feat_pooling, int32_t F, int32_t B, const int32_t* indices, int64_t N,
                                    const int32_t* offsets, const float* per_sample_weights, int32_t pooling_mode, void* out,
                                    int32_t out_f16, int64_t out_row_stride, int32_t* bounds_errors, void* stream) {
  return forward_nbit<int32_t>("tbe_forward_nbit_i32", feat_weights, feat_D, feat_bit_rate, feat_row_bytes, feat_rows,
                               feat_out_offset, feat_pooling, F, B, indices, N, offsets, per_sample_weights, pooling_mode, out,
                               out_f16, out_row_stride, bounds_errors, stream);
}

extern "C" int tbe_forward_nbit_i64(const uint64_t* feat_weights, const int32_t* feat_D, const int32_t* feat_bit_rate,
                                    const int32_t* feat_row_bytes, const int64_t* feat_rows, const int64_t* feat_out_offset,
                                    const int32_t* feat_pooling, int32_t F, int32_t B, const int64_t* indices, int64_t N,
                                    const int64_t* offsets, const float* per_sample_weights, int32_t pooling_mode, void* out,
                                    int32_t out_f16, int64_t out_row_stride, int32_t* bounds_errors, void* stream) {
  return forward_nbit<int64_t>("tbe_forward_nbit_i64", feat_weights, feat_D, feat_bit_rate, feat_row_bytes, feat_rows,
                               feat_out_offset, feat_pooling, F, B, indices, N, offsets, per_sample_weights, pooling_mode, out,
                               out_f16, out_row_stride, bounds_errors, stream);
}
