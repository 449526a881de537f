// Fused DLRM dot interaction for gfx950 — the one MFMA user of the embedding hot path.
//
// Reference: InteractionArch.forward, torchrec/models/dlrm.py:193-219
//   combined = cat(dense[B,1,D], sparse[B,F,D])           (copy)
//   inter    = bmm(combined, combined^T)                    (batched 27x128x27 GEMM)
//   flat     = inter[:, triu_indices(F+1, F+1, offset=1)]   (gather)
//   out      = cat(dense, flat)                             (copy)            -> [B, D + (F+1)F/2]
// and its autograd backward (index_put, 2 bmm, cat backward).  Here each is ONE kernel that reads
// every input byte once and writes every output byte once (HBM-bound: 15.7 KB/sample forward,
// 29.5 KB/sample backward at F = 26, D = 128).
//
// A wave owns one sample at a time: X = [dense; sparse] (R = F+1 <= 32 rows) is staged in an LDS
// tile private to the wave, products run on v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf
// chain, so the oracle reproduces it bit for bit), results are re-staged in LDS and stored
// coalesced.  No inter-wave synchronisation.  The next sample's global loads are issued before
// the current sample's MFMA loop (register double buffering) so HBM latency hides behind it.
//   forward : Z = X X^T, 3 of the 4 16x16 tiles (upper triangle), K = D
//   backward: dX = (G + G^T) X with G the strict upper-triangular matrix of d(flat),
//             2 x D/16 tiles, K = R; d(dense) additionally receives d(out)[:, :D].
#include <algorithm>
#include <cstdlib>

#include "common.hpp"

namespace tbe {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// Synchronisation of a wave's lanes on wave-private LDS data.  The LDS operations of one wave execute in
// program order, so only the compiler has to be kept from moving them: a wave barrier.  (A memory fence here
// would also make the wave wait for every outstanding GLOBAL load — exactly the prefetch of the next sample
// these kernels want to keep in flight.)
__device__ __forceinline__ void wave_lds_fence() { __builtin_amdgcn_wave_barrier(); }

// index of pair (i, j), i < j < R, in torch.triu_indices(R, R, offset=1) row-major order
__device__ __forceinline__ int triu_index(int i, int j, int R) { return i * (2 * R - i - 1) / 2 + (j - i - 1); }

// inverse: row i of pair p (closed form + integer correction; exact for R <= 64)
__device__ __forceinline__ int triu_row(int p, int R) {
  const int t = 2 * R - 1;
  int i = static_cast<int>((static_cast<float>(t) - sqrtf(static_cast<float>(t * t - 8 * p))) * 0.5f);
  i = max(0, min(i, R - 2));
  while (i + 1 <= R - 2 && (i + 1) * (2 * R - (i + 1) - 1) / 2 <= p) ++i;
  while (i > 0 && i * (2 * R - i - 1) / 2 > p) --i;
  return i;
}

// Per-lane chunks of X: VPL float4 per lane cover R*D floats (D a power of two >= 16).
template <int D>
struct XLoader {
  static constexpr int LOG_V = (D == 16 ? 2 : D == 32 ? 3 : D == 64 ? 4 : D == 128 ? 5 : 6);  // log2(D/4)
  __device__ static __forceinline__ const float* src(const float* dense, const float* sparse, int64_t b, int F, int v) {
    const int r = v >> LOG_V;
    const int c = (v & ((1 << LOG_V) - 1)) * 4;
    return r == 0 ? dense + b * D + c : sparse + (b * F + (r - 1)) * D + c;
  }
};

// Forward.  MFMA operands come straight from 16-B global loads, no LDS operand tile: lane (r, q)
// (r = lane & 15, q = lane >> 4) of v_mfma_f32_16x16x4_f32 supplies element k = q of row r, and any
// assignment of columns to (step, k) slots is valid as long as both operands use the same one.  With
// column(segment s, element e, quarter q) = 16 s + 4 q + e a lane's operands for row r are the float4s
// X[r][16 s + 4 q .. +3], s = 0 .. D/16-1: D/16 coalescable 16-B loads per row tile, all issued before
// the first MFMA.  The summation order over columns is therefore (s, e, q) — the oracle walks the
// same order (oracle/dlrm_oracle.c), so results stay bit-exact.  LDS only re-stages the 351 pair
// products for a coalesced store; occupancy is bound by VGPRs (4 waves / SIMD at D = 128), not LDS.
template <int D>
__global__ __launch_bounds__(256, (D <= 128 ? 4 : 2)) void interaction_fwd_kernel(const float* __restrict__ dense,
                                                                                  const float* __restrict__ sparse,
                                                                                  float* __restrict__ out, int B, int F,
                                                                                  int64_t out_stride) {
  extern __shared__ float smem[];
  constexpr int NS = D / 16;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int R = F + 1;
  const int P = R * (R - 1) / 2;
  const int P4 = (P + 3) & ~3;
  float* zs = smem + wave * P4;
  // 16-B stores need 16-B aligned rows with room for the padded pair block (e.g. 480 floats for 128 + 351)
  const bool vec_out = (out_stride & 3) == 0 && out_stride >= D + P4 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (lane < P4 - P) zs[P + lane] = 0.f;  // the pad columns of a padded row read zeros, never garbage
  const int r16 = lane & 15;
  const int kq = lane >> 4;
  // rows >= R alias row R-1: their products only reach Z rows / columns >= R, which are never stored
  const int row0 = min(r16, R - 1);
  const int row1 = min(16 + r16, R - 1);
  const int stride_b = gridDim.x * 4;
  float4 xa[NS], xb[NS];
  float4 dpass = make_float4(0.f, 0.f, 0.f, 0.f);  // out[:, :D] = dense[b]
  // Issues every 16-B load of sample b (operands of both row tiles + the dense pass-through).
  auto issue_loads = [&](int b) {
    const float* x0 = (row0 == 0 ? dense + static_cast<int64_t>(b) * D
                                 : sparse + (static_cast<int64_t>(b) * F + (row0 - 1)) * D) + 4 * kq;
    const float* x1 = sparse + (static_cast<int64_t>(b) * F + (row1 - 1)) * D + 4 * kq;  // row1 >= 1 when R >= 2
#pragma unroll
    for (int s = 0; s < NS; ++s) xa[s] = ld4(x0 + 16 * s);
    if (R > 16) {
#pragma unroll
      for (int s = 0; s < NS; ++s) xb[s] = ld4(x1 + 16 * s);
    } else {
#pragma unroll
      for (int s = 0; s < NS; ++s) xb[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (lane < D / 4) dpass = ld4(dense + static_cast<int64_t>(b) * D + lane * 4);
  };
  int b = blockIdx.x * 4 + wave;
  if (b < B) issue_loads(b);
  for (; b < B; b += stride_b) {
    f32x4 acc00 = {0.f, 0.f, 0.f, 0.f}, acc01 = acc00, acc11 = acc00;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float a0[4] = {xa[s].x, xa[s].y, xa[s].z, xa[s].w};
      const float a1[4] = {xb[s].x, xb[s].y, xb[s].z, xb[s].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], a0[e], acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], a1[e], acc01, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], a1[e], acc11, 0, 0, 0);
      }
    }
    // The operand registers are dead from here on: the NEXT sample's loads go out now and fly while this
    // sample's products are re-staged and stored (ablation: the store phase cost 63 of 285 us when it ran
    // after the loads had been waited for).
    // out[:, :D] = dense[b] goes out BEFORE the next sample's loads are issued: `dpass` is then reloaded in place.  (Kept
    // live across the loads, the compiler parks the new value in a second register and copies it at the loop latch
    // behind an `s_waitcnt vmcnt(0)` — a full stop for every load AND store of the iteration.)
    float* orow = out + static_cast<int64_t>(b) * out_stride;
    if (lane < D / 4) {
      if (vec_out) {
        st4(orow + lane * 4, dpass);
      } else {  // rows of D + P floats are not 16-B aligned in general: scalar stores
        orow[lane * 4 + 0] = dpass.x;
        orow[lane * 4 + 1] = dpass.y;
        orow[lane * 4 + 2] = dpass.z;
        orow[lane * 4 + 3] = dpass.w;
      }
    }
    if (b + stride_b < B) issue_loads(b + stride_b);
    // C/D layout: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = kq * 4 + q;
      const int j = r16;
      if (i < j && j < R) zs[triu_index(i, j, R)] = acc00[q];
      if (16 + j < R && i < R) zs[triu_index(i, 16 + j, R)] = acc01[q];
      if (i < j && 16 + j < R) zs[triu_index(16 + i, 16 + j, R)] = acc11[q];
    }
    // zs is private to the wave and LDS operations of a wave execute in order: a compiler barrier is
    // enough (a memory fence here would also wait for the global loads just issued)
    __builtin_amdgcn_wave_barrier();
    // Straight-line stores (fixed trip counts, predicated): inside a loop with a run-time trip count the compiler puts a
    // full `s_waitcnt vmcnt(0)` in front of the stores, i.e. the wave would sit out the whole latency of the next
    // sample's loads it has just issued before it stores this sample (seen in the ISA; cost ~60 of 270 us).
    constexpr int MAXT = 8;   // pairs: P <= 31 * 32 / 2 = 496 <= 8 * 64
    constexpr int MAXQ = 2;   // float4 groups of the padded pair block: <= 124 <= 2 * 64
    if (vec_out) {  // padded rows (stride % 4 == 0): 16 B per lane, pad columns written as zeros
#pragma unroll
      for (int t = 0; t < MAXQ; ++t) {
        const int q = lane + t * kWave;
        if (q < P4 / 4) st4(orow + D + 4 * q, *reinterpret_cast<const float4*>(zs + 4 * q));
      }
    } else {  // the reference's dense [B, D + P] rows: scalar stores
#pragma unroll
      for (int t = 0; t < MAXT; ++t) {
        const int p = lane + t * kWave;
        if (p < P) orow[D + p] = zs[p];
      }
    }
    __builtin_amdgcn_wave_barrier();  // zs is rewritten by the next sample
  }
}

// A 4-byte global store the compiler cannot merge, split or skip: the LDS-DMA kernel below counts its stores to
// wait for exactly the copies in front of them (s_waitcnt vmcnt(N) retires vector-memory operations in issue order).
__device__ __forceinline__ void vm_store_dword(float* p, float v) {
  asm volatile("global_store_dword %0, %1, off" ::"v"(p), "v"(v) : "memory");
}

template <int N>
__device__ __forceinline__ void vm_wait_all_but() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Waits until at most `n` of this wave's vector-memory operations are outstanding (n <= 12, wave-uniform).
__device__ __forceinline__ void vm_wait_all_but(int n) {
  switch (n) {
    case 1: vm_wait_all_but<1>(); break;
    case 2: vm_wait_all_but<2>(); break;
    case 3: vm_wait_all_but<3>(); break;
    case 4: vm_wait_all_but<4>(); break;
    case 5: vm_wait_all_but<5>(); break;
    case 6: vm_wait_all_but<6>(); break;
    case 7: vm_wait_all_but<7>(); break;
    case 8: vm_wait_all_but<8>(); break;
    case 9: vm_wait_all_but<9>(); break;
    case 10: vm_wait_all_but<10>(); break;
    case 11: vm_wait_all_but<11>(); break;
    case 12: vm_wait_all_but<12>(); break;
    default: vm_wait_all_but<0>(); break;
  }
}

// Forward, LDS-DMA form (D >= 64).  The register form above fetches MFMA-fragment-shaped pieces: one load instruction
// touches 16 rows x 64 B, i.e. 16 half-used 128-B lines, and the texture-address path — not HBM — bounds it (loads alone
// 4.5 TB/s).  Here a sample's rows are copied global -> LDS as whole lines by `global_load_lds_dwordx4` (64 lanes x 16 B
// = 1 KiB contiguous per instruction, no VGPR in between), and the fragments are read from LDS with ds_read_b128.
//   * The LDS image of an instruction is lane-linear (destination = wave-uniform base + 16 * lane), so the bank
//     swizzle goes on the SOURCE address: slot `pp` of row r holds the 16-B piece pp ^ (r & 15) of that row.  A reader
//     of piece p of row r looks at slot p ^ (r & 15): the 16 rows one ds_read_b128 lane group covers land on 16
//     different 16-B bank slots.  Within a row the lanes still cover whole 128-B lines (the XOR permutes pieces inside
//     aligned groups).
//   * Column order of the contraction is the register form's, (segment s, element e, quarter q): bit-identical output.
//   * One LDS image per wave: once the fragments are in registers the image is dead, so the NEXT sample's copy is
//     issued before the MFMAs and flies during the products, the re-staging and the stores.
//   * The wait for that copy must not include the stores issued after it (a store retires only when L2 has taken it:
//     microseconds under load, per sample and per wave).  The dense [B, D + P] layout therefore stores through
//     vm_store_dword — a fixed number of store instructions per sample, every lane active (lanes past the end repeat
//     the last element) — and waits with vmcnt(that number).
template <int D>
__global__ __launch_bounds__(256, 2) void interaction_fwd_glds_kernel(const float* __restrict__ dense,
                                                                     const float* __restrict__ sparse,
                                                                     float* __restrict__ out, int B, int F,
                                                                     int64_t out_stride) {
  extern __shared__ float smem[];
  constexpr int NS = D / 16;
  constexpr int PR = D / 4;          // 16-B pieces per row
  constexpr int RPI = kWave / PR;    // rows per copy instruction
  constexpr int MAXI = 32 / RPI;     // copy instructions for 32 rows
  static_assert(PR >= 16 && PR <= kWave, "LDS-DMA form needs 64 <= D <= 256");
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int R = F + 1;
  const int P = R * (R - 1) / 2;
  const int P4 = (P + 3) & ~3;
  const int NI = (R + RPI - 1) / RPI;
  float* xs = smem + wave * (NI * RPI * D + P4);
  float* zs = xs + NI * RPI * D;
  const bool vec_out = (out_stride & 3) == 0 && out_stride >= D + P4 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (lane < P4 - P) zs[P + lane] = 0.f;
  const int r16 = lane & 15;
  const int kq = lane >> 4;
  const int row0 = min(r16, R - 1);       // rows >= R alias row R-1 (their products are never stored)
  const int row1 = min(16 + r16, R - 1);
  const int stride_b = gridDim.x * 4;
  // this lane's source of copy instruction i: row min(i * RPI + lane / PR, R - 1), piece (lane % PR) ^ (row & 15)
  int src_off[MAXI];  // float offset inside the sample's sparse block; row 0 (the dense row) only occurs at i = 0
#pragma unroll
  for (int i = 0; i < MAXI; ++i) {
    const int row = min(i * RPI + lane / PR, R - 1);
    const int piece = (lane % PR) ^ (row & 15);
    src_off[i] = (row - 1) * D + 4 * piece;
  }
  const bool dense_lane = lane < PR;  // instruction 0 fetches row 0 with its first PR lanes
  auto issue_copy = [&](int b) {
    const float* sp = sparse + static_cast<int64_t>(b) * F * D;
    const float* dn = dense + static_cast<int64_t>(b) * D + D;  // src_off of row 0 is -D + 4 * piece
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      if (i < NI) {
        const float* g = (i == 0 && dense_lane) ? dn + src_off[0] : sp + src_off[i];
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                         (__attribute__((address_space(3))) void*)(xs + i * (kWave * 4)), 16, 0, 0);
      }
    }
  };
  const int T = (P + kWave - 1) / kWave;  // pair stores per sample
  constexpr int DS = (D + kWave - 1) / kWave;  // dense pass-through stores per sample
  int stores_behind_copy = 0;
  int b = blockIdx.x * 4 + wave;
  if (b < B) issue_copy(b);
  for (; b < B; b += stride_b) {
    // the copy of sample b has landed once everything but the stores issued after it has retired (an LDS-DMA counts
    // on the VM counter like a load; operations retire in issue order)
    vm_wait_all_but(stores_behind_copy);
    __builtin_amdgcn_wave_barrier();
    float4 xa[NS], xb[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) xa[s] = *reinterpret_cast<const float4*>(xs + row0 * D + 4 * ((4 * s + kq) ^ (row0 & 15)));
    if (R > 16) {
#pragma unroll
      for (int s = 0; s < NS; ++s) xb[s] = *reinterpret_cast<const float4*>(xs + row1 * D + 4 * ((4 * s + kq) ^ (row1 & 15)));
    } else {
#pragma unroll
      for (int s = 0; s < NS; ++s) xb[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 dpass = make_float4(0.f, 0.f, 0.f, 0.f);
    float dscal[DS];  // row 0 is stored unswizzled
    if (vec_out) {
      if (dense_lane) dpass = *reinterpret_cast<const float4*>(xs + 4 * lane);
    } else {
#pragma unroll
      for (int t = 0; t < DS; ++t) dscal[t] = xs[min(lane + t * kWave, D - 1)];
    }
    // every read of the image has returned before the next copy may overwrite it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (b + stride_b < B) issue_copy(b + stride_b);
    f32x4 acc00 = {0.f, 0.f, 0.f, 0.f}, acc01 = acc00, acc11 = acc00;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float a0[4] = {xa[s].x, xa[s].y, xa[s].z, xa[s].w};
      const float a1[4] = {xb[s].x, xb[s].y, xb[s].z, xb[s].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], a0[e], acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], a1[e], acc01, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], a1[e], acc11, 0, 0, 0);
      }
    }
    float* orow = out + static_cast<int64_t>(b) * out_stride;
    if (vec_out) {
      if (dense_lane) st4(orow + lane * 4, dpass);
    } else {
#pragma unroll
      for (int t = 0; t < DS; ++t) vm_store_dword(orow + min(lane + t * kWave, D - 1), dscal[t]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = kq * 4 + q;
      const int j = r16;
      if (i < j && j < R) zs[triu_index(i, j, R)] = acc00[q];
      if (16 + j < R && i < R) zs[triu_index(i, 16 + j, R)] = acc01[q];
      if (i < j && 16 + j < R) zs[triu_index(16 + i, 16 + j, R)] = acc11[q];
    }
    __builtin_amdgcn_wave_barrier();
    constexpr int MAXT = 8;
    constexpr int MAXQ = 2;
    if (vec_out) {
#pragma unroll
      for (int t = 0; t < MAXQ; ++t) {
        const int q = lane + t * kWave;
        if (q < P4 / 4) st4(orow + D + 4 * q, *reinterpret_cast<const float4*>(zs + 4 * q));
      }
      stores_behind_copy = 0;  // compiler-generated stores: their number is not ours to count, wait for everything
    } else {
      float zv[MAXT];
#pragma unroll
      for (int t = 0; t < MAXT; ++t)
        if (t < T) zv[t] = zs[min(lane + t * kWave, P - 1)];
#pragma unroll
      for (int t = 0; t < MAXT; ++t)
        if (t < T) vm_store_dword(orow + D + min(lane + t * kWave, P - 1), zv[t]);
      stores_behind_copy = DS + T;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

template <int NT>  // NT = D / 16 column tiles
__global__ __launch_bounds__(256, 2) void interaction_bwd_kernel(const float* __restrict__ dense,
                                                                 const float* __restrict__ sparse,
                                                                 const float* __restrict__ grad_out,
                                                                 float* __restrict__ grad_dense,
                                                                 float* __restrict__ grad_sparse, int B, int F,
                                                                 int64_t grad_stride) {
  extern __shared__ float smem[];
  constexpr int D = NT * 16;
  constexpr int XS = D + 16;  // B-operand reads (16k + 16n + c) % 32: conflict-free over a half-wave
  constexpr int GS = 34;      // A-operand reads (2*row + k) % 32: conflict-free
  constexpr int XROWS = 28;   // K steps cover rows 0..27
  constexpr int LOG_V = XLoader<D>::LOG_V;
  constexpr int MAXV = (XROWS * D / 4 + kWave - 1) / kWave;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int R = F + 1;
  const int P = R * (R - 1) / 2;
  float* xs = smem + wave * (XROWS * XS + 32 * GS);
  float* gs = xs + XROWS * XS;
  const int r16 = lane & 15;
  const int kq = lane >> 4;
  const int nvec = R * (D / 4);
  const int ksteps = (R + 3) / 4;
  const int stride_b = gridDim.x * 4;
  // rows R..27 of X and the whole of G start as zeros; per sample only defined entries are rewritten
  for (int e = lane; e < XROWS * XS; e += kWave) xs[e] = 0.f;
  for (int e = lane; e < 32 * GS; e += kWave) gs[e] = 0.f;
  // this lane's pairs (i, j) of the strict upper triangle: p = lane + 64*t
  constexpr int MAXP = (28 * 27 / 2 + kWave - 1) / kWave;  // 6
  int pij[MAXP];
#pragma unroll
  for (int t = 0; t < MAXP; ++t) {
    const int p = lane + t * kWave;
    int i = 0, j = 1;
    if (p < P) {
      i = triu_row(p, R);
      j = i + 1 + (p - i * (2 * R - i - 1) / 2);
    }
    pij[t] = (i << 8) | j;
  }
  wave_lds_fence();

  float4 pre[MAXV];
  float gpre[MAXP];
  int b = blockIdx.x * 4 + wave;
  if (b < B) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int v = lane + i * kWave;
      if (v < nvec) pre[i] = ld4(XLoader<D>::src(dense, sparse, b, F, v));
    }
#pragma unroll
    for (int t = 0; t < MAXP; ++t) {
      const int p = lane + t * kWave;
      gpre[t] = p < P ? grad_out[static_cast<int64_t>(b) * grad_stride + D + p] : 0.f;
    }
  }
  for (; b < B; b += stride_b) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int v = lane + i * kWave;
      if (v < nvec) st4(xs + (v >> LOG_V) * XS + (v & ((1 << LOG_V) - 1)) * 4, pre[i]);
    }
#pragma unroll
    for (int t = 0; t < MAXP; ++t) {
      if (lane + t * kWave < P) {
        const int i = pij[t] >> 8, j = pij[t] & 255;
        gs[i * GS + j] = gpre[t];
        gs[j * GS + i] = gpre[t];
      }
    }
    const float* grow = grad_out + static_cast<int64_t>(b) * grad_stride;
    float4 gdense = make_float4(0.f, 0.f, 0.f, 0.f);  // d(out)[:, :D] slice this lane adds to row 0
    if (lane < D / 4) {
      if (((grad_stride & 3) | (reinterpret_cast<uintptr_t>(grad_out) & 15)) == 0) {
        gdense = ld4(grow + lane * 4);
      } else {
        gdense.x = grow[lane * 4 + 0];
        gdense.y = grow[lane * 4 + 1];
        gdense.z = grow[lane * 4 + 2];
        gdense.w = grow[lane * 4 + 3];
      }
    }
    const int nb = b + stride_b;
    if (nb < B) {
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int v = lane + i * kWave;
        if (v < nvec) pre[i] = ld4(XLoader<D>::src(dense, sparse, nb, F, v));
      }
#pragma unroll
      for (int t = 0; t < MAXP; ++t) {
        const int p = lane + t * kWave;
        gpre[t] = p < P ? grad_out[static_cast<int64_t>(nb) * grad_stride + D + p] : 0.f;
      }
    }
    wave_lds_fence();
    f32x4 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < ksteps; ++ks) {
      const int k = ks * 4 + kq;
      const float a0 = gs[r16 * GS + k];
      const float a1 = gs[(16 + r16) * GS + k];
      const float* xrow = xs + k * XS + r16;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float bn = xrow[16 * n];
        acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bn, acc[0][n], 0, 0, 0);
        acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bn, acc[1][n], 0, 0, 0);
      }
    }
    wave_lds_fence();  // every lane is done reading X before it is overwritten with dX
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = 16 * m + 4 * kq + q;
          if (row < R) xs[row * XS + 16 * n + r16] = acc[m][n][q];
        }
    wave_lds_fence();
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int v = lane + i * kWave;
      if (v < nvec) {
        const int r = v >> LOG_V;
        const int c = (v & ((1 << LOG_V) - 1)) * 4;
        float4 x = ld4(xs + r * XS + c);
        if (r == 0) {  // v == lane < D/4 here
          x.x += gdense.x;
          x.y += gdense.y;
          x.z += gdense.z;
          x.w += gdense.w;
          st4(grad_dense + static_cast<int64_t>(b) * D + c, x);
        } else {
          st4(grad_sparse + (static_cast<int64_t>(b) * F + (r - 1)) * D + c, x);
        }
      }
    }
    wave_lds_fence();
  }
}

// ---- pooling factor 1: the interaction kernels fetch the table rows themselves -------------------------------------
// With exactly one id per bag the pooled buffer is a copy of table rows that the lookup writes and these kernels read
// back.  The two kernels below are interaction_fwd_glds_kernel / interaction_bwd_kernel with ONE change: row r >= 1 of
// sample b comes from feat_weights[r-1] + local_id * D instead of sparse + (b*F + r-1)*D.  Contraction orders, LDS
// images and store paths are untouched, so the results are bit-identical to the lookup + interaction pair.
//
// Who knows which row: lane f < F is the "feature lane" of feature f.  It keeps the feature's window and table base in
// registers, classifies the one id of (f, sample) with classify_id — exactly as tbe_fwd_short_kernel does — and holds the
// resulting row ADDRESS; the lanes that fetch pieces of row r read it from lane r-1 (two ds_bpermute, no LDS memory).

// What a non-local or bad id reads instead of a table row (an LDS-DMA lane that is masked off would leave stale LDS).
__device__ __attribute__((aligned(16))) float g_zero_row[256];

struct GatherLane {
  RowWindow win;
  uint64_t base;  // table base address of this lane's feature
  bool counts;    // lane < F: bad ids are counted once, by their feature lane
};
__device__ __forceinline__ GatherLane load_gather_lane(const uint64_t* feat_weights, const int64_t* feat_rows,
                                                       const int64_t* feat_window, int lane, int F) {
  GatherLane g;
  const int f = min(lane, F - 1);
  g.win = load_window(feat_rows, feat_window, f);
  g.base = feat_weights[f];
  g.counts = lane < F;
  return g;
}
// Address of the row `id` selects (`miss` for a non-local or bad id); counts bad ids into nbad.
template <int D>
__device__ __forceinline__ uint64_t gather_row_address(const GatherLane& g, int64_t id, uint64_t miss, int& nbad) {
  int64_t local;
  const int cls = classify_id(g.win, id, local);
  if (cls == kIdBad && g.counts) ++nbad;
  return cls == kIdLocal ? g.base + static_cast<uint64_t>(local) * (D * sizeof(float)) : miss;
}
__device__ __forceinline__ void report_bad_ids(int nbad, int32_t* bounds_errors) {
  if (bounds_errors == nullptr) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o, kWave);
  if ((threadIdx.x & 63) == 0 && nbad > 0) atomicAdd(bounds_errors, nbad);
}

// Forward.  Everything a sample needs from global memory arrives by LDS-DMA, so the kernel still has no load the compiler
// would wait for (see vm_wait_all_but above: the only waits are the counted ones):
//   * the F ids of a sample — one per feature, B entries apart — by ONE global_load_lds_dword (lane l copies half l & 1 of
//     the id of feature l / 2) into a 256-B slot of the wave, issued right behind the row copy of the sample before it and
//     therefore covered by the same counted wait;
//   * the rows by the parent's copy instructions, whose per-lane source is now dense (row 0), a table row or g_zero_row.
// The copy issue is a rolled loop (one address in flight): the 64 fragment registers are live across it.
template <int D>
__global__ __launch_bounds__(256, 2) void interaction_gather_fwd_kernel(const float* __restrict__ dense,
                                                                       const uint64_t* __restrict__ feat_weights,
                                                                       const int64_t* __restrict__ feat_rows,
                                                                       const int64_t* __restrict__ feat_window,
                                                                       const int64_t* __restrict__ indices,
                                                                       float* __restrict__ out,
                                                                       int32_t* __restrict__ bounds_errors, int B, int F,
                                                                       int64_t out_stride) {
  extern __shared__ float smem[];
  constexpr int NS = D / 16;
  constexpr int PR = D / 4;          // 16-B pieces per row
  constexpr int RPI = kWave / PR;    // rows per copy instruction
  constexpr int IDS = 64;            // floats of the id slot: 32 ids of 8 B
  static_assert(PR >= 16 && PR <= kWave, "LDS-DMA form needs 64 <= D <= 256");
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int R = F + 1;
  const int P = R * (R - 1) / 2;
  const int P4 = (P + 3) & ~3;
  const int NI = (R + RPI - 1) / RPI;
  float* xs = smem + wave * (NI * RPI * D + P4 + IDS);
  float* zs = xs + NI * RPI * D;
  float* ids = zs + P4;  // 8-B aligned: every term above is a multiple of 4 floats
  const bool vec_out = (out_stride & 3) == 0 && out_stride >= D + P4 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (lane < P4 - P) zs[P + lane] = 0.f;
  const int r16 = lane & 15;
  const int kq = lane >> 4;
  const int row0 = min(r16, R - 1);       // rows >= R alias row R-1 (their products are never stored)
  const int row1 = min(16 + r16, R - 1);
  const int stride_b = gridDim.x * 4;
  const GatherLane gl = load_gather_lane(feat_weights, feat_rows, feat_window, lane, F);
  const uint64_t zero_row = reinterpret_cast<uint64_t>(&g_zero_row[0]);
  int nbad = 0;
  // id of (feature min(lane / 2, F-1), sample b), half lane & 1 -> the wave's id slot
  const uint32_t* id_words = reinterpret_cast<const uint32_t*>(indices) +
                             2 * static_cast<int64_t>(min(lane >> 1, F - 1)) * B + (lane & 1);
  auto issue_ids = [&](int b) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(id_words + 2 * static_cast<int64_t>(b)),
                                     (__attribute__((address_space(3))) void*)ids, 4, 0, 0);
  };
  // copy instruction i: row min(i * RPI + lane / PR, R - 1), piece (lane % PR) ^ (row & 15); `row_addr` is the feature
  // lanes' row address for sample b
  auto issue_copy = [&](int b, uint64_t row_addr) {
    const uint64_t dn = reinterpret_cast<uint64_t>(dense + static_cast<int64_t>(b) * D);
#pragma unroll 1
    for (int i = 0; i < NI; ++i) {
      const int row = min(i * RPI + lane / PR, R - 1);
      const int piece = (lane % PR) ^ (row & 15);
      uint64_t src = shflu64(row_addr, max(row - 1, 0));
      if (row == 0) src = dn;
      src += 16 * piece;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(xs + i * (kWave * 4)), 16, 0, 0);
    }
  };
  auto read_id = [&]() { return *reinterpret_cast<const int64_t*>(ids + 2 * min(lane, F - 1)); };
  const bool dense_lane = lane < PR;
  const int T = (P + kWave - 1) / kWave;  // pair stores per sample
  constexpr int DS = (D + kWave - 1) / kWave;  // dense pass-through stores per sample
  int stores_behind_copy = 0;
  int b = blockIdx.x * 4 + wave;
  if (b < B) {
    issue_ids(b);
    vm_wait_all_but<0>();
    __builtin_amdgcn_wave_barrier();
    const int64_t id = read_id();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    issue_copy(b, gather_row_address<D>(gl, id, zero_row, nbad));
    if (b + stride_b < B) issue_ids(b + stride_b);
  }
  for (; b < B; b += stride_b) {
    // the copy of sample b and the ids of the next sample have landed once everything but the stores issued after them
    // has retired
    vm_wait_all_but(stores_behind_copy);
    __builtin_amdgcn_wave_barrier();
    float4 xa[NS], xb[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) xa[s] = *reinterpret_cast<const float4*>(xs + row0 * D + 4 * ((4 * s + kq) ^ (row0 & 15)));
    if (R > 16) {
#pragma unroll
      for (int s = 0; s < NS; ++s) xb[s] = *reinterpret_cast<const float4*>(xs + row1 * D + 4 * ((4 * s + kq) ^ (row1 & 15)));
    } else {
#pragma unroll
      for (int s = 0; s < NS; ++s) xb[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 dpass = make_float4(0.f, 0.f, 0.f, 0.f);
    float dscal[DS];  // row 0 is stored unswizzled
    if (vec_out) {
      if (dense_lane) dpass = *reinterpret_cast<const float4*>(xs + 4 * lane);
    } else {
#pragma unroll
      for (int t = 0; t < DS; ++t) dscal[t] = xs[min(lane + t * kWave, D - 1)];
    }
    const int64_t next_id = read_id();  // of sample b + stride_b (stale when there is none: not used then)
    // every read of the image and of the id slot has returned before the next copies may overwrite them
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (b + stride_b < B) {
      issue_copy(b + stride_b, gather_row_address<D>(gl, next_id, zero_row, nbad));
      if (b + 2 * stride_b < B) issue_ids(b + 2 * stride_b);
    }
    f32x4 acc00 = {0.f, 0.f, 0.f, 0.f}, acc01 = acc00, acc11 = acc00;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float a0[4] = {xa[s].x, xa[s].y, xa[s].z, xa[s].w};
      const float a1[4] = {xb[s].x, xb[s].y, xb[s].z, xb[s].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], a0[e], acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], a1[e], acc01, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], a1[e], acc11, 0, 0, 0);
      }
    }
    float* orow = out + static_cast<int64_t>(b) * out_stride;
    if (vec_out) {
      if (dense_lane) st4(orow + lane * 4, dpass);
    } else {
#pragma unroll
      for (int t = 0; t < DS; ++t) vm_store_dword(orow + min(lane + t * kWave, D - 1), dscal[t]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = kq * 4 + q;
      const int j = r16;
      if (i < j && j < R) zs[triu_index(i, j, R)] = acc00[q];
      if (16 + j < R && i < R) zs[triu_index(i, 16 + j, R)] = acc01[q];
      if (i < j && 16 + j < R) zs[triu_index(16 + i, 16 + j, R)] = acc11[q];
    }
    __builtin_amdgcn_wave_barrier();
    constexpr int MAXT = 8;
    constexpr int MAXQ = 2;
    if (vec_out) {
#pragma unroll
      for (int t = 0; t < MAXQ; ++t) {
        const int q = lane + t * kWave;
        if (q < P4 / 4) st4(orow + D + 4 * q, *reinterpret_cast<const float4*>(zs + 4 * q));
      }
      stores_behind_copy = 0;  // compiler-generated stores: their number is not ours to count, wait for everything
    } else {
      float zv[MAXT];
#pragma unroll
      for (int t = 0; t < MAXT; ++t)
        if (t < T) zv[t] = zs[min(lane + t * kWave, P - 1)];
#pragma unroll
      for (int t = 0; t < MAXT; ++t)
        if (t < T) vm_store_dword(orow + D + min(lane + t * kWave, P - 1), zv[t]);
      stores_behind_copy = DS + T;
    }
    __builtin_amdgcn_wave_barrier();
  }
  report_bad_ids(nbad, bounds_errors);
}

// Backward.  The rows are staged through registers as in interaction_bwd_kernel; the feature lanes load the ids one
// sample further ahead than the rows (one 8-B load per lane and sample), so a row load never waits for its id.
//
// SGD: the variant that also applies the exact-SGD update of the rows a batch touches ONCE.  `single[f * B + b]` (one
// byte per contribution, tbe_backward_single_flags) says that contribution (f, b) is the only one of the call that
// touches its row: the row's gradient is then this sample's dX row alone, the old row w sits in the LDS image until dX
// overwrites it, and the row's address is the one the kernel loaded it from.  Such a row is written to the table as
// fmaf(-lr, dX + 0, w) — what bwd_update_kernel computes for it — instead of to grad_sparse, whose rows of flagged
// contributions stay unwritten; the update kernel of the same call skips them (tbe_backward_apply_skip_single_f32).
// The feature lanes load the flag where they load the id, one sample ahead of the rows.  No extra LDS, no second read of
// a row, no address the plain kernel does not dereference.  No other wave reads a flagged row (no other contribution has
// its key), and a zero row (address 0) is never flagged.  The row loads and the row stores go through plain pointers:
// nothing tells the compiler that the tables are read-only or disjoint from what is stored.
template <int NT, bool SGD = false>  // NT = D / 16 column tiles
__global__ __launch_bounds__(256, 2) void interaction_gather_bwd_kernel(const float* __restrict__ dense,
                                                                       const uint64_t* __restrict__ feat_weights,
                                                                       const int64_t* __restrict__ feat_rows,
                                                                       const int64_t* __restrict__ feat_window,
                                                                       const int64_t* __restrict__ indices,
                                                                       const float* __restrict__ grad_out,
                                                                       float* __restrict__ grad_dense,
                                                                       float* __restrict__ grad_sparse,
                                                                       int32_t* __restrict__ bounds_errors, int B, int F,
                                                                       int64_t grad_stride,
                                                                       const uint8_t* __restrict__ single, float lr) {
  extern __shared__ float smem[];
  constexpr int D = NT * 16;
  constexpr int XS = D + 16;
  constexpr int GS = 34;
  constexpr int XROWS = 28;
  constexpr int LOG_V = XLoader<D>::LOG_V;
  constexpr int MAXV = (XROWS * D / 4 + kWave - 1) / kWave;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int R = F + 1;
  const int P = R * (R - 1) / 2;
  float* xs = smem + wave * (XROWS * XS + 32 * GS);
  float* gs = xs + XROWS * XS;
  const int r16 = lane & 15;
  const int kq = lane >> 4;
  const int nvec = R * (D / 4);
  const int ksteps = (R + 3) / 4;
  const int stride_b = gridDim.x * 4;
  for (int e = lane; e < XROWS * XS; e += kWave) xs[e] = 0.f;
  for (int e = lane; e < 32 * GS; e += kWave) gs[e] = 0.f;
  constexpr int MAXP = (28 * 27 / 2 + kWave - 1) / kWave;  // 6
  int pij[MAXP];
#pragma unroll
  for (int t = 0; t < MAXP; ++t) {
    const int p = lane + t * kWave;
    int i = 0, j = 1;
    if (p < P) {
      i = triu_row(p, R);
      j = i + 1 + (p - i * (2 * R - i - 1) / 2);
    }
    pij[t] = (i << 8) | j;
  }
  wave_lds_fence();

  const GatherLane gl = load_gather_lane(feat_weights, feat_rows, feat_window, lane, F);
  const int64_t* my_ids = indices + static_cast<int64_t>(min(lane, F - 1)) * B;
  // SGD only.  Contribution (f, sample) is "once" when it is flagged and its row address is a table row's.  A ballot
  // makes that a wave-uniform mask (bit f), and the feature lane leaves the address (0 when not once) in the pad columns
  // of row f + 1 of the LDS image — columns D .. D+15 exist for the bank layout and nothing else touches them — for the
  // lanes that store the row.  Two slots per row, used in turn: the sample in flight is published while the sample
  // being computed still needs its own.
  auto my_single = [&](int s) { return single[(my_ids + s) - indices]; };  // (no second per-lane pointer: registers)
  uint32_t once_in_flight = 0;  // wave-uniform mask of the sample whose rows are in flight
  uint32_t next_single = 0;     // feature lane: flag of the sample after it (loaded with next_id)
  int slot = 0;                 // of the sample being computed
  auto publish_once = [&](uint64_t row_addr, uint32_t flag, int into_slot) {
    const bool once = lane < F && row_addr != 0 && flag != 0;
    if (lane < F) reinterpret_cast<uint64_t*>(xs + (lane + 1) * XS + D)[into_slot] = once ? row_addr : 0;
    return static_cast<uint32_t>(__ballot(once));
  };
  int nbad = 0;
  float4 pre[MAXV];
  float gpre[MAXP];
  // X of sample s: row 0 from dense, row r >= 1 from the address lane r-1 holds (0 = a zero row)
  auto load_x = [&](int s, uint64_t row_addr) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int v = lane + i * kWave;
      const int r = min(v >> LOG_V, R - 1);
      const int c = (v & ((1 << LOG_V) - 1)) * 4;
      const uint64_t src = shflu64(row_addr, max(r - 1, 0));
      if (v < nvec) {
        if (r == 0)
          pre[i] = ld4(dense + static_cast<int64_t>(s) * D + c);
        else
          pre[i] = src != 0 ? ld4(reinterpret_cast<const float*>(src) + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  int b = blockIdx.x * 4 + wave;
  int64_t next_id = 0;  // this lane's id of the sample AFTER the one whose rows are in flight
  if (b < B) {
    const uint64_t row_addr = gather_row_address<D>(gl, my_ids[b], 0, nbad);
    if constexpr (SGD) once_in_flight = publish_once(row_addr, my_single(b), 0);
    load_x(b, row_addr);
    if (b + stride_b < B) {
      next_id = my_ids[b + stride_b];
      if constexpr (SGD) next_single = my_single(b + stride_b);
    }
#pragma unroll
    for (int t = 0; t < MAXP; ++t) {
      const int p = lane + t * kWave;
      gpre[t] = p < P ? grad_out[static_cast<int64_t>(b) * grad_stride + D + p] : 0.f;
    }
  }
  for (; b < B; b += stride_b) {
    // SGD: sample b's mask, kept across the prefetch of the next sample; bit r = row r is once (row 0, the dense row, never)
    const uint32_t once_b = once_in_flight << 1;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int v = lane + i * kWave;
      if (v < nvec) st4(xs + (v >> LOG_V) * XS + (v & ((1 << LOG_V) - 1)) * 4, pre[i]);
    }
#pragma unroll
    for (int t = 0; t < MAXP; ++t) {
      if (lane + t * kWave < P) {
        const int i = pij[t] >> 8, j = pij[t] & 255;
        gs[i * GS + j] = gpre[t];
        gs[j * GS + i] = gpre[t];
      }
    }
    const float* grow = grad_out + static_cast<int64_t>(b) * grad_stride;
    float4 gdense = make_float4(0.f, 0.f, 0.f, 0.f);  // d(out)[:, :D] slice this lane adds to row 0
    if (lane < D / 4) {
      if (((grad_stride & 3) | (reinterpret_cast<uintptr_t>(grad_out) & 15)) == 0) {
        gdense = ld4(grow + lane * 4);
      } else {
        gdense.x = grow[lane * 4 + 0];
        gdense.y = grow[lane * 4 + 1];
        gdense.z = grow[lane * 4 + 2];
        gdense.w = grow[lane * 4 + 3];
      }
    }
    const int nb = b + stride_b;
    if (nb < B) {
      const uint64_t row_addr = gather_row_address<D>(gl, next_id, 0, nbad);
      if constexpr (SGD) once_in_flight = publish_once(row_addr, next_single, slot ^ 1);
      load_x(nb, row_addr);
      if (nb + stride_b < B) {
        next_id = my_ids[nb + stride_b];
        if constexpr (SGD) next_single = my_single(nb + stride_b);
      }
#pragma unroll
      for (int t = 0; t < MAXP; ++t) {
        const int p = lane + t * kWave;
        gpre[t] = p < P ? grad_out[static_cast<int64_t>(nb) * grad_stride + D + p] : 0.f;
      }
    }
    wave_lds_fence();
    f32x4 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < ksteps; ++ks) {
      const int k = ks * 4 + kq;
      const float a0 = gs[r16 * GS + k];
      const float a1 = gs[(16 + r16) * GS + k];
      const float* xrow = xs + k * XS + r16;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float bn = xrow[16 * n];
        acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bn, acc[0][n], 0, 0, 0);
        acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bn, acc[1][n], 0, 0, 0);
      }
    }
    wave_lds_fence();  // every lane is done reading X before it is overwritten with dX
    if constexpr (SGD) {
      // A flagged row becomes the NEW table row: w - lr * dX with the operands and roundings of bwd_update_kernel +
      // apply_row (the gradient is first added to the +0 accumulator, then one fmaf), w read from the very LDS word
      // that is overwritten.  One instruction stream for both kinds of row (a select, no divergent copies of the
      // stores): the old words of a row are read whether it is once or not.
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = 16 * m + 4 * kq + q;
          if (row < R) {
            float* xw = xs + row * XS + r16;
            const bool once = ((once_b >> row) & 1u) != 0;
            float w[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) w[n] = xw[16 * n];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
              const float g = acc[m][n][q];
              xw[16 * n] = once ? fmaf(-lr, fmaf(1.f, g, 0.f), w[n]) : g;
            }
          }
        }
    } else {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int row = 16 * m + 4 * kq + q;
            if (row < R) xs[row * XS + 16 * n + r16] = acc[m][n][q];
          }
    }
    wave_lds_fence();
    if constexpr (SGD) {
      // The plain store loop below with its addresses spelled as ONE per-lane base plus a compile-time offset per
      // instruction (v = lane + 64 i gives row r0 + i * RPV, column c0 and grad_sparse element 4 v - D): the kernel has
      // no registers left for fourteen hoisted copies of each.
      constexpr int RPV = kWave >> LOG_V;  // rows per store instruction
      const int r0 = lane >> LOG_V;
      const int c0 = (lane & ((1 << LOG_V) - 1)) * 4;
      const float* xl = xs + r0 * XS + c0;
      const uint64_t* sl = reinterpret_cast<const uint64_t*>(xs + r0 * XS + D) + slot;
      float* gsl = grad_sparse + (static_cast<int64_t>(b) * F - 1) * D + 4 * lane;
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int r = r0 + i * RPV;
        if (r < R) {
          float4 x = ld4(xl + i * RPV * XS);
          if (i == 0 && r == 0) {  // lanes < D/4 of the first instruction: c0 = 4 * lane
            x.x += gdense.x;
            x.y += gdense.y;
            x.z += gdense.z;
            x.w += gdense.w;
            st4(grad_dense + static_cast<int64_t>(b) * D + c0, x);
          } else {
            // where a once row came from, else 0 (a lane of row 0 never gets here)
            const uint64_t table_row = sl[i * RPV * (XS / 2)];
            st4(table_row != 0 ? reinterpret_cast<float*>(table_row) + c0 : gsl + i * (4 * kWave), x);
          }
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int v = lane + i * kWave;
        if (v < nvec) {
          const int r = v >> LOG_V;
          const int c = (v & ((1 << LOG_V) - 1)) * 4;
          float4 x = ld4(xs + r * XS + c);
          if (r == 0) {  // v == lane < D/4 here
            x.x += gdense.x;
            x.y += gdense.y;
            x.z += gdense.z;
            x.w += gdense.w;
            st4(grad_dense + static_cast<int64_t>(b) * D + c, x);
          } else {
            st4(grad_sparse + (static_cast<int64_t>(b) * F + (r - 1)) * D + c, x);
          }
        }
      }
    }
    wave_lds_fence();
    slot ^= 1;
  }
  report_bad_ids(nbad, bounds_errors);
}

}  // namespace tbe

using namespace tbe;

static unsigned interaction_grid(int B) {
  // persistent-style: 2 workgroups per CU, each wave strides over samples
  const int64_t want = (static_cast<int64_t>(B) + 3) / 4;
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(want, 256 * 2)));
}

template <typename K>
static bool reserve_lds(K kernel, size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             static_cast<int>(bytes)) == hipSuccess;
}

extern "C" int tbe_dlrm_interaction_forward_f32(const float* dense, const float* sparse, int32_t B, int32_t F,
                                                int32_t D, float* out, int64_t out_row_stride, void* stream) {
  TBE_REQUIRE(B >= 0 && F >= 1 && F <= 31, "tbe_dlrm_interaction_forward_f32: F=%d outside [1, 31]", F);
  TBE_REQUIRE(out_row_stride >= D + (F + 1) * F / 2, "tbe_dlrm_interaction_forward_f32: out_row_stride %lld < D + F(F+1)/2",
              (long long)out_row_stride);
  TBE_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128 || D == 256,
              "tbe_dlrm_interaction_forward_f32: D=%d not in {16,32,64,128,256}", D);
  if (B == 0) return TBE_OK;
  TBE_REQUIRE(dense && sparse && out, "tbe_dlrm_interaction_forward_f32: null pointer");
  TBE_REQUIRE(((reinterpret_cast<uintptr_t>(dense) | reinterpret_cast<uintptr_t>(sparse)) & 15) == 0,
              "tbe_dlrm_interaction_forward_f32: inputs must be 16-B aligned");
  const int R = F + 1, P = R * (R - 1) / 2;
  const size_t lds = 4 * static_cast<size_t>((P + 3) & ~3) * sizeof(float);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // persistent-style: 4 workgroups per CU (2 at D = 256), each wave strides over samples
  const int64_t want = (static_cast<int64_t>(B) + 3) / 4;
  const dim3 grid(static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(want, 256 * (D <= 128 ? 4 : 2)))));
  if (D == 64 || D == 128) {
    // LDS-DMA form: one [rows, D] image + the pair block per wave, 2 workgroups per CU
    const int rpi = 64 / (D / 4);
    const int rows = (R + rpi - 1) / rpi * rpi;
    const size_t lds_g = 4 * (static_cast<size_t>(rows) * D + ((P + 3) & ~3)) * sizeof(float);
    static bool glds_attr = false;
    if (!glds_attr) {
      const size_t big = 4 * (static_cast<size_t>(32) * 128 + 496) * sizeof(float);
      if (!reserve_lds(interaction_fwd_glds_kernel<128>, big) || !reserve_lds(interaction_fwd_glds_kernel<64>, big)) {
        set_error("tbe_dlrm_interaction_forward_f32: cannot reserve LDS");
        return TBE_ERR_LAUNCH;
      }
      glds_attr = true;
    }
    const dim3 grid_g(static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(want, 256 * 2))));
    if (D == 128)
      hipLaunchKernelGGL(interaction_fwd_glds_kernel<128>, grid_g, dim3(256), lds_g, st, dense, sparse, out, B, F, out_row_stride);
    else
      hipLaunchKernelGGL(interaction_fwd_glds_kernel<64>, grid_g, dim3(256), lds_g, st, dense, sparse, out, B, F, out_row_stride);
    TBE_CHECK_LAUNCH("tbe_dlrm_interaction_forward_f32");
    return TBE_OK;
  }
#define TBE_IF(DD) hipLaunchKernelGGL(interaction_fwd_kernel<DD>, grid, dim3(256), lds, st, dense, sparse, out, B, F, out_row_stride)
  switch (D) {
    case 16: TBE_IF(16); break;
    case 32: TBE_IF(32); break;
    default: TBE_IF(256); break;
  }
#undef TBE_IF
  TBE_CHECK_LAUNCH("tbe_dlrm_interaction_forward_f32");
  return TBE_OK;
}

extern "C" int tbe_dlrm_interaction_backward_f32(const float* dense, const float* sparse, const float* grad_out,
                                                 int64_t grad_row_stride, int32_t B, int32_t F, int32_t D,
                                                 float* grad_dense, float* grad_sparse, void* stream) {
  TBE_REQUIRE(B >= 0 && F >= 1 && F <= 27, "tbe_dlrm_interaction_backward_f32: F=%d outside [1, 27]", F);
  TBE_REQUIRE(grad_row_stride >= D + (F + 1) * F / 2, "tbe_dlrm_interaction_backward_f32: grad_row_stride %lld < D + F(F+1)/2",
              (long long)grad_row_stride);
  TBE_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128, "tbe_dlrm_interaction_backward_f32: D=%d not in {16,32,64,128}", D);
  if (B == 0) return TBE_OK;
  TBE_REQUIRE(dense && sparse && grad_out && grad_dense && grad_sparse, "tbe_dlrm_interaction_backward_f32: null pointer");
  TBE_REQUIRE(((reinterpret_cast<uintptr_t>(dense) | reinterpret_cast<uintptr_t>(sparse) |
                reinterpret_cast<uintptr_t>(grad_dense) | reinterpret_cast<uintptr_t>(grad_sparse)) & 15) == 0,
              "tbe_dlrm_interaction_backward_f32: tensors must be 16-B aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = 4 * (static_cast<size_t>(28) * (D + 16) + 32 * 34) * sizeof(float);
  const dim3 grid(interaction_grid(B));
  static bool attr_set = false;
  if (!attr_set) {
    const size_t big = 4 * (28 * (128 + 16) + 32 * 34) * sizeof(float);
    if (!reserve_lds(interaction_bwd_kernel<8>, big) || !reserve_lds(interaction_bwd_kernel<4>, big)) {
      set_error("tbe_dlrm_interaction_backward_f32: cannot reserve LDS");
      return TBE_ERR_LAUNCH;
    }
    attr_set = true;
  }
#define TBE_IB(NT) \
  hipLaunchKernelGGL(interaction_bwd_kernel<NT>, grid, dim3(256), lds, st, dense, sparse, grad_out, grad_dense, grad_sparse, B, F, grad_row_stride)
  switch (D) {
    case 16: TBE_IB(1); break;
    case 32: TBE_IB(2); break;
    case 64: TBE_IB(4); break;
    default: TBE_IB(8); break;
  }
#undef TBE_IB
  TBE_CHECK_LAUNCH("tbe_dlrm_interaction_backward_f32");
  return TBE_OK;
}

// ---- pooling factor 1: lookup fused into the interaction (kernels above) ------------------------------------------
static int check_gather_args(const char* what, int32_t B, int32_t F, int32_t D, int64_t row_stride) {
  TBE_REQUIRE(B >= 0 && F >= 1 && F <= 27, "%s: F=%d outside [1, 27]", what, F);
  TBE_REQUIRE(D == 64 || D == 128, "%s: D=%d not in {64,128}", what, D);
  TBE_REQUIRE(row_stride >= D + (F + 1) * F / 2, "%s: row stride %lld < D + F(F+1)/2", what, (long long)row_stride);
  return TBE_OK;
}

extern "C" int tbe_dlrm_interaction_gather_forward_f32(const float* dense, const uint64_t* feat_weights,
                                                       const int64_t* feat_rows, const int64_t* feat_window,
                                                       const int64_t* indices, int32_t B, int32_t F, int32_t D, float* out,
                                                       int64_t out_row_stride, int32_t* bounds_errors, void* stream) {
  const char* what = "tbe_dlrm_interaction_gather_forward_f32";
  if (int rc = check_gather_args(what, B, F, D, out_row_stride)) return rc;
  TBE_REQUIRE(dense && feat_weights && feat_rows && indices && out, "%s: null pointer", what);
  TBE_REQUIRE((reinterpret_cast<uintptr_t>(dense) & 15) == 0 && (reinterpret_cast<uintptr_t>(indices) & 7) == 0,
              "%s: dense must be 16-B aligned, indices 8-B aligned", what);
  if (B == 0) return TBE_OK;
  const int R = F + 1, P = R * (R - 1) / 2;
  const int rpi = 64 / (D / 4);
  const int rows = (R + rpi - 1) / rpi * rpi;
  const size_t lds = 4 * (static_cast<size_t>(rows) * D + ((P + 3) & ~3) + 64) * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    const size_t big = 4 * (static_cast<size_t>(28) * 128 + 380 + 64) * sizeof(float);
    if (!reserve_lds(interaction_gather_fwd_kernel<128>, big) || !reserve_lds(interaction_gather_fwd_kernel<64>, big)) {
      set_error("%s: cannot reserve LDS", what);
      return TBE_ERR_LAUNCH;
    }
    attr_set = true;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(interaction_grid(B));
  if (D == 128)
    hipLaunchKernelGGL(interaction_gather_fwd_kernel<128>, grid, dim3(256), lds, st, dense, feat_weights, feat_rows,
                       feat_window, indices, out, bounds_errors, B, F, out_row_stride);
  else
    hipLaunchKernelGGL(interaction_gather_fwd_kernel<64>, grid, dim3(256), lds, st, dense, feat_weights, feat_rows,
                       feat_window, indices, out, bounds_errors, B, F, out_row_stride);
  TBE_CHECK_LAUNCH(what);
  return TBE_OK;
}

extern "C" int tbe_dlrm_interaction_gather_backward_f32(const float* dense, const uint64_t* feat_weights,
                                                        const int64_t* feat_rows, const int64_t* feat_window,
                                                        const int64_t* indices, const float* grad_out,
                                                        int64_t grad_row_stride, int32_t B, int32_t F, int32_t D,
                                                        float* grad_dense, float* grad_sparse, int32_t* bounds_errors,
                                                        void* stream) {
  const char* what = "tbe_dlrm_interaction_gather_backward_f32";
  if (int rc = check_gather_args(what, B, F, D, grad_row_stride)) return rc;
  TBE_REQUIRE(dense && feat_weights && feat_rows && indices && grad_out && grad_dense && grad_sparse, "%s: null pointer",
              what);
  TBE_REQUIRE(((reinterpret_cast<uintptr_t>(dense) | reinterpret_cast<uintptr_t>(grad_dense) |
                reinterpret_cast<uintptr_t>(grad_sparse)) & 15) == 0 && (reinterpret_cast<uintptr_t>(indices) & 7) == 0,
              "%s: tensors must be 16-B aligned, indices 8-B aligned", what);
  if (B == 0) return TBE_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = 4 * (static_cast<size_t>(28) * (D + 16) + 32 * 34) * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    const size_t big = 4 * (28 * (128 + 16) + 32 * 34) * sizeof(float);
    if (!reserve_lds(interaction_gather_bwd_kernel<8>, big) || !reserve_lds(interaction_gather_bwd_kernel<4>, big)) {
      set_error("%s: cannot reserve LDS", what);
      return TBE_ERR_LAUNCH;
    }
    attr_set = true;
  }
  const dim3 grid(interaction_grid(B));
  const uint8_t* const no_flags = nullptr;
  if (D == 128)
    hipLaunchKernelGGL(interaction_gather_bwd_kernel<8>, grid, dim3(256), lds, st, dense, feat_weights, feat_rows,
                       feat_window, indices, grad_out, grad_dense, grad_sparse, bounds_errors, B, F, grad_row_stride,
                       no_flags, 0.f);
  else
    hipLaunchKernelGGL(interaction_gather_bwd_kernel<4>, grid, dim3(256), lds, st, dense, feat_weights, feat_rows,
                       feat_window, indices, grad_out, grad_dense, grad_sparse, bounds_errors, B, F, grad_row_stride,
                       no_flags, 0.f);
  TBE_CHECK_LAUNCH(what);
  return TBE_OK;
}

extern "C" int tbe_dlrm_interaction_gather_backward_sgd_f32(const float* dense, const uint64_t* feat_weights,
                                                            const int64_t* feat_rows, const int64_t* feat_window,
                                                            const int64_t* indices, const float* grad_out,
                                                            int64_t grad_row_stride, int32_t B, int32_t F, int32_t D,
                                                            float* grad_dense, float* grad_sparse,
                                                            int32_t* bounds_errors, const uint8_t* single,
                                                            float learning_rate, void* stream) {
  const char* what = "tbe_dlrm_interaction_gather_backward_sgd_f32";
  if (int rc = check_gather_args(what, B, F, D, grad_row_stride)) return rc;
  TBE_REQUIRE(dense && feat_weights && feat_rows && indices && grad_out && grad_dense && grad_sparse && single,
              "%s: null pointer", what);
  TBE_REQUIRE(((reinterpret_cast<uintptr_t>(dense) | reinterpret_cast<uintptr_t>(grad_dense) |
                reinterpret_cast<uintptr_t>(grad_sparse)) & 15) == 0 && (reinterpret_cast<uintptr_t>(indices) & 7) == 0,
              "%s: tensors must be 16-B aligned, indices 8-B aligned", what);
  if (B == 0) return TBE_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the LDS of the plain kernel, to the byte: two workgroups fill a CU at D = 128
  const size_t lds = 4 * (static_cast<size_t>(28) * (D + 16) + 32 * 34) * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    const size_t big = 4 * (28 * (128 + 16) + 32 * 34) * sizeof(float);
    if (!reserve_lds(interaction_gather_bwd_kernel<8, true>, big) || !reserve_lds(interaction_gather_bwd_kernel<4, true>, big)) {
      set_error("%s: cannot reserve LDS", what);
      return TBE_ERR_LAUNCH;
    }
    attr_set = true;
  }
  const dim3 grid(interaction_grid(B));
  if (D == 128)
    hipLaunchKernelGGL((interaction_gather_bwd_kernel<8, true>), grid, dim3(256), lds, st, dense, feat_weights, feat_rows,
                       feat_window, indices, grad_out, grad_dense, grad_sparse, bounds_errors, B, F, grad_row_stride,
                       single, learning_rate);
  else
    hipLaunchKernelGGL((interaction_gather_bwd_kernel<4, true>), grid, dim3(256), lds, st, dense, feat_weights, feat_rows,
                       feat_window, indices, grad_out, grad_dense, grad_sparse, bounds_errors, B, F, grad_row_stride,
                       single, learning_rate);
  TBE_CHECK_LAUNCH(what);
  return TBE_OK;
}
