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
//
// Five kernels; a block of work they have in common is written once.  What a kernel keeps for itself is how a sample's rows ARRIVE — that is
// where their register budgets differ — and everything behind the arrival is shared:
//   forward   interaction_fwd_kernel         register loads in MFMA-fragment shape, predicated straight-line stores
//             interaction_fwd_glds_kernel    LDS-DMA copy from the pooled buffer, unrolled, per-lane offsets kept in registers
//             interaction_gather_fwd_kernel  LDS-DMA copy from the tables, rolled, ids through an LDS slot
//     shared: FwdWave (the wave's geometry), fwd_contract, fwd_stage_pairs; by the two LDS-DMA kernels also FwdImage (the
//             per-wave LDS image, which the host sizes the launch from), fwd_read_fragments, fwd_read_dense / fwd_store_dense,
//             fwd_store_pairs_counted
//   backward  interaction_bwd_kernel         rows from the pooled buffer (XLoader)
//             interaction_gather_bwd_kernel  rows from the tables (shflu64 of the feature lanes' addresses); <NT, true> also
//                                            applies SGD to once-touched rows (its blocks have this one user and stay inline)
//     shared: BwdTile (the LDS tile, host and device), BwdWave, bwd_zero_tile, bwd_pair_table, bwd_load_pair_grads,
//             bwd_load_gdense, bwd_stage, bwd_contract, bwd_store (the dense kernel spells the store loop itself, and both
//             spell the six-line write-back of dX: see there for what the shared forms cost)
// The helpers are __forceinline__, take register arrays by reference and LDS pointers by value, and leave every order of
// summation, LDS layout and store path as it was in the kernels they were cut from.  Where a helper's form is not the obvious
// one (fragments by value into fwd_contract, locals in interaction_fwd_kernel, bwd_load_rows a function) its comment gives
// the measurement that decided it: the register allocation of these kernels is that close to the edge.
#include <algorithm>
#include <cstdlib>

#include "common.hpp"

namespace tbe {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// Rows X = [dense; sparse] may have.  Forward: the two 16-row MFMA tiles.  Backward and the gather pair: seven K steps of four
// rows, and the LDS tile of which two workgroups fill a CU at D = 128 (BwdTile below).
constexpr int kFwdMaxRows = 32;
constexpr int kBwdMaxRows = 28;
constexpr int pair_count(int R) { return R * (R - 1) / 2; }
constexpr int pad4(int n) { return (n + 3) & ~3; }
constexpr int wave_chunks(int n) { return (n + kWave - 1) / kWave; }  // one-element-per-lane instructions that cover n elements

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

// ---- forward: what the three kernels share ---------------------------------------------------------------------------------
// A wave's view of the forward: its lane's place in the MFMA layout (row r16 of a 16-row tile, k-quarter kq), the pair block
// (P pairs, padded to P4) and whether `out` takes 16-B stores.
template <int D>
struct FwdWave {
  const int lane, wave, R, P, P4, r16, kq, row0, row1, stride_b;
  const bool vec_out;
  __device__ __forceinline__ FwdWave(int F, const float* out, int64_t out_stride)
      : lane(threadIdx.x & 63), wave(threadIdx.x >> 6), R(F + 1), P(pair_count(R)), P4(pad4(P)), r16(lane & 15), kq(lane >> 4),
        // rows >= R alias row R-1: their products only reach Z rows / columns >= R, which are never stored
        row0(min(r16, R - 1)), row1(min(16 + r16, R - 1)), stride_b(gridDim.x * 4),
        // 16-B stores need 16-B aligned rows with room for the padded pair block (e.g. 480 floats for 128 + 351)
        vec_out((out_stride & 3) == 0 && out_stride >= D + P4 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {}
  __device__ __forceinline__ int first_sample() const { return blockIdx.x * 4 + wave; }
  // the pad columns of a padded row read zeros, never garbage
  __device__ __forceinline__ void zero_pad(float* zs) const {
    if (lane < P4 - P) zs[P + lane] = 0.f;
  }
};

// Pair stores of a sample: scalar (the reference's [B, D + P] rows) and 16-B (padded rows), one per lane and instruction.
constexpr int kMaxPairStores = wave_chunks(pair_count(kFwdMaxRows));         // 8: P <= 31 * 32 / 2 = 496
constexpr int kMaxPairStores4 = wave_chunks(pad4(pair_count(kFwdMaxRows)) / 4);  // 2: <= 124 float4 groups
static_assert(kMaxPairStores == 8 && kMaxPairStores4 == 2, "the unrolled store loops cover the pair block of kFwdMaxRows rows");

// Z = X X^T, the three upper 16x16 tiles.  Lane (r, q) of v_mfma_f32_16x16x4_f32 supplies element k = q of row r; its operands
// for segment s are the float4s X[row][16 s + 4 q .. +3], so the summation order over columns is (s, e, q) — the oracle walks
// the same order (oracle/dlrm_oracle.c) and results stay bit-exact.
// The fragments reach the MFMA loop BY VALUE (FwdRows): with the loop reading the kernel's own arrays through references, the
// register form's next loads — issued right behind it — got an address register inside the range they load into, and the
// compiler copied two of the loaded words behind an `s_waitcnt vmcnt(1)`: the wave sat out the loads it had just issued
// (interaction_fwd_kernel<256>: 134 -> 137 us).
template <int NS>
struct FwdRows {
  float4 a[NS], b[NS];  // this lane's operands of row tile 0 and row tile 1, one float4 per segment
};
template <int NS>
__device__ __forceinline__ void fwd_contract(const FwdRows<NS> x, f32x4& acc00, f32x4& acc01, f32x4& acc11) {
  acc00 = f32x4{0.f, 0.f, 0.f, 0.f};
  acc01 = acc00;
  acc11 = acc00;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float a0[4] = {x.a[s].x, x.a[s].y, x.a[s].z, x.a[s].w};
    const float a1[4] = {x.b[s].x, x.b[s].y, x.b[s].z, x.b[s].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], a0[e], acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], a1[e], acc01, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], a1[e], acc11, 0, 0, 0);
    }
  }
}

// The three tiles -> the wave's pair block in triu order.  C/D layout: col = lane & 15, row = (lane >> 4) * 4 + reg.
template <int D>
__device__ __forceinline__ void fwd_stage_pairs(float* zs, const FwdWave<D>& w, const f32x4& acc00, const f32x4& acc01,
                                                const f32x4& acc11) {
  const int R = w.R;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = w.kq * 4 + q;
    const int j = w.r16;
    if (i < j && j < R) zs[triu_index(i, j, R)] = acc00[q];
    if (16 + j < R && i < R) zs[triu_index(i, 16 + j, R)] = acc01[q];
    if (i < j && 16 + j < R) zs[triu_index(16 + i, 16 + j, R)] = acc11[q];
  }
}

// Forward.  MFMA operands come straight from 16-B global loads, no LDS operand tile: lane (r, q)
// (r = lane & 15, q = lane >> 4) of v_mfma_f32_16x16x4_f32 supplies element k = q of row r, and any
// assignment of columns to (step, k) slots is valid as long as both operands use the same one.  With
// column(segment s, element e, quarter q) = 16 s + 4 q + e a lane's operands for row r are the float4s
// X[r][16 s + 4 q .. +3], s = 0 .. D/16-1: D/16 coalescable 16-B loads per row tile, all issued before
// the first MFMA (fwd_contract).  LDS only re-stages the 351 pair
// products for a coalesced store; occupancy is bound by VGPRs (4 waves / SIMD at D = 128), not LDS.
template <int D>
__global__ __launch_bounds__(256, (D <= 128 ? 4 : 2)) void interaction_fwd_kernel(const float* __restrict__ dense,
                                                                                  const float* __restrict__ sparse,
                                                                                  float* __restrict__ out, int B, int F,
                                                                                  int64_t out_stride) {
  extern __shared__ float smem[];
  constexpr int NS = D / 16;
  const FwdWave<D> w(F, out, out_stride);
  // As locals: read through `w` inside issue_loads, the <16> kernel copies two of the words it has just loaded behind an
  // `s_waitcnt vmcnt(0)` (the same stop as the one described at `dpass` below).
  const int lane = w.lane, row0 = w.row0, row1 = w.row1, kq = w.kq, stride_b = w.stride_b;
  float* zs = smem + w.wave * w.P4;
  w.zero_pad(zs);
  float4 xa[NS], xb[NS];
  float4 dpass = make_float4(0.f, 0.f, 0.f, 0.f);  // out[:, :D] = dense[b]
  // Issues every 16-B load of sample b (operands of both row tiles + the dense pass-through).
  auto issue_loads = [&](int b) {
    const float* x0 = (row0 == 0 ? dense + static_cast<int64_t>(b) * D
                                   : sparse + (static_cast<int64_t>(b) * F + (row0 - 1)) * D) + 4 * kq;
    const float* x1 = sparse + (static_cast<int64_t>(b) * F + (row1 - 1)) * D + 4 * kq;  // row1 >= 1 when R >= 2
#pragma unroll
    for (int s = 0; s < NS; ++s) xa[s] = ld4(x0 + 16 * s);
    if (w.R > 16) {
#pragma unroll
      for (int s = 0; s < NS; ++s) xb[s] = ld4(x1 + 16 * s);
    } else {
#pragma unroll
      for (int s = 0; s < NS; ++s) xb[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (lane < D / 4) dpass = ld4(dense + static_cast<int64_t>(b) * D + lane * 4);
  };
  int b = w.first_sample();
  if (b < B) issue_loads(b);
  for (; b < B; b += w.stride_b) {
    f32x4 acc00, acc01, acc11;
    FwdRows<NS> x;  // a copy made HERE, in the kernel's body (see fwd_contract): the arrays the loads write stay the kernel's own
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      x.a[s] = xa[s];
      x.b[s] = xb[s];
    }
    fwd_contract<NS>(x, acc00, acc01, acc11);
    // The operand registers are dead from here on: the NEXT sample's loads go out now and fly while this
    // sample's products are re-staged and stored (ablation: the store phase cost 63 of 285 us when it ran
    // after the loads had been waited for).
    // out[:, :D] = dense[b] goes out BEFORE the next sample's loads are issued: `dpass` is then reloaded in place.  (Kept
    // live across the loads, the compiler parks the new value in a second register and copies it at the loop latch
    // behind an `s_waitcnt vmcnt(0)` — a full stop for every load AND store of the iteration.)
    float* orow = out + static_cast<int64_t>(b) * out_stride;
    if (lane < D / 4) {
      if (w.vec_out) {
        st4(orow + lane * 4, dpass);
      } else {  // rows of D + P floats are not 16-B aligned in general: scalar stores
        orow[lane * 4 + 0] = dpass.x;
        orow[lane * 4 + 1] = dpass.y;
        orow[lane * 4 + 2] = dpass.z;
        orow[lane * 4 + 3] = dpass.w;
      }
    }
    if (b + stride_b < B) issue_loads(b + stride_b);
    fwd_stage_pairs(zs, w, acc00, acc01, acc11);
    wave_lds_fence();
    // Straight-line stores (fixed trip counts, predicated): inside a loop with a run-time trip count the compiler puts a
    // full `s_waitcnt vmcnt(0)` in front of the stores, i.e. the wave would sit out the whole latency of the next
    // sample's loads it has just issued before it stores this sample (seen in the ISA; cost ~60 of 270 us).
    if (w.vec_out) {  // padded rows (stride % 4 == 0): 16 B per lane, pad columns written as zeros
#pragma unroll
      for (int t = 0; t < kMaxPairStores4; ++t) {
        const int q = lane + t * kWave;
        if (q < w.P4 / 4) st4(orow + D + 4 * q, *reinterpret_cast<const float4*>(zs + 4 * q));
      }
    } else {  // the reference's dense [B, D + P] rows: scalar stores
#pragma unroll
      for (int t = 0; t < kMaxPairStores; ++t) {
        const int p = lane + t * kWave;
        if (p < w.P) orow[D + p] = zs[p];
      }
    }
    wave_lds_fence();  // zs is rewritten by the next sample
  }
}

// A 4-byte global store the compiler cannot merge, split or skip: the LDS-DMA kernels below count their stores to
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

// ---- forward: what the two LDS-DMA kernels share -----------------------------------------------------------------------------
// The LDS image of one wave: the rows a whole number of copy instructions brings (R rounded up to RPI), the padded pair block,
// and IDS floats of id slot (the gather kernel).  The kernels carve their pointers from it and the host sizes the launch.
constexpr int kIdSlotFloats = 64;  // 32 ids of 8 B
template <int D, int IDS = 0>
struct FwdImage {
  static constexpr int PR = D / 4;                // 16-B pieces per row
  static constexpr int RPI = kWave / PR;          // rows per copy instruction
  static constexpr int DS = wave_chunks(D);       // dense pass-through stores per sample
  static_assert(PR >= 16 && PR <= kWave, "LDS-DMA form needs 64 <= D <= 256");
  static_assert(DS + kMaxPairStores <= 12, "vm_wait_all_but(n) counts up to 12 stores");
  static constexpr int copies(int R) { return (R + RPI - 1) / RPI; }
  static constexpr int zs_offset(int R) { return copies(R) * RPI * D; }
  static constexpr int ids_offset(int R) { return zs_offset(R) + pad4(pair_count(R)); }  // 8-B aligned: multiples of 4 floats
  static constexpr int floats(int R) { return ids_offset(R) + IDS; }
};

// The MFMA fragments of the sample in the image.  Slot `pp` of row r holds the 16-B piece pp ^ (r & 15) of that row, so a
// reader of piece p of row r looks at slot p ^ (r & 15).
template <int D>
__device__ __forceinline__ void fwd_read_fragments(const float* xs, const FwdWave<D>& w, FwdRows<D / 16>& x) {
  constexpr int NS = D / 16;
  const int row0 = w.row0, row1 = w.row1, kq = w.kq;
#pragma unroll
  for (int s = 0; s < NS; ++s) x.a[s] = *reinterpret_cast<const float4*>(xs + row0 * D + 4 * ((4 * s + kq) ^ (row0 & 15)));
  if (w.R > 16) {
#pragma unroll
    for (int s = 0; s < NS; ++s) x.b[s] = *reinterpret_cast<const float4*>(xs + row1 * D + 4 * ((4 * s + kq) ^ (row1 & 15)));
  } else {
#pragma unroll
    for (int s = 0; s < NS; ++s) x.b[s] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// out[:, :D] = dense[b] from row 0 of the image, which is stored unswizzled: one float4 of the first PR lanes (padded rows) or
// DS counted dwords of every lane (lanes past the end repeat the last element).
template <int D>
__device__ __forceinline__ void fwd_read_dense(const float* xs, const FwdWave<D>& w, float4& dpass,
                                               float (&dscal)[FwdImage<D>::DS]) {
  dpass = make_float4(0.f, 0.f, 0.f, 0.f);
  if (w.vec_out) {
    if (w.lane < FwdImage<D>::PR) dpass = *reinterpret_cast<const float4*>(xs + 4 * w.lane);
  } else {
#pragma unroll
    for (int t = 0; t < FwdImage<D>::DS; ++t) dscal[t] = xs[min(w.lane + t * kWave, D - 1)];
  }
}
template <int D>
__device__ __forceinline__ void fwd_store_dense(float* orow, const FwdWave<D>& w, const float4& dpass,
                                                const float (&dscal)[FwdImage<D>::DS]) {
  if (w.vec_out) {
    if (w.lane < FwdImage<D>::PR) st4(orow + w.lane * 4, dpass);
  } else {
#pragma unroll
    for (int t = 0; t < FwdImage<D>::DS; ++t) vm_store_dword(orow + min(w.lane + t * kWave, D - 1), dscal[t]);
  }
}

// The pair block -> out[b, D:].  Returns the `stores_behind_copy` of the next wait: the sample's counted stores (DS of
// fwd_store_dense + the T here), or 0 = wait for everything.
template <int D>
__device__ __forceinline__ int fwd_store_pairs_counted(float* orow, const float* zs, const FwdWave<D>& w) {
  const int lane = w.lane, P = w.P;
  if (w.vec_out) {
#pragma unroll
    for (int t = 0; t < kMaxPairStores4; ++t) {
      const int q = lane + t * kWave;
      if (q < w.P4 / 4) st4(orow + D + 4 * q, *reinterpret_cast<const float4*>(zs + 4 * q));
    }
    return 0;  // compiler-generated stores: their number is not ours to count, wait for everything
  }
  const int T = wave_chunks(P);  // pair stores per sample
  float zv[kMaxPairStores];
#pragma unroll
  for (int t = 0; t < kMaxPairStores; ++t)
    if (t < T) zv[t] = zs[min(lane + t * kWave, P - 1)];
#pragma unroll
  for (int t = 0; t < kMaxPairStores; ++t)
    if (t < T) vm_store_dword(orow + D + min(lane + t * kWave, P - 1), zv[t]);
  return FwdImage<D>::DS + T;
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
  using Image = FwdImage<D>;
  constexpr int NS = D / 16;
  constexpr int PR = Image::PR;
  constexpr int RPI = Image::RPI;
  constexpr int MAXI = kFwdMaxRows / RPI;  // copy instructions for 32 rows
  const FwdWave<D> w(F, out, out_stride);
  const int lane = w.lane;
  const int R = w.R;
  const int NI = Image::copies(R);
  float* xs = smem + w.wave * Image::floats(R);
  float* zs = xs + Image::zs_offset(R);
  w.zero_pad(zs);
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
  int stores_behind_copy = 0;
  int b = w.first_sample();
  if (b < B) issue_copy(b);
  for (; b < B; b += w.stride_b) {
    // the copy of sample b has landed once everything but the stores issued after it has retired (an LDS-DMA counts
    // on the VM counter like a load; operations retire in issue order)
    vm_wait_all_but(stores_behind_copy);
    wave_lds_fence();
    FwdRows<NS> x;
    float4 dpass;
    float dscal[Image::DS];
    fwd_read_fragments(xs, w, x);
    fwd_read_dense(xs, w, dpass, dscal);
    // every read of the image has returned before the next copy may overwrite it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wave_lds_fence();
    if (b + w.stride_b < B) issue_copy(b + w.stride_b);
    f32x4 acc00, acc01, acc11;
    fwd_contract<NS>(x, acc00, acc01, acc11);
    float* orow = out + static_cast<int64_t>(b) * out_stride;
    fwd_store_dense(orow, w, dpass, dscal);
    fwd_stage_pairs(zs, w, acc00, acc01, acc11);
    wave_lds_fence();
    stores_behind_copy = fwd_store_pairs_counted(orow, zs, w);
    wave_lds_fence();  // zs is rewritten by the next sample
  }
}

// ---- backward: what the two kernels share ------------------------------------------------------------------------------------
// The LDS tile of one wave, host and device: X (later dX) with padded rows, then G + G^T.
template <int NT>  // NT = D / 16 column tiles
struct BwdTile {
  static constexpr int D = NT * 16;
  static constexpr int XS = D + 16;            // B-operand reads (16k + 16n + c) % 32: conflict-free over a half-wave
  static constexpr int GS = 34;                // A-operand reads (2*row + k) % 32: conflict-free
  static constexpr int XROWS = kBwdMaxRows;    // K steps cover rows 0..27
  static constexpr int GROWS = 32;             // both 16-row tiles of the A operand
  static constexpr int LOG_V = XLoader<D>::LOG_V;
  static constexpr int MAXV = wave_chunks(XROWS * D / 4);        // float4s of X per lane
  static constexpr int MAXP = wave_chunks(pair_count(XROWS));    // pairs per lane: 6
  static constexpr int kFloats = XROWS * XS + GROWS * GS;
  static_assert(XROWS % 4 == 0 && XROWS <= GROWS, "whole K steps of 4 rows inside the two MFMA tiles");
};

template <int NT>
struct BwdWave {
  const int lane, wave, R, P, r16, kq, nvec, ksteps, stride_b;
  __device__ __forceinline__ explicit BwdWave(int F)
      : lane(threadIdx.x & 63), wave(threadIdx.x >> 6), R(F + 1), P(pair_count(R)), r16(lane & 15), kq(lane >> 4),
        nvec(R * (NT * 4)), ksteps((R + 3) / 4), stride_b(gridDim.x * 4) {}
  __device__ __forceinline__ int first_sample() const { return blockIdx.x * 4 + wave; }
};

// rows R..27 of X and the whole of G start as zeros; per sample only defined entries are rewritten
template <int NT>
__device__ __forceinline__ void bwd_zero_tile(float* xs, float* gs, int lane) {
  using T = BwdTile<NT>;
  for (int e = lane; e < T::XROWS * T::XS; e += kWave) xs[e] = 0.f;
  for (int e = lane; e < T::GROWS * T::GS; e += kWave) gs[e] = 0.f;
}

// this lane's pairs (i, j) of the strict upper triangle: p = lane + 64*t
template <int NT>
__device__ __forceinline__ void bwd_pair_table(const BwdWave<NT>& w, int (&pij)[BwdTile<NT>::MAXP]) {
  const int R = w.R;
#pragma unroll
  for (int t = 0; t < BwdTile<NT>::MAXP; ++t) {
    const int p = w.lane + t * kWave;
    int i = 0, j = 1;
    if (p < w.P) {
      i = triu_row(p, R);
      j = i + 1 + (p - i * (2 * R - i - 1) / 2);
    }
    pij[t] = (i << 8) | j;
  }
}

// d(out)[b, D + p] of this lane's pairs
template <int NT>
__device__ __forceinline__ void bwd_load_pair_grads(const BwdWave<NT>& w, const float* grad_out, int b, int64_t grad_stride,
                                                    float (&gpre)[BwdTile<NT>::MAXP]) {
#pragma unroll
  for (int t = 0; t < BwdTile<NT>::MAXP; ++t) {
    const int p = w.lane + t * kWave;
    gpre[t] = p < w.P ? grad_out[static_cast<int64_t>(b) * grad_stride + BwdTile<NT>::D + p] : 0.f;
  }
}

// d(out)[b, :D] slice this lane adds to row 0
template <int NT>
__device__ __forceinline__ float4 bwd_load_gdense(const BwdWave<NT>& w, const float* grad_out, int b, int64_t grad_stride) {
  const int lane = w.lane;
  const float* grow = grad_out + static_cast<int64_t>(b) * grad_stride;
  float4 gdense = make_float4(0.f, 0.f, 0.f, 0.f);
  if (lane < BwdTile<NT>::D / 4) {
    if (((grad_stride & 3) | (reinterpret_cast<uintptr_t>(grad_out) & 15)) == 0) {
      gdense = ld4(grow + lane * 4);
    } else {
      gdense.x = grow[lane * 4 + 0];
      gdense.y = grow[lane * 4 + 1];
      gdense.z = grow[lane * 4 + 2];
      gdense.w = grow[lane * 4 + 3];
    }
  }
  return gdense;
}

// X and G + G^T of the sample in registers -> the tile
template <int NT>
__device__ __forceinline__ void bwd_stage(float* xs, float* gs, const BwdWave<NT>& w, const float4 (&pre)[BwdTile<NT>::MAXV],
                                          const float (&gpre)[BwdTile<NT>::MAXP], const int (&pij)[BwdTile<NT>::MAXP]) {
  using T = BwdTile<NT>;
#pragma unroll
  for (int i = 0; i < T::MAXV; ++i) {
    const int v = w.lane + i * kWave;
    if (v < w.nvec) st4(xs + (v >> T::LOG_V) * T::XS + (v & ((1 << T::LOG_V) - 1)) * 4, pre[i]);
  }
#pragma unroll
  for (int t = 0; t < T::MAXP; ++t) {
    if (w.lane + t * kWave < w.P) {
      const int i = pij[t] >> 8, j = pij[t] & 255;
      gs[i * T::GS + j] = gpre[t];
      gs[j * T::GS + i] = gpre[t];
    }
  }
}

// dX = (G + G^T) X: 2 x NT tiles, K = R in steps of 4 rows
template <int NT>
__device__ __forceinline__ void bwd_contract(const float* xs, const float* gs, const BwdWave<NT>& w, f32x4 (&acc)[2][NT]) {
  using T = BwdTile<NT>;
  const int r16 = w.r16, kq = w.kq;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ks = 0; ks < w.ksteps; ++ks) {
    const int k = ks * 4 + kq;
    const float a0 = gs[r16 * T::GS + k];
    const float a1 = gs[(16 + r16) * T::GS + k];
    const float* xrow = xs + k * T::XS + r16;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const float bn = xrow[16 * n];
      acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bn, acc[0][n], 0, 0, 0);
      acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bn, acc[1][n], 0, 0, 0);
    }
  }
}

// The tile's rows -> grad_dense (row 0, plus gdense) and grad_sparse: the plain store loop of the gather kernel.  Its form is
// measured, not chosen: with `gdense` by value and __restrict__ outputs — what the loop has when it is spelled inside a kernel —
// interaction_gather_bwd_kernel<8 / 4> are 5 ... 8 % slower (348 -> 366, 220 -> 234 us), while interaction_bwd_kernel<8> is 3 %
// slower with THIS form (372 -> 385 us) and therefore spells the loop itself.
template <int NT>
__device__ __forceinline__ void bwd_store(const float* xs, const BwdWave<NT>& w, const float4& gdense, float* grad_dense,
                                          float* grad_sparse, int b, int F) {
  using T = BwdTile<NT>;
#pragma unroll
  for (int i = 0; i < T::MAXV; ++i) {
    const int v = w.lane + i * kWave;
    if (v < w.nvec) {
      const int r = v >> T::LOG_V;
      const int c = (v & ((1 << T::LOG_V) - 1)) * 4;
      float4 x = ld4(xs + r * T::XS + c);
      if (r == 0) {  // v == lane < D/4 here
        x.x += gdense.x;
        x.y += gdense.y;
        x.z += gdense.z;
        x.w += gdense.w;
        st4(grad_dense + static_cast<int64_t>(b) * T::D + c, x);
      } else {
        st4(grad_sparse + (static_cast<int64_t>(b) * F + (r - 1)) * T::D + c, x);
      }
    }
  }
}

// X of sample b from the pooled buffer.  (A function, not a lambda of the kernel: from a lambda the compiler no longer hoists the
// row and column part of the fourteen addresses out of the sample loop and spends a 64-bit multiply-add per load instead.)
template <int NT>
__device__ __forceinline__ void bwd_load_rows(const BwdWave<NT>& w, const float* dense, const float* sparse, int b, int F,
                                              float4 (&pre)[BwdTile<NT>::MAXV]) {
#pragma unroll
  for (int i = 0; i < BwdTile<NT>::MAXV; ++i) {
    const int v = w.lane + i * kWave;
    if (v < w.nvec) pre[i] = ld4(XLoader<BwdTile<NT>::D>::src(dense, sparse, b, F, v));
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
  using T = BwdTile<NT>;
  const BwdWave<NT> w(F);
  float* xs = smem + w.wave * T::kFloats;
  float* gs = xs + T::XROWS * T::XS;
  bwd_zero_tile<NT>(xs, gs, w.lane);
  int pij[T::MAXP];
  bwd_pair_table(w, pij);
  wave_lds_fence();

  float4 pre[T::MAXV];
  float gpre[T::MAXP];
  int b = w.first_sample();
  if (b < B) {
    bwd_load_rows(w, dense, sparse, b, F, pre);
    bwd_load_pair_grads(w, grad_out, b, grad_stride, gpre);
  }
  for (; b < B; b += w.stride_b) {
    bwd_stage(xs, gs, w, pre, gpre, pij);
    const float4 gdense = bwd_load_gdense(w, grad_out, b, grad_stride);
    const int nb = b + w.stride_b;
    if (nb < B) {
      bwd_load_rows(w, dense, sparse, nb, F, pre);
      bwd_load_pair_grads(w, grad_out, nb, grad_stride, gpre);
    }
    wave_lds_fence();
    f32x4 acc[2][NT];
    bwd_contract(xs, gs, w, acc);
    wave_lds_fence();  // every lane is done reading X before it is overwritten with dX
    // dX over X in the tile.  Spelled in both kernels: as a shared helper it cost interaction_bwd_kernel<2> two VGPRs (95 -> 97)
    // and with them the fifth wave per SIMD of the compiler's report.
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = 16 * m + 4 * w.kq + q;
          if (row < w.R) xs[row * T::XS + 16 * n + w.r16] = acc[m][n][q];
        }
    wave_lds_fence();
    // bwd_store, spelled here: see there for what the shared form costs this kernel
#pragma unroll
    for (int i = 0; i < T::MAXV; ++i) {
      const int v = w.lane + i * kWave;
      if (v < w.nvec) {
        const int r = v >> T::LOG_V;
        const int c = (v & ((1 << T::LOG_V) - 1)) * 4;
        float4 x = ld4(xs + r * T::XS + c);
        if (r == 0) {  // v == lane < D/4 here
          x.x += gdense.x;
          x.y += gdense.y;
          x.z += gdense.z;
          x.w += gdense.w;
          st4(grad_dense + static_cast<int64_t>(b) * T::D + c, x);
        } else {
          st4(grad_sparse + (static_cast<int64_t>(b) * F + (r - 1)) * T::D + c, x);
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
// images and store paths are the shared helpers above, so the results are bit-identical to the lookup + interaction pair.
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
  using Image = FwdImage<D, kIdSlotFloats>;
  constexpr int NS = D / 16;
  constexpr int PR = Image::PR;
  constexpr int RPI = Image::RPI;
  const FwdWave<D> w(F, out, out_stride);
  const int lane = w.lane;
  const int R = w.R;
  const int NI = Image::copies(R);
  float* xs = smem + w.wave * Image::floats(R);
  float* zs = xs + Image::zs_offset(R);
  float* ids = xs + Image::ids_offset(R);
  w.zero_pad(zs);
  const int stride_b = w.stride_b;
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
  int stores_behind_copy = 0;
  int b = w.first_sample();
  if (b < B) {
    issue_ids(b);
    vm_wait_all_but<0>();
    wave_lds_fence();
    const int64_t id = read_id();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wave_lds_fence();
    issue_copy(b, gather_row_address<D>(gl, id, zero_row, nbad));
    if (b + stride_b < B) issue_ids(b + stride_b);
  }
  for (; b < B; b += stride_b) {
    // the copy of sample b and the ids of the next sample have landed once everything but the stores issued after them
    // has retired
    vm_wait_all_but(stores_behind_copy);
    wave_lds_fence();
    FwdRows<NS> x;
    float4 dpass;
    float dscal[Image::DS];
    fwd_read_fragments(xs, w, x);
    fwd_read_dense(xs, w, dpass, dscal);
    const int64_t next_id = read_id();  // of sample b + stride_b (stale when there is none: not used then)
    // every read of the image and of the id slot has returned before the next copies may overwrite them
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wave_lds_fence();
    if (b + stride_b < B) {
      issue_copy(b + stride_b, gather_row_address<D>(gl, next_id, zero_row, nbad));
      if (b + 2 * stride_b < B) issue_ids(b + 2 * stride_b);
    }
    f32x4 acc00, acc01, acc11;
    fwd_contract<NS>(x, acc00, acc01, acc11);
    float* orow = out + static_cast<int64_t>(b) * out_stride;
    fwd_store_dense(orow, w, dpass, dscal);
    fwd_stage_pairs(zs, w, acc00, acc01, acc11);
    wave_lds_fence();
    stores_behind_copy = fwd_store_pairs_counted(orow, zs, w);
    wave_lds_fence();  // zs is rewritten by the next sample
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
  using T = BwdTile<NT>;
  constexpr int D = T::D;
  constexpr int XS = T::XS;
  constexpr int LOG_V = T::LOG_V;
  constexpr int MAXV = T::MAXV;
  const BwdWave<NT> w(F);
  const int lane = w.lane;
  const int R = w.R;
  const int stride_b = w.stride_b;
  float* xs = smem + w.wave * T::kFloats;
  float* gs = xs + T::XROWS * XS;
  bwd_zero_tile<NT>(xs, gs, lane);
  int pij[T::MAXP];
  bwd_pair_table(w, pij);
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
  float gpre[T::MAXP];
  // X of sample s: row 0 from dense, row r >= 1 from the address lane r-1 holds (0 = a zero row)
  auto load_x = [&](int s, uint64_t row_addr) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int v = lane + i * kWave;
      const int r = min(v >> LOG_V, R - 1);
      const int c = (v & ((1 << LOG_V) - 1)) * 4;
      const uint64_t src = shflu64(row_addr, max(r - 1, 0));
      if (v < w.nvec) {
        if (r == 0)
          pre[i] = ld4(dense + static_cast<int64_t>(s) * D + c);
        else
          pre[i] = src != 0 ? ld4(reinterpret_cast<const float*>(src) + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  int b = w.first_sample();
  int64_t next_id = 0;  // this lane's id of the sample AFTER the one whose rows are in flight
  if (b < B) {
    const uint64_t row_addr = gather_row_address<D>(gl, my_ids[b], 0, nbad);
    if constexpr (SGD) once_in_flight = publish_once(row_addr, my_single(b), 0);
    load_x(b, row_addr);
    if (b + stride_b < B) {
      next_id = my_ids[b + stride_b];
      if constexpr (SGD) next_single = my_single(b + stride_b);
    }
    bwd_load_pair_grads(w, grad_out, b, grad_stride, gpre);
  }
  for (; b < B; b += stride_b) {
    // SGD: sample b's mask, kept across the prefetch of the next sample; bit r = row r is once (row 0, the dense row, never)
    const uint32_t once_b = once_in_flight << 1;
    bwd_stage(xs, gs, w, pre, gpre, pij);
    const float4 gdense = bwd_load_gdense(w, grad_out, b, grad_stride);
    const int nb = b + stride_b;
    if (nb < B) {
      const uint64_t row_addr = gather_row_address<D>(gl, next_id, 0, nbad);
      if constexpr (SGD) once_in_flight = publish_once(row_addr, next_single, slot ^ 1);
      load_x(nb, row_addr);
      if (nb + stride_b < B) {
        next_id = my_ids[nb + stride_b];
        if constexpr (SGD) next_single = my_single(nb + stride_b);
      }
      bwd_load_pair_grads(w, grad_out, nb, grad_stride, gpre);
    }
    wave_lds_fence();
    f32x4 acc[2][NT];
    bwd_contract(xs, gs, w, acc);
    wave_lds_fence();  // every lane is done reading X before it is overwritten with dX
    if constexpr (SGD) {
      // A flagged row becomes the NEW table row: w - lr * dX with the operands and roundings of bwd_update_kernel +
      // apply_row (the gradient is first added to the +0 accumulator, then one fmaf), w read from the very LDS word
      // that is overwritten.  One instruction stream for both kinds of row (a select, no divergent copies of the
      // stores): the old words of a row are read whether it is once or not.
      const int r16 = w.r16, kq = w.kq;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = 16 * m + 4 * kq + q;
          if (row < R) {
            float* xw = xs + row * XS + r16;
            const bool once = ((once_b >> row) & 1u) != 0;
            float wold[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) wold[n] = xw[16 * n];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
              const float g = acc[m][n][q];
              xw[16 * n] = once ? fmaf(-lr, fmaf(1.f, g, 0.f), wold[n]) : g;
            }
          }
        }
    } else {
      // the plain write-back of interaction_bwd_kernel (see there)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int row = 16 * m + 4 * w.kq + q;
            if (row < R) xs[row * XS + 16 * n + w.r16] = acc[m][n][q];
          }
    }
    wave_lds_fence();
    if constexpr (SGD) {
      // The plain store loop (bwd_store) with its addresses spelled as ONE per-lane base plus a compile-time offset per
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
      bwd_store(xs, w, gdense, grad_dense, grad_sparse, b, F);
    }
    wave_lds_fence();
    slot ^= 1;
  }
  report_bad_ids(nbad, bounds_errors);
}

}  // namespace tbe

using namespace tbe;

// ---- host side -----------------------------------------------------------------------------------------------------------------
constexpr size_t kCuLdsBytes = 160 * 1024;  // gfx950
constexpr size_t workgroup_lds_bytes(int floats_per_wave) { return 4 * static_cast<size_t>(floats_per_wave) * sizeof(float); }
template <typename Image>
constexpr bool image_covers(int max_rows) {  // the image of max_rows rows is the largest one
  for (int R = 2; R <= max_rows; ++R)
    if (Image::floats(R) > Image::floats(max_rows)) return false;
  return true;
}
// What makes the F limits of the entries safe: the per-lane arrays and the reservations are those of the row maxima.
static_assert(kBwdMaxRows <= kFwdMaxRows && kFwdMaxRows == 32, "R rows fit the two 16-row MFMA tiles");
static_assert(BwdTile<8>::MAXP * kWave >= pair_count(kBwdMaxRows), "pij / gpre hold every pair of kBwdMaxRows rows");
static_assert(2 * workgroup_lds_bytes(BwdTile<8>::kFloats) <= kCuLdsBytes, "two backward workgroups per CU at D = 128");
static_assert(image_covers<FwdImage<128>>(kFwdMaxRows) && image_covers<FwdImage<64>>(kFwdMaxRows) &&
                  image_covers<FwdImage<128, kIdSlotFloats>>(kBwdMaxRows) && image_covers<FwdImage<64, kIdSlotFloats>>(kBwdMaxRows),
              "the reservation of the row maximum covers every launch");
static_assert(2 * workgroup_lds_bytes(FwdImage<128>::floats(kFwdMaxRows)) <= kCuLdsBytes, "two forward workgroups per CU");

// persistent-style: `wgs_per_cu` workgroups per CU, each wave strides over samples
static dim3 interaction_grid(int B, int wgs_per_cu) {
  const int64_t want = (static_cast<int64_t>(B) + 3) / 4;
  return dim3(static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(want, 256 * wgs_per_cu))));
}

// Lets `Kernel` use up to `bytes` of dynamic LDS; asked of the runtime once per kernel.
template <auto Kernel>
static int reserve_lds_once(const char* what, size_t bytes) {
  static bool reserved = false;
  if (reserved) return TBE_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(bytes)) != hipSuccess) {
    set_error("%s: cannot reserve LDS", what);
    return TBE_ERR_LAUNCH;
  }
  reserved = true;
  return TBE_OK;
}

// One launch: 256 threads, `floats` of LDS per wave, of at most `max_floats` (0: what every kernel may use without asking).
template <auto Kernel, typename... Args>
static int launch_interaction(const char* what, int B, int wgs_per_cu, int floats, int max_floats, void* stream, Args... args) {
  if (max_floats != 0) {
    if (const int rc = reserve_lds_once<Kernel>(what, workgroup_lds_bytes(max_floats))) return rc;
  }
  hipLaunchKernelGGL(Kernel, interaction_grid(B, wgs_per_cu), dim3(256), workgroup_lds_bytes(floats),
                     static_cast<hipStream_t>(stream), args...);
  TBE_CHECK_LAUNCH(what);
  return TBE_OK;
}

extern "C" int tbe_dlrm_interaction_forward_f32(const float* dense, const float* sparse, int32_t B, int32_t F,
                                                int32_t D, float* out, int64_t out_row_stride, void* stream) {
  const char* what = "tbe_dlrm_interaction_forward_f32";
  TBE_REQUIRE(B >= 0 && F >= 1 && F <= kFwdMaxRows - 1, "%s: F=%d outside [1, %d]", what, F, kFwdMaxRows - 1);
  TBE_REQUIRE(out_row_stride >= D + (F + 1) * F / 2, "%s: out_row_stride %lld < D + F(F+1)/2", what, (long long)out_row_stride);
  TBE_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128 || D == 256, "%s: D=%d not in {16,32,64,128,256}", what, D);
  if (B == 0) return TBE_OK;
  TBE_REQUIRE(dense && sparse && out, "%s: null pointer", what);
  TBE_REQUIRE(all_aligned({dense, sparse}, 15), "%s: inputs must be 16-B aligned", what);
  const int R = F + 1;
  int rc = TBE_OK;
  dispatch_value<16, 32, 64, 128, 256>(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    if constexpr (DD == 64 || DD == 128) {  // LDS-DMA form: one [rows, D] image + the pair block per wave, 2 workgroups per CU
      using Image = FwdImage<DD>;
      rc = launch_interaction<interaction_fwd_glds_kernel<DD>>(what, B, 2, Image::floats(R), Image::floats(kFwdMaxRows), stream,
                                                               dense, sparse, out, B, F, out_row_stride);
    } else {  // register form: the pair block per wave, 4 workgroups per CU (2 at D = 256)
      rc = launch_interaction<interaction_fwd_kernel<DD>>(what, B, DD <= 128 ? 4 : 2, pad4(pair_count(R)), 0, stream, dense,
                                                          sparse, out, B, F, out_row_stride);
    }
  });
  return rc;
}

extern "C" int tbe_dlrm_interaction_backward_f32(const float* dense, const float* sparse, const float* grad_out,
                                                 int64_t grad_row_stride, int32_t B, int32_t F, int32_t D,
                                                 float* grad_dense, float* grad_sparse, void* stream) {
  const char* what = "tbe_dlrm_interaction_backward_f32";
  TBE_REQUIRE(B >= 0 && F >= 1 && F <= kBwdMaxRows - 1, "%s: F=%d outside [1, %d]", what, F, kBwdMaxRows - 1);
  TBE_REQUIRE(grad_row_stride >= D + (F + 1) * F / 2, "%s: grad_row_stride %lld < D + F(F+1)/2", what, (long long)grad_row_stride);
  TBE_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128, "%s: D=%d not in {16,32,64,128}", what, D);
  if (B == 0) return TBE_OK;
  TBE_REQUIRE(dense && sparse && grad_out && grad_dense && grad_sparse, "%s: null pointer", what);
  TBE_REQUIRE(all_aligned({dense, sparse, grad_dense, grad_sparse}, 15), "%s: tensors must be 16-B aligned", what);
  int rc = TBE_OK;
  dispatch_value<16, 32, 64, 128>(D, [&](auto d) {
    constexpr int NT = decltype(d)::value / 16;
    rc = launch_interaction<interaction_bwd_kernel<NT>>(what, B, 2, BwdTile<NT>::kFloats, BwdTile<NT>::kFloats, stream, dense,
                                                        sparse, grad_out, grad_dense, grad_sparse, B, F, grad_row_stride);
  });
  return rc;
}

// ---- pooling factor 1: lookup fused into the interaction (kernels above) ------------------------------------------
// The limits and pointers of a gather entry: none of `vec` (which move as float4; `vec_name` in the message), `other` and
// `indices` null, `vec` 16-B and `indices` 8-B aligned.
static int check_gather_args(const char* what, int32_t B, int32_t F, int32_t D, int64_t row_stride,
                             std::initializer_list<const void*> vec, const char* vec_name,
                             std::initializer_list<const void*> other, const int64_t* indices) {
  TBE_REQUIRE(B >= 0 && F >= 1 && F <= kBwdMaxRows - 1, "%s: F=%d outside [1, %d]", what, F, kBwdMaxRows - 1);
  TBE_REQUIRE(D == 64 || D == 128, "%s: D=%d not in {64,128}", what, D);
  TBE_REQUIRE(row_stride >= D + (F + 1) * F / 2, "%s: row stride %lld < D + F(F+1)/2", what, (long long)row_stride);
  const std::initializer_list<const void*> ids = {indices};
  for (const auto& ptrs : {vec, other, ids}) {
    for (const void* p : ptrs) TBE_REQUIRE(p != nullptr, "%s: null pointer", what);
  }
  TBE_REQUIRE(all_aligned(vec, 15) && all_aligned(ids, 7), "%s: %s must be 16-B aligned, indices 8-B aligned", what,
              vec_name);
  return TBE_OK;
}

extern "C" int tbe_dlrm_interaction_gather_forward_f32(const float* dense, const uint64_t* feat_weights,
                                                       const int64_t* feat_rows, const int64_t* feat_window,
                                                       const int64_t* indices, int32_t B, int32_t F, int32_t D, float* out,
                                                       int64_t out_row_stride, int32_t* bounds_errors, void* stream) {
  const char* what = "tbe_dlrm_interaction_gather_forward_f32";
  if (int rc = check_gather_args(what, B, F, D, out_row_stride, {dense}, "dense", {feat_weights, feat_rows, out}, indices)) return rc;
  if (B == 0) return TBE_OK;
  int rc = TBE_OK;
  dispatch_value<64, 128>(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    using Image = FwdImage<DD, kIdSlotFloats>;
    rc = launch_interaction<interaction_gather_fwd_kernel<DD>>(what, B, 2, Image::floats(F + 1), Image::floats(kBwdMaxRows), stream,
                                                               dense, feat_weights, feat_rows, feat_window, indices, out,
                                                               bounds_errors, B, F, out_row_stride);
  });
  return rc;
}

// Both gather backward entries; the plain one has no flags (`single` = nullptr is then not an error) and no learning rate.
// The SGD kernel uses the LDS of the plain kernel, to the byte: two workgroups fill a CU at D = 128.
template <bool SGD>
static int gather_backward(const char* what, const float* dense, const uint64_t* feat_weights, const int64_t* feat_rows,
                           const int64_t* feat_window, const int64_t* indices, const float* grad_out, int64_t grad_row_stride,
                           int32_t B, int32_t F, int32_t D, float* grad_dense, float* grad_sparse, int32_t* bounds_errors,
                           const uint8_t* single, float learning_rate, void* stream) {
  const void* flags = SGD ? static_cast<const void*>(single) : dense;
  if (int rc = check_gather_args(what, B, F, D, grad_row_stride, {dense, grad_dense, grad_sparse}, "tensors",
                                 {feat_weights, feat_rows, grad_out, flags}, indices))
    return rc;
  if (B == 0) return TBE_OK;
  int rc = TBE_OK;
  dispatch_value<64, 128>(D, [&](auto d) {
    constexpr int NT = decltype(d)::value / 16;
    rc = launch_interaction<interaction_gather_bwd_kernel<NT, SGD>>(
        what, B, 2, BwdTile<NT>::kFloats, BwdTile<NT>::kFloats, stream, dense, feat_weights, feat_rows, feat_window, indices,
        grad_out, grad_dense, grad_sparse, bounds_errors, B, F, grad_row_stride, single, learning_rate);
  });
  return rc;
}

extern "C" int tbe_dlrm_interaction_gather_backward_f32(const float* dense, const uint64_t* feat_weights,
                                                        const int64_t* feat_rows, const int64_t* feat_window,
                                                        const int64_t* indices, const float* grad_out,
                                                        int64_t grad_row_stride, int32_t B, int32_t F, int32_t D,
                                                        float* grad_dense, float* grad_sparse, int32_t* bounds_errors,
                                                        void* stream) {
  return gather_backward<false>("tbe_dlrm_interaction_gather_backward_f32", dense, feat_weights, feat_rows, feat_window, indices,
                                grad_out, grad_row_stride, B, F, D, grad_dense, grad_sparse, bounds_errors, nullptr, 0.f, stream);
}

extern "C" int tbe_dlrm_interaction_gather_backward_sgd_f32(const float* dense, const uint64_t* feat_weights,
                                                            const int64_t* feat_rows, const int64_t* feat_window,
                                                            const int64_t* indices, const float* grad_out,
                                                            int64_t grad_row_stride, int32_t B, int32_t F, int32_t D,
                                                            float* grad_dense, float* grad_sparse,
                                                            int32_t* bounds_errors, const uint8_t* single,
                                                            float learning_rate, void* stream) {
  return gather_backward<true>("tbe_dlrm_interaction_gather_backward_sgd_f32", dense, feat_weights, feat_rows, feat_window,
                               indices, grad_out, grad_row_stride, B, F, D, grad_dense, grad_sparse, bounds_errors, single,
                               learning_rate, stream);
}
