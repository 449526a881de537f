// Kernels that keep a whole row of a [B, N] float32 matrix in the registers of the TPR threads that share it: the scheme of
// vector_cross_{fwd,bwd}_kernel (crossnet.hip) and swish_layernorm_{fwd,bwd}_kernel (swish_layernorm.hip), written once.
// Every order below depends on (B, N) only — no float atomics — and is pinned bit for bit by tests/_rowreg_order.py,
// tests/test_rowreg_order_gpu.py:
//   geometry     a workgroup of 256 threads = RP = 256 / TPR thread groups owns RPB rows (grid = row blocks); group `sub` takes
//                the rows sub, sub + RP, ...; thread `lane` of a group holds the float4 columns lane, lane + TPR, ... of its
//                row (kRowSlots of them, so N <= TPR * 16 <= kRowMaxN).  TPR and RPB are the kernel's own rule of N.
//   row sum      a thread adds its own elements from 0.0f in slot order (x, y, z, w inside a float4), then row_sum<TPR>:
//                xor butterfly inside the row's lanes of a wave, then (TPR = 256) ((w0 + w1) + w2) + w3 over the four waves.
//   column sum   a thread adds its column of the rows it takes from 0.0f; the row block's sum is that of sub = 0, 1, ...,
//                RP - 1, left to right (LDS), and goes to partial[row block][sums][N]; ONE second stage over sums * N columns
//                (colsum.hpp) finishes all the sums of a kernel.
#pragma once
#include <initializer_list>

#include "colsum.hpp"

namespace tbe {

constexpr int kRowSlots = 4;                    // float4 slots per thread
constexpr int kRowMaxN = 256 * kRowSlots * 4;  // the widest row a workgroup holds

// Sum of `v` over the G (a power of two <= 64) consecutive lanes of a wave that share a row, the same value in every one of
// them: the xor butterfly  v += shfl_xor(v, o),  o = G / 2 ... 1.
template <int G>
__device__ __forceinline__ float row_sum(float v) {
  static_assert(G >= 1 && G <= kWave && (G & (G - 1)) == 0, "a power-of-two group inside a wave");
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// The same over the TPR (<= 64, or 256 = the workgroup) threads that share a row: for 256 the butterfly of every wave, then the
// four wave sums in wave order through LDS.  Consecutive calls alternate `phase`, so one barrier per call is enough (a slot is
// rewritten only after the barrier of the call in between).
template <int TPR>
__device__ __forceinline__ float row_sum(float v, int& phase) {
  if constexpr (TPR <= kWave) {
    return row_sum<TPR>(v);
  } else {
    static_assert(TPR == 256, "a row is shared by a part of a wave or by the workgroup");
    __shared__ float red[2][4];
    v = row_sum<kWave>(v);
    if ((threadIdx.x & 63) == 0) red[phase][threadIdx.x >> 6] = v;
    __syncthreads();
    v = ((red[phase][0] + red[phase][1]) + red[phase][2]) + red[phase][3];
    phase ^= 1;
    return v;
  }
}

// The geometry of one thread (see above) and what goes through it: the row loop, slot addressing, row sums, the finish of the
// row block's column sums.
template <int TPR, int RPB>
struct RowTile {
  static constexpr int RP = 256 / TPR;  // rows in flight per workgroup
  const int N, lane, sub;
  const int64_t row0, row1;
  int phase = 0;

  __device__ __forceinline__ RowTile(int64_t B, int n)
      : N(n), lane(threadIdx.x % TPR), sub(threadIdx.x / TPR), row0(static_cast<int64_t>(blockIdx.x) * RPB),
        row1(min(B, row0 + RPB)) {}

  // first column of slot k, and whether the row has it
  __device__ __forceinline__ int col(int k) const { return (k * TPR + lane) * 4; }
  __device__ __forceinline__ bool has(int k) const { return col(k) < N; }

  // body(row) for the rows of this thread's group.  The trip count is the same for every thread that meets at a barrier:
  // TPR = 256 has sub = 0 everywhere, and a smaller TPR has no barrier inside the loop (`sum` is shuffles only).
  template <typename Body>
  __device__ __forceinline__ void for_rows(Body body) const {
    for (int64_t r = row0 + sub; r < row1; r += RP) body(r);
  }

  // body(k, first column) for the slots the row has.  A body that loads or stores captures the kernel's __restrict__ pointers
  // BY VALUE and only its arrays and sums by reference ([=, &x, &part]): through a reference the compiler no longer knows that
  // they do not alias, orders the loads otherwise and needs more registers (vector_cross_fwd_kernel<256>: 62 -> 78 VGPRs).
  template <typename Body>
  __device__ __forceinline__ void for_slots(Body body) const {
#pragma unroll
    for (int k = 0; k < kRowSlots; ++k) {
      if (has(k)) body(k, col(k));
    }
  }

  // the slots of the row that starts at `row`; columns beyond N hold zeros
  __device__ __forceinline__ void load(const float* __restrict__ row, float4 (&v)[kRowSlots]) const {
#pragma unroll
    for (int k = 0; k < kRowSlots; ++k) v[k] = has(k) ? ld4(row + col(k)) : make_float4(0.f, 0.f, 0.f, 0.f);
  }

  __device__ __forceinline__ void store(float* __restrict__ row, const float4 (&v)[kRowSlots]) const {
    for_slots([&](int k, int c) { st4(row + c, v[k]); });
  }

  // the sum of the threads' `v` over the row, in every thread of the row
  __device__ __forceinline__ float sum(float v) { return row_sum<TPR>(v, phase); }

  // The row block's column sums from the register sums of its threads: partial[row block][NS][N].  Called once, outside the
  // row loop, by every thread of the workgroup.  LDS: 4 KB unless TPR = 256, where every thread owns its columns alone.
  template <int NS>
  __device__ __forceinline__ void finish(const float4 (&sums)[NS][kRowSlots], float* __restrict__ partial) const {
    float* pb = partial + static_cast<int64_t>(blockIdx.x) * NS * N;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
      for (int k = 0; k < kRowSlots; ++k) {
        float4 v = sums[s][k];
        float* dst = pb + static_cast<int64_t>(s) * N + col(k);
        if constexpr (RP == 1) {
          if (has(k)) st4(dst, v);
        } else {
          __shared__ float4 fin[RP][TPR];
          if (k * TPR * 4 < N) {  // block-uniform: some lane of this slot holds a column
            __syncthreads();      // the previous round's reads of `fin` are done
            fin[sub][lane] = v;
            __syncthreads();
            if (sub == 0 && has(k)) {
              v = fin[0][lane];
#pragma unroll
              for (int j = 1; j < RP; ++j) add4(v, fin[j][lane]);
              st4(dst, v);
            }
          }
        }
      }
    }
  }
};

// ---- host side -----------------------------------------------------------------------------------------------------------
inline size_t rowreg_workspace_bytes(int64_t row_blocks, int sums, int N) {
  if (row_blocks <= 0 || sums <= 0 || N <= 0) return 256;
  return align_up(static_cast<size_t>(row_blocks) * sums * N * sizeof(float), 256);
}

// The limits of an entry; *row_blocks = its grid size.  `more` names the further limits the entry checks itself.
inline int rowreg_limits(const char* name, int64_t B, int N, int rows_per_block, int64_t* row_blocks, const char* more = "") {
  TBE_REQUIRE(B >= 0 && N > 0 && (N & 3) == 0, "%s: B=%lld must be >= 0 and N=%d a positive multiple of 4", name, (long long)B, N);
  TBE_REQUIRE(N <= kRowMaxN, "%s: N=%d beyond the limits N <= %d%s", name, N, kRowMaxN, more);
  *row_blocks = (B + rows_per_block - 1) / rows_per_block;
  TBE_REQUIRE(*row_blocks < (1ll << 31), "%s: B=%lld too large (more than 2^31 - 1 row blocks)", name, (long long)B);
  return TBE_OK;
}

// The column sums a backward entry keeps: out [sums, N] from partial[row blocks][sums][N] in `workspace`.
struct RowColSums {
  int sums;
  float* out;
  void* workspace;
  size_t workspace_bytes;
};

// What an entry does once its limits hold: the empty batch (nothing but zeros for the column sums), the pointers (`vec` and
// the workspace move as float4, `scalar` and the column sums as floats), the workspace size, launch(grid) with its check,
// the second stage.  `cs` = nullptr: an entry without column sums.
template <typename Launch>
int rowreg_run(const char* name, int64_t B, int N, int64_t row_blocks, std::initializer_list<const void*> vec,
               std::initializer_list<const void*> scalar, const RowColSums* cs, hipStream_t st, Launch launch) {
  if (cs != nullptr) {
    const int rc = check_pointers(name, {}, {cs->out});
    if (rc != TBE_OK) return rc;
  }
  if (B == 0) {
    if (cs == nullptr) return TBE_OK;
    return hipMemsetAsync(cs->out, 0, sizeof(float) * cs->sums * N, st) == hipSuccess ? TBE_OK : TBE_ERR_LAUNCH;
  }
  int rc = check_pointers(name, vec, scalar);
  if (rc == TBE_OK && cs != nullptr) rc = check_pointers(name, {cs->workspace});
  if (rc != TBE_OK) return rc;
  if (cs != nullptr) {
    const size_t need = rowreg_workspace_bytes(row_blocks, cs->sums, N);
    TBE_REQUIRE(cs->workspace_bytes >= need, "%s: workspace too small (%zu bytes, %zu needed)", name, cs->workspace_bytes, need);
  }
  launch(dim3(static_cast<unsigned>(row_blocks)));
  TBE_CHECK_LAUNCH(name);
  if (cs == nullptr) return TBE_OK;
  return launch_colsum_partials(name, static_cast<const float*>(cs->workspace), row_blocks, cs->sums * N, cs->out, st);
}

}  // namespace tbe
