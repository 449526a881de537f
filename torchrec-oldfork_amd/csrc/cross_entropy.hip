// Cross-entropy over class indices with ignore_index on gfx950: the loss of BERT4Rec's trainer.
//
// Reference: examples/bert4rec/bert4rec_main.py:278-295 — nn.CrossEntropyLoss(ignore_index=0) over logits.view(B * T, V).
// As torch runs it, log_softmax writes a second [R, V] tensor and keeps it for the backward, which zero-fills a third one,
// scatters into it and reads both again; every row pays, although ~85 % of them carry ignore_index.  Here a row whose label
// is ignore_index is never read: its loss is 0 and its gradient row is written as zeros.
//
// Per valid row r with label t, float32, each product and add rounded on its own (the Makefile builds with -ffp-contract=off):
//   forward   one pass with a running (max, sum) pair:   m = max_v x[r, v],   ls = logf(sum_v expf(x[r, v] - m)),
//             stats[0, r] = m,   stats[1, r] = ls,   row_loss[r] = (m - x[r, t]) + ls
//   backward  grad[r, v] = (expf((x[r, v] - m) - ls) - [v == t]) * s
//             s = grad_out / n_valid (mean), grad_out (sum), grad_out[r] (none)
// The log-sum-exp m + ls is kept as its two terms: as one float32 it would lose ls below the ulp of m (logits of 1e4 have
// an ulp of 1e-3) and every probability of the row with it; (x - m) - ls is what torch's log_softmax computes.
// A (max, sum) pair never holds exp(-inf - -inf): the exponent's reference is 0 while the maximum is still -inf, so -inf
// entries are ordinary values (probability 0, gradient 0).  A row with NaN or +inf, or of -inf only, gives non-finite values.
// A label outside [0, V) that is not ignore_index forms no address: stats, row_loss and the gradient row are NaN.
//
// The rule of V (threads per row, TPR; a workgroup has 256 threads):
//   V <= 256          TPR = 16:  16 rows per workgroup
//   256 < V <= 4096   TPR = 64:  a wave per row, 4 rows per workgroup
//   4096 < V          TPR = 256: the workgroup per row
// A row is cut into groups of 4 consecutive columns; group g belongs to lane g % TPR, which takes its groups in ascending
// order, kCeBatch at a time: one (max, sum) fold per batch.  The lanes' pairs meet in a butterfly over the wave (the fold
// is commutative, so every lane holds the same bits) and, for TPR = 256, in wave order through LDS.  None of this depends on an
// address: a group moves as one 16-byte access where its address is 16-B aligned, as two 8-byte ones or as 4 + 8 + 4 bytes
// where it is not (V % 4 != 0 or an odd row stride shifts every row), and the last, partial group as scalars.  The result
// bits are therefore a function of (R, V) and the values only.  No atomics.
//
// The finishing launch (one workgroup) sums row_loss in an order fixed by R — thread t takes rows t, t + 256, ... in
// ascending order, then butterfly and wave order — and counts the rows whose label is not ignore_index as an exact int64.
// The backward reads that count from device memory: nothing here waits for the host.
#include <algorithm>
#include <cmath>

#include "rowreg.hpp"  // dispatch_value

namespace tbe {

constexpr int kCeThreads = 256;
constexpr int kCeWaves = kCeThreads / kWave;
constexpr int kCeBatch = 4;  // groups of 4 columns a lane loads before it folds them: 16 columns per fold

constexpr int kCeMean = 0, kCeSum = 1, kCeNone = 2;

__host__ __device__ constexpr int ce_tpr(int V) { return V <= 256 ? 16 : V <= 4096 ? 64 : 256; }

struct MaxSum {
  float m, s;  // sum_v expf(x_v - ref(m)) over the columns seen; ref(m) = m, or 0 while m is still -inf
};
__device__ __forceinline__ float ce_ref(const float m) { return m == -INFINITY ? 0.f : m; }

__device__ __forceinline__ MaxSum ce_combine(const MaxSum a, const MaxSum b) {  // commutative bit for bit
  MaxSum r;
  r.m = fmaxf(a.m, b.m);
  const float ref = ce_ref(r.m);
  r.s = a.s * expf(a.m - ref) + b.s * expf(b.m - ref);
  return r;
}

// Four consecutive floats at p (4-B aligned); a = address of the row's column 0 & 15, the same for every full group of a row.
__device__ __forceinline__ float4 ce_load4(const float* p, const unsigned a) {
  if (a == 0) return ld4(p);
  if (a == 8) {
    const float2 lo = *reinterpret_cast<const float2*>(p);
    const float2 hi = *reinterpret_cast<const float2*>(p + 2);
    return make_float4(lo.x, lo.y, hi.x, hi.y);
  }
  const float x0 = p[0];  // a == 4 or 12: p + 1 is 8-B aligned
  const float2 mid = *reinterpret_cast<const float2*>(p + 1);
  return make_float4(x0, mid.x, mid.y, p[3]);
}
__device__ __forceinline__ void ce_store4(float* p, const unsigned a, const float4 v) {
  if (a == 0) {
    st4(p, v);
  } else if (a == 8) {
    *reinterpret_cast<float2*>(p) = make_float2(v.x, v.y);
    *reinterpret_cast<float2*>(p + 2) = make_float2(v.z, v.w);
  } else {
    p[0] = v.x;
    *reinterpret_cast<float2*>(p + 1) = make_float2(v.y, v.z);
    p[3] = v.w;
  }
}
// The last group of a row when V % 4 != 0: n = 1 .. 3 columns, the others read as `pad` / are not written.
__device__ __forceinline__ float4 ce_load_tail(const float* p, const int n, const float pad) {
  return make_float4(p[0], n > 1 ? p[1] : pad, n > 2 ? p[2] : pad, pad);
}
__device__ __forceinline__ void ce_store_tail(float* p, const int n, const float4 v) {
  p[0] = v.x;
  if (n > 1) p[1] = v.y;
  if (n > 2) p[2] = v.z;
}

// The (max, sum) pair of row `row` [V] over this lane's groups, combined over the row's TPR lanes: the same in each of them.
// s_pair: [kCeWaves] (used by TPR = 256 only, where the whole workgroup must call this).
template <int TPR>
__device__ __forceinline__ MaxSum ce_row_max_sum(const float* __restrict__ row, const int V, const int lane, MaxSum* s_pair) {
  const unsigned a = static_cast<unsigned>(reinterpret_cast<uintptr_t>(row)) & 15u;
  const int full = V / 4, ngroups = (V + 3) / 4;
  MaxSum acc{-INFINITY, 0.f};
  for (int g0 = lane; g0 < ngroups; g0 += TPR * kCeBatch) {
    float4 v[kCeBatch];
#pragma unroll
    for (int q = 0; q < kCeBatch; ++q) {
      const int g = g0 + q * TPR;
      if (g < full)
        v[q] = ce_load4(row + 4 * g, a);
      else if (g < ngroups)
        v[q] = ce_load_tail(row + 4 * g, V - 4 * g, -INFINITY);
      else
        v[q] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);  // expf(-inf) = 0: adds nothing
    }
    float m = acc.m;
#pragma unroll
    for (int q = 0; q < kCeBatch; ++q) m = fmaxf(m, fmaxf(fmaxf(v[q].x, v[q].y), fmaxf(v[q].z, v[q].w)));
    const float ref = ce_ref(m);
    float s = acc.s * expf(acc.m - ref);
#pragma unroll
    for (int q = 0; q < kCeBatch; ++q)
      s += (expf(v[q].x - ref) + expf(v[q].y - ref)) + (expf(v[q].z - ref) + expf(v[q].w - ref));
    acc.m = m;
    acc.s = s;
  }
  constexpr int kSpan = TPR < kWave ? TPR : kWave;
#pragma unroll
  for (int o = kSpan / 2; o > 0; o >>= 1) {
    MaxSum other;
    other.m = __shfl_xor(acc.m, o, kWave);
    other.s = __shfl_xor(acc.s, o, kWave);
    acc = ce_combine(acc, other);
  }
  if constexpr (TPR > kWave) {
    if ((threadIdx.x & (kWave - 1)) == 0) s_pair[threadIdx.x / kWave] = acc;
    __syncthreads();
    acc = s_pair[0];
#pragma unroll
    for (int w = 1; w < kCeWaves; ++w) acc = ce_combine(acc, s_pair[w]);
  }
  return acc;
}

template <int TPR>
__global__ __launch_bounds__(kCeThreads) void cross_entropy_fwd_kernel(const float* __restrict__ x, const int64_t row_stride,
                                                                       const int64_t* __restrict__ target, const int64_t R,
                                                                       const int V, const int64_t ignore_index,
                                                                       float* __restrict__ stats, float* __restrict__ row_loss) {
  __shared__ MaxSum s_pair[kCeWaves];
  const int lane = threadIdx.x % TPR;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (kCeThreads / TPR) + threadIdx.x / TPR;
  if (r >= R) return;  // a whole row's lanes leave together (TPR = 256: the whole workgroup)
  const int64_t t = target[r];
  const bool ignored = t == ignore_index;
  if (ignored || static_cast<uint64_t>(t) >= static_cast<uint64_t>(V)) {  // the row is not read
    if (lane == 0) stats[r] = stats[R + r] = row_loss[r] = ignored ? 0.f : NAN;
    return;
  }
  const float* row = x + r * row_stride;
  const MaxSum p = ce_row_max_sum<TPR>(row, V, lane, s_pair);
  if (lane == 0) {
    const float ls = logf(p.s);
    stats[r] = p.m;
    stats[R + r] = ls;
    row_loss[r] = (p.m - row[t]) + ls;
  }
}

// One workgroup.  loss[0] = sum of row_loss (kCeSum) or that / n_valid (kCeMean); kCeNone: only the count.
__global__ __launch_bounds__(kCeThreads) void cross_entropy_finish_kernel(const float* __restrict__ row_loss,
                                                                          const int64_t* __restrict__ target, const int64_t R,
                                                                          const int64_t ignore_index, const int reduction,
                                                                          float* __restrict__ loss, int64_t* __restrict__ n_valid) {
  __shared__ float s_sum[kCeWaves];
  __shared__ unsigned long long s_cnt[kCeWaves];
  float acc = 0.f;
  unsigned long long cnt = 0ull;
  if (reduction == kCeNone) {
    for (int64_t r = threadIdx.x; r < R; r += kCeThreads) cnt += target[r] != ignore_index;
  } else {
#pragma unroll 8
    for (int64_t r = threadIdx.x; r < R; r += kCeThreads) {
      acc += row_loss[r];  // ignored rows hold 0
      cnt += target[r] != ignore_index;
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, kWave);
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(cnt), o, kWave);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(cnt >> 32), o, kWave);
    cnt += (static_cast<unsigned long long>(hi) << 32) | lo;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_sum[threadIdx.x / kWave] = acc;
    s_cnt[threadIdx.x / kWave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = s_sum[0];
    unsigned long long c = s_cnt[0];
#pragma unroll
    for (int w = 1; w < kCeWaves; ++w) {
      s += s_sum[w];
      c += s_cnt[w];
    }
    n_valid[0] = static_cast<int64_t>(c);
    if (reduction == kCeMean) loss[0] = s / static_cast<float>(c);  // 0 / 0 = NaN: no valid row
    if (reduction == kCeSum) loss[0] = s;
  }
}

template <int TPR>
__global__ __launch_bounds__(kCeThreads) void cross_entropy_bwd_kernel(const float* __restrict__ grad_out,
                                                                       const float* __restrict__ x, const int64_t row_stride,
                                                                       const int64_t* __restrict__ target,
                                                                       const float* __restrict__ stats,
                                                                       const int64_t* __restrict__ n_valid, const int64_t R,
                                                                       const int V, const int64_t ignore_index,
                                                                       const int reduction, float* __restrict__ grad,
                                                                       const int64_t grad_row_stride) {
  const int lane = threadIdx.x % TPR;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (kCeThreads / TPR) + threadIdx.x / TPR;
  if (r >= R) return;
  const int64_t t = target[r];
  float* grow = grad + r * grad_row_stride;
  const unsigned ga = static_cast<unsigned>(reinterpret_cast<uintptr_t>(grow)) & 15u;
  const int full = V / 4, ngroups = (V + 3) / 4;
  const bool ignored = t == ignore_index;
  if (ignored || static_cast<uint64_t>(t) >= static_cast<uint64_t>(V)) {  // the row is not read
    const float c = ignored ? 0.f : NAN;
    const float4 fill = make_float4(c, c, c, c);
    for (int g = lane; g < ngroups; g += TPR) {
      if (g < full)
        ce_store4(grow + 4 * g, ga, fill);
      else
        ce_store_tail(grow + 4 * g, V - 4 * g, fill);
    }
    return;
  }
  float s = reduction == kCeNone ? grad_out[r] : grad_out[0];
  if (reduction == kCeMean) s = s / static_cast<float>(n_valid[0]);
  const float m = stats[r], ls = stats[R + r];
  const int tcol = static_cast<int>(t);
  const float* row = x + r * row_stride;
  const unsigned a = static_cast<unsigned>(reinterpret_cast<uintptr_t>(row)) & 15u;
  for (int g0 = lane; g0 < ngroups; g0 += TPR * kCeBatch) {
    float4 v[kCeBatch];
#pragma unroll
    for (int q = 0; q < kCeBatch; ++q) {
      const int g = g0 + q * TPR;
      if (g < full)
        v[q] = ce_load4(row + 4 * g, a);
      else if (g < ngroups)
        v[q] = ce_load_tail(row + 4 * g, V - 4 * g, 0.f);
    }
#pragma unroll
    for (int q = 0; q < kCeBatch; ++q) {
      const int g = g0 + q * TPR;
      if (g >= ngroups) break;
      const int c = 4 * g;
      const float4 o = make_float4((expf((v[q].x - m) - ls) - (c == tcol ? 1.f : 0.f)) * s,
                                   (expf((v[q].y - m) - ls) - (c + 1 == tcol ? 1.f : 0.f)) * s,
                                   (expf((v[q].z - m) - ls) - (c + 2 == tcol ? 1.f : 0.f)) * s,
                                   (expf((v[q].w - m) - ls) - (c + 3 == tcol ? 1.f : 0.f)) * s);
      if (g < full)
        ce_store4(grow + c, ga, o);
      else
        ce_store_tail(grow + c, V - c, o);
    }
  }
}

struct CeGeom {
  int tpr;
  int64_t blocks;
};
// The checks shared by the two entries.
static int ce_limits(const char* name, int64_t R, int32_t V, int32_t reduction, CeGeom* g) {
  TBE_REQUIRE(R >= 0, "%s: R=%lld < 0", name, (long long)R);
  TBE_REQUIRE(V >= 1, "%s: V=%d, must be >= 1", name, V);
  TBE_REQUIRE(reduction >= kCeMean && reduction <= kCeNone, "%s: reduction=%d, must be 0 (mean), 1 (sum) or 2 (none)", name,
              reduction);
  g->tpr = ce_tpr(V);
  const int rows = kCeThreads / g->tpr;
  g->blocks = (R + rows - 1) / rows;
  TBE_REQUIRE(g->blocks <= INT32_MAX, "%s: R=%lld gives more than 2^31 - 1 row blocks of %d rows", name, (long long)R, rows);
  return TBE_OK;
}

}  // namespace tbe

using namespace tbe;

extern "C" size_t tbe_cross_entropy_workspace_bytes(int64_t R) {
  if (R < 0) return 0;
  return align_up(static_cast<size_t>(std::max<int64_t>(R, 1)) * sizeof(float), 256);
}

extern "C" int tbe_cross_entropy_forward_f32(const float* input, int64_t row_stride, const int64_t* target, int64_t R, int32_t V,
                                             int64_t ignore_index, int32_t reduction, float* stats, float* loss, int64_t* n_valid,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "tbe_cross_entropy_forward_f32";
  CeGeom g;
  const int rc = ce_limits(name, R, V, reduction, &g);
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(row_stride >= V, "%s: row_stride=%lld < V=%d", name, (long long)row_stride, V);
  TBE_REQUIRE(loss != nullptr && n_valid != nullptr, "%s: null pointer", name);
  TBE_REQUIRE(R == 0 || (input != nullptr && target != nullptr && stats != nullptr), "%s: null pointer", name);
  TBE_REQUIRE(all_aligned({input, stats, loss}, 3), "%s: input, stats and loss must be 4-B aligned", name);
  TBE_REQUIRE(all_aligned({target, n_valid}, 7), "%s: target and n_valid must be 8-B aligned", name);
  float* row_loss = loss;  // none: the row losses are the result
  if (reduction != kCeNone) {
    TBE_REQUIRE(workspace != nullptr, "%s: null pointer (workspace)", name);
    TBE_REQUIRE(all_aligned({workspace}, 15), "%s: workspace must be 16-B aligned", name);
    const size_t need = tbe_cross_entropy_workspace_bytes(R);
    TBE_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", name, workspace_bytes, need);
    row_loss = static_cast<float*>(workspace);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (R > 0) {
    dispatch_value<16, 64, 256>(g.tpr, [&](auto t) {
      hipLaunchKernelGGL(cross_entropy_fwd_kernel<decltype(t)::value>, dim3(static_cast<unsigned>(g.blocks)), dim3(kCeThreads), 0,
                         st, input, row_stride, target, R, V, ignore_index, stats, row_loss);
    });
    TBE_CHECK_LAUNCH(name);
  }
  hipLaunchKernelGGL(cross_entropy_finish_kernel, dim3(1), dim3(kCeThreads), 0, st, row_loss, target, R, ignore_index, reduction,
                     loss, n_valid);
  TBE_CHECK_LAUNCH("tbe_cross_entropy_forward_f32 (finish)");
  return TBE_OK;
}

extern "C" int tbe_cross_entropy_backward_f32(const float* grad_out, const float* input, int64_t row_stride, const int64_t* target,
                                              const float* stats, const int64_t* n_valid, int64_t R, int32_t V,
                                              int64_t ignore_index, int32_t reduction, float* grad_input,
                                              int64_t grad_row_stride, void* stream) {
  const char* name = "tbe_cross_entropy_backward_f32";
  CeGeom g;
  const int rc = ce_limits(name, R, V, reduction, &g);
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(row_stride >= V && grad_row_stride >= V, "%s: row_stride=%lld / grad_row_stride=%lld < V=%d", name,
              (long long)row_stride, (long long)grad_row_stride, V);
  if (R == 0) return TBE_OK;
  TBE_REQUIRE(grad_out != nullptr && input != nullptr && target != nullptr && stats != nullptr && n_valid != nullptr &&
                  grad_input != nullptr,
              "%s: null pointer", name);
  TBE_REQUIRE(all_aligned({grad_out, input, stats, grad_input}, 3), "%s: float tensors must be 4-B aligned", name);
  TBE_REQUIRE(all_aligned({target, n_valid}, 7), "%s: target and n_valid must be 8-B aligned", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  dispatch_value<16, 64, 256>(g.tpr, [&](auto t) {
    hipLaunchKernelGGL(cross_entropy_bwd_kernel<decltype(t)::value>, dim3(static_cast<unsigned>(g.blocks)), dim3(kCeThreads), 0, st,
                       grad_out, input, row_stride, target, stats, n_valid, R, V, ignore_index, reduction, grad_input,
                       grad_row_stride);
  });
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}
