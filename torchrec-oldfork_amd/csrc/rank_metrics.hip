// Recall@k and NDCG@k of a batch of candidate lists on gfx950, without a sort.
//
// Reference: examples/bert4rec/bert4rec_metrics.py:13-61 (recalls_and_ndcgs_for_ks) and the score gather in front of it,
// examples/bert4rec/bert4rec_main.py:235-248.  The reference sorts all C scores of every row to learn where a handful of
// positives rank, then loops over the batch on the host for the ideal DCG.  Here one workgroup takes a row:
//   stage   the row's C scores (read through `candidates` when given) become order-preserving uint32 keys in LDS, the
//           labels become one byte each.  A candidate outside [0, V) is never an address: its score is NaN and it is
//           counted; a label outside {0, 1} is never a hit: it is 0 and it is counted.
//   rank    for every positive j, one wave counts   pos_j = #{i : s_i > s_j} + #{i < j : s_i == s_j}
//           — its place in np.argsort(-s, kind="stable").  Ties go to the lower index, -0.0 ties with +0.0, a NaN ranks
//           behind every number and NaNs keep index order (every NaN has the smallest key).  Integer compares only.
//           The places are distinct, so pos_j < kmax sets byte pos_j of an occupancy row in LDS.
//   per k   hits = #{p < k : occupied},   Recall = hits / min(k, n_pos),
//           DCG = sum of w[p] over the occupied p < k,   IDCG = sum of w[p] over p < min(k, n_pos),   NDCG = DCG / IDCG.
//           Both sums are taken in float64: the table's floats lie in (2^-4, 1] and k <= 8192, so every partial sum is
//           exact and equals the sum in ascending p, whatever the order.  A row without a positive gives 0 / 0 = NaN.
// The finishing launch (one workgroup) takes the mean of each of the 2 nk per-row columns in float64, in an order fixed by
// B (row lane b % 16 takes its rows in ascending order, then the 16 lanes in order), rounds it to float32, and adds the
// rows' two bad-data counts as integers.  No atomics anywhere: two runs are bit-identical.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace tbe {

constexpr int kRankThreads = 256;
constexpr int kRankWaves = kRankThreads / kWave;
constexpr int kRankMaxC = 8192;
constexpr int kRankMaxKs = 8;
constexpr int kRankCountCols = 2 + kRankMaxKs;  // row_counts[b]: bad candidates, bad labels, hits of k_0 .. k_7
constexpr int kRankRowLanes = 16;               // finishing launch: 16 row lanes x 16 columns

struct RankKs {
  int32_t k[kRankMaxKs];
  int32_t nk;
};

// Descending score order = descending key order; every NaN -> 0, below -inf's key.
__device__ __forceinline__ uint32_t rank_key(const float x) {
  if (x != x) return 0u;
  uint32_t b = __float_as_uint(x);
  if (b == 0x80000000u) b = 0u;  // -0.0 == +0.0 as floats: one key
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// label -> 1 (positive), 0 (negative), 2 (neither)
__device__ __forceinline__ uint32_t rank_label_class(const float y) { return y == 1.0f ? 1u : (y == 0.0f ? 0u : 2u); }
__device__ __forceinline__ uint32_t rank_label_class(const int64_t y) { return y == 1 ? 1u : (y == 0 ? 0u : 2u); }
__device__ __forceinline__ uint32_t rank_label_class(const uint8_t y) { return y == 1 ? 1u : (y == 0 ? 0u : 2u); }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// Dynamic LDS: keys uint32 [C] | lab uint8 [C] | occ uint8 [C]  (6 C bytes, at most 48 KiB).
template <typename LabelT>
__global__ __launch_bounds__(kRankThreads) void rank_metrics_kernel(const float* __restrict__ scores, const int64_t score_stride,
                                                                    const int64_t* __restrict__ candidates, const int64_t V,
                                                                    const LabelT* __restrict__ labels, const int C,
                                                                    const RankKs ks, const float* __restrict__ weights,
                                                                    float* __restrict__ row_values,
                                                                    int32_t* __restrict__ row_counts) {
  extern __shared__ uint32_t s_mem[];
  __shared__ int s_cnt[kRankWaves][3];
  uint32_t* keys = s_mem;
  uint8_t* lab = reinterpret_cast<uint8_t*>(keys + C);
  uint8_t* occ = lab + C;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t b = blockIdx.x;
  const int kmax = ks.k[ks.nk - 1];  // <= C

  int npos = 0, nbadc = 0, nbadl = 0;
  for (int i = tid; i < C; i += kRankThreads) {
    int64_t col = i;
    bool ok = true;
    if (candidates != nullptr) {
      col = candidates[b * C + i];
      ok = static_cast<uint64_t>(col) < static_cast<uint64_t>(V);
    }
    const float s = ok ? scores[b * score_stride + col] : NAN;
    const uint32_t cls = rank_label_class(labels[b * C + i]);
    keys[i] = rank_key(s);
    lab[i] = cls == 1u;
    occ[i] = 0;
    npos += cls == 1u;
    nbadc += !ok;
    nbadl += cls == 2u;
  }
  npos = wave_sum(npos);
  nbadc = wave_sum(nbadc);
  nbadl = wave_sum(nbadl);
  if (lane == 0) {
    s_cnt[wave][0] = npos;
    s_cnt[wave][1] = nbadc;
    s_cnt[wave][2] = nbadl;
  }
  __syncthreads();
  npos = nbadc = nbadl = 0;
#pragma unroll
  for (int w = 0; w < kRankWaves; ++w) {
    npos += s_cnt[w][0];
    nbadc += s_cnt[w][1];
    nbadl += s_cnt[w][2];
  }

  // the positives, in index order, go round the waves
  int seen = 0;
  for (int j0 = 0; j0 < C; j0 += kWave) {  // wave-uniform
    const int jl = j0 + lane;
    unsigned long long mask = __ballot(jl < C && lab[jl] != 0);
    while (mask != 0ull) {
      const int j = j0 + __ffsll(static_cast<long long>(mask)) - 1;
      mask &= mask - 1ull;
      if ((seen++ & (kRankWaves - 1)) != wave) continue;
      const uint32_t kj = keys[j];
      int cnt = 0;
      for (int i = lane; i < C; i += kWave) {
        const uint32_t ki = keys[i];
        cnt += (ki > kj) || (ki == kj && i < j);
      }
      cnt = wave_sum(cnt);
      if (lane == 0 && cnt < kmax) occ[cnt] = 1;
    }
  }
  __syncthreads();

  for (int q = wave; q < ks.nk; q += kRankWaves) {  // a wave per k
    const int k = ks.k[q];
    const int lim = min(k, npos);
    int hits = 0;
    double dcg = 0.0, idcg = 0.0;
    for (int p = lane; p < k; p += kWave) {
      const double w = static_cast<double>(weights[p]);
      if (occ[p] != 0) {
        hits += 1;
        dcg += w;
      }
      if (p < lim) idcg += w;
    }
    hits = wave_sum(hits);
    dcg = wave_sum(dcg);
    idcg = wave_sum(idcg);
    if (lane == 0) {
      row_values[b * (2 * ks.nk) + q] = static_cast<float>(hits) / static_cast<float>(lim);  // 0 / 0 = NaN: no positive
      row_values[b * (2 * ks.nk) + ks.nk + q] = static_cast<float>(dcg / idcg);
      row_counts[b * kRankCountCols + 2 + q] = hits;
    }
  }
  if (tid == 0) {
    row_counts[b * kRankCountCols + 0] = nbadc;
    row_counts[b * kRankCountCols + 1] = nbadl;
  }
}

// One workgroup: metrics[c] = float32(mean_b row_values[b, c]), counts = {sum_b bad candidates, sum_b bad labels}.
__global__ __launch_bounds__(kRankThreads) void rank_metrics_finish_kernel(const float* __restrict__ row_values,
                                                                           const int32_t* __restrict__ row_counts,
                                                                           const int64_t B, const int ncol,
                                                                           float* __restrict__ metrics,
                                                                           int64_t* __restrict__ counts) {
  __shared__ double s_acc[kRankRowLanes][2 * kRankMaxKs];
  __shared__ long long s_bad[kRankWaves][2];
  const int tid = threadIdx.x, col = tid % (2 * kRankMaxKs), rl = tid / (2 * kRankMaxKs);
  double acc = 0.0;
  if (col < ncol) {
    for (int64_t b = rl; b < B; b += kRankRowLanes) acc += static_cast<double>(row_values[b * ncol + col]);
  }
  s_acc[rl][col] = acc;
  long long c0 = 0, c1 = 0;  // at most 8192 per row and 2^31 - 1 rows
  for (int64_t b = tid; b < B; b += kRankThreads) {
    c0 += row_counts[b * kRankCountCols + 0];
    c1 += row_counts[b * kRankCountCols + 1];
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    c0 += __shfl_xor(c0, o, kWave);
    c1 += __shfl_xor(c1, o, kWave);
  }
  if ((tid & (kWave - 1)) == 0) {
    s_bad[tid / kWave][0] = c0;
    s_bad[tid / kWave][1] = c1;
  }
  __syncthreads();
  if (tid < ncol) {
    double s = s_acc[0][tid];
#pragma unroll
    for (int l = 1; l < kRankRowLanes; ++l) s += s_acc[l][tid];
    metrics[tid] = static_cast<float>(s / static_cast<double>(B));  // B == 0: NaN, the mean of nothing
  }
  if (tid < 2) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kRankWaves; ++w) s += s_bad[w][tid];
    counts[tid] = s;
  }
}

struct RankWorkspace {
  float* row_values;    // [B, 2 nk]
  int32_t* row_counts;  // [B, kRankCountCols]
  size_t bytes;
};
inline RankWorkspace rank_carve(void* base, int64_t B, int nk) {
  Carver c(base);
  RankWorkspace w;
  const size_t rows = static_cast<size_t>(std::max<int64_t>(B, 1));
  w.row_values = c.take<float>(rows * 2 * nk);
  w.row_counts = c.take<int32_t>(rows * kRankCountCols);
  w.bytes = c.total();
  return w;
}

}  // namespace tbe

using namespace tbe;

extern "C" size_t tbe_rank_metrics_workspace_bytes(int64_t B, int32_t nk) {
  if (B < 0 || B > INT32_MAX || nk < 1 || nk > kRankMaxKs) return 0;
  return rank_carve(nullptr, B, nk).bytes;
}

extern "C" int tbe_rank_metrics_f32(const float* scores, int64_t score_row_stride, const int64_t* candidates, int64_t V,
                                    const void* labels, int32_t label_elem_size, int64_t B, int32_t C, const int32_t* ks,
                                    int32_t nk, const float* weights, float* metrics, int64_t* counts, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const char* name = "tbe_rank_metrics_f32";
  TBE_REQUIRE(B >= 0 && B <= INT32_MAX, "%s: B=%lld outside 0 .. 2^31 - 1", name, (long long)B);
  TBE_REQUIRE(C >= 1 && C <= kRankMaxC, "%s: C=%d outside 1 .. %d", name, C, kRankMaxC);
  TBE_REQUIRE(nk >= 1 && nk <= kRankMaxKs, "%s: nk=%d outside 1 .. %d", name, nk, kRankMaxKs);
  TBE_REQUIRE(ks != nullptr, "%s: null pointer (ks)", name);
  RankKs kk{};
  kk.nk = nk;
  for (int q = 0; q < nk; ++q) {
    TBE_REQUIRE(ks[q] >= 1 && ks[q] <= C, "%s: k=%d outside 1 .. C=%d", name, ks[q], C);
    TBE_REQUIRE(q == 0 || ks[q] > ks[q - 1], "%s: ks must be distinct and ascending", name);
    kk.k[q] = ks[q];
  }
  TBE_REQUIRE(label_elem_size == 1 || label_elem_size == 4 || label_elem_size == 8,
              "%s: labels must be uint8 / bool (1), float32 (4) or int64 (8)", name);
  const int64_t width = candidates != nullptr ? V : C;
  TBE_REQUIRE(candidates == nullptr || V >= 1, "%s: V=%lld < 1 with candidates", name, (long long)V);
  TBE_REQUIRE(score_row_stride >= width, "%s: score_row_stride=%lld < row width %lld", name, (long long)score_row_stride,
              (long long)width);
  TBE_REQUIRE(weights != nullptr && metrics != nullptr && counts != nullptr && workspace != nullptr &&
                  (B == 0 || (scores != nullptr && labels != nullptr)),
              "%s: null pointer", name);
  TBE_REQUIRE(all_aligned({scores, weights, metrics}, 3), "%s: scores, weights and metrics must be 4-B aligned", name);
  TBE_REQUIRE(all_aligned({candidates, counts}, 7), "%s: candidates and counts must be 8-B aligned", name);
  TBE_REQUIRE((reinterpret_cast<uintptr_t>(labels) & static_cast<uintptr_t>(label_elem_size - 1)) == 0,
              "%s: labels are not aligned to their element size", name);
  TBE_REQUIRE(all_aligned({workspace}, 255), "%s: workspace must be 256-B aligned", name);
  const RankWorkspace ws = rank_carve(workspace, B, nk);
  if (ws.bytes > workspace_bytes) {
    set_error("%s: workspace too small (%zu < %zu)", name, workspace_bytes, ws.bytes);
    return TBE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (B > 0) {
    const dim3 grid(static_cast<unsigned>(B)), block(kRankThreads);
    const size_t lds = static_cast<size_t>(C) * 6;
    if (label_elem_size == 8)
      hipLaunchKernelGGL(rank_metrics_kernel<int64_t>, grid, block, lds, st, scores, score_row_stride, candidates, V,
                         static_cast<const int64_t*>(labels), C, kk, weights, ws.row_values, ws.row_counts);
    else if (label_elem_size == 4)
      hipLaunchKernelGGL(rank_metrics_kernel<float>, grid, block, lds, st, scores, score_row_stride, candidates, V,
                         static_cast<const float*>(labels), C, kk, weights, ws.row_values, ws.row_counts);
    else
      hipLaunchKernelGGL(rank_metrics_kernel<uint8_t>, grid, block, lds, st, scores, score_row_stride, candidates, V,
                         static_cast<const uint8_t*>(labels), C, kk, weights, ws.row_values, ws.row_counts);
    TBE_CHECK_LAUNCH(name);
  }
  hipLaunchKernelGGL(rank_metrics_finish_kernel, dim3(1), dim3(kRankThreads), 0, st, ws.row_values, ws.row_counts, B, 2 * nk,
                     metrics, counts);
  TBE_CHECK_LAUNCH("tbe_rank_metrics_f32 (finish)");
  return TBE_OK;
}
