// Exact binary AUROC and thresholded accuracy counts over an evaluation set, in integers.
//
// What the reference computes with torchmetrics.AUROC / Accuracy in examples/dlrm/dlrm_main.py:252-265 (_evaluate).
// For predictions x_i and labels y_i in {0, 1} with P positives and N negatives
//   2U = sum over positives p of ( 2 * #{negatives with x < x_p} + #{negatives with x == x_p} ),  AUROC = 2U / (2 P N).
// Three steps on the stream, no float arithmetic anywhere (so two runs are bit-identical and the host can pin the result):
//   auroc_prepare_kernel : preds -> order-preserving uint32 keys (-0.0 canonicalised to +0.0 so that it ties with it; inf
//                          and denormals are ordinary values), labels -> payload 0 / 1, and the five plain counters
//                          (P, N, n_correct, n_nan, n_bad_label) in the same pass (block sums, then one integer atomic
//                          per counter and block: the final value does not depend on the order).
//   radix_sort_pairs     : ascending on the 32 key bits (radix_sort.hpp: 4 passes of 8 bits).
//   auroc_reduce_kernel  : 2U from the sorted pairs.  With Pc[i], Nc[i] the exclusive positive / negative counts and the
//                          tie groups (runs of equal keys) [b_j, b_{j+1}),
//                            2U = sum_j (Pc[b_{j+1}] - Pc[b_j]) * (Nc[b_j] + Nc[b_{j+1}]).
//                          A group is closed where the NEXT one starts (and at n), so an element only ever looks at its
//                          predecessor's key.  The counts at b_j travel through the scans as part of the state
//                          {p, n, flag, bp, bn}: positives / negatives of a span, whether a group starts inside it, and the
//                          counts in front of the LAST group start inside it;  A . B = {A.p + B.p, A.n + B.n,
//                          B.flag ? (1, A.p + B.bp, A.n + B.bn) : (A.flag, A.bp, A.bn)} is associative, so a group may
//                          start in one tile and end any number of tiles (or segments) later.
//                          Two launches of one kernel template: the first leaves one state per SEGMENT (a run of tiles
//                          owned by one workgroup, <= 1024 segments), the second folds the states of the segments in front
//                          of its own and then walks its tiles again, adding the closed groups' terms.  Block sums of the
//                          terms go to counts[0] with one 64-bit integer atomic per workgroup.
#include <algorithm>

#include "radix_sort.hpp"

namespace tbe {

constexpr int kAucThreads = 256;
constexpr int kAucWaves = kAucThreads / kWave;
constexpr int kAucPerThread = 8;                          // consecutive elements of one thread: two 16-B loads per array
constexpr int kAucTile = kAucThreads * kAucPerThread;     // 2048
constexpr int kAucMaxSegments = 1024;                     // 4 workgroups per CU
constexpr int kAucKeyBits = 32;
constexpr int kAucPrepMaxBlocks = 2048;

// counts[] of tbe_auroc_counts_f32: slot 0 = 2U (reduce kernel), 1 .. 5 = P, N, n_correct, n_nan, n_bad_label (prepare kernel)
constexpr int kCnt2U = 0;

__device__ __forceinline__ uint32_t auroc_key(float x) {
  uint32_t b = __float_as_uint(x);
  if (b == 0x80000000u) b = 0u;  // -0.0 == +0.0 as floats: one key
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// label -> 1 (positive), 0 (negative), 2 (neither)
__device__ __forceinline__ uint32_t label_class(float y) { return y == 1.0f ? 1u : (y == 0.0f ? 0u : 2u); }
__device__ __forceinline__ uint32_t label_class(int64_t y) { return y == 1 ? 1u : (y == 0 ? 0u : 2u); }

struct PrepCounts {
  uint32_t pos = 0, neg = 0, correct = 0, nan = 0, bad = 0;
};
// One sample: returns its key, sets its payload, counts it.  A label outside {0, 1} gets payload 0.
template <typename LabelT>
__device__ __forceinline__ uint32_t prep_one(float x, LabelT y, float threshold, uint32_t& payload, PrepCounts& c) {
  const uint32_t cls = label_class(y);
  payload = cls == 1u ? 1u : 0u;
  c.pos += cls == 1u;
  c.neg += cls == 0u;
  c.bad += cls == 2u;
  c.nan += x != x;
  c.correct += (x >= threshold) == (cls == 1u);
  return auroc_key(x);
}

template <typename LabelT>
__global__ __launch_bounds__(kAucThreads) void auroc_prepare_kernel(const float* __restrict__ preds,
                                                                    const LabelT* __restrict__ labels, int64_t n,
                                                                    float threshold, uint32_t* __restrict__ keys,
                                                                    uint32_t* __restrict__ vals,
                                                                    unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_cnt[kAucWaves][5];
  PrepCounts c;
  // 16-B loads need 16-B aligned inputs (keys / vals are carved 256-B aligned); otherwise every sample goes one by one
  const bool vec = ((reinterpret_cast<uintptr_t>(preds) | reinterpret_cast<uintptr_t>(labels)) & 15) == 0;
  const int64_t nvec = vec ? n / 4 : 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kAucThreads;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kAucThreads + threadIdx.x;
  for (int64_t i = first; i < nvec; i += stride) {
    const float4 x = *reinterpret_cast<const float4*>(preds + 4 * i);
    LabelT y[4];
    if constexpr (sizeof(LabelT) == 4) {
      *reinterpret_cast<float4*>(y) = *reinterpret_cast<const float4*>(labels + 4 * i);
    } else {
      *reinterpret_cast<longlong2*>(y) = *reinterpret_cast<const longlong2*>(labels + 4 * i);
      *reinterpret_cast<longlong2*>(y + 2) = *reinterpret_cast<const longlong2*>(labels + 4 * i + 2);
    }
    uint4 k, v;
    k.x = prep_one(x.x, y[0], threshold, v.x, c);
    k.y = prep_one(x.y, y[1], threshold, v.y, c);
    k.z = prep_one(x.z, y[2], threshold, v.z, c);
    k.w = prep_one(x.w, y[3], threshold, v.w, c);
    *reinterpret_cast<uint4*>(keys + 4 * i) = k;
    *reinterpret_cast<uint4*>(vals + 4 * i) = v;
  }
  for (int64_t i = nvec * 4 + first; i < n; i += stride) {
    uint32_t v;
    keys[i] = prep_one(preds[i], labels[i], threshold, v, c);
    vals[i] = v;
  }
  uint32_t r[5] = {c.pos, c.neg, c.correct, c.nan, c.bad};
#pragma unroll
  for (int q = 0; q < 5; ++q) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) r[q] += __shfl_xor(r[q], o, kWave);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 5; ++q) s_cnt[wave][q] = r[q];
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kAucWaves; ++w) s += s_cnt[w][threadIdx.x];
    // slot order of counts[]: P, N, n_correct, n_nan, n_bad_label = 1 .. 5
    if (s != 0u) atomicAdd(&counts[1 + threadIdx.x], static_cast<unsigned long long>(s));
  }
}

// The scan state of a span of sorted samples (header comment).  flag == 0 implies bp == bn == 0.
struct alignas(16) AucState {
  uint32_t p, n, bp, bn, flag, pad0, pad1, pad2;
};
__device__ __forceinline__ AucState auc_identity() { return AucState{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}; }
__device__ __forceinline__ AucState auc_combine(const AucState& a, const AucState& b) {  // a in front of b
  AucState r;
  r.p = a.p + b.p;
  r.n = a.n + b.n;
  r.bp = b.flag ? a.p + b.bp : a.bp;
  r.bn = b.flag ? a.n + b.bn : a.bn;
  r.flag = a.flag | b.flag;
  r.pad0 = r.pad1 = r.pad2 = 0u;
  return r;
}
__device__ __forceinline__ AucState auc_shfl_up(const AucState& s, int o) {
  AucState r;
  r.p = __shfl_up(s.p, o, kWave);
  r.n = __shfl_up(s.n, o, kWave);
  r.bp = __shfl_up(s.bp, o, kWave);
  r.bn = __shfl_up(s.bn, o, kWave);
  r.flag = __shfl_up(s.flag, o, kWave);
  r.pad0 = r.pad1 = r.pad2 = 0u;
  return r;
}
// one more sample behind the span `s`
__device__ __forceinline__ void auc_append(AucState& s, bool start, uint32_t pos, uint32_t neg) {
  if (start) {
    s.bp = s.p;
    s.bn = s.n;
    s.flag = 1u;
  }
  s.p += pos;
  s.n += neg;
}
// the term of the tie group that ends where the span `s` ends
__device__ __forceinline__ unsigned long long auc_group_term(const AucState& s) {
  return static_cast<unsigned long long>(s.p - s.bp) * static_cast<unsigned long long>(s.bn + s.n);
}

// Ordered scan over the workgroup's threads: `excl` = states of the threads in front of this one, `total` = all of them.
// s_wave: [kAucWaves] states.  Contains two workgroup barriers.
__device__ __forceinline__ void auc_block_scan(const AucState& mine, AucState* s_wave, AucState& excl, AucState& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  AucState inc = mine;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const AucState y = auc_shfl_up(inc, o);
    if (lane >= o) inc = auc_combine(y, inc);
  }
  AucState up = auc_shfl_up(inc, 1);
  if (lane == 0) up = auc_identity();
  __syncthreads();  // s_wave reuse
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  AucState front = auc_identity();
  total = auc_identity();
#pragma unroll
  for (int w = 0; w < kAucWaves; ++w) {
    const AucState t = s_wave[w];
    if (w < wave) front = auc_combine(front, t);
    total = auc_combine(total, t);
  }
  excl = auc_combine(front, up);
}

// kFinish == false: seg_state[b] = state of segment b.  kFinish == true: adds the segment's closed groups to two_u.
template <bool kFinish>
__global__ __launch_bounds__(kAucThreads) void auroc_reduce_kernel(const uint32_t* __restrict__ keys,
                                                                   const uint32_t* __restrict__ vals, int64_t n,
                                                                   int tiles_per_segment, AucState* __restrict__ seg_state,
                                                                   unsigned long long* __restrict__ two_u) {
  __shared__ AucState s_wave[kAucWaves];
  __shared__ uint32_t s_last[kAucThreads];
  __shared__ unsigned long long s_sum[kAucWaves];
  const int tid = threadIdx.x;
  const int64_t seg_begin = static_cast<int64_t>(blockIdx.x) * tiles_per_segment * kAucTile;
  const int64_t seg_end = min(n, seg_begin + static_cast<int64_t>(tiles_per_segment) * kAucTile);

  AucState carry = auc_identity();  // everything in front of the current tile
  if constexpr (kFinish) {
    // the segments in front of this one: <= 1024 states, four consecutive ones per thread
    AucState mine = auc_identity();
#pragma unroll
    for (int q = 0; q < kAucMaxSegments / kAucThreads; ++q) {
      const int j = tid * (kAucMaxSegments / kAucThreads) + q;
      if (j < static_cast<int>(blockIdx.x)) mine = auc_combine(mine, seg_state[j]);
    }
    AucState excl;
    auc_block_scan(mine, s_wave, excl, carry);
  }

  unsigned long long acc = 0ull;
  for (int64_t tile_begin = seg_begin; tile_begin < seg_end; tile_begin += kAucTile) {  // block-uniform
    const int64_t base = tile_begin + static_cast<int64_t>(tid) * kAucPerThread;
    uint32_t k[kAucPerThread], v[kAucPerThread];
    if (base + kAucPerThread <= n) {  // keys / vals are 256-B aligned and base is a multiple of 8
      *reinterpret_cast<uint4*>(k) = *reinterpret_cast<const uint4*>(keys + base);
      *reinterpret_cast<uint4*>(k + 4) = *reinterpret_cast<const uint4*>(keys + base + 4);
      *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(vals + base);
      *reinterpret_cast<uint4*>(v + 4) = *reinterpret_cast<const uint4*>(vals + base + 4);
    } else {
#pragma unroll
      for (int e = 0; e < kAucPerThread; ++e) {
        const bool valid = base + e < n;
        k[e] = valid ? keys[base + e] : 0u;
        v[e] = valid ? vals[base + e] : 0u;
      }
    }
    __syncthreads();  // s_last reuse
    s_last[tid] = k[kAucPerThread - 1];
    __syncthreads();
    // the key in front of this thread's first sample (unused for sample 0, which starts a group by definition)
    uint32_t prev = tid > 0 ? s_last[tid - 1] : (tile_begin > 0 ? keys[tile_begin - 1] : 0u);
    bool start[kAucPerThread];
    uint32_t pos[kAucPerThread], neg[kAucPerThread];
    AucState mine = auc_identity();
#pragma unroll
    for (int e = 0; e < kAucPerThread; ++e) {
      const bool valid = base + e < n;
      start[e] = valid && (base + e == 0 || k[e] != prev);
      pos[e] = (valid && v[e] == 1u) ? 1u : 0u;
      neg[e] = (valid && v[e] != 1u) ? 1u : 0u;
      prev = k[e];
      auc_append(mine, start[e], pos[e], neg[e]);
    }
    AucState excl, total;
    auc_block_scan(mine, s_wave, excl, total);
    if constexpr (kFinish) {
      AucState run = auc_combine(carry, excl);
#pragma unroll
      for (int e = 0; e < kAucPerThread; ++e) {
        if (start[e]) acc += auc_group_term(run);  // the group in front of this one is complete (nothing in front of sample 0: term 0)
        auc_append(run, start[e], pos[e], neg[e]);
      }
    }
    carry = auc_combine(carry, total);
  }

  if constexpr (!kFinish) {
    if (tid == 0) seg_state[blockIdx.x] = carry;
  } else {
    if (tid == 0 && seg_end == n) acc += auc_group_term(carry);  // the last group ends with the input
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      const uint32_t lo = __shfl_xor(static_cast<uint32_t>(acc), o, kWave);
      const uint32_t hi = __shfl_xor(static_cast<uint32_t>(acc >> 32), o, kWave);
      acc += (static_cast<unsigned long long>(hi) << 32) | lo;
    }
    if ((tid & 63) == 0) s_sum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      unsigned long long s = 0ull;
#pragma unroll
      for (int w = 0; w < kAucWaves; ++w) s += s_sum[w];
      if (s != 0ull) atomicAdd(two_u, s);
    }
  }
}

struct AucGeom {
  int64_t ntiles;
  int tiles_per_segment;
  int segments;
};
inline AucGeom auc_geom(int64_t n) {
  AucGeom g;
  g.ntiles = (n + kAucTile - 1) / kAucTile;
  g.tiles_per_segment = static_cast<int>(std::max<int64_t>(1, (g.ntiles + kAucMaxSegments - 1) / kAucMaxSegments));
  g.segments = static_cast<int>((g.ntiles + g.tiles_per_segment - 1) / g.tiles_per_segment);
  return g;
}

struct AucWorkspace {
  uint32_t *k0, *k1, *v0, *v1;
  AucState* seg_state;  // [kAucMaxSegments]
  void* sort;
  size_t bytes;
};
inline AucWorkspace auc_carve(void* base, int64_t n) {
  Carver c(base);
  AucWorkspace w;
  const size_t cnt = static_cast<size_t>(std::max<int64_t>(n, 1));
  w.k0 = c.take<uint32_t>(cnt);
  w.k1 = c.take<uint32_t>(cnt);
  w.v0 = c.take<uint32_t>(cnt);
  w.v1 = c.take<uint32_t>(cnt);
  w.seg_state = c.take<AucState>(kAucMaxSegments);
  w.sort = c.take_bytes(radix_carve(nullptr, n, kAucKeyBits).bytes);
  w.bytes = c.total();
  return w;
}

}  // namespace tbe

using namespace tbe;

extern "C" size_t tbe_auroc_workspace_bytes(int64_t n) {
  if (n < 0 || n >= kSortMaxPairs) return 0;
  return auc_carve(nullptr, n).bytes;
}

extern "C" int tbe_auroc_counts_f32(const float* preds, const void* labels, int32_t label_elem_size, int64_t n,
                                    float threshold, int64_t* counts, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  TBE_REQUIRE(n >= 0, "tbe_auroc_counts_f32: n < 0");
  TBE_REQUIRE(n < kSortMaxPairs, "tbe_auroc_counts_f32: n=%lld, must be < 2^29 (the pair sort's limit)", (long long)n);
  TBE_REQUIRE(label_elem_size == 4 || label_elem_size == 8, "tbe_auroc_counts_f32: labels must be float32 (4) or int64 (8)");
  TBE_REQUIRE(counts != nullptr && workspace != nullptr && (n == 0 || (preds != nullptr && labels != nullptr)),
              "tbe_auroc_counts_f32: null pointer");
  TBE_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0, "tbe_auroc_counts_f32: counts must be 8-B aligned");
  TBE_REQUIRE((reinterpret_cast<uintptr_t>(preds) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(labels) & static_cast<uintptr_t>(label_elem_size - 1)) == 0,
              "tbe_auroc_counts_f32: preds / labels are not aligned to their element size");
  TBE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "tbe_auroc_counts_f32: workspace must be 256-B aligned");
  const AucWorkspace ws = auc_carve(workspace, n);
  if (ws.bytes > workspace_bytes) {
    set_error("tbe_auroc_counts_f32: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);
    return TBE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, 6 * sizeof(int64_t), st) != hipSuccess) {
    set_error("tbe_auroc_counts_f32: hipMemsetAsync failed");
    return TBE_ERR_LAUNCH;
  }
  if (n == 0) return TBE_OK;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  const unsigned pgrid = static_cast<unsigned>(
      std::min<int64_t>(kAucPrepMaxBlocks, (n + 4 * kAucThreads - 1) / (4 * kAucThreads)));
  if (label_elem_size == 4)
    hipLaunchKernelGGL(auroc_prepare_kernel<float>, dim3(pgrid), dim3(kAucThreads), 0, st, preds,
                       static_cast<const float*>(labels), n, threshold, ws.k0, ws.v0, cnt);
  else
    hipLaunchKernelGGL(auroc_prepare_kernel<int64_t>, dim3(pgrid), dim3(kAucThreads), 0, st, preds,
                       static_cast<const int64_t*>(labels), n, threshold, ws.k0, ws.v0, cnt);
  TBE_CHECK_LAUNCH("tbe_auroc_counts_f32 (prepare)");
  const RadixWorkspace rws = radix_carve(ws.sort, n, kAucKeyBits);
  const int where = radix_sort_pairs<uint32_t, uint32_t>(ws.k0, ws.k1, ws.v0, ws.v1, n, kAucKeyBits, rws, st);
  if (where < 0) return where;
  const uint32_t* sk = where ? ws.k1 : ws.k0;
  const uint32_t* sv = where ? ws.v1 : ws.v0;
  const AucGeom g = auc_geom(n);
  hipLaunchKernelGGL(auroc_reduce_kernel<false>, dim3(static_cast<unsigned>(g.segments)), dim3(kAucThreads), 0, st, sk, sv, n,
                     g.tiles_per_segment, ws.seg_state, cnt + kCnt2U);
  hipLaunchKernelGGL(auroc_reduce_kernel<true>, dim3(static_cast<unsigned>(g.segments)), dim3(kAucThreads), 0, st, sk, sv, n,
                     g.tiles_per_segment, ws.seg_state, cnt + kCnt2U);
  TBE_CHECK_LAUNCH("tbe_auroc_counts_f32 (reduce)");
  return TBE_OK;
}
