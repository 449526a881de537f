// BERT4Rec's HistoryArch on gfx950 in one launch each way: item-table lookup, pad / truncate to L rows, positional add,
// LayerNorm over the whole [L, E] sample and dropout.
//
// Reference: examples/bert4rec/models/bert4rec.py:323-409 — EmbeddingCollection, jagged_2d_to_dense, `+ positional`,
// nn.LayerNorm([L, E]), nn.Dropout: five or six passes over [B, L, E] each way, with the embeddings, the LayerNorm's input
// and the dropout mask kept for the backward.  Here, per sample b with n = min(len_b, L):
//   forward   x[l, :] = table[id_{b,l}, :] + positional[l, :] (l < n),  positional[l, :] (l >= n)
//             mean = (sum x) / (L E);  var = (sum (x - mean)^2) / (L E) (two-pass);  rstd = 1 / sqrtf(var + eps)
//             y = drop(((x - mean) * rstd) * gamma + beta);   stats[b] = (mean, rstd)
//   backward  g' = drop'(g_y);  xhat = (x - mean) * rstd from the table rows again;  d = g' * gamma
//             c1 = (sum d) / (L E);  c2 = (sum d * xhat) / (L E);  g_x = rstd * ((d - c1) - xhat * c2)
//             grad_emb[offsets[b] + l, :] = g_x[l, :] (l < n, id local), +0 (bad / foreign id, positions >= L)
//             grad_params = (sum_b g_x, sum_b g' * xhat, sum_b g')
//
// Geometry: ONE workgroup owns one sample at a time and keeps the whole L * E row in REGISTERS between the reduction passes:
// thread t holds the float4 groups t, t + T, ... (S compile-time slots).  The class (T, S) follows from L * E alone:
//   L E / 4 <= 256 S, S = 1 | 2 | 4 | 8 : T = 256;    L E / 4 <= 4096 : (1024, 4);    L E / 4 <= 8192 : (1024, 8)
// so the cap is L * E <= 32 768.  Registers rather than an LDS image: the backward needs TWO arrays between its passes
// (d and xhat, 2 x 128 KB at the cap, more than the CU's 160 KB of LDS) while the CU's register file holds 512 KB; and the
// row never crosses LDS, which carries only the cross-wave sums.  A (1024, 8) workgroup has 64 row registers per thread in
// the backward, within the 128 a 1024-thread workgroup may use: one workgroup (16 waves) per CU; the T = 256 classes run
// several workgroups per CU.  A float4 group lies inside one table row (E % 4 == 0): its row index is q * 4 / E.
// Sums: a thread adds its elements from 0.0f in slot order (x, y, z, w inside a float4), a wave by the xor butterfly, the
// workgroup's waves left to right through LDS — an order fixed by (L, E).
// Batch sums (row-block scheme): workgroup r owns the samples [r * rpb, (r + 1) * rpb), rpb = ceil(B / max blocks); its
// thread of an element writes the first sample's addend to partial[r][3][L E] and adds the following samples' to it in sample
// order (the three accumulators of a row do not fit beside d and xhat in registers); history_finish_kernel then adds the
// row blocks in colsum_partials_kernel's order.  No float atomics: fixed by (B, L, E).
#include <cmath>

#include "rowreg.hpp"  // row_sum

#include "rln_draw.hpp"

namespace tbe {

constexpr int kHistMaxElems = 1024 * 8 * 4;  // L * E of the widest class
constexpr int kHistWantPos = 1, kHistWantGamma = 2, kHistWantBeta = 4;

static bool hist_supported(int64_t L, int64_t E) {
  return L >= 1 && E >= 4 && E <= 2048 && (E & 3) == 0 && L <= kHistMaxElems && L * E <= kHistMaxElems;
}
// the class of L * E: threads per workgroup and slots per thread
static void hist_class(int64_t LE, int* T, int* S) {
  const int64_t n4 = LE / 4;
  *T = n4 <= 256 * 8 ? 256 : 1024;
  *S = 1;
  while (static_cast<int64_t>(*T) * *S < n4) *S *= 2;
  if (*T == 1024 && *S < 4) *S = 4;
}
// samples per workgroup: at most 1024 (T = 256) / 256 (T = 1024) workgroups
static int64_t hist_rows_per_block(int64_t B, int T) {
  const int64_t cap = T == 256 ? 1024 : 256;
  return B <= cap ? 1 : (B + cap - 1) / cap;
}

struct HistArgs {
  const uint64_t* feat_weights;
  const int64_t *feat_rows, *feat_window, *ids, *offsets;
  const float *positional, *gamma, *beta, *stats_in, *gy;
  float *y, *stats, *grad_emb, *partial;
  int32_t* bounds_errors;
  int64_t N, B, rpb;
  int32_t L, E, want;
  float eps;
  RlnDrop drop;
};

// Sum over the workgroup's T threads of each v[i], the same value in every thread: the butterfly of every wave, then the
// waves left to right.  Consecutive calls alternate `phase` (see row_sum): one barrier per call.
template <int T, int NV>
__device__ __forceinline__ void hist_block_sum(float (&v)[NV], int& phase) {
  constexpr int NW = T / kWave;
  __shared__ float red[2][NV][NW];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i] = row_sum<kWave>(v[i]);
    if ((threadIdx.x & 63) == 0) red[phase][i][threadIdx.x >> 6] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    float acc = red[phase][i][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) acc += red[phase][i][w];
    v[i] = acc;
  }
  phase ^= 1;
}

__device__ __forceinline__ float hist_sum4(const float4 a, float acc) {
  acc += a.x;
  acc += a.y;
  acc += a.z;
  acc += a.w;
  return acc;
}

// Element offsets are unsigned 32-bit words beside a workgroup-uniform base, so that an access is one scalar base plus one
// vector offset: a 64-bit address per slot and array would take the registers the row needs.
__device__ __forceinline__ float4 hist_ld4(const float* __restrict__ base, uint32_t e) {
  return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + static_cast<size_t>(e * 4u));
}
__device__ __forceinline__ void hist_st4(float* __restrict__ base, uint32_t e, const float4 v) {
  *reinterpret_cast<float4*>(reinterpret_cast<char*>(base) + static_cast<size_t>(e * 4u)) = v;
}

// One sample's bag: the first row of its ids and how many of them the dense form keeps.  A malformed bag is empty.
struct HistBag {
  int64_t start, len;
  int n;
};
__device__ __forceinline__ HistBag hist_bag(const HistArgs& a, int64_t b, bool* malformed) {
  HistBag g;
  g.start = a.offsets[b];
  const int64_t end = a.offsets[b + 1];
  *malformed = g.start < 0 || end > a.N || g.start > end;
  g.len = *malformed ? 0 : end - g.start;
  g.n = static_cast<int>(min(g.len, static_cast<int64_t>(a.L)));
  return g;
}

// What a sample reads that does not depend on the sample.  A 1024-thread class hides it from the compiler once per sample:
// otherwise the positional and gamma loads and the row / column of every slot are hoisted out of the sample loop, where they
// take the registers the row needs (a thread of such a workgroup has 128) and are spilled.  This leans on one compiler's
// scheduling; after a ROCm update check it with the Makefile's flags plus the resource remarks,
//   hipcc $(CXXFLAGS) -Rpass-analysis=kernel-resource-usage -c history_arch.hip -o /dev/null
// which with ROCm 7.2 reports for the <1024, 8> kernels: forward 88 / 98 VGPRs and no scratch, backward 125 ... 128 VGPRs and
// 20 bytes of scratch per lane (412 without the hiding); every other class without scratch.
struct HistRowConst {
  const float *positional, *gamma, *beta;
  uint32_t E;
};
template <int T>
__device__ __forceinline__ HistRowConst hist_row_const(const HistArgs& a) {
  HistRowConst rc{a.positional, a.gamma, a.beta, static_cast<uint32_t>(a.E)};
  if (T == 1024) asm volatile("" : "+s"(rc.positional), "+s"(rc.gamma), "+s"(rc.beta), "+s"(rc.E));
  return rc;
}

// x of the float4 group at element e0 = l * E + c: positional, plus the table row of a kept position with a local id.
// *local says whether such a row was read; *bad whether the position holds an id outside the table (reported by c == 0).
__device__ __forceinline__ float4 hist_x4(const HistArgs& a, const HistRowConst& rc, const float* __restrict__ table,
                                          const RowWindow& w, const HistBag& g, uint32_t e0, uint32_t* c_out, bool* local,
                                          bool* bad) {
  const uint32_t l = e0 / rc.E;
  const uint32_t c = e0 - l * rc.E;
  float4 v = hist_ld4(rc.positional, e0);
  *local = *bad = false;
  if (l < static_cast<uint32_t>(g.n)) {
    int64_t row;
    const int kind = classify_id(w, a.ids[g.start + l], row);
    if (kind == kIdLocal) {
      const float4 r = ld4(table + row * rc.E + c);
      v = make_float4(r.x + v.x, r.y + v.y, r.z + v.z, r.w + v.w);
      *local = true;
    }
    *bad = kind == kIdBad;
  }
  *c_out = c;
  return v;
}

template <int T, int S, bool DROP>
__global__ __launch_bounds__(T) void history_fwd_kernel(const HistArgs a) {
  const uint32_t LE = a.L * a.E;
  const float fn = static_cast<float>(LE);
  const float* __restrict__ table = reinterpret_cast<const float*>(a.feat_weights[0]);
  const RowWindow w = load_window(a.feat_rows, a.feat_window, 0);
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * a.rpb, b1 = min(a.B, b0 + a.rpb);
  int phase = 0, nbad = 0;
  for (int64_t b = b0; b < b1; ++b) {
    bool malformed;
    const HistBag g = hist_bag(a, b, &malformed);
    const HistRowConst rc = hist_row_const<T>(a);
    if (malformed && threadIdx.x == 0) ++nbad;
    float4 v[S];
    float part[1] = {0.f};
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const uint32_t e0 = (k * T + threadIdx.x) * 4u;
      v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e0 < LE) {
        uint32_t c;
        bool local, bad;
        v[k] = hist_x4(a, rc, table, w, g, e0, &c, &local, &bad);
        if (bad && c == 0) ++nbad;
      }
      part[0] = hist_sum4(v[k], part[0]);  // groups beyond L * E hold zeros
    }
    hist_block_sum<T, 1>(part, phase);
    const float mean = part[0] / fn;
    part[0] = 0.f;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      if ((k * T + threadIdx.x) * 4u < LE) {
        const float4 d = make_float4(v[k].x - mean, v[k].y - mean, v[k].z - mean, v[k].w - mean);
        part[0] = hist_sum4(make_float4(d.x * d.x, d.y * d.y, d.z * d.z, d.w * d.w), part[0]);
      }
    }
    hist_block_sum<T, 1>(part, phase);
    const float rstd = 1.f / sqrtf(part[0] / fn + a.eps);
    if (threadIdx.x == 0) {
      a.stats[2 * b] = mean;
      a.stats[2 * b + 1] = rstd;
    }
    const uint32_t w2 = DROP ? rln_row_word(a.drop, static_cast<uint32_t>(b)) : 0u;
    float* __restrict__ yb = a.y + b * LE;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const uint32_t e0 = (k * T + threadIdx.x) * 4u;
      if (e0 < LE) {
        const float4 ga = hist_ld4(rc.gamma, e0), be = hist_ld4(rc.beta, e0);
        float4 o = make_float4(((v[k].x - mean) * rstd) * ga.x + be.x, ((v[k].y - mean) * rstd) * ga.y + be.y,
                               ((v[k].z - mean) * rstd) * ga.z + be.z, ((v[k].w - mean) * rstd) * ga.w + be.w);
        if (DROP) o = rln_keep4(o, w2, a.drop, e0);
        hist_st4(yb, e0, o);
      }
    }
  }
  if (a.bounds_errors != nullptr && nbad > 0) atomicAdd(a.bounds_errors, nbad);
}

// the element's addend of one batch sum: the row block's first sample writes it, the following ones add to it
__device__ __forceinline__ void hist_accumulate(float* __restrict__ plane, uint32_t e0, const float4 v, bool first) {
  float4 acc = v;
  if (!first) {
    acc = hist_ld4(plane, e0);
    acc = make_float4(acc.x + v.x, acc.y + v.y, acc.z + v.z, acc.w + v.w);
  }
  hist_st4(plane, e0, acc);
}

// PG: some parameter gradient is wanted (a.want says which).
template <int T, int S, bool DROP, bool PG>
__global__ __launch_bounds__(T) void history_bwd_kernel(const HistArgs a) {
  const uint32_t LE = a.L * a.E;
  const float fn = static_cast<float>(LE);
  const float* __restrict__ table = reinterpret_cast<const float*>(a.feat_weights[0]);
  const RowWindow w = load_window(a.feat_rows, a.feat_window, 0);
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * a.rpb, b1 = min(a.B, b0 + a.rpb);
  float* pb0 = PG ? a.partial + static_cast<int64_t>(blockIdx.x) * 3 * LE : nullptr;  // [3][L E]
  const bool want_pos = PG && (a.want & kHistWantPos), want_gamma = PG && (a.want & kHistWantGamma),
             want_beta = PG && (a.want & kHistWantBeta);
  int phase = 0;
  for (int64_t b = b0; b < b1; ++b) {
    const bool first = b == b0;
    bool malformed;
    const HistBag g = hist_bag(a, b, &malformed);
    const HistRowConst rc = hist_row_const<T>(a);
    if (PG && T == 1024) asm volatile("" : "+s"(pb0));  // as hist_row_const
    float* __restrict__ pb = pb0;
    const float mean = a.stats_in[2 * b], rstd = a.stats_in[2 * b + 1];
    const uint32_t w2 = DROP ? rln_row_word(a.drop, static_cast<uint32_t>(b)) : 0u;
    const float* __restrict__ gyb = a.gy + b * LE;
    float4 d[S], xh[S];
    float part[2] = {0.f, 0.f};
    uint32_t local_mask = 0;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const uint32_t e0 = (k * T + threadIdx.x) * 4u;
      d[k] = xh[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e0 < LE) {
        uint32_t c;
        bool local, bad;
        const float4 x = hist_x4(a, rc, table, w, g, e0, &c, &local, &bad);
        local_mask |= local ? 1u << k : 0u;
        float4 gy = hist_ld4(gyb, e0);
        if (DROP) gy = rln_keep4(gy, w2, a.drop, e0);
        const float4 ga = hist_ld4(rc.gamma, e0);
        xh[k] = make_float4((x.x - mean) * rstd, (x.y - mean) * rstd, (x.z - mean) * rstd, (x.w - mean) * rstd);
        d[k] = make_float4(gy.x * ga.x, gy.y * ga.y, gy.z * ga.z, gy.w * ga.w);
        if (want_gamma)
          hist_accumulate(pb + LE, e0, make_float4(gy.x * xh[k].x, gy.y * xh[k].y, gy.z * xh[k].z, gy.w * xh[k].w), first);
        if (want_beta) hist_accumulate(pb + 2 * LE, e0, gy, first);
      }
      part[0] = hist_sum4(d[k], part[0]);  // groups beyond L * E hold zeros
      part[1] = hist_sum4(make_float4(d[k].x * xh[k].x, d[k].y * xh[k].y, d[k].z * xh[k].z, d[k].w * xh[k].w), part[1]);
    }
    hist_block_sum<T, 2>(part, phase);
    const float c1 = part[0] / fn, c2 = part[1] / fn;
    float* __restrict__ ge = a.grad_emb + g.start * a.E;  // the bag's rows (unused when it is empty)
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const uint32_t e0 = (k * T + threadIdx.x) * 4u;
      if (e0 < LE) {
        const float4 gx = make_float4(rstd * ((d[k].x - c1) - xh[k].x * c2), rstd * ((d[k].y - c1) - xh[k].y * c2),
                                      rstd * ((d[k].z - c1) - xh[k].z * c2), rstd * ((d[k].w - c1) - xh[k].w * c2));
        if (want_pos) hist_accumulate(pb, e0, gx, first);
        if (e0 < g.n * rc.E) hist_st4(ge, e0, (local_mask >> k) & 1u ? gx : make_float4(0.f, 0.f, 0.f, 0.f));
      }
    }
    // the positions >= L of an over-long history
    const int64_t tail4 = (g.len - g.n) * (a.E / 4);
    float* __restrict__ gt = ge + static_cast<int64_t>(g.n) * a.E;
    for (int64_t i = threadIdx.x; i < tail4; i += T) st4(gt + 4 * i, make_float4(0.f, 0.f, 0.f, 0.f));
  }
}

// out[plane][c] = sum over the row blocks of partial[row block][plane][c] for the wanted planes, in colsum_partials_kernel's
// order: wave w adds the blocks w, w + 4, ... from 0.0f, then ((a0 + a1) + a2) + a3.  No row blocks: zeros.  grid = (tiles
// of 64 columns, 3).
__global__ __launch_bounds__(256) void history_finish_kernel(const float* __restrict__ partial, int64_t nblocks, int LE, int want,
                                                             float* __restrict__ out) {
  __shared__ float red[4][64];
  const int plane = blockIdx.y;
  if (!((want >> plane) & 1)) return;  // block-uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float acc = 0.f;
  if (c < LE) {
#pragma unroll 8
    for (int64_t rb = wave; rb < nblocks; rb += 4) acc += partial[(rb * 3 + plane) * LE + c];
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && c < LE) out[static_cast<int64_t>(plane) * LE + c] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// ---- host side
// The checks the two entries share; *T, *S the class, *rpb / *nrb the samples per workgroup and the grid size.
static int hist_check(const char* name, const uint64_t* feat_weights, const int64_t* feat_rows, const int64_t* feat_window,
                      const int64_t* ids, int64_t N, const int64_t* offsets, int64_t B, int32_t L, int32_t E, float p, int* T,
                      int* S, int64_t* rpb, int64_t* nrb) {
  TBE_REQUIRE(B >= 0 && N >= 0 && B < (1ll << 31), "%s: bad sizes B=%lld N=%lld (0 <= B < 2^31, N >= 0)", name,
              static_cast<long long>(B), static_cast<long long>(N));
  TBE_REQUIRE(hist_supported(L, E), "%s: unsupported (L, E) = (%d, %d): E %% 4 == 0, 4 <= E <= 2048, L >= 1, L * E <= %d", name, L,
              E, kHistMaxElems);
  TBE_REQUIRE(rln_p_ok(p), "%s: dropout p=%g outside [0, 1)", name, static_cast<double>(p));
  hist_class(static_cast<int64_t>(L) * E, T, S);
  *rpb = hist_rows_per_block(B, *T);
  *nrb = (B + *rpb - 1) / *rpb;
  if (B == 0) return TBE_OK;
  TBE_REQUIRE(feat_weights != nullptr && feat_rows != nullptr && offsets != nullptr && (N == 0 || ids != nullptr),
              "%s: null pointer", name);
  TBE_REQUIRE(all_aligned({feat_weights, feat_rows, feat_window, ids, offsets}, 7), "%s: integer arrays must be 8-B aligned", name);
  return TBE_OK;
}

}  // namespace tbe

using namespace tbe;

// launch(T, S) for the class of the row
#define TBE_HIST_CLASSES(T, S, LAUNCH)              \
  do {                                              \
    if (T == 256 && S == 1) LAUNCH(256, 1);         \
    else if (T == 256 && S == 2) LAUNCH(256, 2);    \
    else if (T == 256 && S == 4) LAUNCH(256, 4);    \
    else if (T == 256) LAUNCH(256, 8);              \
    else if (S == 4) LAUNCH(1024, 4);               \
    else LAUNCH(1024, 8);                           \
  } while (0)

extern "C" int tbe_history_supported(int64_t L, int64_t E) { return hist_supported(L, E) ? 1 : 0; }

extern "C" int tbe_history_forward_f32(const uint64_t* feat_weights, const int64_t* feat_rows, const int64_t* feat_window,
                                       const int64_t* ids, int64_t N, const int64_t* offsets, int64_t B, int32_t L, int32_t E,
                                       const float* positional, const float* gamma, const float* beta, float eps, float p,
                                       uint32_t site, uint64_t seed, int64_t call, float* y, float* stats,
                                       int32_t* bounds_errors, void* stream) {
  const char* name = "tbe_history_forward_f32";
  int T, S;
  int64_t rpb, nrb;
  int rc = hist_check(name, feat_weights, feat_rows, feat_window, ids, N, offsets, B, L, E, p, &T, &S, &rpb, &nrb);
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(std::isfinite(eps) && eps >= 0.f, "%s: eps=%g must be finite and >= 0", name, static_cast<double>(eps));
  if (B == 0) return TBE_OK;
  rc = check_pointers(name, {positional, gamma, beta, y}, {stats});
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(all_aligned({bounds_errors}, 3), "%s: tensors must be 4-B aligned", name);
  HistArgs a{};
  a.feat_weights = feat_weights, a.feat_rows = feat_rows, a.feat_window = feat_window, a.ids = ids, a.offsets = offsets;
  a.positional = positional, a.gamma = gamma, a.beta = beta, a.y = y, a.stats = stats, a.bounds_errors = bounds_errors;
  a.N = N, a.B = B, a.rpb = rpb, a.L = L, a.E = E, a.eps = eps, a.drop = rln_drop(seed, call, p, site);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(nrb));
#define TBE_HIST_FWD(TT, SS)                                                                                       \
  do {                                                                                                             \
    if (p > 0.f) hipLaunchKernelGGL((history_fwd_kernel<TT, SS, true>), grid, dim3(TT), 0, st, a);                 \
    else hipLaunchKernelGGL((history_fwd_kernel<TT, SS, false>), grid, dim3(TT), 0, st, a);                        \
  } while (0)
  TBE_HIST_CLASSES(T, S, TBE_HIST_FWD);
#undef TBE_HIST_FWD
  TBE_CHECK_LAUNCH(name);
  return TBE_OK;
}

extern "C" size_t tbe_history_backward_workspace_bytes(int64_t B, int32_t L, int32_t E, int32_t want) {
  if (want == 0) return 0;
  if (B <= 0 || !hist_supported(L, E)) return 256;
  int T, S;
  hist_class(static_cast<int64_t>(L) * E, &T, &S);
  const int64_t rpb = hist_rows_per_block(B, T);
  return align_up(static_cast<size_t>((B + rpb - 1) / rpb) * 3 * L * E * sizeof(float), 256);
}

extern "C" int tbe_history_backward_f32(const float* grad_y, const uint64_t* feat_weights, const int64_t* feat_rows,
                                        const int64_t* feat_window, const int64_t* ids, int64_t N, const int64_t* offsets,
                                        int64_t B, int32_t L, int32_t E, const float* positional, const float* gamma,
                                        const float* stats, float p, uint32_t site, uint64_t seed, int64_t call,
                                        float* grad_emb, float* grad_params, int32_t want, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  const char* name = "tbe_history_backward_f32";
  int T, S;
  int64_t rpb, nrb;
  int rc = hist_check(name, feat_weights, feat_rows, feat_window, ids, N, offsets, B, L, E, p, &T, &S, &rpb, &nrb);
  if (rc != TBE_OK) return rc;
  TBE_REQUIRE(want >= 0 && want <= 7, "%s: want=%d is no mask of positional (1) | gamma (2) | beta (4)", name, want);
  if (want != 0) {
    rc = check_pointers(name, {grad_params});
    if (rc != TBE_OK) return rc;
  }
  if (B > 0) {
    rc = check_pointers(name, {grad_y, positional, gamma}, {stats});
    if (rc != TBE_OK) return rc;
    TBE_REQUIRE(N == 0 || grad_emb != nullptr, "%s: null pointer", name);
    TBE_REQUIRE(all_aligned({grad_emb}, 15), "%s: tensors must be 16-B aligned", name);
    if (want != 0) {
      rc = check_pointers(name, {workspace});
      if (rc != TBE_OK) return rc;
      const size_t need = tbe_history_backward_workspace_bytes(B, L, E, want);
      TBE_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu bytes, %zu needed)", name, workspace_bytes, need);
    }
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int LE = L * E;
  if (B > 0) {
    HistArgs a{};
    a.feat_weights = feat_weights, a.feat_rows = feat_rows, a.feat_window = feat_window, a.ids = ids, a.offsets = offsets;
    a.positional = positional, a.gamma = gamma, a.stats_in = stats, a.gy = grad_y, a.grad_emb = grad_emb;
    a.partial = static_cast<float*>(workspace), a.want = want;
    a.N = N, a.B = B, a.rpb = rpb, a.L = L, a.E = E, a.drop = rln_drop(seed, call, p, site);
    const dim3 grid(static_cast<unsigned>(nrb));
#define TBE_HIST_BWD(TT, SS)                                                                                        \
  do {                                                                                                              \
    if (p > 0.f && want) hipLaunchKernelGGL((history_bwd_kernel<TT, SS, true, true>), grid, dim3(TT), 0, st, a);    \
    else if (p > 0.f) hipLaunchKernelGGL((history_bwd_kernel<TT, SS, true, false>), grid, dim3(TT), 0, st, a);      \
    else if (want) hipLaunchKernelGGL((history_bwd_kernel<TT, SS, false, true>), grid, dim3(TT), 0, st, a);         \
    else hipLaunchKernelGGL((history_bwd_kernel<TT, SS, false, false>), grid, dim3(TT), 0, st, a);                  \
  } while (0)
    TBE_HIST_CLASSES(T, S, TBE_HIST_BWD);
#undef TBE_HIST_BWD
    TBE_CHECK_LAUNCH(name);
  }
  if (want != 0) {  // B == 0: no row blocks, the wanted sums are zeros
    hipLaunchKernelGGL(history_finish_kernel, dim3((LE + 63) / 64, 3), dim3(256), 0, st, static_cast<const float*>(workspace), nrb,
                       LE, want, grad_params);
    TBE_CHECK_LAUNCH(name);
  }
  return TBE_OK;
}
