// ReLU backward + bias gradient of one MLP layer in ONE pass (gfx950).
//
// Reference: torchrec/modules/mlp.py:14-170 (Perceptron = Linear + relu) trained through autograd,
// which runs per layer  g' = threshold_backward(g, act)  and  bias.grad = g'.sum(0)  as two kernels
// (4 passes over a [B, N] matrix: read g, read act, write g', read g').  Here one kernel reads g and
// act once, writes g' and accumulates the column sums (3 passes); the column sums of the row blocks
// are combined by a second small kernel in fixed order (deterministic, no float atomics).
// HBM-bound elementwise work between the library GEMMs of the dense MLPs — the only place, besides
// the dot interaction, where this build touches the dense side.
#include <algorithm>
#include <cstring>

#include "colsum.hpp"

namespace tbe {

// block = 256 threads = TY rows x TX float4-columns; grid = (column tiles, row blocks): colsum.hpp
template <int TX>
__global__ __launch_bounds__(256) void drelu_bgrad_kernel(const float* __restrict__ gy, const float* __restrict__ act,
                                                          float* __restrict__ gx, float* __restrict__ partial,
                                                          int64_t B, int N) {
  colsum_row_block<TX>(partial, B, N, [=](int64_t, int64_t o, float4& sum) {
    float4 g = ld4(gy + o);
    const float4 a = ld4(act + o);
    g.x = a.x > 0.f ? g.x : 0.f;
    g.y = a.y > 0.f ? g.y : 0.f;
    g.z = a.z > 0.f ? g.z : 0.f;
    g.w = a.w > 0.f ? g.w : 0.f;
    st4(gx + o, g);
    add4(sum, g);
  });
}

// partial[rb][c] = sum over the block's rows of w[b] * x[b, c]  (weight gradient of a Linear with ONE output:
// dW[0, c] = sum_b dy[b] * x[b, c] — a GEMM with N = 1 that the BLAS libraries run at ~1 % of HBM speed)
template <int TX>
__global__ __launch_bounds__(256) void wcolsum_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      float* __restrict__ partial, int64_t B, int N) {
  colsum_row_block<TX>(partial, B, N, [=](int64_t r, int64_t o, float4& sum) {
    const float4 v = ld4(x + o);
    const float s = w[r];
    sum.x = fmaf(s, v.x, sum.x);
    sum.y = fmaf(s, v.y, sum.y);
    sum.z = fmaf(s, v.z, sum.z);
    sum.w = fmaf(s, v.w, sum.w);
  });
}

// Backward of y = relu(.) W2^T behind a hidden layer with ReLU, W2 = w [1, N] (the last two layers of DLRM's over arch), in
// ONE pass over act [B, N]: the gradient of the hidden layer's pre-activation and both column sums that hang on it —
//   g = dy[b] * w[c]                       (one multiply: what the K = 1 GEMM dy w writes)
//   gx[b, c] = act[b, c] > 0 ? g : 0       partial[rb][0][c] += gx[b, c]                  (drelu_bgrad_kernel's addend)
//                                          partial[rb][1][c]  = fmaf(dy[b], act[b, c], .)  (wcolsum_kernel's)
// instead of that GEMM (writes [B, N]), wcolsum_kernel (reads act) and drelu_bgrad_kernel (reads both, writes gx).
// Addresses: the row block's (uniform) base + a 32-bit offset inside the block (N <= kHeadMaxN keeps 256 rows below 4 GB),
// one VGPR per row for the load and the store instead of two 64-bit addresses — with those the kernel took 66 VGPRs, two
// more than 8 waves per SIMD (drelu_bgrad_kernel's figure) allow.
constexpr int kHeadMaxN = 1 << 20;
template <int TX>
__global__ __launch_bounds__(256) void relu_linear1_bwd_kernel(const float* __restrict__ act, const float* __restrict__ dy,
                                                               const float* __restrict__ w, float* __restrict__ gx,
                                                               float* __restrict__ partial, int64_t B, int N) {
  const int col = (blockIdx.x * TX + threadIdx.x % TX) * 4;
  const float4 wc = col < N ? ld4(w + col) : make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t row0 = static_cast<int64_t>(blockIdx.y) * rows_per_block(N);
  const char* __restrict__ act_b = reinterpret_cast<const char*>(act + row0 * N);
  char* __restrict__ gx_b = reinterpret_cast<char*>(gx + row0 * N);
  const float* __restrict__ dy_b = dy + row0;
  colsum_row_block_n<TX, 2>(partial, B, N, [=](int64_t r, int64_t, float4(&sum)[2]) {
    const unsigned lr = static_cast<unsigned>(r - row0);  // < rows_per_block(N)
    const unsigned off = (lr * static_cast<unsigned>(N) + static_cast<unsigned>(col)) * 4u;
    const float4 a = *reinterpret_cast<const float4*>(act_b + off);
    const float d = dy_b[lr];
    float4 g;
    g.x = a.x > 0.f ? d * wc.x : 0.f;
    g.y = a.y > 0.f ? d * wc.y : 0.f;
    g.z = a.z > 0.f ? d * wc.z : 0.f;
    g.w = a.w > 0.f ? d * wc.w : 0.f;
    *reinterpret_cast<float4*>(gx_b + off) = g;
    add4(sum[0], g);
    sum[1].x = fmaf(d, a.x, sum[1].x);
    sum[1].y = fmaf(d, a.y, sum[1].y);
    sum[1].z = fmaf(d, a.z, sum[1].z);
    sum[1].w = fmaf(d, a.w, sum[1].w);
  });
}

// bias_grad[c] = sum over row blocks of partial[rb][c], fixed order: wave w takes blocks w, w+4, ...
__global__ __launch_bounds__(256) void colsum_partials_kernel(const float* __restrict__ partial, int64_t nblocks, int N,
                                                              float* __restrict__ out) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float acc = 0.f;
  if (c < N) {
#pragma unroll 8
    for (int64_t rb = wave; rb < nblocks; rb += 4) acc += partial[rb * N + c];
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && c < N) out[c] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// dst[off_s + i] = scale * sum_{c < chunks_s} src_s[c * numel_s + i], chunk order fixed (deterministic), for every segment s
// of a table {src address, chunks, numel, dst element offset} held in device memory: ONE launch that finishes every
// split-K weight gradient (chunks = batch slices of the batched wgrad GEMM), every bias gradient (chunks = row blocks of
// drelu_bgrad_kernel / wcolsum_kernel) and the gradients that are already complete (chunks = 1) of a captured backward,
// scaled by 1 / world size, straight into the flat gradient buffer — instead of one reduce kernel per layer, one
// colsum_partials launch per layer, a cat and a mul (≈ 18 launches of ≈ 5 us inside the per-rank step's graphs).
// chunks = 0 writes zeros (a parameter that received no gradient).  grid = (tiles of 256 elements, segments).
struct ChunkSeg {
  const float* src;
  int64_t chunks;
  int64_t numel;
  int64_t dst_off;
};
constexpr int kChunkSegsByValue = 32;
struct ChunkSegs32 {
  ChunkSeg s[kChunkSegsByValue];
};
__device__ __forceinline__ void multi_chunk_sum_body(const ChunkSeg sg, float* __restrict__ dst, float scale);

// segment table in device memory (captured backward graphs: a static table per segment)
__global__ __launch_bounds__(256) void multi_chunk_sum_kernel(const ChunkSeg* __restrict__ segs, float* __restrict__ dst,
                                                              float scale) {
  multi_chunk_sum_body(segs[blockIdx.y], dst, scale);
}
// segment table passed BY VALUE in the kernel arguments (eager steps: sources and destinations change every step, and a
// host buffer the GPU reads later could be overwritten by a host that runs many steps ahead)
__global__ __launch_bounds__(256) void multi_chunk_sum_args_kernel(const ChunkSegs32 segs, float* __restrict__ dst, float scale) {
  multi_chunk_sum_body(segs.s[blockIdx.y], dst, scale);
}

// A table of TBE_CHUNKS_WAVE_ORDER segments only (the row-block sums of an eager backward: up to 1024 row blocks of a few
// hundred columns each) in colsum_partials_kernel's own geometry — 64 columns x 4 waves per block, four times the blocks of
// the float4 form — and 32 loads in flight per lane: a wave's chain of up to 256 row blocks is what the launch waits for.
// grid = (tiles of 64 elements, segments).  Same order: wave w adds w, w + 4, ... from 0, then ((a0 + a1) + a2) + a3.
__global__ __launch_bounds__(256) void multi_colsum_partials_kernel(const ChunkSegs32 segs, float* __restrict__ dst, float scale) {
  __shared__ float red[4][64];
  const ChunkSeg sg = segs.s[blockIdx.y];
  const int64_t chunks = sg.chunks & ~TBE_CHUNKS_WAVE_ORDER;
  if (static_cast<int64_t>(blockIdx.x) * 64 >= sg.numel) return;  // block-uniform
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 64 + lane;
  float acc = 0.f;
  if (c < sg.numel) {
    const float* p = sg.src + c;
    int64_t rb = wave;
    for (; rb + 4 * 31 < chunks; rb += 4 * 32) {
      float a[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) a[u] = p[(rb + 4 * u) * sg.numel];
#pragma unroll
      for (int u = 0; u < 32; ++u) acc += a[u];
    }
#pragma unroll 8
    for (; rb < chunks; rb += 4) acc += p[rb * sg.numel];
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && c < sg.numel) dst[sg.dst_off + c] = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) * scale;
}

__device__ __forceinline__ void multi_chunk_sum_body(ChunkSeg sg, float* __restrict__ dst, float scale) {
  // many chunks (row-block sums of a bias: 32 ... 1024): block = 64 float4 columns x 4 waves; wave w adds chunks w, w + 4,
  // w + 8, ... (8 loads in flight), the four wave sums are combined through LDS in wave order.  Few chunks (split-K
  // slices of a weight: <= 16): block = 256 float4 columns, every thread adds all chunks of its column (all loads in
  // flight).  Either way the summation order is a function of (chunks) only.  TBE_CHUNKS_WAVE_ORDER in `chunks` takes the
  // first form at every count: colsum_partials_kernel's order, for row-block sums of few row blocks.
  __shared__ float4 red[4][64];
  const bool wave_order = (sg.chunks & TBE_CHUNKS_WAVE_ORDER) != 0;
  sg.chunks &= ~TBE_CHUNKS_WAVE_ORDER;
  if (!wave_order && sg.chunks <= 16) {  // segment-uniform, hence block-uniform
    const int64_t j0 = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * 4;
    if (j0 >= sg.numel) return;
    float* o = dst + sg.dst_off + j0;
    const bool v16 = ((sg.numel & 3) == 0) && ((reinterpret_cast<uintptr_t>(sg.src) & 15) == 0) &&
                     ((reinterpret_cast<uintptr_t>(dst + sg.dst_off) & 15) == 0);
    if (v16) {
      float4 a[16];
#pragma unroll
      for (int c = 0; c < 16; ++c)
        a[c] = c < sg.chunks ? ld4(sg.src + c * sg.numel + j0) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 acc = a[0];
#pragma unroll
      for (int c = 1; c < 16; ++c) {
        if (c < sg.chunks) {
          acc.x += a[c].x;
          acc.y += a[c].y;
          acc.z += a[c].z;
          acc.w += a[c].w;
        }
      }
      st4(o, make_float4(acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale));
    } else {
      for (int k = 0; k < 4 && j0 + k < sg.numel; ++k) {
        float acc = 0.f;
        for (int64_t c = 0; c < sg.chunks; ++c) acc += sg.src[c * sg.numel + j0 + k];
        o[k] = acc * scale;
      }
    }
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t i0 = (static_cast<int64_t>(blockIdx.x) * 64 + lane) * 4;
  if (static_cast<int64_t>(blockIdx.x) * 256 >= sg.numel) return;  // block-uniform
  const bool in = i0 < sg.numel;
  float* out = dst + sg.dst_off + i0;
  const bool vec = ((sg.numel & 3) == 0) && ((reinterpret_cast<uintptr_t>(sg.src) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(dst + sg.dst_off) & 15) == 0);
  const int nk = in ? static_cast<int>(min<int64_t>(4, sg.numel - i0)) : 0;
  auto load = [&](int64_t c) -> float4 {
    const float* p = sg.src + c * sg.numel + i0;
    if (vec) return ld4(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (nk > 0) v.x = p[0];
    if (nk > 1) v.y = p[1];
    if (nk > 2) v.z = p[2];
    if (nk > 3) v.w = p[3];
    return v;
  };
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (in) {
    int64_t c = wave;
    for (; c + 28 < sg.chunks; c += 32) {
      float4 a[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = load(c + 4 * u);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        acc.x += a[u].x;
        acc.y += a[u].y;
        acc.z += a[u].z;
        acc.w += a[u].w;
      }
    }
    for (; c < sg.chunks; c += 4) {
      const float4 a = load(c);
      acc.x += a.x;
      acc.y += a.y;
      acc.z += a.z;
      acc.w += a.w;
    }
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && in) {
    float4 r;
    r.x = (((red[0][lane].x + red[1][lane].x) + red[2][lane].x) + red[3][lane].x) * scale;
    r.y = (((red[0][lane].y + red[1][lane].y) + red[2][lane].y) + red[3][lane].y) * scale;
    r.z = (((red[0][lane].z + red[1][lane].z) + red[2][lane].z) + red[3][lane].z) * scale;
    r.w = (((red[0][lane].w + red[1][lane].w) + red[2][lane].w) + red[3][lane].w) * scale;
    if (vec) {
      st4(out, r);
    } else {
      if (nk > 0) out[0] = r.x;
      if (nk > 1) out[1] = r.y;
      if (nk > 2) out[2] = r.z;
      if (nk > 3) out[3] = r.w;
    }
  }
}

// Binary cross entropy with logits, mean over the batch, forward AND gradient in one launch (the reference's train wrapper
// applies nn.BCEWithLogitsLoss: examples/dlrm/modules/dlrm_train.py; through torch that is 8 element-wise / reduce
// kernels forward and 5 backward, ~5 us each inside a graph):
//   l_i = max(x_i, 0) - x_i * y_i + log1p(exp(-|x_i|));  loss = (1 / B) sum_i l_i;  dlogits_i = (sigmoid(x_i) - y_i) / B
// Blocks own contiguous ranges and reduce in a fixed order; the last block to finish (ticket) adds the block partials in
// index order and resets the ticket: deterministic, one launch.  labels: float32 or int64.
constexpr int kBceMaxBlocks = 64;
template <typename LabelT>
__global__ __launch_bounds__(256) void bce_with_logits_kernel(const float* __restrict__ x, const LabelT* __restrict__ y, int64_t B,
                                                              float* __restrict__ loss, float* __restrict__ dx,
                                                              float* __restrict__ partial, unsigned int* __restrict__ ticket) {
  __shared__ float red[256];
  __shared__ bool is_last;
  const int nblk = gridDim.x;
  const int64_t per = (B + nblk - 1) / nblk;
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * per;
  const int64_t hi = min(B, lo + per);
  const float invB = 1.f / static_cast<float>(B);
  float acc = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float xi = x[i];
    const float yi = static_cast<float>(y[i]);
    const float e = __expf(-fabsf(xi));
    acc += fmaxf(xi, 0.f) - xi * yi + log1pf(e);
    if (dx != nullptr) {
      const float sig = xi >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      dx[i] = (sig - yi) * invB;
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (static_cast<int>(threadIdx.x) < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(&partial[blockIdx.x], red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    is_last = atomicAdd(ticket, 1u) == static_cast<unsigned>(nblk - 1);
  }
  __syncthreads();
  if (is_last && threadIdx.x == 0) {
    __threadfence();
    float tot = 0.f;
    for (int b = 0; b < nblk; ++b) tot += __hip_atomic_load(&partial[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *loss = tot * invB;
    *ticket = 0u;  // ready for the next launch on this workspace
  }
}

}  // namespace tbe

using namespace tbe;

int tbe::launch_colsum_partials(const char* name, const float* partial, int64_t row_blocks, int N, float* out, hipStream_t st) {
  if (row_blocks == 0) return hipMemsetAsync(out, 0, sizeof(float) * N, st) == hipSuccess ? TBE_OK : TBE_ERR_LAUNCH;
  hipLaunchKernelGGL(colsum_partials_kernel, dim3((N + 63) / 64), dim3(256), 0, st, partial, row_blocks, N, out);
  TBE_CHECK_LAUNCH((std::string(name) + " colsum").c_str());
  return TBE_OK;
}

// ---- first stages: alone (`_partials`: the column sums of the row blocks are left in `partial` [row blocks][N] for a later
//      tbe_multi_chunk_sum_f32, one launch for every layer of a captured backward) or followed by the second stage ----------
static int relu_backward_first_stage(const char* name, bool one_pass, const float* grad_out, const float* act, int64_t B, int32_t N,
                                     float* grad_in, void* partial, size_t partial_bytes, hipStream_t st, int64_t* nrb) {
  return colsum_first_stage(name, one_pass, B, N, {grad_out, act, grad_in}, partial, partial_bytes, nrb, [&](auto tx, dim3 grid) {
    hipLaunchKernelGGL(drelu_bgrad_kernel<decltype(tx)::value>, grid, dim3(256), 0, st, grad_out, act, grad_in,
                       static_cast<float*>(partial), B, N);
  });
}

static int weighted_colsum_first_stage(const char* name, bool one_pass, const float* x, const float* w, int64_t B, int32_t N,
                                       void* partial, size_t partial_bytes, hipStream_t st, int64_t* nrb) {
  TBE_REQUIRE(w != nullptr || B == 0, "%s: null pointer", name);
  return colsum_first_stage(name, one_pass, B, N, {x}, partial, partial_bytes, nrb, [&](auto tx, dim3 grid) {
    hipLaunchKernelGGL(wcolsum_kernel<decltype(tx)::value>, grid, dim3(256), 0, st, x, w, static_cast<float*>(partial), B, N);
  });
}

// two sums per column: `partial` is [row blocks][2 N], so half its bytes must hold a one-sum kernel's [row blocks][N]
static int relu_linear1_first_stage(const char* name, bool one_pass, const float* act, const float* dy, const float* w, int64_t B,
                                    int32_t N, float* grad_in, void* partial, size_t partial_bytes, hipStream_t st, int64_t* nrb) {
  TBE_REQUIRE(dy != nullptr || B == 0, "%s: null pointer", name);
  TBE_REQUIRE(N <= kHeadMaxN, "%s: N=%d above %d", name, N, kHeadMaxN);
  return colsum_first_stage(name, one_pass, B, N, {act, w, grad_in}, partial, partial_bytes / 2, nrb, [&](auto tx, dim3 grid) {
    hipLaunchKernelGGL(relu_linear1_bwd_kernel<decltype(tx)::value>, grid, dim3(256), 0, st, act, dy, w, grad_in,
                       static_cast<float*>(partial), B, N);
  });
}

extern "C" int64_t tbe_colsum_row_blocks(int64_t B, int32_t N) { return B <= 0 || N <= 0 ? 0 : colsum_row_blocks(B, N); }
extern "C" size_t tbe_relu_backward_bias_grad_workspace_bytes(int64_t B, int32_t N) { return colsum_workspace_bytes(B, N); }
extern "C" size_t tbe_weighted_colsum_workspace_bytes(int64_t B, int32_t N) { return colsum_workspace_bytes(B, N); }

extern "C" int tbe_relu_backward_bias_grad_f32(const float* grad_out, const float* act, int64_t B, int32_t N,
                                               float* grad_in, float* bias_grad, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  const char* name = "tbe_relu_backward_bias_grad_f32";
  TBE_REQUIRE(bias_grad != nullptr, "%s: null bias_grad", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int64_t nrb;
  const int rc = relu_backward_first_stage(name, true, grad_out, act, B, N, grad_in, workspace, workspace_bytes, st, &nrb);
  return rc != TBE_OK ? rc : launch_colsum_partials(name, static_cast<const float*>(workspace), nrb, N, bias_grad, st);
}

extern "C" int tbe_relu_backward_bias_partials_f32(const float* grad_out, const float* act, int64_t B, int32_t N,
                                                   float* grad_in, float* partial, size_t partial_bytes, void* stream) {
  int64_t nrb;
  return relu_backward_first_stage("tbe_relu_backward_bias_partials_f32", false, grad_out, act, B, N, grad_in, partial,
                                   partial_bytes, static_cast<hipStream_t>(stream), &nrb);
}

extern "C" int tbe_weighted_colsum_f32(const float* x, const float* w, int64_t B, int32_t N, float* out,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "tbe_weighted_colsum_f32";
  TBE_REQUIRE(out != nullptr, "%s: null out", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int64_t nrb;
  const int rc = weighted_colsum_first_stage(name, true, x, w, B, N, workspace, workspace_bytes, st, &nrb);
  return rc != TBE_OK ? rc : launch_colsum_partials(name, static_cast<const float*>(workspace), nrb, N, out, st);
}

extern "C" int tbe_weighted_colsum_partials_f32(const float* x, const float* w, int64_t B, int32_t N, float* partial,
                                                size_t partial_bytes, void* stream) {
  int64_t nrb;
  return weighted_colsum_first_stage("tbe_weighted_colsum_partials_f32", false, x, w, B, N, partial, partial_bytes,
                                     static_cast<hipStream_t>(stream), &nrb);
}

extern "C" size_t tbe_relu_linear1_backward_workspace_bytes(int64_t B, int32_t N) { return 2 * colsum_workspace_bytes(B, N); }

extern "C" int tbe_relu_linear1_backward_f32(const float* act, const float* dy, const float* w, int64_t B, int32_t N,
                                             float* grad_in, float* sums, void* workspace, size_t workspace_bytes,
                                             void* stream) {
  const char* name = "tbe_relu_linear1_backward_f32";
  TBE_REQUIRE(sums != nullptr, "%s: null sums", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int64_t nrb;
  const int rc = relu_linear1_first_stage(name, true, act, dy, w, B, N, grad_in, workspace, workspace_bytes, st, &nrb);
  return rc != TBE_OK ? rc : launch_colsum_partials(name, static_cast<const float*>(workspace), nrb, 2 * N, sums, st);
}

extern "C" int tbe_relu_linear1_backward_partials_f32(const float* act, const float* dy, const float* w, int64_t B, int32_t N,
                                                      float* grad_in, float* partial, size_t partial_bytes, void* stream) {
  int64_t nrb;
  return relu_linear1_first_stage("tbe_relu_linear1_backward_partials_f32", false, act, dy, w, B, N, grad_in, partial,
                                  partial_bytes, static_cast<hipStream_t>(stream), &nrb);
}

extern "C" int tbe_multi_chunk_sum_f32(const int64_t* seg_table, int32_t nseg, int64_t max_numel, float* dst, float scale,
                                       void* stream) {
  TBE_REQUIRE(nseg >= 0 && max_numel >= 0, "tbe_multi_chunk_sum_f32: bad sizes");
  if (nseg == 0 || max_numel == 0) return TBE_OK;
  TBE_REQUIRE(seg_table && dst, "tbe_multi_chunk_sum_f32: null pointer");
  TBE_REQUIRE(nseg <= 65535, "tbe_multi_chunk_sum_f32: more than 65535 segments");
  static_assert(sizeof(ChunkSeg) == 4 * sizeof(int64_t), "segment table layout");
  const int64_t tiles = (max_numel + 255) / 256;
  TBE_REQUIRE(tiles < (1ll << 31), "tbe_multi_chunk_sum_f32: segment too long");
  hipLaunchKernelGGL(multi_chunk_sum_kernel, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(nseg)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<const ChunkSeg*>(seg_table), dst, scale);
  TBE_CHECK_LAUNCH("tbe_multi_chunk_sum_f32");
  return TBE_OK;
}

extern "C" int tbe_multi_chunk_sum_host_table_f32(const int64_t* host_seg_table, int32_t nseg, int64_t max_numel, float* dst,
                                                  float scale, void* stream) {
  TBE_REQUIRE(nseg >= 0 && nseg <= kChunkSegsByValue && max_numel >= 0,
              "tbe_multi_chunk_sum_host_table_f32: 0 <= nseg <= %d required", kChunkSegsByValue);
  if (nseg == 0 || max_numel == 0) return TBE_OK;
  TBE_REQUIRE(host_seg_table != nullptr, "tbe_multi_chunk_sum_host_table_f32: null table");
  ChunkSegs32 segs{};
  memcpy(segs.s, host_seg_table, static_cast<size_t>(nseg) * sizeof(ChunkSeg));
  bool all_wave_order = true;
  for (int s = 0; s < nseg; ++s) all_wave_order = all_wave_order && (segs.s[s].chunks & TBE_CHUNKS_WAVE_ORDER) != 0;
  if (all_wave_order) {  // row-block sums only: the narrow form (same order, more blocks, more loads in flight)
    const int64_t tiles64 = (max_numel + 63) / 64;
    TBE_REQUIRE(tiles64 < (1ll << 31), "tbe_multi_chunk_sum_host_table_f32: segment too long");
    hipLaunchKernelGGL(multi_colsum_partials_kernel, dim3(static_cast<unsigned>(tiles64), static_cast<unsigned>(nseg)), dim3(256),
                       0, static_cast<hipStream_t>(stream), segs, dst, scale);
    TBE_CHECK_LAUNCH("tbe_multi_chunk_sum_host_table_f32");
    return TBE_OK;
  }
  const int64_t tiles = (max_numel + 255) / 256;
  TBE_REQUIRE(tiles < (1ll << 31), "tbe_multi_chunk_sum_host_table_f32: segment too long");
  hipLaunchKernelGGL(multi_chunk_sum_args_kernel, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(nseg)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), segs, dst, scale);
  TBE_CHECK_LAUNCH("tbe_multi_chunk_sum_host_table_f32");
  return TBE_OK;
}

extern "C" size_t tbe_bce_with_logits_workspace_bytes(void) { return 512; }  // [64 block partials | ticket], zeroed ONCE

extern "C" int tbe_bce_with_logits_f32(const float* logits, const void* labels, int32_t label_elem_size, int64_t B, float* loss,
                                       float* dlogits, void* workspace, size_t workspace_bytes, void* stream) {
  TBE_REQUIRE(B > 0, "tbe_bce_with_logits_f32: empty batch");
  TBE_REQUIRE(label_elem_size == 4 || label_elem_size == 8, "tbe_bce_with_logits_f32: labels must be float32 (4) or int64 (8)");
  TBE_REQUIRE(logits && labels && loss && workspace, "tbe_bce_with_logits_f32: null pointer");
  TBE_REQUIRE(workspace_bytes >= tbe_bce_with_logits_workspace_bytes() && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
              "tbe_bce_with_logits_f32: workspace too small or misaligned");
  float* partial = static_cast<float*>(workspace);
  unsigned int* ticket = reinterpret_cast<unsigned int*>(partial + kBceMaxBlocks);
  const unsigned nblk = static_cast<unsigned>(std::min<int64_t>(kBceMaxBlocks, (B + 2047) / 2048));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (label_elem_size == 4)
    hipLaunchKernelGGL(bce_with_logits_kernel<float>, dim3(nblk), dim3(256), 0, st, logits, static_cast<const float*>(labels), B,
                       loss, dlogits, partial, ticket);
  else
    hipLaunchKernelGGL(bce_with_logits_kernel<int64_t>, dim3(nblk), dim3(256), 0, st, logits, static_cast<const int64_t*>(labels),
                       B, loss, dlogits, partial, ticket);
  TBE_CHECK_LAUNCH("tbe_bce_with_logits_f32");
  return TBE_OK;
}
