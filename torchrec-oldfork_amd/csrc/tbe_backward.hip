// TBE backward + fused "exact" optimizer for gfx950.
//
// Reference wiring: torchrec/distributed/batched_embedding_kernel.py:604-665
// (BatchedFusedEmbeddingBag) and :53-257 (EmbeddingFusedOptimizer); the arithmetic itself
// lives in fbgemm_gpu, which is absent from the reference tree.  "Exact" optimizers sum
// every contribution a batch makes to one table row BEFORE applying a single update
// (pinned for EXACT_SGD by torchrec/distributed/test_utils/test_model_parallel_base.py:257-283,
// which compares against nn.EmbeddingBag + torch.optim.SGD).
//
// Pipeline (all on `stream`, no host sync, no atomics on floats => bitwise reproducible):
//  1. linearize : key[p] = feat_row_base[f] + indices[p]  (invalid index -> sentinel),
//                 payload[p] = bag  or  (bag << 32) | p    (thread per bag, coalesced at L = 1)
//  2. sort      : stable LSD radix sort of (key, payload) on the low key_bits bits
//                 (hand-written, radix_sort.hpp: one launch per 10-bit digit pass).  The payload is
//                 the 32-bit bag number for pooled lookups without per-sample weights (the update
//                 needs nothing else), (bag << 32) | position otherwise.
//  3. update    : the sorted contributions are cut into fixed chunks of C; one G-lane group
//                 walks a chunk, 4 gradient rows + 4 weight rows in flight, accumulates
//                 runs of equal keys in registers and applies the optimizer when a run
//                 ends inside the chunk.  Runs that cross a chunk boundary leave a
//                 partial row in the workspace.
//  4. fixup     : the chunk where a crossing run started sums the partials in chunk
//                 order and applies the update.
// Fixed chunks keep the work balanced no matter how skewed the ids are (a 3-row table
// receives B contributions per row).
// Between 2 and 3 a caller at one id per bag may ask which contributions touch their row alone
// (tbe_backward_single_flags), apply exact SGD to those rows where it computes their gradient, and have the
// update leave them out (tbe_backward_apply_skip_single_f32; key_is_single in tbe_backward_impl.hpp is the rule of both).
#include "tbe_backward_impl.hpp"

namespace tbe {

// One launch instead of two memsets: every key starts as all-ones (= invalid: positions that inconsistent
// offsets leave uncovered must not reach the update kernel as garbage rows) and the sort's state block
// (tickets, digit totals, histogram rows; origin_count lives among the tickets) starts as zero.
__global__ __launch_bounds__(256) void bwd_fill_kernel(uint4* __restrict__ keys16, int64_t n_keys16,
                                                        uint4* __restrict__ state16, int64_t n_state16) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  for (int64_t i = t; i < n_keys16; i += stride) keys16[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
  for (int64_t i = t; i < n_state16; i += stride) state16[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <typename KeyT, typename PayT>
__global__ __launch_bounds__(256) void bwd_linearize_pooled_kernel(
    const int64_t* __restrict__ indices, const int64_t* __restrict__ offsets,
    const int64_t* __restrict__ feat_rows, const int64_t* __restrict__ feat_row_base,
    const int64_t* __restrict__ feat_window, int F, int B,
    int64_t N, int key_bits, KeyT* __restrict__ keys, PayT* __restrict__ payload,
    int32_t* bounds_errors) {
  const int64_t bag = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (bag >= static_cast<int64_t>(F) * B) return;
  const int f = static_cast<int>(bag / B);
  const int64_t s = offsets[bag];
  const int64_t e = offsets[bag + 1];
  if (s < 0 || e > N || s > e) {
    // malformed offsets: never touch memory through them.  The positions such a bag fails to cover keep the
    // all-ones key the caller pre-filled, which the update kernel treats as "no row".
    if (bounds_errors != nullptr) atomicAdd(bounds_errors, 1);
    return;
  }
  const RowWindow win = load_window(feat_rows, feat_window, f);
  const int64_t base = feat_row_base[f];
  const KeyT sentinel = static_cast<KeyT>((key_bits >= 64) ? ~0ull : ((1ull << key_bits) - 1ull));
  int nbad = 0;
  for (int64_t p = s; p < e; ++p) {
    int64_t lidx;
    const int cls = classify_id(win, indices[p], lidx);  // rows of other shards: no key, not an error
    if (cls == kIdBad) ++nbad;
    keys[p] = cls == kIdLocal ? static_cast<KeyT>(base + lidx) : sentinel;
    payload[p] = make_payload<PayT>(static_cast<uint32_t>(bag), static_cast<uint32_t>(p));
  }
  if (nbad > 0 && bounds_errors != nullptr) atomicAdd(bounds_errors, nbad);
}

// PoolingMode.NONE: position p belongs to feature f(p); "bag" is encoded as f*B so that the
// update kernel recovers f with the same division.
template <typename KeyT>
__global__ __launch_bounds__(256) void bwd_linearize_nobag_kernel(
    const int64_t* __restrict__ indices, const int64_t* __restrict__ offsets,
    const int64_t* __restrict__ feat_rows, const int64_t* __restrict__ feat_row_base, int F, int B,
    int64_t N, int key_bits, KeyT* __restrict__ keys, uint64_t* __restrict__ payload,
    int32_t* bounds_errors) {
  extern __shared__ int64_t fb[];
  for (int i = threadIdx.x; i <= F; i += blockDim.x) fb[i] = offsets[static_cast<int64_t>(i) * B];
  __syncthreads();
  const KeyT sentinel = static_cast<KeyT>((key_bits >= 64) ? ~0ull : ((1ull << key_bits) - 1ull));
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < N;
       p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    int lo = 0, hi = F;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (fb[mid] <= p) lo = mid; else hi = mid;
    }
    const int f = lo;
    const int64_t idx = indices[p];
    const bool ok = static_cast<uint64_t>(idx) < static_cast<uint64_t>(feat_rows[f]);
    if (!ok && bounds_errors != nullptr) atomicAdd(bounds_errors, 1);
    keys[p] = ok ? static_cast<KeyT>(feat_row_base[f] + idx) : sentinel;
    payload[p] = (static_cast<uint64_t>(static_cast<int64_t>(f) * B) << 32) | static_cast<uint32_t>(p);
  }
}

template <typename KeyT, typename PayT>
static int prepare(const BwdArgs& a, const BwdWorkspace& w, hipStream_t st) {
  ProfileSpan prep_span(TBE_PROFILE_BWD_PREPARE, st);
  KeyT* kin = static_cast<KeyT*>(w.keys_in);
  KeyT* kout = static_cast<KeyT*>(w.keys_out);
  PayT* pin = static_cast<PayT*>(w.pay_in);
  PayT* pout = static_cast<PayT*>(w.pay_out);
  {
    // 16-B units; both buffers start 256-B aligned and the carver pads each to the next 256-B boundary
    const int64_t n_keys16 = a.pooling_mode == TBE_POOL_NONE ? 0 : (a.N * static_cast<int64_t>(sizeof(KeyT)) + 15) / 16;
    const int64_t n_state16 = (static_cast<int64_t>(radix_state_words(a.N, a.key_bits, sizeof(KeyT) + sizeof(PayT))) + 3) / 4;
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>((std::max(n_keys16, n_state16) + 255) / 256, 2048));
    hipLaunchKernelGGL(bwd_fill_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<uint4*>(kin), n_keys16,
                       reinterpret_cast<uint4*>(w.sort.state), n_state16);
  }
  if (a.pooling_mode == TBE_POOL_NONE) {
    if constexpr (sizeof(PayT) == 8) {
      const size_t lds = (static_cast<size_t>(a.F) + 1) * sizeof(int64_t);
      const unsigned grid = static_cast<unsigned>(std::min<int64_t>((a.N + 255) / 256, 256 * 16));
      hipLaunchKernelGGL((bwd_linearize_nobag_kernel<KeyT>), dim3(grid), dim3(256), lds, st, a.indices, a.offsets,
                         a.feat_rows, a.feat_row_base, a.F, a.B, a.N, a.key_bits, kin, pin, a.bounds_errors);
    }
  } else {
    const int64_t nbags = static_cast<int64_t>(a.F) * a.B;
    const unsigned grid = static_cast<unsigned>((nbags + 255) / 256);
    hipLaunchKernelGGL((bwd_linearize_pooled_kernel<KeyT, PayT>), dim3(grid), dim3(256), 0, st, a.indices, a.offsets,
                       a.feat_rows, a.feat_row_base, a.feat_window, a.F, a.B, a.N, a.key_bits, kin, pin, a.bounds_errors);
  }
  TBE_CHECK_LAUNCH("tbe_backward linearize");
  const int where = radix_sort_pairs<KeyT, PayT>(kin, kout, pin, pout, a.N, a.key_bits, w.sort, st, kSortStateZeroed);
  return where < 0 ? where : TBE_OK;
}

// single[payload of sorted position k] = key_is_single.  With one id per bag (offsets[i] == i, what the entry is for) the
// payloads are the bag numbers 0 .. N-1, each once, so every byte of the array is written, zeros included.  A position
// that malformed offsets left uncovered carries no payload: whatever it holds is bounded by N before it is used.
template <typename KeyT>
__global__ __launch_bounds__(256) void bwd_single_flags_kernel(const KeyT* __restrict__ skey, const uint32_t* __restrict__ spay,
                                                                int64_t N, int key_bits, uint8_t* __restrict__ single) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= N) return;
  const KeyT sentinel = static_cast<KeyT>((key_bits >= 64) ? ~0ull : ((1ull << key_bits) - 1ull));
  const KeyT key = skey[k];
  const KeyT prev = k > 0 ? skey[k - 1] : sentinel;
  const KeyT next = k + 1 < N ? skey[k + 1] : sentinel;
  const uint32_t i = spay[k];
  if (i < N) single[i] = key_is_single<KeyT>(key, prev, k > 0, next, k + 1 < N, sentinel) ? 1 : 0;
}

int run_prepare(const BwdArgs& a, const BwdWorkspace& w, bool wide_payload, hipStream_t st) {
  if (a.key_bits > 32) return wide_payload ? prepare<uint64_t, uint64_t>(a, w, st) : prepare<uint64_t, uint32_t>(a, w, st);
  return wide_payload ? prepare<uint32_t, uint64_t>(a, w, st) : prepare<uint32_t, uint32_t>(a, w, st);
}

}  // namespace tbe

using namespace tbe;

extern "C" size_t tbe_backward_workspace_bytes(int64_t N, int32_t F, int32_t B, int32_t max_D,
                                               int32_t key_bits) {
  (void)F;
  (void)B;
  if (N <= 0) return 256;
  if (N >= kSortMaxPairs) return 0;  // not sortable in one call (the backward entry points say why)
  BwdWorkspace w;
  if (carve(nullptr, N, max_D, key_bits, &w) != TBE_OK) return 0;
  return w.total;
}

extern "C" int tbe_backward_fused_f32(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window, void* stream) {
  BwdCall c{feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base, feat_state0, feat_state1, F, B, max_D,
            key_bits, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling, grad_out, grad_row_stride,
            opt, flags, workspace, workspace_bytes};
  c.stream = stream;
  c.who = "tbe_backward_fused_f32";
  c.phase = kPhasePrepare | kPhaseApply;
  c.bounds_errors = bounds_errors;
  c.feat_window = feat_window;
  return backward_entry<float>(c);
}

extern "C" int tbe_backward_prepare(const int64_t* feat_rows, const int64_t* feat_row_base, int32_t F, int32_t B,
                                    int32_t max_D, int32_t key_bits, const int64_t* indices, int64_t N,
                                    const int64_t* offsets, int32_t pooling_mode, int32_t flags, void* workspace,
                                    size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window,
                                    void* stream) {
  BwdCall c{};  // no tables, no gradient, no optimizer (bwd_setup gives this phase a stride and an optimizer that validate)
  c.feat_rows = feat_rows;
  c.feat_row_base = feat_row_base;
  c.F = F;
  c.B = B;
  c.max_D = max_D;
  c.key_bits = key_bits;
  c.indices = indices;
  c.N = N;
  c.offsets = offsets;
  c.pooling_mode = pooling_mode;
  c.flags = flags & TBE_FLAG_WEIGHTED;
  c.workspace = workspace;
  c.workspace_bytes = workspace_bytes;
  c.stream = stream;
  c.who = "tbe_backward_prepare";
  c.phase = kPhasePrepare;
  c.bounds_errors = bounds_errors;
  c.feat_window = feat_window;
  return backward_entry<float>(c);
}

extern "C" int tbe_backward_apply_f32(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, void* stream) {
  BwdCall c{feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base, feat_state0, feat_state1, F, B, max_D,
            key_bits, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling, grad_out, grad_row_stride,
            opt, flags, workspace, workspace_bytes};
  c.stream = stream;
  c.who = "tbe_backward_apply_f32";
  c.phase = kPhaseApply;
  return backward_entry<float>(c);
}

extern "C" int tbe_backward_single_flags(int32_t F, int32_t B, int32_t max_D, int32_t key_bits, int64_t N, void* workspace,
                                         size_t workspace_bytes, uint8_t* single, void* stream) {
  const char* who = "tbe_backward_single_flags";
  TBE_REQUIRE(F > 0 && B >= 0 && N == static_cast<int64_t>(F) * B, "%s: needs exactly one id per bag (N == F * B)", who);
  TBE_REQUIRE(max_D > 0 && max_D <= 2048 && key_bits >= 1 && key_bits <= 64, "%s: max_D=%d key_bits=%d", who, max_D, key_bits);
  TBE_REQUIRE(N < kSortMaxPairs, "%s: N = %lld ids in one call; the limit is 2^29 - 1", who, static_cast<long long>(N));
  if (N == 0) return TBE_OK;
  TBE_REQUIRE(workspace && single, "%s: null pointer", who);
  TBE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "%s: workspace must be 256-B aligned", who);
  BwdWorkspace w;
  if (int rc = carve(workspace, N, max_D, key_bits, &w)) return rc;
  if (w.total > workspace_bytes) {
    set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, w.total);
    return TBE_ERR_WORKSPACE;
  }
  // where bwd_setup finds the sorted pairs
  const bool in_second = (radix_passes(key_bits) & 1) != 0;
  const void* keys = in_second ? w.keys_out : w.keys_in;
  const uint32_t* pay = static_cast<const uint32_t*>(in_second ? w.pay_out : w.pay_in);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((N + 255) / 256));
  if (key_bits > 32)
    hipLaunchKernelGGL(bwd_single_flags_kernel<uint64_t>, grid, dim3(256), 0, st, static_cast<const uint64_t*>(keys), pay, N,
                       key_bits, single);
  else
    hipLaunchKernelGGL(bwd_single_flags_kernel<uint32_t>, grid, dim3(256), 0, st, static_cast<const uint32_t*>(keys), pay, N,
                       key_bits, single);
  TBE_CHECK_LAUNCH(who);
  return TBE_OK;
}

extern "C" int tbe_backward_apply_skip_single_f32(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, void* stream) {
  BwdCall c{feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base, feat_state0, feat_state1, F, B, max_D,
            key_bits, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling, grad_out, grad_row_stride,
            opt, flags, workspace, workspace_bytes};
  c.stream = stream;
  c.who = "tbe_backward_apply_skip_single_f32";
  c.phase = kPhaseApply;
  c.skip_single = true;
  return backward_entry<float>(c);
}

// The twins that also take the row-norm optimizer family and gradient clipping (include/tbe_hip.h); with ext == NULL and
// an optimizer of the twin they are the twin.
extern "C" int tbe_backward_fused_ex_f32(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window, const tbe_optimizer_ext* ext,
    void* stream) {
  BwdCall c{feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base, feat_state0, feat_state1, F, B, max_D,
            key_bits, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling, grad_out, grad_row_stride,
            opt, flags, workspace, workspace_bytes};
  c.stream = stream;
  c.who = "tbe_backward_fused_ex_f32";
  c.phase = kPhasePrepare | kPhaseApply;
  c.bounds_errors = bounds_errors;
  c.feat_window = feat_window;
  c.ex = true;
  c.ext = ext;
  return backward_entry<float>(c);
}

extern "C" int tbe_backward_apply_ex_f32(
    const uint64_t* feat_weights, const int32_t* feat_D, const int64_t* feat_out_offset,
    const int64_t* feat_rows, const int64_t* feat_row_base, const uint64_t* feat_state0,
    const uint64_t* feat_state1, int32_t F, int32_t B, int32_t max_D,
    int32_t key_bits, const int64_t* indices, int64_t N, const int64_t* offsets,
    const float* per_sample_weights, int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
    int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags, void* workspace,
    size_t workspace_bytes, const tbe_optimizer_ext* ext, void* stream) {
  BwdCall c{feat_weights, feat_D, feat_out_offset, feat_rows, feat_row_base, feat_state0, feat_state1, F, B, max_D,
            key_bits, indices, N, offsets, per_sample_weights, pooling_mode, feat_pooling, grad_out, grad_row_stride,
            opt, flags, workspace, workspace_bytes};
  c.stream = stream;
  c.who = "tbe_backward_apply_ex_f32";
  c.phase = kPhaseApply;
  c.ex = true;
  c.ext = ext;
  return backward_entry<float>(c);
}

// ---- the pair sort as a public entry (tests, micro-benchmarks) ---------------------------------------
extern "C" size_t tbe_sort_pairs_workspace_bytes(int64_t n, int32_t key_bits) {
  if (key_bits < 1 || key_bits > 64) return 0;
  return radix_carve(nullptr, n, key_bits).bytes;
}

extern "C" int tbe_sort_pairs(void* keys, void* keys_tmp, void* payload, void* payload_tmp, int64_t n, int32_t key_bits,
                              int32_t key_bytes, int32_t payload_bytes, void* workspace, size_t workspace_bytes,
                              void* stream) {
  TBE_REQUIRE(n >= 0, "tbe_sort_pairs: n < 0");
  TBE_REQUIRE(key_bytes == 4 || key_bytes == 8, "tbe_sort_pairs: key_bytes must be 4 or 8");
  TBE_REQUIRE(payload_bytes == 4 || payload_bytes == 8, "tbe_sort_pairs: payload_bytes must be 4 or 8");
  TBE_REQUIRE(key_bits >= 1 && key_bits <= 8 * key_bytes, "tbe_sort_pairs: key_bits=%d", key_bits);
  if (n == 0) return TBE_OK;
  TBE_REQUIRE(keys && keys_tmp && payload && payload_tmp && workspace, "tbe_sort_pairs: null pointer");
  TBE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "tbe_sort_pairs: workspace must be 256-B aligned");
  const RadixWorkspace ws = radix_carve(workspace, n, key_bits);
  if (ws.bytes > workspace_bytes) {
    set_error("tbe_sort_pairs: workspace too small (%zu < %zu)", workspace_bytes, ws.bytes);
    return TBE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  int where;
  if (key_bytes == 4 && payload_bytes == 4)
    where = radix_sort_pairs<uint32_t, uint32_t>(static_cast<uint32_t*>(keys), static_cast<uint32_t*>(keys_tmp),
                                                 static_cast<uint32_t*>(payload), static_cast<uint32_t*>(payload_tmp), n,
                                                 key_bits, ws, st);
  else if (key_bytes == 4)
    where = radix_sort_pairs<uint32_t, uint64_t>(static_cast<uint32_t*>(keys), static_cast<uint32_t*>(keys_tmp),
                                                 static_cast<uint64_t*>(payload), static_cast<uint64_t*>(payload_tmp), n,
                                                 key_bits, ws, st);
  else if (payload_bytes == 4)
    where = radix_sort_pairs<uint64_t, uint32_t>(static_cast<uint64_t*>(keys), static_cast<uint64_t*>(keys_tmp),
                                                 static_cast<uint32_t*>(payload), static_cast<uint32_t*>(payload_tmp), n,
                                                 key_bits, ws, st);
  else
    where = radix_sort_pairs<uint64_t, uint64_t>(static_cast<uint64_t*>(keys), static_cast<uint64_t*>(keys_tmp),
                                                 static_cast<uint64_t*>(payload), static_cast<uint64_t*>(payload_tmp), n,
                                                 key_bits, ws, st);
  if (where < 0) return where;
  if (where == 1) {
    if (hipMemcpyAsync(keys, keys_tmp, static_cast<size_t>(n) * key_bytes, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(payload, payload_tmp, static_cast<size_t>(n) * payload_bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      set_error("tbe_sort_pairs: copy back failed");
      return TBE_ERR_LAUNCH;
    }
  }
  return TBE_OK;
}

extern "C" int tbe_debug_sort_timeouts(int64_t* count) {
  TBE_REQUIRE(count != nullptr, "tbe_debug_sort_timeouts: null pointer");
  if (hipDeviceSynchronize() != hipSuccess) {
    set_error("tbe_debug_sort_timeouts: hipDeviceSynchronize failed");
    return TBE_ERR_LAUNCH;
  }
  return tbe_fault_status(count);
}

// the device side of a give-up without a sort that hangs: what radix_pass_kernel does when a wait outlives kSpinLimit
__global__ void inject_sort_giveup_kernel(uint32_t* fault) { report_sort_giveup(fault); }
extern "C" int tbe_debug_inject_sort_giveup(void* stream) {
  uint32_t* const fault = fault_word_device();
  TBE_REQUIRE(fault != nullptr, "tbe_debug_inject_sort_giveup: no fault word (no HIP device?)");
  hipLaunchKernelGGL(inject_sort_giveup_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), fault);
  TBE_CHECK_LAUNCH("tbe_debug_inject_sort_giveup");
  return TBE_OK;
}
