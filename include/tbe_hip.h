/*
 * tbe_hip.h — C ABI of the MI355X (gfx950) sharded-embedding hot path.
 *
 * This is the drop-in boundary.  The reference (samiwilf/torchrec-oldfork) has no C
 * ABI of its own for this path: it calls the un-vendored `fbgemm_gpu` Python module /
 * `torch.ops.fbgemm.*` dispatcher ops (third_party/fbgemm is an empty submodule,
 * .gitmodules:1-4).  Every entry point below replaces one of those call sites; the
 * reference file:line it serves is cited on each declaration.  The Python host side
 * (`torchrec-oldfork_amd/fbgemm_gpu/`) binds this header with ctypes and re-exposes
 * the reference's names (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - Every pointer is a DEVICE-visible address (hipMalloc, or pinned-host memory
 *    mapped into the GPU for EmbeddingLocation.MANAGED/HOST tables) unless marked
 *    `host`.  No torch types; no allocation; no host synchronisation: every call
 *    only enqueues kernels on `stream` (a hipStream_t passed as void*), so callers
 *    may capture them into a hipGraph.
 *  - Return value: 0 on success, negative TBE_ERR_* otherwise;
 *    `tbe_last_error()` gives a thread-local message.
 *  - "feature metadata" arrays (feat_*) have one entry per FEATURE (not per table):
 *    feature f of the KeyedJaggedTensor looks up table feature_table_map[f]; the
 *    host resolves that indirection once at module construction.
 *  - Jagged layout is the reference's (torchrec/sparse/jagged_tensor.py:614-1081):
 *    `offsets[f*B + b] .. offsets[f*B + b + 1]` delimits bag (feature f, sample b)
 *    inside `indices`; offsets has F*B+1 entries.
 */
#ifndef TBE_HIP_H_
#define TBE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TBE_OK 0
#define TBE_ERR_INVALID_ARGUMENT (-1)
#define TBE_ERR_LAUNCH (-2)
#define TBE_ERR_WORKSPACE (-3)
#define TBE_ERR_UNSUPPORTED (-4)

/* fbgemm_gpu.split_table_batched_embeddings_ops.PoolingMode
 * (torchrec/distributed/batched_embedding_kernel.py:18-25, embedding_configs.py:59-73) */
#define TBE_POOL_SUM 0
#define TBE_POOL_MEAN 1
#define TBE_POOL_NONE 2

/* fbgemm_gpu.split_embedding_configs.EmbOptimType as used through fused_params
 * (torchrec/distributed/tests/test_fused_optim.py:52-58, examples/bert4rec/bert4rec_main.py:488-491).
 * TBE_OPT_DENSE_GRAD is the DenseTableBatchedEmbeddingBagsCodegen backward
 * (batched_embedding_kernel.py:677-704): the coalesced row gradient is written to a
 * dense gradient table instead of being applied. */
#define TBE_OPT_EXACT_SGD 0
#define TBE_OPT_EXACT_ROWWISE_ADAGRAD 1
#define TBE_OPT_ADAM 2
#define TBE_OPT_EXACT_ADAGRAD 3
/* the row-norm family: accepted by the tbe_backward_*_ex_* entries only (formulas there) */
#define TBE_OPT_LAMB 4
#define TBE_OPT_PARTIAL_ROWWISE_ADAM 5
#define TBE_OPT_PARTIAL_ROWWISE_LAMB 6
#define TBE_OPT_LARS_SGD 7
#define TBE_OPT_DENSE_GRAD 100

/* An id with this value is skipped silently by every lookup (no row, no bounds error): how the row cache hands
 * "this row belongs to another rank's shard" to the lookup kernels. */
#define TBE_ID_SKIP INT64_MIN

#define TBE_FLAG_UNIFORM_ALIGNED 1
#define TBE_FLAG_WEIGHTED 2 /* per_sample_weights will be / are given (backward: selects the sort payload layout) */

/* Hyper-parameters of the fused optimizer, passed by value. */
typedef struct tbe_optimizer_args {
  int32_t optimizer;     /* TBE_OPT_* */
  float learning_rate;   /* set_learning_rate(), batched_embedding_kernel.py:250-257 */
  float eps;
  float weight_decay;
  float beta1;
  float beta2;
  int64_t iteration;     /* 1-based step count, used by ADAM bias correction */
} tbe_optimizer_args;

/* What tbe_optimizer_args (frozen: passed by value by every tbe_backward_* entry) has no room for; handed to the
 * tbe_backward_*_ex_* entries as a pointer to HOST memory that is read during the call.  NULL = no clipping,
 * momentum = eta = 0. */
typedef struct tbe_optimizer_ext {
  float momentum;            /* LARS_SGD: momentum of the velocity m1 */
  float eta;                 /* LARS_SGD: trust coefficient */
  float max_gradient;        /* gradient clipping bound, finite and >= 0 when gradient_clipping != 0 */
  int32_t gradient_clipping; /* != 0: every element of grad_out is clamped to [-max_gradient, max_gradient] as loaded */
} tbe_optimizer_ext;

const char* tbe_last_error(void);
int32_t tbe_abi_version(void); /* 3 */

/* Faults that make RESULTS wrong without failing a call (everything here only enqueues kernels, so a kernel that
 * gives up cannot fail the call that launched it).  Today there is one: a spin-wait of the pair sort (backward, row
 * cache prefetch) that outlived its bound because a predecessor workgroup never published — the sorted order, and
 * with it the row updates, are garbage then.  Kernels report into ONE line of GPU-mapped pinned host memory, so this
 * call neither synchronises nor touches a stream: it returns what has arrived so far (everything from work whose
 * completion the caller has observed).  Must stay 0; the Python host side raises on any increase at its check points
 * (optimizer step, flush(), bounds_check_errors(), split_embedding_weights()) — the reference's counterpart of those
 * points: torchrec/distributed/batched_embedding_kernel.py:250-257, 563.  On a box without a HIP device the word is
 * plain host memory (nothing can write it but tbe_debug_inject_fault_host). */
int tbe_fault_status(int64_t* sort_giveups);
/* test hooks: the host-side / device-side write of one give-up without a sort that hangs */
int tbe_debug_inject_fault_host(void);
int tbe_debug_inject_sort_giveup(void* stream);

/* Optional kernel timing for the measurement harness (bench.py `roofline`): when enabled the
 * library brackets its dominant kernels with HIP events recorded on the launch stream.
 * tbe_profile_read(slot) synchronises on the recorded events, returns the summed duration and
 * launch count since the last read, and clears the slot.  Never enabled by the product path. */
#define TBE_PROFILE_FWD_KERNEL 0        /* tbe_fwd_*_kernel, one launch per forward call */
#define TBE_PROFILE_BWD_UPDATE_KERNEL 1 /* bwd_update_kernel, one launch per backward call */
#define TBE_PROFILE_BWD_TOTAL 2         /* fused call: linearize + sort + update + fix-up; apply call: update + fix-up */
#define TBE_PROFILE_BWD_PREPARE 3       /* linearize + sort (gradient independent) */
#define TBE_PROFILE_NUM_SLOTS 4
int tbe_profile_enable(int32_t on);
int tbe_profile_read(int32_t slot, double* total_ms, int64_t* count);
/* table rows updated by backward launches since the last read (distinct rows per batch = the U of
 * SURVEY.md §8d's byte formula); synchronises the device. */
int tbe_profile_read_rows(int64_t* rows_updated);

/* ------------------------------------------------------------------------------------
 * TBE forward (pooled): replaces SplitTableBatchedEmbeddingBagsCodegen.__call__ /
 * DenseTableBatchedEmbeddingBagsCodegen.__call__ as called at
 * torchrec/distributed/batched_embedding_kernel.py:546-554.
 *
 *   out[b * out_row_stride + feat_out_offset[f] + d] = sum_{i in bag(f,b)} w_i * W_f[indices[i], d]
 *   (w_i = per_sample_weights[i] or 1; MEAN divides by the bag length)
 *
 * feat_weights   [F] device array of table base addresses (const float*), one per feature
 * feat_D         [F] embedding dim of the feature's table
 * feat_out_offset [F] int64 element offset of the feature's block for sample 0.  The reference layout
 *                [B, sum D] is offset = prefix sum of feat_D, stride = sum D; an all-to-all-ready
 *                layout [dst rank][B_local][D_local] (removes the split+cat copies of
 *                torchrec/distributed/comm_ops.py:555-561 / :418-428) is expressed by making each
 *                (src rank, feature) pair a pseudo-feature with offset = rank*B_local*D_local + col.
 * feat_rows      [F] number of rows of the feature's table (bounds check)
 * indices [N] int64, offsets [F*B+1] int64, per_sample_weights [N] float or NULL
 * out: float buffer addressed as above; out_row_stride in elements
 * max_D          must be >= every feat_D[f] (and <= 2048).  It ALONE selects the kernel class — lanes per row group
 *                and 16-B column slots per lane: (16, 1) up to 64, (32, 1) up to 128, (64, 1) / (64, 2) / (64, 4) /
 *                (64, 8) up to 256 / 512 / 1024 / 2048 — whatever the feat_D are: a narrow feature in a wide module
 *                runs in the wide class with idle lanes.  The library does not read feat_D on the host, so a
 *                max_D below some feat_D[f] is NOT an error it can report: columns of that feature beyond the
 *                class's reach (4 * lanes * slots) are silently not written.
 * bounds_errors  optional device int32 counter: incremented for every index outside
 *                [0, rows); such an index contributes a zero row (never dereferenced).  Also incremented for
 *                every bag whose offsets are malformed (start < 0, end > N, start > end): such a bag is
 *                empty in forward and contributes nothing in backward — no memory is touched through it.
 * feat_pooling   optional [F] int32 (TBE_POOL_SUM / TBE_POOL_MEAN per feature), honoured when pooling_mode is
 *                TBE_POOL_MEAN: tables of both pooling types in ONE lookup (the reference builds one TBE per
 *                pooling type and concatenates: embedding_sharding.py:393-490, embedding_lookup.py:219-253).
 *                NULL = every feature pools as pooling_mode says.  Same parameter in tbe_backward_*.
 * feat_window    optional [2F] int64: (first global row held, global rows of the table) per feature, for
 *                row-wise shards whose ids arrive un-bucketized (the reference bucketizes instead:
 *                torchrec/distributed/embedding_sharding.py:121-184, sharding/rw_sharding.py:229-236).  Ids are
 *                then GLOBAL rows: those in [first, first + feat_rows) are looked up at id - first, other
 *                ids in [0, global rows) belong to another rank's shard and are skipped SILENTLY, ids outside
 *                [0, global rows) count as bounds errors.  NULL = every feature holds its whole table.
 *                The same parameter of tbe_backward_* and tbe_cache_prefetch means the same.
 * ---------------------------------------------------------------------------------- */
int tbe_forward_pooled_f32(const uint64_t* feat_weights, const int32_t* feat_D,
                           const int64_t* feat_out_offset, const int64_t* feat_rows, int32_t F,
                           int32_t B, int32_t max_D, const int64_t* indices,
                           int64_t N, const int64_t* offsets, const float* per_sample_weights,
                           int32_t pooling_mode, const int32_t* feat_pooling, float* out, int64_t out_row_stride,
                           int32_t* bounds_errors, const int64_t* feat_window, void* stream);

/* TBE forward, PoolingMode.NONE (sequence / unpooled): out[i, :] = W_f(i)[indices[i], :]
 * with f(i) the feature whose offsets range contains i.  All features must share one
 * dim D.  Replaces batched_embedding_kernel.py:332-335 (BatchedFusedEmbedding.forward). */
int tbe_forward_nobag_f32(const uint64_t* feat_weights, const int64_t* feat_rows, int32_t F,
                          int32_t B, int32_t D, const int64_t* indices, int64_t N,
                          const int64_t* offsets, float* out, int32_t* bounds_errors,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * TBE backward + fused "exact" optimizer: the autograd backward of the call above
 * plus the in-backward optimizer fbgemm fuses into it (wired by
 * batched_embedding_kernel.py:604-665 BatchedFusedEmbeddingBag and :53-257
 * EmbeddingFusedOptimizer).  "Exact" = all contributions of one batch to the same
 * table row are summed first (deterministic, position order), then ONE update is
 * applied to the row.
 *
 * feat_row_base [F]  global row number of row 0 of the feature's table (features that
 *                    share a table share the base); key_bits = bits needed to hold the
 *                    largest global row number.
 * feat_state0/1 [F]  base addresses of optimizer state of the feature's table
 *                    (rowwise Adagrad: float[rows] momentum1; ADAM: float[rows*D] m, v;
 *                    DENSE_GRAD: state0 = float[rows*D] dense gradient table; the row-norm family:
 *                    see tbe_backward_*_ex_*). May be NULL for SGD.
 * grad_out: same addressing as the forward output (feat_out_offset, grad_row_stride) when pooled,
 *           or [N, D] rows (grad_row_stride = D) for pooling_mode NONE.
 * flags: TBE_FLAG_UNIFORM_ALIGNED = the host asserts that every feature has dim == max_D
 *        (a multiple of 4) and that every table / state base, out offset and the gradient rows
 *        are 16-B aligned; enables the specialised kernels.  0 is always correct.
 * workspace: at least tbe_backward_workspace_bytes(N, F, B, max_D, key_bits) bytes.
 * Limits: F*B < 2^32 and N < 2^29 ids per call (the pair sort counts in 29 bits); tbe_backward_workspace_bytes
 *         returns 0 and the entry points TBE_ERR_INVALID_ARGUMENT beyond them, before anything is launched.
 *         The same N < 2^29 holds for tbe_cache_prefetch and tbe_sort_pairs.
 * ---------------------------------------------------------------------------------- */
size_t tbe_backward_workspace_bytes(int64_t N, int32_t F, int32_t B, int32_t max_D,
                                    int32_t key_bits);

int tbe_backward_fused_f32(const uint64_t* feat_weights, const int32_t* feat_D,
                           const int64_t* feat_out_offset, const int64_t* feat_rows,
                           const int64_t* feat_row_base, const uint64_t* feat_state0,
                           const uint64_t* feat_state1, int32_t F, int32_t B,
                           int32_t max_D, int32_t key_bits, const int64_t* indices, int64_t N,
                           const int64_t* offsets, const float* per_sample_weights,
                           int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
                           int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags,
                           void* workspace, size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window,
                           void* stream);

/* The backward in two phases, so that the gradient-independent half (linearize + stable sort of
 * the batch's row keys) can be enqueued on a side stream right after the forward call and overlap
 * the dense MLPs; `apply` then needs only update + fix-up once grad_out exists.
 * tbe_backward_fused_f32 == prepare followed by apply on one stream.  `apply` must receive the
 * workspace a `prepare` call filled for the same (indices, offsets, N, F, B, max_D, key_bits).
 * flags (prepare): TBE_FLAG_WEIGHTED when `apply` will be given per_sample_weights (the sort then
 * carries (bag, position) payloads instead of bag numbers); `apply` must get the same bit. */
int tbe_backward_prepare(const int64_t* feat_rows, const int64_t* feat_row_base, int32_t F,
                         int32_t B, int32_t max_D, int32_t key_bits, const int64_t* indices,
                         int64_t N, const int64_t* offsets, int32_t pooling_mode, int32_t flags,
                         void* workspace, size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window,
                         void* stream);

/* The stable pair sort the backward and the row cache use, exposed for tests and micro-benchmarks
 * (no reference counterpart: fbgemm's backward sorts with cub inside the absent submodule).
 * Sorts n (key, payload) pairs on the low key_bits bits of the keys; equal keys keep input order.
 * key_bytes / payload_bytes: 4 or 8.  keys / payload are overwritten with the sorted result; keys_tmp /
 * payload_tmp are scratch of the same size.  workspace >= tbe_sort_pairs_workspace_bytes(n, key_bits).
 * tbe_debug_sort_timeouts: tbe_fault_status after a device synchronisation (tests). */
size_t tbe_sort_pairs_workspace_bytes(int64_t n, int32_t key_bits);
int tbe_sort_pairs(void* keys, void* keys_tmp, void* payload, void* payload_tmp, int64_t n,
                   int32_t key_bits, int32_t key_bytes, int32_t payload_bytes, void* workspace,
                   size_t workspace_bytes, void* stream);
int tbe_debug_sort_timeouts(int64_t* count);
int tbe_backward_apply_f32(const uint64_t* feat_weights, const int32_t* feat_D,
                           const int64_t* feat_out_offset, const int64_t* feat_rows,
                           const int64_t* feat_row_base, const uint64_t* feat_state0,
                           const uint64_t* feat_state1, int32_t F, int32_t B,
                           int32_t max_D, int32_t key_bits, const int64_t* indices, int64_t N,
                           const int64_t* offsets, const float* per_sample_weights,
                           int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
                           int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Once-touched rows (pooling factor 1, EXACT_SGD, FP32 tables): a contribution whose row no other contribution of the
 * call touches needs no coalescing, so whoever computes its gradient row can apply the update on the spot
 * (tbe_dlrm_interaction_gather_backward_sgd_f32 below) and the update kernel can leave it out.
 *   tbe_backward_single_flags: on the workspace a tbe_backward_prepare call filled for (N = F*B ids, one per bag, no
 *     TBE_FLAG_WEIGHTED, pooled), on the same stream or after it.  Writes all of single[N]: single[f*B + b] = 1 exactly
 *     when the id of bag (f, b) gave a valid row key that no other id of the call gave, else 0.
 *   tbe_backward_apply_skip_single_f32: tbe_backward_apply_f32 for a caller that has ALREADY written
 *     w <- fmaf(-learning_rate, g + 0, w) into every row flagged by tbe_backward_single_flags (g = the row's gradient):
 *     those contributions are neither loaded nor applied (the decision is the flags' rule, taken on the same sorted keys,
 *     so every valid contribution is applied exactly once); their grad_out rows are never read.  Everything else, the
 *     profiling row counter included, is tbe_backward_apply_f32.  EXACT_SGD, SUM pooling, no per-sample weights,
 *     N == F*B, max_D <= 128. */
int tbe_backward_single_flags(int32_t F, int32_t B, int32_t max_D, int32_t key_bits, int64_t N, void* workspace,
                              size_t workspace_bytes, uint8_t* single, void* stream);
int tbe_backward_apply_skip_single_f32(const uint64_t* feat_weights, const int32_t* feat_D,
                                       const int64_t* feat_out_offset, const int64_t* feat_rows,
                                       const int64_t* feat_row_base, const uint64_t* feat_state0,
                                       const uint64_t* feat_state1, int32_t F, int32_t B,
                                       int32_t max_D, int32_t key_bits, const int64_t* indices, int64_t N,
                                       const int64_t* offsets, const float* per_sample_weights,
                                       int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
                                       int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags,
                                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Gradient of the pooled lookup with respect to per_sample_weights (fbgemm's grad_indice_weights): what
 * trains the position weights of torchrec/modules/feature_processor.py:29-74 (PositionWeightedModule) in
 * front of a weighted EmbeddingBagCollection, whose unsharded form gets it from nn.EmbeddingBag's
 * per_sample_weights gradient (torchrec/modules/embedding_modules.py:165-193).  Arguments that share a name
 * with tbe_forward_pooled_* mean the same; grad_out is addressed like the forward output.
 *
 *   position i of a well-formed bag (f, b):
 *   giw[i] = s * sum_d grad_out[b * grad_row_stride + feat_out_offset[f] + d] * float(W_f[local row of indices[i], d])
 *
 *  - s = 1 for SUM, 1 / len(bag) for a MEAN feature (uniform / per-feature rule of pooling_mode and
 *    feat_pooling as in the forward; applied as one correctly rounded division of the dot by the length).
 *    s does not contain the weight itself, so the weights are not an argument.
 *  - giw[i] = 0, with no table memory touched through it, when the id is TBE_ID_SKIP, outside the feature's
 *    feat_window or out of range; when feat_requires_grad[f] == 0 (feat_requires_grad: optional [F] int32,
 *    NULL = every feature, fbgemm's feature_requires_grad); when i lies in no well-formed bag (malformed
 *    offsets are classified exactly as in the forward: start < 0, end > N, start > end).
 *  - Every element of giw[0..N) is written by the call.  No bounds-error counter: the forward has already
 *    counted these ids and bags.
 *  - TBE_POOL_NONE returns TBE_ERR_UNSUPPORTED; the size and null checks are the forward's and return
 *    TBE_ERR_INVALID_ARGUMENT before anything is launched; N == 0 or B == 0 is TBE_OK.
 *  - Only enqueues (one memset node + one kernel): no allocation, no host synchronisation, capturable.
 *    Tables are read-only, so on a stream the call must precede a fused backward that rewrites them.
 *  - Deterministic: every summation order is fixed by the launch shape (max_D, F, B, N); no atomics.
 * _f16w reads _Float16 tables (8 B per lane) and is bit-identical to _f32 on the up-cast table.
 * ---------------------------------------------------------------------------------- */
int tbe_backward_indice_weights_f32(const uint64_t* feat_weights, const int32_t* feat_D,
                                    const int64_t* feat_out_offset, const int64_t* feat_rows, int32_t F,
                                    int32_t B, int32_t max_D, const int64_t* indices, int64_t N,
                                    const int64_t* offsets, int32_t pooling_mode, const int32_t* feat_pooling,
                                    const float* grad_out, int64_t grad_row_stride,
                                    const int32_t* feat_requires_grad, float* grad_indice_weights,
                                    const int64_t* feat_window, void* stream);
int tbe_backward_indice_weights_f16w(const uint64_t* feat_weights, const int32_t* feat_D,
                                     const int64_t* feat_out_offset, const int64_t* feat_rows, int32_t F,
                                     int32_t B, int32_t max_D, const int64_t* indices, int64_t N,
                                     const int64_t* offsets, int32_t pooling_mode, const int32_t* feat_pooling,
                                     const float* grad_out, int64_t grad_row_stride,
                                     const int32_t* feat_requires_grad, float* grad_indice_weights,
                                     const int64_t* feat_window, void* stream);

/* ------------------------------------------------------------------------------------
 * FP16 tables (EmbeddingBagConfig.data_type = DataType.FP16 -> weights_precision = SparseType.FP16:
 * torchrec/distributed/batched_embedding_kernel.py:406-417, 625-636).  Storage of the tables only:
 * feat_weights holds base addresses of _Float16 rows with a row stride of feat_D[f] halves; accumulation,
 * pooled outputs, gradients and optimizer state stay float, and every other argument means what it means
 * for the _f32 twin.  The arithmetic is the _f32 arithmetic on float(w16), so the forward output is
 * bit-identical to the _f32 kernels run on the up-cast table; only the final store of an updated row
 * converts.  Rows move as 8 B per lane when feat_D[f] is a multiple of 4 and the table base is 8-B
 * aligned, element by element otherwise.  TBE_FLAG_UNIFORM_ALIGNED asserts 16-B aligned row bases here
 * too, i.e. a dim that is a multiple of 8.  tbe_backward_workspace_bytes, tbe_backward_prepare and the
 * pair sort do not touch the tables and are shared.
 *
 * rounding (backward): how the float result x of a row update becomes a half.
 *   TBE_ROUND_NEAREST_EVEN  the IEEE conversion.
 *   TBE_ROUND_STOCHASTIC    with lo <= x <= hi the FP16 neighbours of a finite x (equal when x is
 *                           representable), the stored value is hi with probability (x - lo) / (hi - lo)
 *                           in steps of 2^-13, else lo.  The random bits are a counter-based hash of
 *                           (seed, opt.iteration, global row key = feat_row_base[f] + row, column) and nothing
 *                           else: the stored table is a pure function of the call's inputs.
 * TBE_OPT_DENSE_GRAD with FP16 tables returns TBE_ERR_UNSUPPORTED before anything is launched
 * (DenseTableBatchedEmbeddingBagsCodegen keeps float parameters: batched_embedding_kernel.py:677-704).
 * ---------------------------------------------------------------------------------- */
#define TBE_ROUND_NEAREST_EVEN 0
#define TBE_ROUND_STOCHASTIC 1

/* batched_embedding_kernel.py:546-554 with weights_precision FP16 (pooled lookup) */
int tbe_forward_pooled_f16w(const uint64_t* feat_weights, const int32_t* feat_D,
                            const int64_t* feat_out_offset, const int64_t* feat_rows, int32_t F,
                            int32_t B, int32_t max_D, const int64_t* indices,
                            int64_t N, const int64_t* offsets, const float* per_sample_weights,
                            int32_t pooling_mode, const int32_t* feat_pooling, float* out, int64_t out_row_stride,
                            int32_t* bounds_errors, const int64_t* feat_window, void* stream);

/* batched_embedding_kernel.py:332-335 with weights_precision FP16 (sequence lookup) */
int tbe_forward_nobag_f16w(const uint64_t* feat_weights, const int64_t* feat_rows, int32_t F,
                           int32_t B, int32_t D, const int64_t* indices, int64_t N,
                           const int64_t* offsets, float* out, int32_t* bounds_errors,
                           void* stream);

/* batched_embedding_kernel.py:604-665 with weights_precision FP16: prepare + apply on one stream */
int tbe_backward_fused_f16w(const uint64_t* feat_weights, const int32_t* feat_D,
                            const int64_t* feat_out_offset, const int64_t* feat_rows,
                            const int64_t* feat_row_base, const uint64_t* feat_state0,
                            const uint64_t* feat_state1, int32_t F, int32_t B,
                            int32_t max_D, int32_t key_bits, const int64_t* indices, int64_t N,
                            const int64_t* offsets, const float* per_sample_weights,
                            int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
                            int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags,
                            void* workspace, size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window,
                            int32_t rounding, uint64_t seed, void* stream);

/* the apply phase after tbe_backward_prepare (same wiring, side-stream sort) for FP16 tables */
int tbe_backward_apply_f16w(const uint64_t* feat_weights, const int32_t* feat_D,
                            const int64_t* feat_out_offset, const int64_t* feat_rows,
                            const int64_t* feat_row_base, const uint64_t* feat_state0,
                            const uint64_t* feat_state1, int32_t F, int32_t B,
                            int32_t max_D, int32_t key_bits, const int64_t* indices, int64_t N,
                            const int64_t* offsets, const float* per_sample_weights,
                            int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
                            int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags,
                            void* workspace, size_t workspace_bytes, int32_t rounding, uint64_t seed, void* stream);

/* ------------------------------------------------------------------------------------
 * The fused backward with the optimizers that need row norms, and with gradient clipping: the rest of
 * fbgemm_gpu.split_embedding_configs.EmbOptimType that the reference hands through fused_params unchanged
 * (torchrec/distributed/batched_embedding_kernel.py:604-665) and whose states it exposes as <table>.momentum1/2
 * (:133-249; the 1-D state of the PARTIAL_ROWWISE pair on its own at :215-227).  Each entry takes its twin's arguments
 * plus `ext` (host memory, may be NULL) before `stream`; with ext == NULL and an optimizer code of the twin it launches
 * the twin's kernels and the results are bit-identical.  The twins themselves keep answering TBE_ERR_UNSUPPORTED
 * ("unknown optimizer") for the codes 4-7.
 *
 * g = the coalesced ("exact") row gradient, w = the current row (float(w16) for FP16 tables), D = the row's dim,
 * t = opt.iteration >= 1, |.| = the Euclidean norm over the row's D columns.  FP32 arithmetic; the row is stored as by
 * the twins (nearest-even / stochastic rounding for FP16 tables).  Every optimizer reads and writes a touched row and
 * its state exactly once.
 *   TBE_OPT_LAMB (state0 = m1 float[rows*D], state1 = m2 float[rows*D]):
 *     m1 = beta1 m1 + (1-beta1) g;  m2 = beta2 m2 + (1-beta2) g^2;  u = m1 / (sqrt(m2) + eps) + weight_decay w
 *     r = |w| / |u| if both norms are > 0, else 1;  w -= learning_rate r u                  (no bias correction)
 *   TBE_OPT_PARTIAL_ROWWISE_ADAM (state0 = m1 float[rows*D], state1 = v float[rows]):
 *     m1 as above;  v = beta2 v + (1-beta2) mean_d(g^2)
 *     w -= learning_rate ((m1 / (1-beta1^t)) / (sqrt(v / (1-beta2^t)) + eps) + weight_decay w)
 *   TBE_OPT_PARTIAL_ROWWISE_LAMB (states as PARTIAL_ROWWISE_ADAM):
 *     m1, v as there;  u = m1 / (sqrt(v) + eps) + weight_decay w;  r as LAMB;  w -= learning_rate r u
 *   TBE_OPT_LARS_SGD (state0 = m1 float[rows*D]):
 *     alr = learning_rate eta |w| / (|g| + weight_decay |w|) if |w| > 0 and |g| > 0, else learning_rate
 *     m1 = momentum m1 + alr (g + weight_decay w);  w -= m1
 *   gradient clipping (any optimizer, TBE_OPT_DENSE_GRAD included): every element of grad_out is clamped to
 *     [-max_gradient, max_gradient] where it is loaded, i.e. before the per-sample weight and the MEAN division.
 * The forms follow fbgemm's code generator, which is absent from the reference tree (third_party/fbgemm is an empty
 * submodule): parity with fbgemm is UNPINNED, as for row-wise Adagrad and Adam.  Deliberate difference: the two
 * "> 0" guards (fbgemm's unguarded quotients give inf * 0 = NaN on a touched row whose gradient is zero).
 * Norms are summed per lane in column order, then across the lanes of the row's group in a fixed butterfly: no atomics,
 * two runs are bit-identical.
 * Errors, before anything is launched: TBE_ERR_INVALID_ARGUMENT for a missing state (LAMB and the PARTIAL_ROWWISE pair
 * need feat_state0 and feat_state1, LARS_SGD feat_state0), PARTIAL_ROWWISE_ADAM with opt.iteration < 1, clipping with a
 * max_gradient that is negative or not finite; TBE_ERR_UNSUPPORTED for an unknown optimizer code.
 * ---------------------------------------------------------------------------------- */
/* batched_embedding_kernel.py:604-665 (BatchedFusedEmbeddingBag with fused_params optimizer / gradient_clipping) */
int tbe_backward_fused_ex_f32(const uint64_t* feat_weights, const int32_t* feat_D,
                              const int64_t* feat_out_offset, const int64_t* feat_rows,
                              const int64_t* feat_row_base, const uint64_t* feat_state0,
                              const uint64_t* feat_state1, int32_t F, int32_t B,
                              int32_t max_D, int32_t key_bits, const int64_t* indices, int64_t N,
                              const int64_t* offsets, const float* per_sample_weights,
                              int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
                              int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags,
                              void* workspace, size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window,
                              const tbe_optimizer_ext* ext, void* stream);
/* the same call site, apply phase after tbe_backward_prepare (side-stream sort) */
int tbe_backward_apply_ex_f32(const uint64_t* feat_weights, const int32_t* feat_D,
                              const int64_t* feat_out_offset, const int64_t* feat_rows,
                              const int64_t* feat_row_base, const uint64_t* feat_state0,
                              const uint64_t* feat_state1, int32_t F, int32_t B,
                              int32_t max_D, int32_t key_bits, const int64_t* indices, int64_t N,
                              const int64_t* offsets, const float* per_sample_weights,
                              int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
                              int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags,
                              void* workspace, size_t workspace_bytes, const tbe_optimizer_ext* ext, void* stream);
/* batched_embedding_kernel.py:604-665 with weights_precision FP16 (:625-636) */
int tbe_backward_fused_ex_f16w(const uint64_t* feat_weights, const int32_t* feat_D,
                               const int64_t* feat_out_offset, const int64_t* feat_rows,
                               const int64_t* feat_row_base, const uint64_t* feat_state0,
                               const uint64_t* feat_state1, int32_t F, int32_t B,
                               int32_t max_D, int32_t key_bits, const int64_t* indices, int64_t N,
                               const int64_t* offsets, const float* per_sample_weights,
                               int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
                               int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags,
                               void* workspace, size_t workspace_bytes, int32_t* bounds_errors, const int64_t* feat_window,
                               int32_t rounding, uint64_t seed, const tbe_optimizer_ext* ext, void* stream);
/* the same call site with FP16 tables, apply phase after tbe_backward_prepare */
int tbe_backward_apply_ex_f16w(const uint64_t* feat_weights, const int32_t* feat_D,
                               const int64_t* feat_out_offset, const int64_t* feat_rows,
                               const int64_t* feat_row_base, const uint64_t* feat_state0,
                               const uint64_t* feat_state1, int32_t F, int32_t B,
                               int32_t max_D, int32_t key_bits, const int64_t* indices, int64_t N,
                               const int64_t* offsets, const float* per_sample_weights,
                               int32_t pooling_mode, const int32_t* feat_pooling, const float* grad_out,
                               int64_t grad_row_stride, tbe_optimizer_args opt, int32_t flags,
                               void* workspace, size_t workspace_bytes, int32_t rounding, uint64_t seed,
                               const tbe_optimizer_ext* ext, void* stream);

/* ------------------------------------------------------------------------------------
 * HBM row cache for EmbeddingLocation.MANAGED_CACHING tables (the `batched_fused_uvm_caching`
 * compute kernel: torchrec/distributed/embedding_types.py:57-76; `flush()` before weights are
 * read: batched_embedding_kernel.py:563,664; default cache_load_factor 0.2:
 * planner/constants.py:26).  The tables stay in pinned, GPU-mapped host memory; a 64-way
 * set-associative cache in HBM holds the rows in use.  The TBE kernels above are unchanged:
 * tbe_cache_prefetch rewrites the ids of cached features into slot numbers of ONE pseudo-table
 * [num_sets*64 cache slots | staging_cap staging slots] (`rows`, row stride `row_stride`), and the
 * caller points the feat_* metadata of those features at it (feat_weights = rows, feat_rows =
 * num_sets*64 + staging_cap, feat_state0 = state).  Rows that find no evictable way are held in
 * the staging slots for this batch; tbe_cache_writeback_staging copies them home after backward.
 * Results are identical to an uncached table.
 *
 *   tags [slots] int64  cached-row key (tab_key_base[t] + local row), -1 = empty; must be 16-B aligned (a set's tags
 *                       are loaded four at a time).  Slots s*64 .. s*64+63 are the ways of set s, and a key lives
 *                       only in the set  (((key * 0x9E3779B97F4A7C15) mod 2^64) >> 32) % num_sets.
 *                       Within a set a missed key takes the way with the smallest (lru, way number) among the ways
 *                       not used by this iteration; with none left the row goes to a staging slot.
 *   lru  [slots] int32  iteration of last use, -1 = never; `iteration` must increase per prefetch and stay
 *                       in [0, 2^25): the victim order packs (lru + 1) * 64 + way into 32 bits
 *   rows [(slots + staging_cap) * row_stride] float;  state: same slots, rowwise optimizer state or NULL
 *   staging_keys [staging_cap] int64;  counters [8] int32: 0 staging rows of this batch, 1 hits,
 *   2 misses, 3 evictions (write-backs), 4 unique cached rows of this batch, 5 misses of this batch
 *   tab_* : the cached tables (num_tables entries; tab_key_base has num_tables+1 = prefix sum of rows);
 *           tab_D[t] <= row_stride, and only columns 0 .. tab_D[t] of a slot that holds a row of table t are touched
 * tbe_cache_prefetch: feat_cached_table[f] = index into tab_* or -1 (ids of such features are copied
 *   unchanged); key_bits = bits of the total cached rows; staging_cap must be >= N.
 * tbe_cache_flush: every valid slot -> host table; invalidate != 0 also empties the cache.
 * ---------------------------------------------------------------------------------- */
typedef struct tbe_cache_desc {
  int64_t* tags;
  int32_t* lru;
  float* rows;
  float* state;
  int64_t* staging_keys;
  int32_t* counters;
  const int64_t* tab_key_base;
  const uint64_t* tab_weights;
  const uint64_t* tab_state;
  const int32_t* tab_D;
  int32_t num_sets;
  int32_t row_stride;
  int32_t staging_cap;
  int32_t num_tables;
} tbe_cache_desc;
size_t tbe_cache_prefetch_workspace_bytes(int64_t N, int32_t key_bits);
int tbe_cache_prefetch(const tbe_cache_desc* desc, const int32_t* feat_cached_table,
                       const int64_t* feat_rows, int32_t F, int32_t B, const int64_t* indices,
                       int64_t N, const int64_t* offsets, int32_t key_bits, int32_t iteration,
                       int64_t* remapped_indices, void* workspace, size_t workspace_bytes,
                       const int64_t* feat_window, void* stream);
int tbe_cache_writeback_staging(const tbe_cache_desc* desc, void* stream);
int tbe_cache_flush(const tbe_cache_desc* desc, int32_t invalidate, void* stream);

/* ------------------------------------------------------------------------------------
 * torch.ops.fbgemm.asynchronous_complete_cumsum (torchrec/sparse/jagged_tensor.py:35-36):
 * out[0] = 0, out[i+1] = sum(in[0..i]); out has n+1 entries.  elem_size 4 (int32) or
 * 8 (int64).  workspace >= tbe_cumsum_workspace_bytes(n).
 * `mode`: 0 = complete (n+1 outputs), 1 = inclusive (n outputs), 2 = exclusive (n outputs)
 * ---------------------------------------------------------------------------------- */
size_t tbe_cumsum_workspace_bytes(int64_t n);
int tbe_cumsum(const void* in, void* out, int64_t n, int32_t elem_size, int32_t mode,
               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * torch.ops.fbgemm.permute_2D_sparse_data (torchrec/sparse/jagged_tensor.py:946-952,
 * torchrec/distributed/dist_data.py:257-263, comm_ops.py:633-639,691-697).
 * Two steps so that the host can size the outputs without a sync when it already
 * knows permuted_lengths_sum:
 *  1. tbe_permute_2d_lengths: out_lengths[t', b] = lengths[permute[t'], b]
 *     and in_offsets / out_offsets = exclusive complete cumsums (T*B+1 / T'*B+1 entries,
 *     int64) written to caller buffers.
 *  2. tbe_permute_2d_data: for each (t', b) copy the segment of `values` (and `weights`).
 * lengths elem size 4 or 8; values/weights element size 1, 2, 4 or 8 bytes (opaque copy).
 * ---------------------------------------------------------------------------------- */
size_t tbe_permute_2d_workspace_bytes(int32_t T_in, int32_t T_out, int32_t B);
int tbe_permute_2d_lengths(const int32_t* permute, int32_t T_in, int32_t T_out, int32_t B,
                           const void* lengths, int32_t len_elem_size, void* out_lengths,
                           int64_t* in_offsets, int64_t* out_offsets, void* workspace,
                           size_t workspace_bytes, void* stream);
int tbe_permute_2d_data(const int32_t* permute, int32_t T_out, int32_t B,
                        const int64_t* in_offsets, const int64_t* out_offsets,
                        const void* values, void* out_values, int32_t val_elem_size,
                        const void* weights, void* out_weights, int32_t w_elem_size,
                        void* stream);

/* ------------------------------------------------------------------------------------
 * torch.ops.fbgemm.permute_1D_sparse_data (torchrec/distributed/dist_data.py:249-255: the
 * recat of a variable-batch KJTAllToAll).  The B = 1 case of permute_2D, in the same two
 * steps: lengths [L] (elem 4|8), permute [P] int32 with entries in [0, L), P need not
 * equal L (entries may repeat or be left out).
 *  1. tbe_permute_1d_lengths: out_lengths[i] = lengths[permute[i]]; in_offsets [L+1] /
 *     out_offsets [P+1] = complete cumsums (int64) written to caller buffers.
 *  2. tbe_permute_1d_data: segment i of out_values (and out_weights) = segment permute[i].
 * The 2-D kernels count segments in `int`: L or P outside [0, 2^31) is
 * TBE_ERR_INVALID_ARGUMENT (workspace query: 0), never a wrapped count.
 * ---------------------------------------------------------------------------------- */
size_t tbe_permute_1d_workspace_bytes(int64_t L, int64_t P);
int tbe_permute_1d_lengths(const int32_t* permute, int64_t L, int64_t P, const void* lengths,
                           int32_t len_elem_size, void* out_lengths, int64_t* in_offsets,
                           int64_t* out_offsets, void* workspace, size_t workspace_bytes,
                           void* stream);
int tbe_permute_1d_data(const int32_t* permute, int64_t P, const int64_t* in_offsets,
                        const int64_t* out_offsets, const void* values, void* out_values,
                        int32_t val_elem_size, const void* weights, void* out_weights,
                        int32_t w_elem_size, void* stream);

/* ------------------------------------------------------------------------------------
 * torch.ops.fbgemm.expand_into_jagged_permute (torchrec/distributed/dist_data.py:110-115:
 * the element-level recat of a variable-batch KJTAllToAll).
 *   out[output_offset[i] + k] = input_offset[permute[i]] + k
 *   for i in [0, P), k in [0, output_offset[i+1] - output_offset[i]).
 * permute [P], input_offset [P+1], output_offset [P+1] and out [output_size] share one
 * element size, 4 (int32) or 8 (int64).  The segment length is read from output_offset; that
 * it equals the input segment's is the caller's contract.  Nothing is stored outside
 * [0, output_size).  P == 0 or output_size == 0 launches nothing.
 * ---------------------------------------------------------------------------------- */
int tbe_expand_into_jagged_permute(const void* permute, const void* input_offset,
                                   const void* output_offset, int64_t P, int64_t output_size,
                                   int32_t elem_size, void* out, void* stream);

/* ------------------------------------------------------------------------------------
 * torch.ops.fbgemm.block_bucketize_sparse_features
 * (torchrec/distributed/embedding_sharding.py:121-184; python reference of the result:
 * torchrec/distributed/tests/test_utils.py:83-236).
 *   bucket = idx / block_sizes[f];  new idx = idx % block_sizes[f]
 *   new_lengths[bucket*F*B + f*B + b] counts; new_indices ordered (bucket, f, b), stable.
 *   indices whose bucket >= my_size are dropped (as the python reference does).
 * lengths [F*B] (elem 4|8), indices [N] (elem 4|8), block_sizes [F] (same elem size as indices)
 * weights [N] float or NULL; out pos [N] (same elem as indices) if bucketize_pos;
 * unbucketize_permute [N] (same elem as indices) if sequence.
 * workspace >= tbe_bucketize_workspace_bytes(F*B, my_size).
 * new_offsets_out: optional int64 [my_size*F*B + 1] complete cumsum of new_lengths
 *   (lets the host read per-bucket totals without recomputing).
 * ---------------------------------------------------------------------------------- */
size_t tbe_bucketize_workspace_bytes(int64_t lengths_size, int32_t my_size);
int tbe_block_bucketize(const void* lengths, int32_t len_elem_size, int64_t lengths_size,
                        const void* indices, int32_t idx_elem_size, int64_t N,
                        const void* block_sizes, int32_t F, int32_t my_size,
                        const float* weights, int32_t bucketize_pos, int32_t sequence,
                        void* new_lengths, void* new_indices, float* new_weights,
                        void* new_pos, void* unbucketize_permute, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Pooled-embedding all-to-all layout ops.  The reference does these with
 * torch split + cat copies (torchrec/distributed/comm_ops.py:555-561 forward,
 * :418-428 `_recat_pooled_embedding_grad_out` backward, flagged slow by its own TODO :417).
 *   tbe_a2a_pooled_unpack : recv[src][B_local][D_src] slabs -> out[B_local, sum D_src]
 *   tbe_a2a_pooled_pack   : grad[B_local, sum D_src]       -> send[src][B_local][D_src]
 * dim_sum_per_rank [W] int32 device array; dims_multiple_of_4 != 0 asserts every entry is a
 * multiple of 4 (enables 16-B accesses); scale multiplies every element (the 1/W gradient
 * division of comm_ops.py:527-528 can be fused here).
 * ---------------------------------------------------------------------------------- */
int tbe_a2a_pooled_unpack(const float* recv, float* out, const int32_t* dim_sum_per_rank,
                          int32_t W, int32_t B_local, int32_t D_total,
                          int32_t dims_multiple_of_4, float scale, void* stream);
int tbe_a2a_pooled_pack(const float* grad, float* send, const int32_t* dim_sum_per_rank,
                        int32_t W, int32_t B_local, int32_t D_total,
                        int32_t dims_multiple_of_4, float scale, void* stream);

/* ------------------------------------------------------------------------------------
 * Mixed table-wise + row-wise pooled exchange through ONE all-to-all (xGMI is point-to-point:
 * an all-to-all drives all 7 links, a ring reduce-scatter is bound by one).  Replaces, on the
 * receiver, All2All_Pooled_Wait's split+cat (torchrec/distributed/comm_ops.py:555-561), the
 * reduce_scatter of row-wise partial pools (comm_ops.py:848-930) and the cross-sharding-type
 * torch.cat (torchrec/distributed/embeddingbag.py:212-223); `pack` is the gradient transpose
 * (comm_ops.py:418-428 recat + :922-927 all_gather), with the 1/W division fused as `scale`.
 *   exchange buffer: W slabs, slab r = [B_local][slab_stride[r]] at element slab_offset[r]
 *   matrix:          [B_local, D_total], global feature g occupies columns
 *                    [feat_out_col[g], feat_out_col[g+1])
 *   feat_src[g] >= 0 : table-wise, lives in slab feat_src[g] at column feat_slab_col[g]
 *   feat_src[g] == -1: row-wise, every slab holds a partial pool at column feat_slab_col[g];
 *                      unpack sums them in rank order 0..W-1, pack broadcasts the gradient.
 *   feat_src[g] <= -2: replicated (data-parallel) feature: its columns are skipped by both
 *                      kernels (a local lookup writes / reads them, see embeddingbag.py).
 * all_multiple_of_4 != 0 asserts every column offset / dim / stride is a multiple of 4.
 * ---------------------------------------------------------------------------------- */
int tbe_pooled_exchange_unpack(const float* recv, float* out, const int32_t* feat_out_col,
                               const int32_t* feat_src, const int32_t* feat_slab_col,
                               const int64_t* slab_offset, const int32_t* slab_stride,
                               int32_t Fg, int32_t W, int32_t B_local, int32_t D_total,
                               int32_t all_multiple_of_4, float scale, void* stream);
int tbe_pooled_exchange_pack(const float* grad, float* send, const int32_t* feat_out_col,
                             const int32_t* feat_src, const int32_t* feat_slab_col,
                             const int64_t* slab_offset, const int32_t* slab_stride,
                             int32_t Fg, int32_t W, int32_t B_local, int32_t D_total,
                             int32_t all_multiple_of_4, float scale, void* stream);

/* ------------------------------------------------------------------------------------
 * permute_pooled_embs: reorders the column segments of a pooled-embedding matrix — the op behind
 * fbgemm_gpu.permute_pooled_embedding_modules.PermutePooledEmbeddings, which the reference's column-wise
 * sharding installs as the callback of its pooled all-to-all
 * (torchrec/distributed/sharding/cw_sharding.py:221-231) to put a table's column shards, which arrive
 * grouped by rank, back next to each other.
 *   in / out [B, D_total] float32, contiguous, distinct buffers; T segments
 *   offset_dim_list [T+1]     int64 device: complete cumsum of the input segments' dims
 *   permute_list [T]          int64 device: output segment i is input segment permute_list[i]
 *   inv_offset_dim_list [T+1] int64 device: complete cumsum of dims[permute_list[i]]
 *   out[:, inv_offset[i]:inv_offset[i+1]] = in[:, offset[permute[i]]:offset[permute[i]+1]]
 * The backward is the same call with (inv_offset_dim_list, inv_permute_list, offset_dim_list).
 * all_multiple_of_4 != 0 asserts every dim is a multiple of 4 (16-B accesses when both pointers are
 * 16-B aligned too; a scalar kernel otherwise).  One launch on `stream`, no synchronisation (capturable
 * into a HIP graph); B * D_total == 0 is TBE_OK without a launch; a T beyond the LDS budget of the
 * staged lists (about 7 000 segments) returns TBE_ERR_UNSUPPORTED.  Inconsistent lists never make the
 * kernel touch memory outside the two matrices: such segments are left unwritten.
 * ---------------------------------------------------------------------------------- */
int tbe_permute_pooled_embs_f32(const float* in, float* out, const int64_t* offset_dim_list,
                                const int64_t* permute_list, const int64_t* inv_offset_dim_list, int32_t T,
                                int32_t B, int32_t D_total, int32_t all_multiple_of_4, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused DLRM dot interaction (the path's only MFMA user): InteractionArch.forward,
 * torchrec/models/dlrm.py:193-219 — cat + bmm(X, X^T) + triu gather + cat — and its autograd
 * backward, each as one kernel on v_mfma_f32_16x16x4_f32 (exact f32).
 *   dense [B, D], sparse [B, F, D] contiguous, out / grad_out [B, D + (F+1)F/2]:
 *   out[b] = [dense[b] | <X_i, X_j> for i < j in torch.triu_indices(F+1, F+1, 1) order],
 *   X = [dense[b]; sparse[b]].
 * forward: 1 <= F <= 31, D in {16, 32, 64, 128, 256}.  backward: F <= 27, D in {16, 32, 64, 128}.
 * out_row_stride / grad_row_stride (elements, >= D + (F+1)F/2): rows of `out` / `grad_out` may be padded.  The
 * reference's dense rows (stride 479 floats at F = 26, D = 128) are not 16-B aligned; with a stride that is a
 * multiple of 4 and leaves room for the pair block rounded up to 4 (480) the forward stores 16 B per lane and
 * writes the pad columns as zeros, and the GEMMs of the next layer read aligned rows (lda = 480, K = 479).
 * Alignment: dense, sparse, grad_dense and grad_sparse 16 B; `out` and `grad_out` need only 4 B.  With P = (F+1)F/2 and
 * P4 = P rounded up to 4, the forward takes its 16-B path exactly when `out` is 16-B aligned, out_row_stride % 4 == 0 and
 * out_row_stride >= D + P4; any other pointer or stride takes 4-B stores.  Columns of a row the forward writes:
 *   16-B path: [0, D + P) and zeros in [D + P, D + P4);   4-B path: [0, D + P).
 * Nothing else is written: columns from D + P4 (16-B path) or D + P (4-B path) up to the stride keep their contents, as
 * does everything outside the B rows.  The backward reads columns [0, D + P) of a grad_out row and nothing beyond (the
 * pad columns may hold anything, NaN included); it reads the first D of them 16 B at a time when grad_out is 16-B
 * aligned and grad_row_stride % 4 == 0, else 4 B at a time.  No call modifies its inputs; B = 0 returns 0 and touches
 * nothing; a non-finite value in one sample changes no other sample's results.  tests/test_interaction_abi_gpu.py holds
 * every statement of this block bit for bit against oracle/dlrm_oracle.c.
 * ---------------------------------------------------------------------------------- */
int tbe_dlrm_interaction_forward_f32(const float* dense, const float* sparse, int32_t B,
                                     int32_t F, int32_t D, float* out, int64_t out_row_stride,
                                     void* stream);
int tbe_dlrm_interaction_backward_f32(const float* dense, const float* sparse,
                                      const float* grad_out, int64_t grad_row_stride, int32_t B, int32_t F, int32_t D,
                                      float* grad_dense, float* grad_sparse, void* stream);

/* The two calls above with the pooled lookup folded in, for a pooling factor of exactly 1 (Criteo): the lookup is then
 * a copy of one table row per (sample, feature) into `sparse`, which the interaction reads straight back; here the
 * interaction kernels fetch the rows from the tables themselves and the pooled buffer does not exist.
 *   feat_weights / feat_rows / feat_window: the [F] / [F] / [2F] layout arrays of tbe_forward_pooled_f32 (every table
 *   of dim D, bases 16-B aligned); indices [F*B] int64, feature-major, ONE id per bag: bag (f, b) owns indices[f*B + b].
 *   X[0] = dense[b], X[r] = W_{r-1}[indices[(r-1)*B + b]] for r >= 1; an id outside the feature's window, TBE_ID_SKIP or
 *   out of range gives a zero row.  out / grad_dense / grad_sparse [B, F*D] are bit-identical to
 *   tbe_forward_pooled_f32 (SUM, no weights) followed by the calls above.
 * bounds_errors: optional device int32 counter, incremented once per id outside [0, global rows).  The backward gathers
 *   the same ids again: pass NULL there so that an id is counted once per step, as on the two-kernel path.
 * 1 <= F <= 27, D in {64, 128}. */
int tbe_dlrm_interaction_gather_forward_f32(const float* dense, const uint64_t* feat_weights, const int64_t* feat_rows,
                                            const int64_t* feat_window, const int64_t* indices, int32_t B, int32_t F,
                                            int32_t D, float* out, int64_t out_row_stride, int32_t* bounds_errors,
                                            void* stream);
int tbe_dlrm_interaction_gather_backward_f32(const float* dense, const uint64_t* feat_weights, const int64_t* feat_rows,
                                             const int64_t* feat_window, const int64_t* indices, const float* grad_out,
                                             int64_t grad_row_stride, int32_t B, int32_t F, int32_t D, float* grad_dense,
                                             float* grad_sparse, int32_t* bounds_errors, void* stream);
/* The gather backward that also applies exact SGD to the once-touched rows: where single[f*B + b] != 0
 * (tbe_backward_single_flags) and the id selects a table row, that row becomes fmaf(-learning_rate, g + 0, w) in place
 * (g = the contribution's gradient row, w = the row as the kernel loaded it) and grad_sparse[b, f*D .. (f+1)*D) is NOT
 * written.  Everything else is tbe_dlrm_interaction_gather_backward_f32, bit for bit; follow it with
 * tbe_backward_apply_skip_single_f32 on the same sort and the tables end exactly as after the plain pair of calls. */
int tbe_dlrm_interaction_gather_backward_sgd_f32(const float* dense, const uint64_t* feat_weights, const int64_t* feat_rows,
                                                 const int64_t* feat_window, const int64_t* indices, const float* grad_out,
                                                 int64_t grad_row_stride, int32_t B, int32_t F, int32_t D, float* grad_dense,
                                                 float* grad_sparse, int32_t* bounds_errors, const uint8_t* single,
                                                 float learning_rate, void* stream);

/* ReLU backward + bias gradient of one MLP layer in one pass (torchrec/modules/mlp.py:14-170 Perceptron
 * trained through autograd: threshold_backward + sum(0)):
 *   grad_in[b, c] = act[b, c] > 0 ? grad_out[b, c] : 0;   bias_grad[c] = sum_b grad_in[b, c]
 * [B, N] row-major, N a multiple of 4, 16-B aligned; column sums in fixed order (deterministic). */
size_t tbe_relu_backward_bias_grad_workspace_bytes(int64_t B, int32_t N);
int tbe_relu_backward_bias_grad_f32(const float* grad_out, const float* act, int64_t B, int32_t N,
                                    float* grad_in, float* bias_grad, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* Weight gradient of a Linear with ONE output feature (DLRM's last layer, torchrec/models/dlrm.py OverArch:
 * `nn.Linear(layer_sizes[-2], 1)`): out[c] = sum_b w[b] * x[b, c] for x [B, N] row-major, w [B] — the
 * N = 1 GEMM the BLAS libraries run at ~1 % of HBM speed.  N a multiple of 4; fixed summation order. */
size_t tbe_weighted_colsum_workspace_bytes(int64_t B, int32_t N);
int tbe_weighted_colsum_f32(const float* x, const float* w, int64_t B, int32_t N, float* out,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The first stages of the two above alone: the column sums of the row blocks stay in `partial`
 * [tbe_colsum_row_blocks(B, N)][N] (16-B aligned, B > 0) for ONE later tbe_multi_chunk_sum_f32 over every layer of a
 * captured backward. */
int64_t tbe_colsum_row_blocks(int64_t B, int32_t N);
int tbe_relu_backward_bias_partials_f32(const float* grad_out, const float* act, int64_t B, int32_t N,
                                        float* grad_in, float* partial, size_t partial_bytes, void* stream);
int tbe_weighted_colsum_partials_f32(const float* x, const float* w, int64_t B, int32_t N, float* partial,
                                     size_t partial_bytes, void* stream);

/* Backward of the last two layers of DLRM's over arch, h = relu(x W1^T + b1) and y = h w^T + b2 with ONE output
 * (torchrec/models/dlrm.py OverArch), in one pass over act = h [B, N], given dy [B] and w [N]:
 *   grad_in[b, c] = act[b, c] > 0 ? dy[b] * w[c] : 0     (the gradient of the hidden layer's pre-activation)
 *   sums[0 .. N)  = sum_b grad_in[b, c]                   (b1's gradient: tbe_relu_backward_bias_grad_f32 of dy w, bit for bit)
 *   sums[N .. 2N) = sum_b dy[b] * act[b, c]               (w's gradient: tbe_weighted_colsum_f32(act, dy), bit for bit)
 * N a multiple of 4, tensors 16-B aligned.  `_partials` is the first stage alone (B > 0): the row blocks' sums stay in
 * `partial` [tbe_colsum_row_blocks(B, N)][2 N] for a later tbe_multi_chunk_sum_*; the other entry finishes them itself
 * (workspace: tbe_relu_linear1_backward_workspace_bytes, B = 0 gives zeros). */
size_t tbe_relu_linear1_backward_workspace_bytes(int64_t B, int32_t N);
int tbe_relu_linear1_backward_f32(const float* act, const float* dy, const float* w, int64_t B, int32_t N, float* grad_in,
                                  float* sums, void* workspace, size_t workspace_bytes, void* stream);
int tbe_relu_linear1_backward_partials_f32(const float* act, const float* dy, const float* w, int64_t B, int32_t N,
                                           float* grad_in, float* partial, size_t partial_bytes, void* stream);

/* dst[off_s + i] = scale * sum_{c < chunks_s} src_s[c * numel_s + i] for every segment s of `seg_table` — device int64
 * [nseg][4] = {src address, chunks, numel, dst element offset}; chunk order fixed (deterministic); chunks = 0 writes
 * zeros.  A segment of at most 16 chunks is added in plain sequence, a longer one in the order of the column sums'
 * second stage (wave w of 4 adds the chunks w, w + 4, ... from 0; the result is ((a0 + a1) + a2) + a3);
 * chunks | TBE_CHUNKS_WAVE_ORDER asks for that order at every count, so that a row-block segment ends as
 * tbe_relu_backward_bias_grad_f32 / tbe_weighted_colsum_f32 end it, bit for bit, 1 row block included.
 * max_numel = the largest numel.  Finishes, in one launch, the split-K weight gradients (chunks = batch slices of
 * the batched GEMM), the bias gradients (chunks = row blocks of the kernels above) and the already complete gradients
 * (chunks = 1) of the dense MLPs' backward, scaled by 1 / world size, into the flat gradient buffer that is all-reduced —
 * what the reference leaves to per-parameter autograd kernels + DistributedDataParallel's bucket copies
 * (torchrec/distributed/model_parallel.py:101-111). */
#define TBE_CHUNKS_WAVE_ORDER (1ll << 62)
int tbe_multi_chunk_sum_f32(const int64_t* seg_table, int32_t nseg, int64_t max_numel, float* dst, float scale,
                            void* stream);
/* The same with the table in HOST memory, at most 32 segments: it travels by value in the kernel arguments (no copy the
 * GPU performs later, so the caller may reuse the host buffer at once) — for eager steps, whose sources and destinations
 * change every step.  With dst = NULL the destination offsets are absolute addresses / 4.  A table in which every segment
 * carries TBE_CHUNKS_WAVE_ORDER (the row-block sums of an eager backward) runs in the second stage's own geometry, 64
 * columns per workgroup, with more loads in flight: same order, same bits. */
int tbe_multi_chunk_sum_host_table_f32(const int64_t* host_seg_table, int32_t nseg, int64_t max_numel, float* dst,
                                       float scale, void* stream);

/* Backward epilogue of one layer of a GEMM-based cross network — CrossNet (torchrec/modules/crossnet.py:19-89, the
 * layer at :85-87) and LowRankCrossNet (:92-188, the layer at :177-186):  x_{l+1} = x_0 * t + x_l,  t = y + b,
 * y = x_l K^T  or  (x_l V^T) W^T.  Given grad_out = dL/dx_{l+1}, ONE pass over [B, N]:
 *   grad_y[b, c] = grad_out[b, c] * x0[b, c]                 (the gradient of y, and of b before its column sum)
 *   acc[b, c]    = grad_out[b, c] * t[b, c]                  if first != 0
 *   acc[b, c]    = acc[b, c] + grad_out[b, c] * t[b, c]      otherwise (the running gradient of x_0)
 *   bias_grad[c] = sum_b grad_y[b, c]                        (row-block sums, then a fixed-order second stage)
 * Each product and each add is rounded on its own; no float atomics; two runs are bit-identical.  The forward of these nets
 * needs no entry: torch.addmm carries the bias and torch.addcmul forms x_0 * t + x_l.
 * fp32, [B, N] row-major and contiguous, N a positive multiple of 4, every base 16-B aligned, no two buffers overlapping;
 * workspace: tbe_cross_backward_workspace_bytes(B, N) bytes.  B == 0 zeroes bias_grad and touches nothing else.
 * Errors, before anything is launched: TBE_ERR_INVALID_ARGUMENT for a bad N, a null or misaligned pointer, a short
 * workspace, or more than 65535 row blocks (B > 65535 * 64 for N < 512, * 256 otherwise). */
size_t tbe_cross_backward_workspace_bytes(int64_t B, int32_t N);
int tbe_cross_backward_f32(const float* grad_out, const float* x0, const float* t, int64_t B, int32_t N, int32_t first,
                           float* grad_y, float* acc, float* bias_grad, void* workspace, size_t workspace_bytes,
                           void* stream);

/* VectorCrossNet (torchrec/modules/crossnet.py:191-268; the layer at :257-266), all L layers in one kernel each way:
 *   s[l, b] = x_l[b, :] . weights[l, :];   x_{l+1} = (x_0 * s[l] + bias[l, :]) + x_l   (the reference's operation order)
 * forward: reads x0 [B, N] once, writes out = x_L [B, N] and s [L, B].
 * backward: reads grad_out, x0 and s, recomputes every x_l in the forward's operation order (bit for bit the forward's) and
 * writes grad_in [B, N] and grad_params [2 L, N]: rows 0 .. L-1 the gradients of bias[l], rows L .. 2L-1 those of
 * weights[l] — row-block sums in `workspace` (tbe_vector_cross_backward_workspace_bytes(B, N, L) bytes), finished in fixed
 * order by one launch over 2 L N columns.  Row dots and column sums run in an order that depends on (B, N, L) only: two
 * runs are bit-identical.  weights, bias: [L, N] (the module stacks its L [N, 1] parameters).
 * Limits: N <= 4096 and a multiple of 4, 1 <= L <= 8; beyond them TBE_ERR_INVALID_ARGUMENT with a message that names the
 * limits, as for a null or misaligned (16 B; s and grad_params 4 B) pointer or a short workspace, before anything is
 * launched.  B == 0: the forward does nothing, the backward zeroes grad_params and touches nothing else. */
size_t tbe_vector_cross_backward_workspace_bytes(int64_t B, int32_t N, int32_t L);
int tbe_vector_cross_forward_f32(const float* x0, const float* weights, const float* bias, int64_t B, int32_t N, int32_t L,
                                 float* out, float* s, void* stream);
int tbe_vector_cross_backward_f32(const float* grad_out, const float* x0, const float* s, const float* weights,
                                  const float* bias, int64_t B, int32_t N, int32_t L, float* grad_in, float* grad_params,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* LowRankMixtureCrossNet (torchrec/modules/crossnet.py:271-446; the layer at :403-444) with the K experts folded into one
 * low-rank layer of rank K r:  sum_k p_k x_0 (U_k h_k + b) = x_0 ([p_1 h_1 | ... | p_K h_K] Ucat^T + b), since the softmax
 * weights p sum to 1.  These two entries are the narrow pass between the folded GEMMs: softmax of the gate logits, the
 * second ReLU, the scale by p_k and the change of layout from the batched expert GEMM's to the Ucat GEMM's.
 *   a2, grad_a2 [K, B, r];  m, grad_m [B, K r];  logits, p, grad_logits [B, K];  all contiguous fp32.
 * With relu(a) = a > 0 ? a : +0, per row b:
 *   forward    mx = max_k logits[b, k];  e_k = expf(logits[b, k] - mx);  s = ((e_0 + e_1) + ...) + e_{K-1}  (k order);
 *              p[b, k] = e_k / s;   m[b, k r + j] = p[b, k] * relu(a2[k, b, j])           (one product, rounded once)
 *   backward   d_k = sum_j grad_m[b, k r + j] * relu(a2[k, b, j])            (a fixed order that depends on r only);
 *              t = ((p_0 d_0 + p_1 d_1) + ...) + p_{K-1} d_{K-1}  (k order);   grad_logits[b, k] = p_k * (d_k - t);
 *              grad_a2[k, b, j] = a2[k, b, j] > 0 ? p_k * grad_m[b, k r + j] : 0
 * Each product and each add is rounded on its own; no float atomics; two runs are bit-identical.  With r % 4 == 0 and every
 * base 16-B aligned the data moves as float4, otherwise as scalars: the choice changes no result bit.
 * Limits: 2 <= K <= 16, 1 <= r <= 2^26, B >= 0.  Errors, before anything is launched: TBE_ERR_INVALID_ARGUMENT, with a
 * message that names the entry, for K or r beyond the limits, a null pointer or a base off the 4-byte grid.  B == 0 is
 * success and touches nothing. */
int tbe_mixture_gate_forward_f32(const float* a2, const float* logits, int64_t B, int32_t K, int32_t r, float* m, float* p,
                                 void* stream);
int tbe_mixture_gate_backward_f32(const float* grad_m, const float* a2, const float* p, int64_t B, int32_t K, int32_t r,
                                  float* grad_a2, float* grad_logits, void* stream);

/* SwishLayerNorm (torchrec/modules/activation.py:18-55):  out = y * sigmoid(LayerNorm(y)) over the N elements of every row of
 * y [B, N], gamma, beta [N], one kernel each way with the row in registers.  Per row b:
 *   forward   mean = (sum_c y[c]) / N;   var = (sum_c (y[c] - mean)^2) / N   (two-pass, never E[y^2] - mean^2)
 *             rstd = 1 / sqrtf(var + eps);   n = (y - mean) * rstd;   z = n * gamma + beta;   s = 1 / (1 + expf(-z))
 *             out = y * s;   stats[0, b] = mean, stats[1, b] = rstd   (stats [2, B]: all the backward needs besides y)
 *   backward  n, z, s recomputed from y and stats in the forward's operation order;   g = grad_out
 *             dz = ((g * y) * s) * (1 - s);   dn = dz * gamma;   c1 = (sum_c dn) / N;   c2 = (sum_c dn * n) / N
 *             grad_y = g * s + rstd * ((dn - c1) - n * c2)
 *             grad_params[0, :] = grad_gamma = sum_b dz * n;   grad_params[1, :] = grad_beta = sum_b dz
 * forward: reads y once, writes out and stats.  backward: reads grad_out, y and stats once, writes grad_y and the row blocks'
 * sums of both parameter gradients into `workspace` (tbe_swish_layernorm_backward_workspace_bytes(B, N) bytes), which one
 * launch over 2 N columns finishes in fixed order.  Each product and each add is rounded on its own; no float atomics; row
 * sums and column sums run in an order that depends on (B, N) only: two runs are bit-identical.  A constant row gives
 * var = 0, n = 0, rstd = 1 / sqrtf(eps); z of large magnitude gives s = exactly 0 or 1; every result stays finite.
 * Limits: fp32, contiguous, N a positive multiple of 4 and <= 4096, eps finite and >= 0; y, gamma, beta, out, grad_out,
 * grad_y and workspace 16-B aligned (stats and grad_params 4 B); no two buffers overlapping.  Errors, before anything is
 * launched: TBE_ERR_INVALID_ARGUMENT, with a message that names the limit, for a bad N or eps, a null or misaligned pointer,
 * a short workspace, or more than 2^31 - 1 row blocks (of 128 rows for N <= 64, 32 for N <= 1024, 16 beyond).
 * B == 0: the forward does nothing, the backward zeroes grad_params and touches nothing else. */
size_t tbe_swish_layernorm_backward_workspace_bytes(int64_t B, int32_t N);
int tbe_swish_layernorm_forward_f32(const float* y, const float* gamma, const float* beta, float eps, int64_t B, int32_t N,
                                    float* out, float* stats, void* stream);
int tbe_swish_layernorm_backward_f32(const float* grad_out, const float* y, const float* stats, const float* gamma,
                                     const float* beta, int64_t B, int32_t N, float* grad_y,
                                     float* grad_params /* [2, N]: gamma row, beta row */, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* DeepFM interaction: the factorization-machine term and the deep branch's concatenated row in one pass each way.
 * Replaces torchrec/modules/deepfm.py:28-32 (_get_flatten_input: torch.cat of all inputs, once per branch), :209-215
 * (FactorizationMachine.forward: x * x, two row sums, a square) and what torchrec/models/deepfm.py:175-184 builds from
 * them, with autograd's backward.
 * The logical row x[b, 0:N] is a list of 1 .. TBE_FM_MAX_SEGMENTS column blocks, each with its own base and row stride (in
 * elements); N = sum of the widths, segment k starts at column off_k = sum of the widths before it.  `segs` and `grads` are
 * HOST arrays: they travel by value in the kernel arguments (no device table, no copy), so both calls can be captured into a
 * HIP graph.  fp32 only.
 *   forward : s = sum_c x[b, c], q = sum_c x[b, c]^2; fm[b * fm_stride] = (s * s - q) * 0.5; row_sum[b] = s;
 *             cat[b, off_k + c] = x_k[b, c] when cat != NULL.  Every input element is read once.
 *   backward: grads[k].g[b, c] = (grad_cat ? grad_cat[b, off_k + c] : 0) + grad_fm[b * grad_fm_stride] * (row_sum[b] - x_k[b, c])
 *             for every segment whose g is not NULL; the others are neither read nor written.
 * A segment moves as 16-byte vectors when its base, row stride, width and (with cat / grad_cat) column offset and N are
 * multiples of 16 bytes / 4 elements (and, backward, its gradient's base and stride), else as 4-byte scalars; one launch
 * may mix both, and the choice changes no result bit.  Sums run in an order that depends on (N, segment geometry) only; no
 * float atomics; two runs are bit-identical.  No buffers may overlap.
 * Errors, before anything is launched: TBE_ERR_INVALID_ARGUMENT for nseg outside 1 .. TBE_FM_MAX_SEGMENTS, a width < 1, a row
 * stride smaller than the width, a null or 4-byte-misaligned pointer, fm_stride / grad_fm_stride < 1, or B beyond 2^31 - 1
 * row blocks of 4 rows.  B == 0 launches nothing and returns TBE_OK. */
#define TBE_FM_MAX_SEGMENTS 8
typedef struct { const float* x; int64_t row_stride; int32_t width; } tbe_fm_segment;   /* elements */
typedef struct { float* g;       int64_t row_stride; }                tbe_fm_grad_segment; /* g may be NULL: not wanted */
/* torchrec/modules/deepfm.py:28-32, 209-215; torchrec/models/deepfm.py:175-184 */
int tbe_fm_forward_f32(const tbe_fm_segment* segs, int32_t nseg, int64_t B,
                       float* fm, int64_t fm_stride,   /* fm[b*fm_stride] = 0.5 * (s*s - q) */
                       float* row_sum,                 /* [B]: s = sum_c x[b,c], kept for the backward */
                       float* cat,                     /* NULL, or [B, N] contiguous: the concatenated row */
                       void* stream);
/* the backward autograd builds for torchrec/modules/deepfm.py:28-32, 209-215 */
int tbe_fm_backward_f32(const tbe_fm_segment* segs, const tbe_fm_grad_segment* grads, int32_t nseg, int64_t B,
                        const float* grad_fm, int64_t grad_fm_stride, const float* row_sum,
                        const float* grad_cat,         /* NULL, or [B, N] contiguous: gradient of `cat` */
                        void* stream);

/* nn.BCEWithLogitsLoss (mean) forward + gradient in one launch — the loss of the reference's train wrapper
 * (examples/dlrm/modules/dlrm_train.py):  loss = mean_i [max(x_i, 0) - x_i y_i + log1p(exp(-|x_i|))],
 * dlogits_i = (sigmoid(x_i) - y_i) / B  (dlogits may be NULL).  labels: float32 (label_elem_size 4) or int64 (8).
 * Deterministic (fixed block ranges, block partials added in index order by the last block).  workspace:
 * tbe_bce_with_logits_workspace_bytes() bytes, 16-B aligned, ZEROED ONCE by the caller before its first use and then
 * reusable launch after launch (the kernel resets its ticket). */
size_t tbe_bce_with_logits_workspace_bytes(void);
int tbe_bce_with_logits_f32(const float* logits, const void* labels, int32_t label_elem_size, int64_t B, float* loss,
                            float* dlogits, void* workspace, size_t workspace_bytes, void* stream);

/* Exact binary AUROC and thresholded accuracy of an evaluation set, as integer counts — what the reference's _evaluate
 * feeds torchmetrics.AUROC / Accuracy for (examples/dlrm/dlrm_main.py:252-265).  preds [n] float32 (probabilities or any
 * score), labels [n] float32 (label_elem_size 4) or int64 (8) with values 0 / 1.  counts: DEVICE int64 [6], 8-B aligned,
 * written (not accumulated) by the call:
 *   0  2U = sum over positives p of ( 2 * #{negatives with x < x_p} + #{negatives with x == x_p} );  AUROC = 2U / (2 P N)
 *   1  P, 2  N (labels equal to 1 / 0),  3  n_correct = #{ (x >= threshold) == (label == 1) },
 *   4  n_nan (NaN predictions),  5  n_bad_label (labels that are neither 0 nor 1)
 * -0.0 ties with +0.0, the infinities are ordinary values, denormals are not flushed.  With n_nan > 0 or n_bad_label > 0
 * slots 0 .. 3 are unspecified.  Integer arithmetic only: two runs are bit-identical.  The inputs are not modified; keys,
 * payloads and scratch live in `workspace` (tbe_auroc_workspace_bytes(n) bytes, 256-B aligned, no zeroing needed).
 * n == 0 is legal (preds / labels may be NULL then; all six counters are 0).
 * Errors, before anything is launched: TBE_ERR_INVALID_ARGUMENT for n < 0, n >= 2^29 (the pair sort's limit;
 * tbe_auroc_workspace_bytes returns 0), a label_elem_size other than 4 / 8, a null or misaligned pointer;
 * TBE_ERR_WORKSPACE for a short workspace.  A give-up inside the sort is reported through tbe_fault_status. */
/* examples/dlrm/dlrm_main.py:252-265 */
size_t tbe_auroc_workspace_bytes(int64_t n);
/* examples/dlrm/dlrm_main.py:252-265 */
int tbe_auroc_counts_f32(const float* preds, const void* labels, int32_t label_elem_size, int64_t n, float threshold,
                         int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* torch.ops.fbgemm.jagged_2d_to_dense (examples/bert4rec/models/bert4rec.py:394-400):
 * values [N, D] + offsets [B+1] -> dense [B, max_L, D], zero padded / truncated. */
int tbe_jagged_2d_to_dense_f32(const float* values, const int64_t* offsets, int32_t B,
                               int32_t D, int32_t max_L, float* dense, void* stream);

/* Gradient of the above: values_grad [N, D] <- dense_grad [B, max_L, D] (rows beyond max_L get 0). */
int tbe_dense_to_jagged_2d_f32(const float* dense, const int64_t* offsets, int32_t B, int32_t D,
                               int32_t max_L, int64_t N, float* values, void* stream);

/* torch.ops.fbgemm.offsets_range (torchrec/modules/feature_processor.py:65):
 * out[i] = i - offsets[bag(i)] for i in [0, range_size). offsets has n entries (no total). */
int tbe_offsets_range(const int64_t* offsets, int64_t n, int64_t range_size, int64_t* out,
                      void* stream);

/* dst[y, :] = src[rows[y], :] for y in [0, n_rows): rows of `row_bytes` bytes (a multiple of 16, 16-byte aligned bases).
 * The send-order gather of the input exchange when every feature has the same number of ids per batch (the
 * reference permutes the whole KJT: torchrec/distributed/dist_data.py:257-263); `rows` is a device int32 array whose
 * entries the caller guarantees are < src_rows (not checked on the device). */
int tbe_copy_rows(const void* src, int64_t src_rows, const int32_t* rows, int32_t n_rows,
                  int64_t row_bytes, void* dst, void* stream);

/* Fused masked attention of BERT4Rec (examples/bert4rec/models/bert4rec.py:72-82 inside :152-170), float32, one launch
 * each way.  Per sample b and head h:
 *   S = Q K^T / sqrt(d);  S[:, j] = -1e9 where key j is not valid;  P = softmax_j(S);  P~ = dropout(P);  O = P~ V
 * Layout: q, k, v are logically [B, L, H, d], read where they are: element (b, l, h, c) sits at
 *   base + b * batch_stride + l * row_stride + h * d + c          (strides in floats, given per tensor, multiples of 4)
 * out, grad_out, dq, dk, dv are contiguous [B, L, H * d]; lse is [B, H, L].  All float pointers 16-B aligned (lse: 4-B).
 * Mask: key_valid is uint8 [B, L], non-zero = valid; NULL = every key valid.  Masked keys get the finite -1e9 (the
 *   reference's masked_fill), so a sample with no valid key yields the uniform 1 / L over all L keys and O = mean of V.
 *   In the backward dS is 0 at every masked key (masked_fill cuts the gradient): such a sample has dQ = 0, adds nothing to
 *   dK, and its dV = P~^T dO.
 * Softmax: the row maximum is subtracted.  The forward writes lse[b, h, i] = max_j S_ij + log sum_j exp(S_ij - max), the only
 *   state kept; the backward recomputes P = exp(S - lse) (1 / L for a sample with no valid key, where -1e9 absorbs log L),
 *   D_i = sum_j P~_ij (dO_i . V_j) = dO_i . O_i,  dP = keep * scale * (dO V^T),  dS = P * (dP - D_i) / sqrt(d),
 *   dQ = dS K,  dK = dS^T Q,  dV = P~^T dO.  dq / dk / dv may each be NULL (not wanted: not computed).
 *   No [L, L] tensor reaches global memory.
 * Dropout, 0 <= p < 1: with uint32 arithmetic (wrapping), fmix32 the murmur3 finalizer
 *       fmix32(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16
 *   and  c   = fmix32(fmix32(fmix32(fmix32(lo32(seed) ^ 0x9e3779b9) ^ hi32(seed)) ^ lo32(call)) ^ hi32(call))
 *        w1  = fmix32(c  ^ ((b * H + h) * 0x9e3779b1))
 *        w2  = fmix32(w1 ^ (i * 0x85ebca6b))
 *        r   = fmix32(w2 ^ (j * 0xc2b2ae35))
 *   element (b, h, i, j) is kept iff r >= min(2^32 - 1, floor((double)p * 2^32)); kept elements are multiplied by the float
 *   1 / (1 - p).  The draw depends on (seed, call, b, H, h, i, j) only; the backward regenerates it from the same arguments.
 *   p == 0 keeps everything, multiplies by nothing, and (seed, call) do not matter.
 * Determinism: no atomics, every sum in an order fixed by (L, d); two runs are bit-identical.
 * Supported (tbe_attention_supported returns 1): d % 4 == 0, 4 <= d <= 128, 1 <= L <= 256, and the LDS image
 *   4 * (2 L (d + 4) + 33 * roundup(L, 4)) bytes within 160 KiB — (100, 128), (200, 64), (256, 32), (137, 128) are inside.
 * Errors, before anything is launched and with no byte changed: TBE_ERR_INVALID_ARGUMENT for a null or misaligned pointer,
 *   B < 0, H / L / d < 1, an unsupported (L, d), a row stride below H * d, a batch stride below (L - 1) * row_stride + H * d,
 *   a stride that is no multiple of 4, p outside [0, 1), B * H beyond 2^31 - 1.  B == 0 launches nothing: TBE_OK. */
int tbe_attention_supported(int64_t L, int64_t d);
/* examples/bert4rec/models/bert4rec.py:72-82, 152-170 */
int tbe_attention_forward_f32(const float* q, int64_t q_batch_stride, int64_t q_row_stride,
                              const float* k, int64_t k_batch_stride, int64_t k_row_stride,
                              const float* v, int64_t v_batch_stride, int64_t v_row_stride,
                              const uint8_t* key_valid, int64_t B, int32_t H, int32_t L, int32_t d,
                              float p, uint64_t seed, int64_t call, float* out, float* lse, void* stream);
/* the backward autograd builds for examples/bert4rec/models/bert4rec.py:72-82, 152-170 */
int tbe_attention_backward_f32(const float* grad_out,
                               const float* q, int64_t q_batch_stride, int64_t q_row_stride,
                               const float* k, int64_t k_batch_stride, int64_t k_row_stride,
                               const float* v, int64_t v_batch_stride, int64_t v_row_stride,
                               const uint8_t* key_valid, const float* lse, int64_t B, int32_t H, int32_t L, int32_t d,
                               float p, uint64_t seed, int64_t call, float* dq, float* dk, float* dv, void* stream);

/* JaggedTensor.to_padded_dense (torchrec/sparse/jagged_tensor.py:344-363) in one launch: out [B, N] float32 from the bags
 * values[offsets[b] .. offsets[b + 1]).  A bag of at most N values is padded with padding_value: in front of the values
 * (right-aligned values) with pad_from_beginning, behind them otherwise.  A longer bag keeps its LAST N values with
 * chop_from_beginning, its first N otherwise.  Integer values are converted as torch's cast does (round to nearest even:
 * 2^24 + 1 -> 16777216.0).  values may be NULL when every bag is empty; the entry cannot check that (the offsets are on
 * the device): a NULL values with any non-empty bag is undefined behaviour.  B == 0 or N == 0 launches nothing. */
/* torchrec/sparse/jagged_tensor.py:303-364 */
int tbe_jagged_to_padded_dense_i64(const int64_t* values, const int64_t* offsets, int32_t B, int32_t N, float padding_value,
                                   int32_t pad_from_beginning, int32_t chop_from_beginning, float* out, void* stream);
/* torchrec/sparse/jagged_tensor.py:303-364 */
int tbe_jagged_to_padded_dense_i32(const int32_t* values, const int64_t* offsets, int32_t B, int32_t N, float padding_value,
                                   int32_t pad_from_beginning, int32_t chop_from_beginning, float* out, void* stream);
/* torchrec/sparse/jagged_tensor.py:303-364 */
int tbe_jagged_to_padded_dense_f32(const float* values, const int64_t* offsets, int32_t B, int32_t N, float padding_value,
                                   int32_t pad_from_beginning, int32_t chop_from_beginning, float* out, void* stream);

/* Cross-entropy over class indices with ignore_index — nn.CrossEntropyLoss(ignore_index=0) of the BERT4Rec trainer
 * (examples/bert4rec/bert4rec_main.py:278-295) and the backward autograd builds for it.  input [R, V] float32 with inner
 * stride 1 and row_stride >= V (elements), target [R] int64, reduction 0 = mean, 1 = sum, 2 = none.
 *   forward : a row whose target is ignore_index is NOT READ: its stats and its loss are 0.  Every other row is streamed once
 *             with a running (max, sum) pair:  stats[0, r] = m = max_v x[r, v],  stats[1, r] = ls = logf(sum_v expf(x[r, v] - m)),
 *             row loss = (m - x[r, t]) + ls.  stats [2, R] is all the backward needs besides input and target; the
 *             log-sum-exp m + ls stays in two terms because one float32 would lose ls below the ulp of m (1e-3 at 1e4).
 *             One finishing launch (one workgroup) writes n_valid[0] = #{r : target[r] != ignore_index}, an exact int64, and
 *             loss[0] = sum of the row losses (sum) or that sum / (float)n_valid (mean: 0 / 0 = NaN when no row is valid, R == 0
 *             included).  none: loss is [R] and holds the row losses.  mean / sum keep the row losses in `workspace`
 *             (tbe_cross_entropy_workspace_bytes(R) bytes, 16-B aligned, no zeroing needed); none does not look at it.
 *   backward: grad_input[r, v] = (expf((x[r, v] - m) - ls) - [v == t]) * s  with  s = grad_out[0] / (float)n_valid[0] (mean),
 *             grad_out[0] (sum), grad_out[r] (none);  exact zeros in the rows whose target is ignore_index, which are not read.
 *             n_valid is read on the device: neither call waits for the host, both can be captured into a HIP graph.
 *             grad_input has its own row stride (>= V) and may not overlap anything.
 * A target outside [0, V) that is not ignore_index forms no address: the row's stats, its loss and its gradient row are NaN (and
 * so is a mean / sum loss); it counts as valid.  -inf entries are ordinary values (probability 0, gradient 0); a row that
 * holds NaN or +inf, or -inf only, yields non-finite values.
 * Geometry, a function of V only: 16 threads per row and 16 rows per workgroup for V <= 256, a wave per row and 4 rows per
 * workgroup for V <= 4096, the workgroup (256 threads) per row beyond.  Columns are taken in groups of 4; group g belongs to
 * thread g % (threads per row), which folds its groups in ascending order, 4 groups (16 columns) per fold; the threads' pairs
 * meet in a butterfly over the wave and then in wave order.  The row losses are summed by thread r % 256 in ascending r, then
 * butterfly and wave order: an order that depends on R only.  A group moves as one 16-byte access where its address allows,
 * as 8 + 8 or 4 + 8 + 4 bytes elsewhere (V % 4 != 0, odd strides); the choice changes no bit: the results depend on (R, V) and
 * the values only, not on base alignment or row stride.  Each product and add is rounded on its own; no atomics; two runs
 * are bit-identical.
 * Errors, before anything is launched and with no byte changed: TBE_ERR_INVALID_ARGUMENT for R < 0, V < 1, a reduction
 * outside 0 .. 2, a row stride below V, a null pointer, a float pointer off the 4-byte grid (target, n_valid: 8 bytes;
 * workspace: 16), a workspace shorter than tbe_cross_entropy_workspace_bytes(R) (mean / sum), more than 2^31 - 1 row blocks.
 * R == 0: the forward runs the finishing launch only, the backward does nothing. */
/* examples/bert4rec/bert4rec_main.py:278-295 */
size_t tbe_cross_entropy_workspace_bytes(int64_t R);
/* examples/bert4rec/bert4rec_main.py:278-295 */
int tbe_cross_entropy_forward_f32(const float* input, int64_t row_stride, const int64_t* target, int64_t R, int32_t V,
                                  int64_t ignore_index, int32_t reduction, float* stats /* [2, R] */,
                                  float* loss /* [1]; none: [R] */, int64_t* n_valid /* [1] */, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* the backward autograd builds for examples/bert4rec/bert4rec_main.py:278-295 */
int tbe_cross_entropy_backward_f32(const float* grad_out /* [1]; none: [R] */, const float* input, int64_t row_stride,
                                   const int64_t* target, const float* stats, const int64_t* n_valid, int64_t R, int32_t V,
                                   int64_t ignore_index, int32_t reduction, float* grad_input, int64_t grad_row_stride,
                                   void* stream);

/* Recall@k and NDCG@k of B candidate lists — recalls_and_ndcgs_for_ks (examples/bert4rec/bert4rec_metrics.py:13-61) with the
 * score gather in front of it (examples/bert4rec/bert4rec_main.py:244-245) — in one kernel and one finishing launch, no sort.
 * scores: float32, inner stride 1, score_row_stride (elements) >= the row width.  candidates == NULL: scores is [B, C].
 * Otherwise scores is [B, V] and candidates [B, C] int64 (contiguous): list entry i of row b is scores[b, candidates[b, i]].
 * labels [B, C] contiguous: uint8 / bool (label_elem_size 1), float32 (4) or int64 (8), values 0 / 1.
 * ks: HOST array of nk distinct, ascending k with 1 <= k <= C (copied into the kernel arguments: the call can be captured).
 * weights: DEVICE float32 [ks[nk - 1]], w[p] = 1 / log2(p + 2) as the caller computed it (the reference's expression,
 * bert4rec_metrics.py:50-51); no logarithm is taken on the device.
 * Per row, with s the list's scores:  pos_j = #{i : s_i > s_j} + #{i < j : s_i == s_j}  for every positive j — its place in
 * np.argsort(-s, kind="stable").  TIE RULE: ties go to the lower index, -0.0 ties with +0.0, a NaN ranks behind every number
 * and NaNs keep index order (the reference's unstable sort leaves ties to chance).  For each k, n_pos the row's positives:
 *   hits = #{j positive : pos_j < k};  Recall = hits / min(k, n_pos);  DCG = sum of w[pos_j] over those hits in ascending
 *   pos_j;  IDCG = sum of w[0 : min(k, n_pos)];  NDCG = DCG / IDCG.  Both sums run in float64, where they are exact for this
 *   table and k <= 8192, so their order changes nothing.  A row without a positive yields NaN, and so does the mean.
 * metrics: DEVICE float32 [2 nk] = {Recall@k_0 .., NDCG@k_0 ..}: the float32 rounding of the float64 mean over the rows, taken
 * in an order that depends on B only.  counts: DEVICE int64 [2] = {candidates outside [0, V), labels outside {0, 1}}; such a
 * candidate is never an address (its score is NaN) and such a label never a hit (it is 0): with a non-zero count the
 * metrics are unspecified.  Integer compares and fixed orders only, no atomics: two runs are bit-identical.
 * workspace: tbe_rank_metrics_workspace_bytes(B, nk) bytes, 256-B aligned, no zeroing needed.  It holds the per-row
 * results: float32 row_values [B, 2 nk] (the layout of metrics) at offset 0 and, at the next multiple of 256 bytes, int32
 * row_counts [B, 10] = {bad candidates, bad labels, hits of k_0 .. k_7}.
 * Limits: 1 <= C <= 8192, 1 <= nk <= 8, 0 <= B <= 2^31 - 1.  Errors, before anything is launched and with no byte changed:
 * TBE_ERR_INVALID_ARGUMENT for a value beyond a limit, a k outside 1 .. C or out of order, a label_elem_size other than
 * 1 / 4 / 8, V < 1 with candidates, a row stride below the row width, a null or misaligned pointer; TBE_ERR_WORKSPACE for a
 * short workspace (tbe_rank_metrics_workspace_bytes returns 0 for B or nk beyond the limits).  B == 0 is legal: the metrics
 * are NaN (the mean of nothing), the counts 0. */
/* examples/bert4rec/bert4rec_metrics.py:13-61 */
size_t tbe_rank_metrics_workspace_bytes(int64_t B, int32_t nk);
/* examples/bert4rec/bert4rec_metrics.py:13-61; examples/bert4rec/bert4rec_main.py:244-245 */
int tbe_rank_metrics_f32(const float* scores, int64_t score_row_stride, const int64_t* candidates, int64_t V,
                         const void* labels, int32_t label_elem_size, int64_t B, int32_t C, const int32_t* ks, int32_t nk,
                         const float* weights, float* metrics, int64_t* counts, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Criteo batch builder: raw rows of the preprocessed day files -> dense_features, feature-major hashed ids and labels of one
 * batch, in one launch.  It replaces, on the device, what the reference does per batch on the host: np.concatenate of the
 * file slices (torchrec/datasets/criteo.py:798), the three fancy-index gathers under the batch's permutation, the strided
 * `sparse.transpose(1, 0).reshape(-1)` copy and `labels.reshape(-1)` (_np_arrays_to_batch, criteo.py:760-784), the
 * load-time `sparse_arr %= hashes` (criteo.py:755-758) and the later `.long()` of the ids
 * (fbgemm_gpu/split_table_batched_embeddings_ops.py:565-566).
 * segs: HOST array of nseg in 0 .. TBE_CRITEO_MAX_SEGMENTS descriptors, copied BY VALUE into the kernel arguments (no device
 *   table: the call can be captured into a HIP graph).  A segment is `rows` consecutive rows of one file, as DEVICE pointers
 *   to row-major dense [rows, 13] float32, sparse [rows, 26] int32 and labels [rows, 1] int32, each 4-byte aligned (a row
 *   range starts wherever its first row does: no wider alignment is asked for).  The batch's source rows are numbered by
 *   running through the segments in order; a segment with rows == 0 is skipped and its pointers are not looked at.
 * B: rows of the batch; must equal the sum of the segment rows.
 * hashes: DEVICE int32 [26], every entry in [1, 2^31 - 1] (the caller checks: the array lives on the device), or NULL: ids
 *   pass through, sign-extended.  perm: DEVICE int64 [B] or NULL (identity).  bad_perm: DEVICE int32 counter or NULL.
 * Output row j takes source row s = perm ? perm[j] : j:
 *   dense_out[j, 0:13] = dense[s, 0:13];  labels_out[j] = labels[s, 0];
 *   values_out[f * B + j] = floormod(sparse[s, f], hashes[f]) widened to the output type (feature-major, the layout of a
 *   KeyedJaggedTensor with one id per bag), where floormod is numpy's: r = v % h; r += r < 0 ? h : 0, in 32-bit signed
 *   arithmetic (no overflow for h <= 2^31 - 1): -7 mod 3 = 2, -2^31 mod (2^31 - 1) = 2^31 - 2.
 * A perm[j] outside [0, B) forms no address: row j of all three outputs is written as zeros and *bad_perm is incremented (the
 * library's rule for bad ids; the only atomic).  Repeats in perm are legal.  Everything is a copy or an integer operation:
 * the result bits depend on neither alignment, segmentation nor the tile (TBE_CRITEO_TILE_ROWS output rows per workgroup).
 * Errors, before anything is launched and with no byte changed: TBE_ERR_INVALID_ARGUMENT for nseg outside
 * 0 .. TBE_CRITEO_MAX_SEGMENTS, a negative B or rows, a null or 4-byte-misaligned pointer in a segment with rows > 0, B not the
 * sum of the segment rows, a null or misaligned output, 26 * B beyond 2^31 - 1 for the _i32 entry, more than 2^31 - 1 row
 * tiles.  B == 0 launches nothing and returns TBE_OK. */
#define TBE_CRITEO_MAX_SEGMENTS 8
#define TBE_CRITEO_TILE_ROWS 64
typedef struct { const float* dense; const int32_t* sparse; const int32_t* labels; int64_t rows; } tbe_criteo_segment;
/* torchrec/datasets/criteo.py:760-784 */
int tbe_criteo_batch_i64(const tbe_criteo_segment* segs, int32_t nseg, int64_t B, const int32_t* hashes, const int64_t* perm,
                         float* dense_out, int64_t* values_out, int32_t* labels_out, int32_t* bad_perm, void* stream);
/* torchrec/datasets/criteo.py:760-784; values as int32, the dtype of the reference's host batches */
int tbe_criteo_batch_i32(const tbe_criteo_segment* segs, int32_t nseg, int64_t B, const int32_t* hashes, const int64_t* perm,
                         float* dense_out, int32_t* values_out, int32_t* labels_out, int32_t* bad_perm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TBE_HIP_H_ */
