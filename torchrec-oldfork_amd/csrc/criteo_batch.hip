// Criteo batch builder on gfx950: raw rows of the preprocessed day files -> the tensors the model consumes, in one launch.
//
// Reference: torchrec/datasets/criteo.py — _load_data_for_rank :755-758 (`sparse_arr %= hashes`, numpy's floor modulo),
// __iter__ :798 (np.concatenate of the file slices of one batch) and _np_arrays_to_batch :760-784 (three fancy-index
// gathers under the batch's permutation, `sparse.transpose(1, 0).reshape(-1)`, `labels.reshape(-1)`); the ids are widened
// to int64 later, on the device (fbgemm_gpu/split_table_batched_embeddings_ops.py:565-566).  All of that is host work on
// the training thread there.  Here the rows stay raw, a batch is up to TBE_CRITEO_MAX_SEGMENTS row ranges that travel BY
// VALUE in the kernel arguments (no device table, no copy: the launch can be captured into a HIP graph), and one kernel
// hashes, shuffles, transposes and widens.  Every operation is a copy or an integer operation: results are exact.
//
// A workgroup of 256 threads owns a tile of T = TBE_CRITEO_TILE_ROWS consecutive OUTPUT rows.
//   phase 0: thread r < T resolves output row j = tile + r: source row s = perm ? perm[j] : j, then a linear scan of the
//            by-value descriptors turns s into (segment, row inside it); the three row addresses go to LDS.  An s outside
//            [0, B) forms no address: the row is marked bad, counted in bad_perm, and written as zeros below.
//   phase 1: the tile's T * 26 ids in row-major order, one dword load each — without perm consecutive threads read
//            consecutive dwords of a segment piece, with perm each row is a 104-byte run; dword loads, because a sparse row
//            range starts 16-byte aligned at even rows only.  The id is hashed on the way in and stored to an LDS tile whose
//            row stride is 27 dwords.
//   phase 2: each of the 26 columns leaves as T consecutive output elements (one wave per column: the stores coalesce).
//            Lane r reads LDS dword r * 27 + c with ds_read_b32, whose bank is (dword index) mod 32 within each 32-lane half
//            of the wave: stride 27 is odd, so the 32 lanes of a half fall on 32 different banks (no conflict); stride 26
//            shares a factor 2 with 32 and would put two lanes on every other bank (a 2-way conflict).
//   dense and labels are row-major on both sides: copied dword by dword, gathered by row through the addresses of phase 0
//            (dense rows are 52 bytes: 4 bytes off every wider grid).
// No atomics but the bad_perm counter; the result bits depend on neither alignment, segmentation nor T.
#include "common.hpp"

namespace tbe {

constexpr int kCriteoTile = TBE_CRITEO_TILE_ROWS;
constexpr int kCriteoDense = 13;
constexpr int kCriteoCat = 26;
constexpr int kCriteoLdsStride = kCriteoCat + 1;  // odd: the column reads of phase 2 are conflict-free

struct CriteoArgs {
  tbe_criteo_segment seg[TBE_CRITEO_MAX_SEGMENTS];  // rows == 0 beyond nseg
};

// numpy's floor modulo for h in [1, 2^31 - 1], in 32-bit signed arithmetic: |v % h| < h, so the add cannot overflow
__device__ __forceinline__ int32_t floormod(int32_t v, int32_t h) {
  int32_t r = v % h;
  r += r < 0 ? h : 0;
  return r;
}

template <typename OutT>
__global__ __launch_bounds__(256) void criteo_batch_kernel(const CriteoArgs a, int64_t B, const int32_t* __restrict__ hashes,
                                                           const int64_t* __restrict__ perm, float* __restrict__ dense_out,
                                                           OutT* __restrict__ values_out, int32_t* __restrict__ labels_out,
                                                           int32_t* __restrict__ bad_perm) {
  __shared__ int32_t tile[kCriteoTile * kCriteoLdsStride];
  __shared__ const int32_t* sparse_row[kCriteoTile];  // nullptr: a bad perm entry, the row is written as zeros
  __shared__ const float* dense_row[kCriteoTile];
  __shared__ const int32_t* label_row[kCriteoTile];
  __shared__ int32_t hash_s[kCriteoCat];

  const int tid = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kCriteoTile;
  const int n = static_cast<int>(B - row0 < kCriteoTile ? B - row0 : kCriteoTile);  // rows of this tile: 1 .. T

  // phase 0
  if (tid < n) {
    const int64_t j = row0 + tid;
    int64_t s = perm != nullptr ? perm[j] : j;
    const int32_t* sp = nullptr;
    const float* dn = nullptr;
    const int32_t* lb = nullptr;
    if (static_cast<uint64_t>(s) < static_cast<uint64_t>(B)) {
#pragma unroll
      for (int k = 0; k < TBE_CRITEO_MAX_SEGMENTS; ++k) {
        const int64_t rows = a.seg[k].rows;
        if (sp == nullptr && s < rows) {  // rows == 0 never takes a row; the host checked that the rows sum to B
          sp = a.seg[k].sparse + s * kCriteoCat;
          dn = a.seg[k].dense + s * kCriteoDense;
          lb = a.seg[k].labels + s;
        }
        s -= rows;
      }
    } else if (bad_perm != nullptr) {
      atomicAdd(bad_perm, 1);
    }
    sparse_row[tid] = sp;
    dense_row[tid] = dn;
    label_row[tid] = lb;
  }
  if (tid >= 64 && tid < 64 + kCriteoCat) hash_s[tid - 64] = hashes != nullptr ? hashes[tid - 64] : 0;
  __syncthreads();

  // phase 1
  for (int i = tid; i < n * kCriteoCat; i += 256) {
    const int r = i / kCriteoCat, c = i - r * kCriteoCat;
    const int32_t* sp = sparse_row[r];
    int32_t v = 0;
    if (sp != nullptr) {
      v = sp[c];
      if (hashes != nullptr) v = floormod(v, hash_s[c]);
    }
    tile[r * kCriteoLdsStride + c] = v;
  }
  // dense and labels meanwhile: they do not go through the tile
  for (int i = tid; i < n * kCriteoDense; i += 256) {
    const int r = i / kCriteoDense, c = i - r * kCriteoDense;
    const float* dn = dense_row[r];
    dense_out[row0 * kCriteoDense + i] = dn != nullptr ? dn[c] : 0.f;
  }
  if (tid < n) {
    const int32_t* lb = label_row[tid];
    labels_out[row0 + tid] = lb != nullptr ? *lb : 0;
  }
  __syncthreads();

  // phase 2
  for (int i = tid; i < n * kCriteoCat; i += 256) {
    const int c = i / n, r = i - c * n;
    values_out[static_cast<int64_t>(c) * B + row0 + r] = static_cast<OutT>(tile[r * kCriteoLdsStride + c]);
  }
}

static bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <typename OutT>
static int criteo_batch(const char* what, const tbe_criteo_segment* segs, int32_t nseg, int64_t B, const int32_t* hashes,
                        const int64_t* perm, float* dense_out, OutT* values_out, int32_t* labels_out, int32_t* bad_perm,
                        void* stream) {
  TBE_REQUIRE(nseg >= 0 && nseg <= TBE_CRITEO_MAX_SEGMENTS, "%s: nseg=%d must be in 0 .. %d", what, nseg,
              TBE_CRITEO_MAX_SEGMENTS);
  TBE_REQUIRE(nseg == 0 || segs != nullptr, "%s: null segment list", what);
  TBE_REQUIRE(B >= 0, "%s: B=%lld is negative", what, (long long)B);
  CriteoArgs a;
  int64_t total = 0;
  for (int k = 0; k < TBE_CRITEO_MAX_SEGMENTS; ++k) {
    a.seg[k] = tbe_criteo_segment{nullptr, nullptr, nullptr, 0};
    if (k >= nseg) continue;
    const tbe_criteo_segment& s = segs[k];
    TBE_REQUIRE(s.rows >= 0, "%s: segment %d has rows=%lld, negative", what, k, (long long)s.rows);
    TBE_REQUIRE(s.rows <= (1ll << 40), "%s: segment %d has rows=%lld, too large", what, k, (long long)s.rows);
    if (s.rows == 0) continue;  // skipped: its pointers are never looked at
    TBE_REQUIRE(s.dense && s.sparse && s.labels, "%s: segment %d: null pointer with rows=%lld", what, k, (long long)s.rows);
    TBE_REQUIRE(aligned_to(s.dense, 4) && aligned_to(s.sparse, 4) && aligned_to(s.labels, 4),
                "%s: segment %d: 4-byte-misaligned pointer", what, k);
    a.seg[k] = s;
    total += s.rows;
  }
  TBE_REQUIRE(total == B, "%s: B=%lld is not the sum of the segment rows, %lld", what, (long long)B, (long long)total);
  if (sizeof(OutT) == 4) {
    TBE_REQUIRE(kCriteoCat * B < (1ll << 31), "%s: B=%lld too large: 26 * B beyond 2^31 - 1 int32 ids", what, (long long)B);
  }
  TBE_REQUIRE((B + kCriteoTile - 1) / kCriteoTile < (1ll << 31), "%s: B=%lld too large (more than 2^31 - 1 row tiles)", what,
              (long long)B);
  if (B == 0) return TBE_OK;
  TBE_REQUIRE(dense_out && values_out && labels_out, "%s: null output pointer", what);
  TBE_REQUIRE(aligned_to(dense_out, 4) && aligned_to(values_out, sizeof(OutT)) && aligned_to(labels_out, 4) &&
                  aligned_to(hashes, 4) && aligned_to(perm, 8) && aligned_to(bad_perm, 4),
              "%s: misaligned dense_out / values_out / labels_out / hashes / perm / bad_perm", what);
  const dim3 grid(static_cast<unsigned>((B + kCriteoTile - 1) / kCriteoTile));
  hipLaunchKernelGGL((criteo_batch_kernel<OutT>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), a, B, hashes, perm,
                     dense_out, values_out, labels_out, bad_perm);
  TBE_CHECK_LAUNCH(what);
  return TBE_OK;
}

}  // namespace tbe

extern "C" int tbe_criteo_batch_i64(const tbe_criteo_segment* segs, int32_t nseg, int64_t B, const int32_t* hashes,
                                    const int64_t* perm, float* dense_out, int64_t* values_out, int32_t* labels_out,
                                    int32_t* bad_perm, void* stream) {
  return tbe::criteo_batch<int64_t>("tbe_criteo_batch_i64", segs, nseg, B, hashes, perm, dense_out, values_out, labels_out,
                                    bad_perm, stream);
}

extern "C" int tbe_criteo_batch_i32(const tbe_criteo_segment* segs, int32_t nseg, int64_t B, const int32_t* hashes,
                                    const int64_t* perm, float* dense_out, int32_t* values_out, int32_t* labels_out,
                                    int32_t* bad_perm, void* stream) {
  return tbe::criteo_batch<int32_t>("tbe_criteo_batch_i32", segs, nseg, B, hashes, perm, dense_out, values_out, labels_out,
                                    bad_perm, stream);
}
