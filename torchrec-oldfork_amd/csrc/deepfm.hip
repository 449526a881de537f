// DeepFM interaction on gfx950: the factorization-machine term and the concatenated row of the deep branch in one pass each
// way.
//
// Reference: torchrec/modules/deepfm.py — _get_flatten_input :28-32 (torch.cat of every input, once per branch) and
// FactorizationMachine.forward :209-215 (x * x, two row sums, a square, a subtraction) — and torchrec/models/deepfm.py
// :175-184 (FMInteractionArch: the list goes through both branches); the backward is autograd's, which expands, multiplies
// and adds three gradients into every input.
//
// Here the logical row x[b, 0:N] is a short list of SEGMENTS (column blocks, each with its own base and row stride) that
// travels BY VALUE in the kernel arguments: no device table, no copy, so both launches can be captured into a HIP graph.
//
//   forward :  s = sum_c x[b, c],  q = sum_c x[b, c]^2,  fm[b] = (s * s - q) * 0.5,  row_sum[b] = s,  cat[b, :] = x[b, :]
//   backward:  g_k[b, c] = grad_cat[b, off_k + c] + grad_fm[b] * (row_sum[b] - x_k[b, c])
//
// Row mapping: G lanes share a row (G = 8: eight rows per wave, for rows of a few dozen floats; G = 64: a wave per row).  A
// segment is cut into QUADS of four columns (the last one of a width that is no multiple of 4 is partial); lane l of the row's
// group takes quads l, l + G, ... of segment 0, then of segment 1, ... and adds their elements to its s and q in column
// order; the G lane sums are then added in a fixed xor butterfly.  A quad is ONE 16-byte access on the vector path and up to
// four 4-byte accesses on the scalar path — the same elements in the same lane in the same order, so the path a segment
// takes changes no result bit, and the order depends on (N, segment geometry) only.  No atomics; every product and add is
// rounded on its own (-ffp-contract=off).
#include "rowreg.hpp"  // row_sum<G>: the fixed xor butterfly over the G lanes of a row

namespace tbe {

struct FmSeg {
  const float* x;      // forward / backward input
  float* g;            // backward: gradient of this segment, nullptr = not wanted
  int64_t x_stride;    // elements
  int64_t g_stride;
  int32_t width;
  int32_t cat_off;     // first column of the segment inside cat / grad_cat
  int32_t vec;         // 16-byte path allowed (decided on the host)
  int32_t pad;
};

struct FmArgs {
  FmSeg seg[TBE_FM_MAX_SEGMENTS];
  int32_t nseg;
  int32_t N;
};

// block = 256 threads = 256 / G rows; grid.x = row blocks
template <int G, bool CAT>
__global__ __launch_bounds__(256) void fm_fwd_kernel(const FmArgs a, int64_t B, float* __restrict__ fm, int64_t fm_stride,
                                                     float* __restrict__ row_sum, float* __restrict__ cat) {
  const int lane = threadIdx.x % G;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (256 / G) + threadIdx.x / G;
  const bool live = r < B;  // no early return: the butterfly below runs in every lane
  float s = 0.f, q = 0.f;
  if (live) {
#pragma unroll
    for (int k = 0; k < TBE_FM_MAX_SEGMENTS; ++k) {
      if (k >= a.nseg) break;
      const float* xr = a.seg[k].x + r * a.seg[k].x_stride;
      float* cr = CAT ? cat + r * a.N + a.seg[k].cat_off : nullptr;
      const int w = a.seg[k].width;
      const int nq = (w + 3) >> 2;
      if (a.seg[k].vec) {
#pragma unroll 4
        for (int j = lane; j < nq; j += G) {
          const float4 v = ld4(xr + 4 * j);
          if (CAT) st4(cr + 4 * j, v);
          s += v.x;
          q += v.x * v.x;
          s += v.y;
          q += v.y * v.y;
          s += v.z;
          q += v.z * v.z;
          s += v.w;
          q += v.w * v.w;
        }
      } else {
        for (int j = lane; j < nq; j += G) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int c = 4 * j + i;
            if (c < w) {
              const float v = xr[c];
              if (CAT) cr[c] = v;
              s += v;
              q += v * v;
            }
          }
        }
      }
    }
  }
  s = tbe::row_sum<G>(s);  // qualified: the parameter `row_sum` hides the function
  q = tbe::row_sum<G>(q);
  if (live && lane == 0) {
    row_sum[r] = s;
    fm[r * fm_stride] = (s * s - q) * 0.5f;  // the reference's order: square of sum - sum of squares, then * 0.5
  }
}

template <int G, bool GCAT>
__global__ __launch_bounds__(256) void fm_bwd_kernel(const FmArgs a, int64_t B, const float* __restrict__ grad_fm,
                                                     int64_t grad_fm_stride, const float* __restrict__ row_sum,
                                                     const float* __restrict__ grad_cat) {
  const int lane = threadIdx.x % G;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (256 / G) + threadIdx.x / G;
  if (r >= B) return;
  const float s = row_sum[r];
  const float gf = grad_fm[r * grad_fm_stride];
#pragma unroll
  for (int k = 0; k < TBE_FM_MAX_SEGMENTS; ++k) {
    if (k >= a.nseg) break;
    if (a.seg[k].g == nullptr) continue;
    const float* xr = a.seg[k].x + r * a.seg[k].x_stride;
    float* gr = a.seg[k].g + r * a.seg[k].g_stride;
    const float* cr = GCAT ? grad_cat + r * a.N + a.seg[k].cat_off : nullptr;
    const int w = a.seg[k].width;
    const int nq = (w + 3) >> 2;
    if (a.seg[k].vec) {
#pragma unroll 4
      for (int j = lane; j < nq; j += G) {
        const float4 v = ld4(xr + 4 * j);
        float4 o = make_float4(gf * (s - v.x), gf * (s - v.y), gf * (s - v.z), gf * (s - v.w));
        if (GCAT) {
          const float4 c = ld4(cr + 4 * j);
          o = make_float4(c.x + o.x, c.y + o.y, c.z + o.z, c.w + o.w);
        }
        st4(gr + 4 * j, o);
      }
    } else {
      for (int j = lane; j < nq; j += G) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = 4 * j + i;
          if (c < w) {
            float o = gf * (s - xr[c]);
            if (GCAT) o = cr[c] + o;
            gr[c] = o;
          }
        }
      }
    }
  }
}

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// rows of up to 32 quads (four trips of an 8-lane group) share a wave eight at a time; wider rows take a wave each
static int fm_group(const FmArgs& a) {
  int64_t quads = 0;
  for (int k = 0; k < a.nseg; ++k) quads += (a.seg[k].width + 3) / 4;
  return quads <= 32 ? 8 : 64;
}

}  // namespace tbe

using namespace tbe;

// Shape checks shared by both entries; fills widths, strides, x and the column offsets.
static int fm_fill(const char* what, const tbe_fm_segment* segs, int32_t nseg, int64_t B, FmArgs* a) {
  TBE_REQUIRE(segs != nullptr, "%s: null segment list", what);
  TBE_REQUIRE(nseg >= 1 && nseg <= TBE_FM_MAX_SEGMENTS, "%s: nseg=%d must be in 1 .. %d", what, nseg, TBE_FM_MAX_SEGMENTS);
  TBE_REQUIRE(B >= 0, "%s: B=%lld is negative", what, (long long)B);
  int64_t N = 0;
  for (int k = 0; k < nseg; ++k) {
    TBE_REQUIRE(segs[k].width >= 1, "%s: segment %d has width %d < 1", what, k, segs[k].width);
    TBE_REQUIRE(segs[k].row_stride >= segs[k].width, "%s: segment %d has row stride %lld smaller than its width %d", what, k,
                (long long)segs[k].row_stride, segs[k].width);
    a->seg[k].x = segs[k].x;
    a->seg[k].g = nullptr;
    a->seg[k].x_stride = segs[k].row_stride;
    a->seg[k].g_stride = 0;
    a->seg[k].width = segs[k].width;
    a->seg[k].cat_off = static_cast<int32_t>(N);
    a->seg[k].vec = 0;
    a->seg[k].pad = 0;
    N += segs[k].width;
    TBE_REQUIRE(N < (1ll << 31), "%s: the row is wider than 2^31 - 1 columns", what);
  }
  for (int k = nseg; k < TBE_FM_MAX_SEGMENTS; ++k) a->seg[k] = FmSeg{nullptr, nullptr, 0, 0, 0, 0, 0, 0};
  a->nseg = nseg;
  a->N = static_cast<int32_t>(N);
  // at least 4 rows per block (G = 64): the grid's x dimension holds 2^31 - 1 blocks
  TBE_REQUIRE((B + 3) / 4 < (1ll << 31), "%s: B=%lld too large (more than 2^31 - 1 row blocks)", what, (long long)B);
  return TBE_OK;
}

extern "C" int tbe_fm_forward_f32(const tbe_fm_segment* segs, int32_t nseg, int64_t B, float* fm, int64_t fm_stride,
                                  float* row_sum, float* cat, void* stream) {
  static const char* what = "tbe_fm_forward_f32";
  FmArgs a;
  if (int rc = fm_fill(what, segs, nseg, B, &a)) return rc;
  TBE_REQUIRE(fm_stride >= 1, "%s: fm_stride=%lld < 1", what, (long long)fm_stride);
  if (B == 0) return TBE_OK;
  TBE_REQUIRE(fm && row_sum && aligned(fm, 4) && aligned(row_sum, 4) && aligned(cat, 4),
              "%s: null or 4-byte-misaligned fm / row_sum / cat", what);
  const bool cat_vec = aligned(cat, 16) && a.N % 4 == 0;  // a row of cat starts on the 16-byte grid
  for (int k = 0; k < nseg; ++k) {
    const FmSeg& sg = a.seg[k];
    TBE_REQUIRE(sg.x && aligned(sg.x, 4), "%s: segment %d: null or 4-byte-misaligned pointer", what, k);
    a.seg[k].vec = aligned(sg.x, 16) && sg.x_stride % 4 == 0 && sg.width % 4 == 0 &&
                   (cat == nullptr || (cat_vec && sg.cat_off % 4 == 0));
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int G = fm_group(a);
  const dim3 grid(static_cast<unsigned>((B + 256 / G - 1) / (256 / G)));
#define TBE_FM_FWD(GG, C) hipLaunchKernelGGL((fm_fwd_kernel<GG, C>), grid, dim3(256), 0, st, a, B, fm, fm_stride, row_sum, cat)
  if (G == 8) {
    if (cat) TBE_FM_FWD(8, true); else TBE_FM_FWD(8, false);
  } else {
    if (cat) TBE_FM_FWD(64, true); else TBE_FM_FWD(64, false);
  }
#undef TBE_FM_FWD
  TBE_CHECK_LAUNCH(what);
  return TBE_OK;
}

extern "C" int tbe_fm_backward_f32(const tbe_fm_segment* segs, const tbe_fm_grad_segment* grads, int32_t nseg, int64_t B,
                                   const float* grad_fm, int64_t grad_fm_stride, const float* row_sum, const float* grad_cat,
                                   void* stream) {
  static const char* what = "tbe_fm_backward_f32";
  FmArgs a;
  if (int rc = fm_fill(what, segs, nseg, B, &a)) return rc;
  TBE_REQUIRE(grads != nullptr, "%s: null gradient segment list", what);
  TBE_REQUIRE(grad_fm_stride >= 1, "%s: grad_fm_stride=%lld < 1", what, (long long)grad_fm_stride);
  bool any = false;
  for (int k = 0; k < nseg; ++k) {
    if (grads[k].g == nullptr) continue;
    any = true;
    TBE_REQUIRE(grads[k].row_stride >= a.seg[k].width, "%s: gradient segment %d has row stride %lld smaller than its width %d",
                what, k, (long long)grads[k].row_stride, a.seg[k].width);
  }
  if (B == 0) return TBE_OK;
  TBE_REQUIRE(grad_fm && row_sum && aligned(grad_fm, 4) && aligned(row_sum, 4) && aligned(grad_cat, 4),
              "%s: null or 4-byte-misaligned grad_fm / row_sum / grad_cat", what);
  const bool cat_vec = aligned(grad_cat, 16) && a.N % 4 == 0;
  for (int k = 0; k < nseg; ++k) {
    FmSeg& sg = a.seg[k];
    TBE_REQUIRE(sg.x && aligned(sg.x, 4) && aligned(grads[k].g, 4), "%s: segment %d: null or 4-byte-misaligned pointer", what,
                k);
    sg.g = grads[k].g;
    sg.g_stride = grads[k].row_stride;
    sg.vec = aligned(sg.x, 16) && sg.x_stride % 4 == 0 && sg.width % 4 == 0 && aligned(sg.g, 16) && sg.g_stride % 4 == 0 &&
             (grad_cat == nullptr || (cat_vec && sg.cat_off % 4 == 0));
  }
  if (!any) return TBE_OK;  // nothing wanted: nothing to write
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int G = fm_group(a);
  const dim3 grid(static_cast<unsigned>((B + 256 / G - 1) / (256 / G)));
#define TBE_FM_BWD(GG, C) \
  hipLaunchKernelGGL((fm_bwd_kernel<GG, C>), grid, dim3(256), 0, st, a, B, grad_fm, grad_fm_stride, row_sum, grad_cat)
  if (G == 8) {
    if (grad_cat) TBE_FM_BWD(8, true); else TBE_FM_BWD(8, false);
  } else {
    if (grad_cat) TBE_FM_BWD(64, true); else TBE_FM_BWD(64, false);
  }
#undef TBE_FM_BWD
  TBE_CHECK_LAUNCH(what);
  return TBE_OK;
}
