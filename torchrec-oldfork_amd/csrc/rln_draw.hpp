// The counter-based dropout draw of the residual-LayerNorm domain (include/tbe_hip.h), shared by residual_layernorm.hip and
// history_arch.hip: c = call_hash(seed, call) as the attention kernel, c2 = fmix32(c ^ 0x52dce729) so that no draw coincides
// with the attention's, then one word per site (host), one per row (once per row and dropout) and one fmix32 per element.
#pragma once
#include <cmath>

#include "tbe_backward_impl.hpp"  // fmix32, call_hash

namespace tbe {

constexpr uint32_t kRlnDomain = 0x52dce729u;

// One dropout of a launch: kept iff draw >= thr, kept elements times scale; `on` = p > 0.
struct RlnDrop {
  uint32_t w1, thr;
  float scale;
  int32_t on;
};

static RlnDrop rln_drop(uint64_t seed, int64_t call, float p, uint32_t site) {
  RlnDrop d;
  d.on = p > 0.f;
  d.w1 = fmix32(fmix32(call_hash(seed, call) ^ kRlnDomain) ^ (site * 0x9e3779b1u));
  const double thr = std::floor(static_cast<double>(p) * 4294967296.0);
  d.thr = thr >= 4294967295.0 ? 4294967295u : static_cast<uint32_t>(thr);
  d.scale = 1.f / (1.f - p);
  return d;
}

__device__ __forceinline__ uint32_t rln_row_word(const RlnDrop& d, uint32_t row) { return fmix32(d.w1 ^ (row * 0x85ebca6bu)); }

__device__ __forceinline__ float rln_keep1(float v, uint32_t w2, const RlnDrop& d, uint32_t col) {
  return fmix32(w2 ^ (col * 0xc2b2ae35u)) >= d.thr ? v * d.scale : 0.f;
}

// the four elements of the row word w2 that start at column `col`
__device__ __forceinline__ float4 rln_keep4(const float4 v, uint32_t w2, const RlnDrop& d, uint32_t col) {
  return make_float4(rln_keep1(v.x, w2, d, col), rln_keep1(v.y, w2, d, col + 1), rln_keep1(v.z, w2, d, col + 2),
                     rln_keep1(v.w, w2, d, col + 3));
}

static bool rln_p_ok(float p) { return p >= 0.f && p < 1.f; }  // false for NaN

}  // namespace tbe
