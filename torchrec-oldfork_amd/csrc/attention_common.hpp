// What the two attention kernel families share (attention.hip: one workgroup holds a whole (b, h) in LDS; attention_tiled.hip:
// keys stream through LDS in blocks): the argument block and its checks, the MFMA tile vocabulary, the row butterflies and
// the counter-based dropout draw of include/tbe_hip.h.
#pragma once
#include <cmath>

#include "common.hpp"
#include "tbe_backward_impl.hpp"  // fmix32, call_hash

namespace tbe {

constexpr int kAttnTile = 16;         // rows a wave owns at a time, and staged rows per MFMA tile
using attn_f4 = float __attribute__((ext_vector_type(4)));  // one MFMA accumulator
constexpr int kAttnMaxD = 128;

__host__ __device__ constexpr int attn_ds(int d) { return d + 4; }  // the LDS row stride of a staged [rows, d] matrix

struct AttnArgs {
  const float *q, *k, *v;            // element (b, l, h, c) at base + b * bs + l * rs + h * d + c
  int64_t q_bs, q_rs, k_bs, k_rs, v_bs, v_rs;
  const uint8_t* key_valid;          // [B, L] or null
  const float* dout;                 // backward: [B, L, H * d]
  float* lse;                        // [B, H, L]: written by the forward, read by the backward
  float *out, *dq, *dk, *dv;         // [B, L, H * d]; forward: out; backward: dq / dk / dv, each may be null (not wanted)
  int32_t H, L, d;
  uint32_t callh, drop_thr;          // call_hash(seed, call); keep iff draw >= drop_thr
  float drop_scale;                  // 1 / (1 - p)
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// over the 16 lanes that share a row
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
  for (int o = kAttnTile / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = kAttnTile / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// The dropout draw of element (b, h, i, j): three words, each the murmur3 finalizer of the one before xor an index times an
// odd constant (include/tbe_hip.h states it for the tests).
__device__ __forceinline__ uint32_t attn_word_bh(uint32_t callh, uint32_t bh) { return fmix32(callh ^ (bh * 0x9e3779b1u)); }
__device__ __forceinline__ uint32_t attn_word_i(uint32_t wbh, uint32_t i) { return fmix32(wbh ^ (i * 0x85ebca6bu)); }
__device__ __forceinline__ uint32_t attn_draw(uint32_t wi, uint32_t j) { return fmix32(wi ^ (j * 0xc2b2ae35u)); }

// The checks every entry shares; fills the sizes and the dropout words of `a`.  `supported` is the caller's support rule
// applied to (L, d), `rule` its public name.
inline int attn_check(const char* name, AttnArgs& a, int64_t B, int32_t H, int32_t L, int32_t d, float p, uint64_t seed,
                      int64_t call, bool supported, const char* rule) {
  TBE_REQUIRE(B >= 0 && H >= 1 && L >= 1 && d >= 1, "%s: bad sizes B=%lld H=%d L=%d d=%d", name, static_cast<long long>(B), H,
              L, d);
  TBE_REQUIRE(supported, "%s: (L, d) = (%d, %d) is not supported (%s)", name, L, d, rule);
  TBE_REQUIRE(B * H <= INT32_MAX, "%s: B * H = %lld workgroups exceed the grid", name, static_cast<long long>(B * H));
  TBE_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout p=%g outside [0, 1)", name, static_cast<double>(p));
  const int64_t row = static_cast<int64_t>(H) * d;
  const int64_t strides[3][2] = {{a.q_bs, a.q_rs}, {a.k_bs, a.k_rs}, {a.v_bs, a.v_rs}};
  for (const auto& s : strides) {
    TBE_REQUIRE(s[1] >= row && s[1] % 4 == 0, "%s: row stride %lld below the row of %lld floats, or no multiple of 4", name,
                static_cast<long long>(s[1]), static_cast<long long>(row));
    TBE_REQUIRE(s[0] >= (L - 1) * s[1] + row && s[0] % 4 == 0,
                "%s: batch stride %lld below the sample's extent, or no multiple of 4", name, static_cast<long long>(s[0]));
  }
  a.H = H;
  a.L = L;
  a.d = d;
  a.callh = call_hash(seed, call);
  const double thr = std::floor(static_cast<double>(p) * 4294967296.0);
  a.drop_thr = thr >= 4294967295.0 ? 4294967295u : static_cast<uint32_t>(thr);
  a.drop_scale = 1.f / (1.f - p);
  return TBE_OK;
}

}  // namespace tbe
