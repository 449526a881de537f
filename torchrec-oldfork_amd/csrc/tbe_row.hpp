// The row vocabulary of the TBE kernels (forward, per-sample-weight gradient, backward + optimizer): a lane holds
// columns [d, d+4) of a row as one float4, whatever the table element type WT (float or _Float16).  Here, once: when a
// row may move as one vector per lane, the guarded load and store of a lane's columns, and the float4 arithmetic the
// kernels are written in.  Every sum keeps its column order x, y, z, w (-ffp-contract=off keeps the fmaf's as written).
#pragma once
#include "common.hpp"

namespace tbe {

// Is a row base on the grid of its 4-element vectors (16 B of float, 8 B of _Float16)?
template <typename WT>
__device__ __forceinline__ bool row_aligned(const WT* row) {
  return (reinterpret_cast<uintptr_t>(row) & kRowAlignMask<WT>) == 0;
}
// May the rows of width D that start at `row` move as one 4-element vector per lane?  Whole vectors only, and a base on
// their grid.  A second row of the same width (an optimizer state beside a table row that passed) needs `vec &&
// row_aligned(state)` only.
template <typename WT>
__device__ __forceinline__ bool row_vec(int D, const WT* row) {
  return ((D & 3) == 0) && row_aligned(row);
}
// ... for table rows paired with the column block [Doff, Doff + D) of an FP32 matrix (the pooled output, its gradient)
template <typename WT>
__device__ __forceinline__ bool row_vec(int D, const WT* row, int64_t Doff, int64_t stride, const float* block) {
  return ((D & 3) == 0) && ((Doff & 3) == 0) && ((stride & 3) == 0) && row_aligned(row) && row_aligned(block);
}

// Loads columns [d, d+4) of a row; `vec` selects the one-vector path, otherwise 4 guarded scalars (zero beyond D).
__device__ __forceinline__ float4 load_cols(const float* row, int d, int D, bool vec) {
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    x = ld4(row + d);
  } else {
    if (d + 0 < D) x.x = row[d + 0];
    if (d + 1 < D) x.y = row[d + 1];
    if (d + 2 < D) x.z = row[d + 2];
    if (d + 3 < D) x.w = row[d + 3];
  }
  return x;
}
// _Float16 rows: one 8-B load of 4 halves (hipcc does not merge scalar half loads), plain up-casts.
__device__ __forceinline__ float4 load_cols(const _Float16* row, int d, int D, bool vec) {
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    const half4 h = ldh4(row + d);
    x = make_float4(static_cast<float>(h.x), static_cast<float>(h.y), static_cast<float>(h.z), static_cast<float>(h.w));
  } else {
    if (d + 0 < D) x.x = static_cast<float>(row[d + 0]);
    if (d + 1 < D) x.y = static_cast<float>(row[d + 1]);
    if (d + 2 < D) x.z = static_cast<float>(row[d + 2]);
    if (d + 3 < D) x.w = static_cast<float>(row[d + 3]);
  }
  return x;
}
// Stores columns [d, d+4) of a row; the caller has converted a _Float16 row's values (how is the optimizer's business).
__device__ __forceinline__ void store_cols(float* row, int d, int D, bool vec, float4 x) {
  if (vec) {
    st4(row + d, x);
  } else {
    if (d + 0 < D) row[d + 0] = x.x;
    if (d + 1 < D) row[d + 1] = x.y;
    if (d + 2 < D) row[d + 2] = x.z;
    if (d + 3 < D) row[d + 3] = x.w;
  }
}
__device__ __forceinline__ void store_cols(_Float16* row, int d, int D, bool vec, half4 h) {
  if (vec) {
    sth4(row + d, h);
  } else {
    if (d + 0 < D) row[d + 0] = h.x;
    if (d + 1 < D) row[d + 1] = h.y;
    if (d + 2 < D) row[d + 2] = h.z;
    if (d + 3 < D) row[d + 3] = h.w;
  }
}

// s * x + a per column.
__device__ __forceinline__ float4 fmaf4(float s, const float4& x, const float4& a) {
  return make_float4(fmaf(s, x.x, a.x), fmaf(s, x.y, a.y), fmaf(s, x.z, a.z), fmaf(s, x.w, a.w));
}
__device__ __forceinline__ void fma4(float4& a, float s, const float4& x) { a = fmaf4(s, x, a); }
__device__ __forceinline__ void add4(float4& a, const float4& x) {
  a.x += x.x;
  a.y += x.y;
  a.z += x.z;
  a.w += x.w;
}
__device__ __forceinline__ float4 clamp4(const float4& x, float lo, float hi) {
  return make_float4(fminf(fmaxf(x.x, lo), hi), fminf(fmaxf(x.y, lo), hi), fminf(fmaxf(x.z, lo), hi), fminf(fmaxf(x.w, lo), hi));
}
// <g, x> over the lane's 4 columns added to acc in column order.
__device__ __forceinline__ float dot4(const float4& g, const float4& x, float acc) {
  acc = fmaf(g.x, x.x, acc);
  acc = fmaf(g.y, x.y, acc);
  acc = fmaf(g.z, x.z, acc);
  return fmaf(g.w, x.w, acc);
}
// x . x added to s in column order; columns beyond D must be zero in x.
__device__ __forceinline__ float sumsq4(const float4& x, float s) { return dot4(x, x, s); }
// Zeroes the columns of x (columns [d, d+4)) that lie beyond D: values computed from zero-filled loads need not be zero.
__device__ __forceinline__ float4 mask_tail(float4 x, int d, int D) {
  if (d + 1 >= D) x.y = 0.f;
  if (d + 2 >= D) x.z = 0.f;
  if (d + 3 >= D) x.w = 0.f;
  return x;
}

// f(v.x...), f(v.y...), f(v.z...), f(v.w...): an element formula applied to the four columns of its float4 operands, in
// column order.  f takes what it updates by reference.
template <typename F, typename... V>
__device__ __forceinline__ void each4(F f, V&... v) {
  f(v.x...);
  f(v.y...);
  f(v.z...);
  f(v.w...);
}

}  // namespace tbe
