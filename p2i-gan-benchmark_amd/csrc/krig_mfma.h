// The c0 slab core of the kernels that multiply a matrix with k(p) = [c0(p, i)]_i on v_mfma_f32_32x32x2_f32 (krig_uq.hip's variance
// map, krig_cs.hip's and stkrig_cs.hip's members predictors): D = A c0 with A = a 32 x 32 operand tile (m = row), B = c0 (n = pixel),
// K = gauge.  A workgroup of 256 threads owns PT pixels, wave w the pixels 32 w .. 32 w + 31.  Per 32-gauge slab all threads evaluate
// c0 [32][PT] into LDS (k(p) never touches HBM) next to the staged operand tiles, and the waves feed both to the MFMAs.  The kernels
// keep their own loops over slabs and tiles; the layout, the fill, the stage and the product are here once.
#pragma once
#include "krig_common.h"

namespace p2i {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PT = 128;            // pixels per workgroup: one 32-pixel MFMA column tile per wave
constexpr int SLAB_LD = PT + 32;   // row stride of the c0 slab: the two k rows a wave reads fall into different halves of the 64 banks
constexpr int A_LD = TS + 1;       // row stride of a staged 32 x 32 operand tile: lanes walk rows, so an odd stride

// row of accumulator register e of a 32 x 32 MFMA result in lane half lhi; the column is lane & 31
__device__ __forceinline__ int acc_row(int e, int lhi) { return (e & 3) + 8 * (e >> 2) + 4 * lhi; }

// ---- slab sb of c0 between the workgroup's pixels and the gauges 32 sb .. 32 sb + 31 of gp (n gauges; zeros past them): thread ->
// pixel tid & 127 at (py, px), gauges 16 (tid >> 7) .. + 15.  visit(i, c0, at) sees every gauge i < n of the thread, at: the gauge is
// the pixel.
template <class Visit>
__device__ __forceinline__ void slab_fill(float (*slab)[SLAB_LD], const int* __restrict__ gp, int n, int sb, int py, int px, float nug,
                                          float psill, float a, int model, Visit visit) {
  const int bp = threadIdx.x & (PT - 1), bg = threadIdx.x >> 7;
#pragma unroll 1
  for (int j = 0; j < TS / 2; ++j) {
    const int g = bg * (TS / 2) + j, i = sb * TS + g;
    float c0 = 0.f;
    if (i < n) {
      const int gq = gp[i];
      const int dy = py - (gq >> 16), dx = px - (gq & 0xffff);
      const int d2 = dy * dy + dx * dx;
      c0 = cov_f(sqrtf((float)d2), psill, a, model) + (d2 == 0 ? nug : 0.f);
      visit(i, c0, d2 == 0);
    }
    slab[g][bp] = c0;
  }
}

// ---- the space-time slab: the workgroup's pixels in frame t against the points 32 sb .. 32 sb + 31 of a sample's point set (gp the
// pixels, gt the frames), c0 = cov_f(st_dist(d2, dt, k2)) + nugget [(d2 | dt) = 0], the space-time predictor's expression.
// visit(i, c0, at) as above, at: the point is the pixel in this frame.
template <class Visit>
__device__ __forceinline__ void slab_fill(float (*slab)[SLAB_LD], const int* __restrict__ gp, const int* __restrict__ gt, int n, int sb,
                                          int py, int px, int t, float nug, float psill, float a, float k2, int model, Visit visit) {
  const int bp = threadIdx.x & (PT - 1), bg = threadIdx.x >> 7;
#pragma unroll 1
  for (int j = 0; j < TS / 2; ++j) {
    const int g = bg * (TS / 2) + j, i = sb * TS + g;
    float c0 = 0.f;
    if (i < n) {
      const int gq = gp[i];
      const int dy = py - (gq >> 16), dx = px - (gq & 0xffff), dt = t - gt[i];
      const int d2 = dy * dy + dx * dx;
      c0 = cov_f(st_dist(d2, dt, k2), psill, a, model) + ((d2 | dt) == 0 ? nug : 0.f);
      visit(i, c0, (d2 | dt) == 0);
    }
    slab[g][bp] = c0;
  }
}

// ---- stage a 32 x 32 operand tile (top-left entry at src, row stride ld floats, 16-byte aligned rows): one float4 per thread; rows
// from `rows` on are zeros
__device__ __forceinline__ void tile_stage(float (*At)[A_LD], const float* __restrict__ src, int ld, int rows) {
  const int ar = threadIdx.x >> 3, ac = (threadIdx.x & 7) * 4;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ar < rows) v = *reinterpret_cast<const float4*>(src + (size_t)ar * ld + ac);
  At[ar][ac] = v.x;
  At[ar][ac + 1] = v.y;
  At[ar][ac + 2] = v.z;
  At[ar][ac + 3] = v.w;
}

// ---- acc += At (32 x 32) times the wave's 32 columns of the slab: 16 MFMAs, k in order
__device__ __forceinline__ f32x16 tile_mfma(const float (*At)[A_LD], const float (*slab)[SLAB_LD], f32x16 acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
#pragma unroll
  for (int kk = 0; kk < TS / 2; ++kk)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(At[l31][2 * kk + lhi], slab[2 * kk + lhi][wave * 32 + l31], acc, 0, 0, 0);
  return acc;
}

}  // namespace
}  // namespace p2i
