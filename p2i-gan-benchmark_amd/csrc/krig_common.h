// What the classical baselines (classical.hip) and their uncertainty / cross-validation kernels (krig_uq.hip) share: the tile and
// size limits, the covariance function, the fixed-tree fp64 block sum and the check of a system range.
#pragma once
#include "common.h"

namespace p2i {
namespace {

constexpr int TS = 32;            // tile of the factorisation; systems are padded to a multiple of it
constexpr int PCHUNK = 128;       // gauges staged in LDS per predictor pass
constexpr int MAX_NP = 4096;      // fp64 vector of the solve in LDS: 32 KiB
constexpr int MAX_SIDE = 16384;   // squared pixel distances stay in int32

__device__ __forceinline__ double block_sum_d(double v, double* red) {   // red: 256 doubles of LDS; fixed tree, 256 threads
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// C(h) = psill (1 - g(h / a)): exponential g(r) = 1 - exp(-r); spherical g(r) = 1.5 r - 0.5 r^3 below 1, 1 beyond
__device__ __forceinline__ float cov_f(float h, float psill, float a, int model) {
  const float r = h / a;
  if (model == 0) return psill * expf(-r);
  return r < 1.f ? psill * (1.f - (1.5f * r - 0.5f * r * r * r)) : 0.f;
}

// the one space-time distance of stkrig.hip's build and predictor and of lkrig.hip (an explicit fma: all round alike, so a gauge is
// reproduced in its own frame)
__device__ __forceinline__ float st_dist(int d2, int dt, float k2) {
  const float ft = (float)dt;
  return sqrtf(fmaf(k2, ft * ft, (float)d2));
}

// the one Lagrangian distance of lagkrig.hip's build and predictor and of lkrig.hip's LAG kernels (lag_dist = sqrt of lag_d2): fdy,
// fdx, ft are the integer differences (point a minus point b) as floats.  fmaf rounds -v ft + d once, and swapping a and b negates all
// three exactly, so both orders give the same value bit for bit; at ft = 0 it is sqrt(dy^2 + dx^2), whatever v is.
__device__ __forceinline__ float lag_d2(float fdy, float fdx, float ft, float vy, float vx, float k2) {
  const float ey = fmaf(-vy, ft, fdy), ex = fmaf(-vx, ft, fdx);
  return fmaf(ey, ey, fmaf(ex, ex, k2 * (ft * ft)));
}
__device__ __forceinline__ float lag_dist(float fdy, float fdx, float ft, float vy, float vx, float k2) {
  return sqrtf(lag_d2(fdy, fdx, ft, vy, vx, k2));
}

}  // namespace

static inline int krig_sys_check(int f0, int R, int T, int nsys, int np, int cap) {
  P2I_REQUIRE(R > 0 && T > 0 && f0 >= 0 && nsys > 0 && nsys <= 65535, "bad system range");
  P2I_REQUIRE(R == 1 || (R == T && f0 % T == 0), "a system spans one frame or one whole sample");
  P2I_REQUIRE(np > 0 && np % TS == 0 && np <= cap && cap <= MAX_NP, "padded size %d must be a multiple of %d within cap %d", np, TS, cap);
  return P2I_OK;
}

// classical.hip: the right-looking tiled Cholesky (panel, trailing update per 32 columns) over nsys systems whose lower tiles are
// already built in L [nsys][np][np]; status[s] is set where a pivot is not > 0.  The caller checks launch_status().
void krig_factor_tiles(float* L, int nsys, int np, int* status, hipStream_t s);

}  // namespace p2i
