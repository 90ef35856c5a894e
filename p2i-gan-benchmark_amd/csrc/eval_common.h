// Device helpers shared by the benchmark's scoring units (eval_exp1.hip, eval_exp3.hip): the reference's rain-rate transform
// (experiments/exp1.py transform_mmhr) in fp64 and the Welford / Chan updates of (n, mean, M2).  Both units compile with
// -ffp-contract=off, so every helper rounds as numpy's separate operations do.
#pragma once
#include "common.h"

namespace p2i {

__device__ __forceinline__ double mmhr(double x, int div3) {
  // np.maximum propagates NaN (fmax would drop it); np.clip(e, None, 38) and np.clip(out, 0, 200) keep NaN as well
  if (!(x != x) && x < 0.001) x = 0.001;
  if (div3) x = x / 3.0;
  double e = x * 0.0625;
  if (e > 38.0) e = 38.0;
  double out = pow(10.0, e) * 0.036;
  if (out < 0.0) out = 0.0;
  if (out > 200.0) out = 200.0;
  return out;
}

// element i of an input, transformed: uint8 through the host's 256-entry table, f32 / f64 through the device pow
template <typename T> __device__ __forceinline__ double tload(const T* p, long long i, const double* lut, int div3);
template <> __device__ __forceinline__ double tload<uint8_t>(const uint8_t* p, long long i, const double* lut, int) { return lut[p[i]]; }
template <> __device__ __forceinline__ double tload<float>(const float* p, long long i, const double*, int div3) { return mmhr((double)p[i], div3); }
template <> __device__ __forceinline__ double tload<double>(const double* p, long long i, const double*, int div3) { return mmhr(p[i], div3); }

// Welford: (n, mean, M2) <- (n, mean, M2) + one value g
__device__ __forceinline__ void welford_push(double& n, double& mean, double& m2, double g) {
  n += 1.0;
  const double dg = g - mean;
  mean += dg / n;
  m2 += dg * (g - mean);
}

// Chan et al.'s pairwise update: (n, mean, M2) <- (n, mean, M2) (+) (bn, bmean, bm2)
__device__ __forceinline__ void chan_merge(double& n, double& mean, double& m2, double bn, double bmean, double bm2) {
  const double nn = n + bn;
  if (bn > 0.0) {
    const double d = bmean - mean;
    mean = mean + d * (bn / nn);
    m2 = m2 + bm2 + d * d * (n * bn / nn);
  }
  n = nn;
}

static inline bool eval_dtype_ok(int d) { return d == P2I_EXP1_U8 || d == P2I_EXP1_F32 || d == P2I_EXP1_F64; }

}  // namespace p2i
