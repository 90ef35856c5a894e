// Shared by the benchmark's evaluation units (eval_exp1.hip, eval_exp3.hip, eval_exp2.hip).  Device side: the reference's rain-rate
// transform (experiments/exp1.py transform_mmhr) in fp64, the cropped-input view Crop<T> every kernel reads its inputs through, the
// Welford / Chan updates of (n, mean, M2) and the fixed-order workgroup tree that folds per-thread records.  Host side: the crop
// check and the dtype dispatch of the entry points.  The units compile with -ffp-contract=off, so every helper rounds as numpy's
// separate operations do.
#pragma once
#include "common.h"
#include <stddef.h>
#include <type_traits>

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

// An input [T][h][w] of uint8 / f32 / f64 seen through its crop at (top, left): at(t, y, x) is the transformed value of crop pixel
// (y, x) of frame t.  row(t, y) is the element offset of a crop row's first pixel and at(row, x) reads along it, for a kernel that
// walks one row.  Offsets are 64-bit.  A pointer inside a by-value kernel argument carries no noalias.  The kernels that only load
// in their loops take the view as their argument at no cost; exp1_accumulate_kernel, which stores in the loop that loads its
// inputs, measured 5 % slower in run_exp1 with it and keeps loose `const T* __restrict__` arguments (see there).
template <typename T> struct Crop {
  const T* p;
  int h, w, top, left;
  __device__ __forceinline__ long long row(long long t, int y) const { return t * h * w + (long long)(top + y) * w + left; }
  __device__ __forceinline__ double at(long long row, int x, const double* lut, int div3) const { return tload<T>(p, row + x, lut, div3); }
  __device__ __forceinline__ double at(long long t, int y, int x, const double* lut, int div3) const { return at(row(t, y), x, lut, div3); }
};

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

// The workgroup's N per-thread records folded in a fixed order: thread i takes thread i + o for o = N/2, ..., 1, through
// red[N * R::WORDS] doubles of LDS; thread 0 ends with the whole.  R has store(double*), a static load(const double*) and
// merge(const R&).  Every thread of the workgroup calls it (it has barriers).
template <int N, typename R> __device__ __forceinline__ void block_tree(R& r, double* red) {
  r.store(red + threadIdx.x * R::WORDS);
  __syncthreads();
  for (int o = N / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      r.merge(R::load(red + (threadIdx.x + o) * R::WORDS));
      r.store(red + threadIdx.x * R::WORDS);
    }
    __syncthreads();
  }
}

// ---- host side: the entry points' input descriptor (p2i_eval_input of p2i_hip.h), its checks and its dtype dispatch
static_assert(sizeof(p2i_eval_input) == 32 && offsetof(p2i_eval_input, data) == 0 && offsetof(p2i_eval_input, dtype) == 8 &&
                  offsetof(p2i_eval_input, h) == 12 && offsetof(p2i_eval_input, w) == 16 && offsetof(p2i_eval_input, top) == 20 &&
                  offsetof(p2i_eval_input, left) == 24,
              "p2i_eval_input is mirrored field by field by the ctypes binding");

static inline bool eval_dtype_ok(int d) { return d == P2I_EXP1_U8 || d == P2I_EXP1_F32 || d == P2I_EXP1_F64; }
// a descriptor that names an array (a NULL descriptor or NULL data names none) / whose rows x cols crop lies inside its h x w
static inline bool input_set(const p2i_eval_input* in) { return in && in->data; }
static inline bool crop_ok(const p2i_eval_input* in, int rows, int cols) {
  return in->top >= 0 && in->left >= 0 && in->top + rows <= in->h && in->left + cols <= in->w;
}

// dtype dispatch of the entry points (after eval_dtype_ok): f(Crop<T>) with the input's typed view, f(Crop<PT>, Crop<GT>) for a pair.
// Elem<decltype(view)> is T, to name the kernel's instantiation.
template <typename T> static Crop<T> view(const p2i_eval_input* in) { return Crop<T>{(const T*)in->data, in->h, in->w, in->top, in->left}; }
template <typename V> using Elem = std::remove_cv_t<std::remove_pointer_t<decltype(V::p)>>;
template <typename F> static void dispatch1(const p2i_eval_input* in, F&& f) {
  if (in->dtype == P2I_EXP1_U8) f(view<uint8_t>(in));
  else if (in->dtype == P2I_EXP1_F32) f(view<float>(in));
  else f(view<double>(in));
}
template <typename F> static void dispatch2(const p2i_eval_input* pin, const p2i_eval_input* gin, F&& f) {
  dispatch1(pin, [&](auto p) { dispatch1(gin, [&](auto g) { f(p, g); }); });
}

}  // namespace p2i
