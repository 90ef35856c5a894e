// What the kriging files (classical.hip, krig_uq.hip, krig_cs.hip, stkrig_cs.hip, stkrig.hip, stkrig_loso.hip, lagkrig.hip, lkrig.hip) share: the tile
// and size limits, the covariance function and the space-time distances, the fixed-tree fp64 block sum, the "no model" rule, the
// variogram's bin image and fit candidate, the covariance tile writer and the host-side checks.  krig_mfma.h adds the c0 slab core.
#pragma once
#include "common.h"

namespace p2i {
namespace {

constexpr int TS = 32;            // tile of the factorisation; systems are padded to a multiple of it
constexpr int PCHUNK = 128;       // gauges staged in LDS per predictor pass
constexpr int MAX_NP = 4096;      // fp64 vector of the solve in LDS: 32 KiB
constexpr int MAX_SIDE = 16384;   // squared pixel distances stay in int32
constexpr int MAX_LAGS = 32;      // spatial variogram bins
constexpr int MAX_TLAGS = 7;      // temporal lags u = 0 .. 7
constexpr int BIN_THREADS = 64;   // threads of a variogram bins workgroup
constexpr int FG = 8;             // target frames fed from one (pixel, point) pair of the space-time predictor

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

// u^T 1 over the n gauges of a system (u = K^-1 1, row 0 of its solutions), in every thread of the 256
__device__ __forceinline__ double sum_u(const double* __restrict__ u, int n, double* red) {
  double su = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) su += u[i];
  return block_sum_d(su, red);
}

// a system has no model: its factorisation met a non-positive pivot (status), or the fit of its sample b is degenerate (cand, null
// with fixed parameters).  Each caller joins its own count condition (no gauges, fewer than 2, one site only).
__device__ __forceinline__ bool no_model(int status, const int* __restrict__ cand, int b) {
  return status != 0 || (cand != nullptr && cand[b] < 0);
}

// C(h) = psill (1 - g(h / a)): exponential g(r) = 1 - exp(-r); spherical g(r) = 1.5 r - 0.5 r^3 below 1, 1 beyond
__device__ __forceinline__ float cov_f(float h, float psill, float a, int model) {
  const float r = h / a;
  if (model == 0) return psill * expf(-r);
  return r < 1.f ? psill * (1.f - (1.5f * r - 0.5f * r * r * r)) : 0.f;
}

// the variogram's g(r) in fp64, as the fits evaluate it
__device__ __forceinline__ double g_d(double r, int model) {
  return model == 0 ? 1.0 - exp(-r) : (r < 1.0 ? 1.5 * r - 0.5 * r * r * r : 1.0);
}

// the one space-time distance of stkrig.hip's build and predictor and of lkrig.hip (an explicit fma: all round alike, so a gauge is
// reproduced in its own frame)
__device__ __forceinline__ float st_dist(int d2, int dt, float k2) {
  const float ft = (float)dt;
  return sqrtf(fmaf(k2, ft * ft, (float)d2));
}

// the one Lagrangian distance of stkrig.hip's LAG build and predictor and of lkrig.hip's LAG kernels (lag_dist = sqrt of lag_d2): fdy,
// fdx, ft are the integer differences (point a minus point b) as floats.  fmaf rounds -v ft + d once, and swapping a and b negates all
// three exactly, so both orders give the same value bit for bit; at ft = 0 it is sqrt(dy^2 + dx^2), whatever v is.
__device__ __forceinline__ float lag_d2(float fdy, float fdx, float ft, float vy, float vx, float k2) {
  const float ey = fmaf(-vy, ft, fdy), ex = fmaf(-vx, ft, fdx);
  return fmaf(ey, ey, fmaf(ex, ex, k2 * (ft * ft)));
}
__device__ __forceinline__ float lag_dist(float fdy, float fdx, float ft, float vy, float vx, float k2) {
  return sqrtf(lag_d2(fdy, fdx, ft, vy, vx, k2));
}

// ---- the variogram bins of one workgroup of BIN_THREADS threads: three [bin][thread] arrays in LDS (40 KiB; vario_bins_lds() below
// hands them out).  Every thread keeps its own bins (no conflicts, no dynamic register indexing); reduce() adds the threads in
// thread order.
struct VarioBins {
  double (*sg)[BIN_THREADS];
  double (*sh)[BIN_THREADS];
  unsigned (*sc)[BIN_THREADS];

  __device__ __forceinline__ void clear(int n_lags) {
    const int tid = threadIdx.x;
    for (int k = 0; k < n_lags; ++k) {
      sg[k][tid] = 0.0;
      sh[k][tid] = 0.0;
      sc[k][tid] = 0u;
    }
  }
  // one pair at distance h (kept if below hmax = n_lags lagw) with the values zi and *zj; *zj is read only for a pair that is kept
  __device__ __forceinline__ void add(double h, double hmax, double lagw, int n_lags, double zi, const float* __restrict__ zj) {
    const int tid = threadIdx.x;
    if (h < hmax) {
      const int k = min((int)floor(h / lagw), n_lags - 1);
      const double d = zi - (double)*zj;
      sg[k][tid] += 0.5 * (d * d);
      sh[k][tid] += h;
      sc[k][tid] += 1u;
    }
  }
  // row `row` of part [rows][n_lags][3] = (pairs, sum of (z_i - z_j)^2 / 2, sum of h)
  __device__ __forceinline__ void reduce(int n_lags, double* __restrict__ part, size_t row) {
    __syncthreads();
    for (int k = threadIdx.x; k < n_lags; k += BIN_THREADS) {
      double g = 0.0, h = 0.0, c = 0.0;
      for (int t = 0; t < BIN_THREADS; ++t) {
        g += sg[k][t];
        h += sh[k][t];
        c += (double)sc[k][t];
      }
      double* o = part + (row * n_lags + k) * 3;
      o[0] = c;
      o[1] = g;
      o[2] = h;
    }
  }
};
__device__ __forceinline__ VarioBins vario_bins_lds() {
  __shared__ double sg[MAX_LAGS][BIN_THREADS];
  __shared__ double sh[MAX_LAGS][BIN_THREADS];
  __shared__ unsigned sc[MAX_LAGS][BIN_THREADS];
  return VarioBins{sg, sh, sc};
}

// ---- one candidate of a variogram fit: (nugget, psill) of gamma = nugget + psill g by count-weighted least squares over the nb bins
// with sn[e] > 0 pairs and mean semivariance sgam[e]; g_of(e) is the candidate's g at bin e.  A singular system or a negative
// nugget falls back to nugget = 0.  ok: the candidate has pairs and a positive psill.
struct FitCand {
  int ok;
  double nug, ps, sse;
};
template <class G>
__device__ __forceinline__ FitCand vario_fit_candidate(const double* sn, const double* sgam, int nb, G g_of) {
  double S0 = 0.0, S1 = 0.0, S2 = 0.0, T0 = 0.0, T1 = 0.0;
  for (int e = 0; e < nb; ++e) {
    if (!(sn[e] > 0.0)) continue;
    const double g = g_of(e);
    S0 += sn[e];
    S1 += sn[e] * g;
    S2 += sn[e] * g * g;
    T0 += sn[e] * sgam[e];
    T1 += sn[e] * g * sgam[e];
  }
  const double det = S0 * S2 - S1 * S1;
  double nug = -1.0, ps = 0.0;
  if (det > 1e-12 * S0 * S2) {
    ps = (S0 * T1 - S1 * T0) / det;
    nug = (T0 - ps * S1) / S0;
  }
  if (nug < 0.0) {
    nug = 0.0;
    ps = S2 > 0.0 ? T1 / S2 : 0.0;
  }
  double sse = 0.0;
  for (int e = 0; e < nb; ++e) {
    if (!(sn[e] > 0.0)) continue;
    const double r = sgam[e] - nug - ps * g_of(e);
    sse += sn[e] * r * r;
  }
  return FitCand{(S0 > 0.0 && ps > 0.0) ? 1 : 0, nug, ps, sse};
}

// ---- one 32 x 32 tile of a covariance matrix As [np][np] by 256 threads over a (tiles, tiles, systems) grid: lower tiles only,
// entry(i, j) where both are below the n points of the system, identity on the padding
template <class Entry>
__device__ __forceinline__ void cov_tile_write(float* __restrict__ As, int n, int np, Entry entry) {
  if (blockIdx.x > blockIdx.y) return;
  const int j = blockIdx.x * TS + (threadIdx.x & 31);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int i = blockIdx.y * TS + (threadIdx.x >> 5) + 8 * rr;
    float v = i == j ? 1.f : 0.f;
    if (i < n && j < n) v = entry(i, j);
    As[(size_t)i * np + j] = v;
  }
}

}  // namespace

// ---- host-side checks shared by the entry points
static inline int krig_model_check(int model) {
  P2I_REQUIRE(model == 0 || model == 1, "variogram model must be 0 (exponential) or 1 (spherical)");
  return P2I_OK;
}
static inline int krig_frame_check(int model, int H, int W) {          // a predictor's model and frame
  if (int rc = krig_model_check(model)) return rc;
  P2I_REQUIRE(H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE, "bad frame shape");
  return P2I_OK;
}
static inline int krig_cap_check(int cap) {
  P2I_REQUIRE(cap > 0 && cap % TS == 0 && cap <= MAX_NP, "cap must be a multiple of %d, at most %d (got %d)", TS, MAX_NP, cap);
  return P2I_OK;
}
static inline int krig_lags_check(int n_lags, double lag_width) {
  P2I_REQUIRE(n_lags > 0 && n_lags <= MAX_LAGS && lag_width > 0.0, "n_lags must be 1..%d with a positive lag width", MAX_LAGS);
  return P2I_OK;
}

// ---- a chunk of systems (p2i_krig_systems of p2i_hip.h).  `reads`: the fields an entry point reads; a pointer field it does not read
// may be NULL (cand wherever it is read), model is checked with KS_MODEL only, np stands at one tile without KS_NP.  `own`: its other
// pointers are there.  krig_sys_check: null pointers, model and frame, range and sizes; p2i_stkrig_loso calls the halves around its own.
using ks_t = p2i_krig_systems;
static_assert(sizeof(p2i_krig_systems) == 80 && offsetof(ks_t, pix) == 0 && offsetof(ks_t, z) == 8 && offsetof(ks_t, counts) == 16 &&
                  offsetof(ks_t, params) == 24 && offsetof(ks_t, cand) == 32 && offsetof(ks_t, status) == 40 && offsetof(ks_t, model) == 48 &&
                  offsetof(ks_t, f0) == 52 && offsetof(ks_t, R) == 56 && offsetof(ks_t, T) == 60 && offsetof(ks_t, nsys) == 64 &&
                  offsetof(ks_t, np) == 68 && offsetof(ks_t, cap) == 72,
              "p2i_krig_systems is mirrored field by field by the ctypes binding");
enum : unsigned { KS_PIX = 1, KS_Z = 2, KS_COUNTS = 4, KS_PARAMS = 8, KS_STATUS = 16, KS_MODEL = 32, KS_NP = 64 };
static inline int krig_sys_ptrs(const p2i_krig_systems* k, unsigned reads, bool own) {
  P2I_REQUIRE(k && own && (!(reads & KS_PIX) || k->pix) && (!(reads & KS_Z) || k->z) && (!(reads & KS_COUNTS) || k->counts) &&
                  (!(reads & KS_PARAMS) || k->params) && (!(reads & KS_STATUS) || k->status),
              "null pointer");
  return P2I_OK;
}
static inline int krig_sys_range(const p2i_krig_systems* k, unsigned reads) {
  const int np = (reads & KS_NP) ? k->np : TS;
  P2I_REQUIRE(k->R > 0 && k->T > 0 && k->f0 >= 0 && k->nsys > 0 && k->nsys <= 65535, "bad system range");
  P2I_REQUIRE(k->R == 1 || (k->R == k->T && k->f0 % k->T == 0), "a system spans one frame or one whole sample");
  P2I_REQUIRE(np > 0 && np % TS == 0 && np <= k->cap && k->cap <= MAX_NP, "padded size %d must be a multiple of %d within cap %d", np, TS,
              k->cap);
  return P2I_OK;
}
static inline int krig_sys_check(const p2i_krig_systems* k, unsigned reads, bool own, int H = 1, int W = 1) {
  if (int rc = krig_sys_ptrs(k, reads, own)) return rc;
  if (int rc = (reads & KS_MODEL) ? krig_frame_check(k->model, H, W) : P2I_OK) return rc;
  return krig_sys_range(k, reads);
}

// classical.hip: the variogram fit of B samples from part [B][nu][nch][n_lags][3] (the fit kernel's comment has the outputs).
// st = false: range candidates only, nu = 1, fit [B][4]; st = true: (kappa, range) candidates, fit [B][5].  The caller has checked
// the arguments and checks launch_status().
void krig_fit_launch(bool st, const double* part, int B, int nu, int nch, int n_lags, double lagw, int model, double* bins, double* fit,
                     int* cand, float* params, hipStream_t s);

// classical.hip: the right-looking tiled Cholesky (panel, trailing update per 32 columns) over nsys systems whose lower tiles are
// already built in L [nsys][np][np]; status[s] is set where a pivot is not > 0.  The caller checks launch_status().
void krig_factor_tiles(float* L, int nsys, int np, int* status, hipStream_t s);

}  // namespace p2i
