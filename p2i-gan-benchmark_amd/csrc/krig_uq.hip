// Uncertainty and cross-validation of the classical baselines: the kriging variance map and the leave-one-out
// (LOO) residuals of ordinary kriging and of all-gauge IDW, with their scores.  Everything rests on W = L^-1, the inverse of the
// Cholesky factor that p2i_krig_factor leaves behind (K = L L^T, section 14):
//   sigma^2(p) = c00 - |W k(p)|^2 + (1 - u^T k(p))^2 / s          k(p) = [c0(p, i)]_i, u = K^-1 1, s = 1^T u
//   B_ii = sum_k W_ki^2 - u_i^2 / s,  e_i = alpha_i / B_ii,  sigma^2_-i = 1 / B_ii     (Dubrule 1983)
// Number formats: W is fp32 (fmaf tile products); the variance GEMM runs on the f32 matrix pipe with fp32 accumulators down the
// gauge axis, and everything after it (the squares, u^T k, the formula) is fp64; column square-sums, LOO and scores are fp64.  Every
// sum has a fixed order and there are no atomics: results are identical from run to run.
#include "krig_mfma.h"

namespace p2i {
namespace {

constexpr int RB = 4;              // row tiles of W per row block of the variance GEMM (section 16: exponentials against MFMA cycles)

// ---- W tile (i, i) = inverse of the factor's diagonal tile, and zeros in the tiles right of it.  Thread c < 32 solves T x = e_c by
// forward substitution with x in registers and T read as LDS broadcasts.  Identity padding inverts to identity exactly.
__global__ __launch_bounds__(256) void krig_invdiag_kernel(const float* __restrict__ L, int np, float* __restrict__ Wi) {
  __shared__ float D[TS][TS + 1];
  __shared__ float X[TS][TS + 1];
  const float* Ls = L + (size_t)blockIdx.y * np * np;
  float* Ws = Wi + (size_t)blockIdx.y * np * np;
  const int k0 = blockIdx.x * TS;
  const int tid = threadIdx.x, c = tid & 31, r0 = tid >> 5;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) D[r0 + 8 * rr][c] = Ls[(size_t)(k0 + r0 + 8 * rr) * np + k0 + c];
  __syncthreads();
  if (tid < TS) {
    float x[TS];
#pragma unroll
    for (int i = 0; i < TS; ++i) {
      float acc = i == c ? 1.f : 0.f;
#pragma unroll
      for (int m = 0; m < i; ++m) acc = fmaf(-D[i][m], x[m], acc);
      x[i] = acc / D[i][i];
    }
#pragma unroll
    for (int i = 0; i < TS; ++i) X[i][c] = i >= c ? x[i] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    float* row = Ws + (size_t)(k0 + r0 + 8 * rr) * np;
    row[k0 + c] = X[r0 + 8 * rr][c];
    for (int j0 = k0 + TS; j0 < np; j0 += TS) row[j0 + c] = 0.f;
  }
}

// ---- tile column j of W below its diagonal tile, one workgroup per (column, system), rows in order:
// W[i][j] = -W[i][i] sum_{k = j}^{i - 1} L[i][k] W[k][j].  The tiles W[k][j], k > j, are this workgroup's own earlier stores (visible
// after the barrier); the diagonal tiles are krig_invdiag_kernel's.
__global__ __launch_bounds__(256) void krig_invcol_kernel(const float* __restrict__ L, int np, float* Wi) {
  __shared__ float Lt[TS][TS + 1];
  __shared__ float Wt[TS][TS + 1];
  const float* Ls = L + (size_t)blockIdx.y * np * np;
  float* Ws = Wi + (size_t)blockIdx.y * np * np;
  const int j0 = blockIdx.x * TS;
  const int tid = threadIdx.x, c = tid & 31, r0 = tid >> 5;
  for (int i0 = j0 + TS; i0 < np; i0 += TS) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float nl[4], nw[4], dg[4];                       // the next step's tiles and the row's diagonal tile, in flight while this step computes
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int r = r0 + 8 * rr;
      nl[rr] = Ls[(size_t)(i0 + r) * np + j0 + c];
      nw[rr] = Ws[(size_t)(j0 + r) * np + j0 + c];
      dg[rr] = Ws[(size_t)(i0 + r) * np + i0 + c];
    }
    for (int k0 = j0; k0 < i0; k0 += TS) {
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        Lt[r0 + 8 * rr][c] = nl[rr];
        Wt[r0 + 8 * rr][c] = nw[rr];
      }
      __syncthreads();
      if (k0 + TS < i0) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int r = r0 + 8 * rr;
          nl[rr] = Ls[(size_t)(i0 + r) * np + k0 + TS + c];
          nw[rr] = Ws[(size_t)(k0 + TS + r) * np + j0 + c];
        }
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int m = 0; m < TS; ++m) acc[rr] = fmaf(Lt[r0 + 8 * rr][m], Wt[m][c], acc[rr]);
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      Wt[r0 + 8 * rr][c] = acc[rr];
      Lt[r0 + 8 * rr][c] = dg[rr];
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int r = r0 + 8 * rr;
      float o = 0.f;
#pragma unroll
      for (int m = 0; m < TS; ++m) o = fmaf(-Lt[r][m], Wt[m][c], o);
      Ws[(size_t)(i0 + r) * np + j0 + c] = o;
    }
    __syncthreads();                                  // the stores are visible to the next row's loads
  }
}

// ---- variance map of system s (gauges of frame fs = f0 + s R) on a tile of PT pixels.  D = W k on the slab core of krig_mfma.h: A =
// W (m = gauge row), K = gauge column; a wave holds RB row tiles at a time.  Per 32-gauge slab the c0 slab is filled next to the row
// block's W tiles; tiles right of the diagonal are skipped.  When a row block's last slab is done its accumulators are squared and
// added down the gauge axis in fp64.  The last row block's sweep sees every slab once: u^T k and the gauge-pixel flag ride on it.
__global__ __launch_bounds__(256, 4) void krig_variance_kernel(const float* __restrict__ Wi, const double* __restrict__ sol,
                                                            const int* __restrict__ pix, const int* __restrict__ counts,
                                                            const int* __restrict__ status, const int* __restrict__ cand,
                                                            const float* __restrict__ params, int model, int f0, int R, int T, int W,
                                                            int HW, int cap, int np, float* __restrict__ var) {
  __shared__ float slab[TS][SLAB_LD];
  __shared__ float At[RB][TS][A_LD];
  __shared__ double red[256];
  __shared__ int hits[256];
  const int s = blockIdx.y, fs = f0 + s * R, b = fs / T;
  const int n = min(counts[fs], np);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int p0 = blockIdx.x * PT;
  if (n == 0 || no_model(status[s], cand, b)) {       // NaN
    if (tid < PT && p0 + tid < HW)
      for (int t = 0; t < R; ++t) var[(size_t)(fs + t) * HW + p0 + tid] = __builtin_nanf("");
    return;
  }
  const float nug = params[b * 4], psill = params[b * 4 + 1], a = params[b * 4 + 2];
  const double* u = sol + (size_t)s * (R + 1) * np;
  const float* Ws = Wi + (size_t)s * np * np;
  const int* gp = pix + (size_t)fs * cap;
  const double su = sum_u(u, n, red);
  const int p = min(p0 + (tid & (PT - 1)), HW - 1);
  const int py = p / W, px = p % W;
  const int nt = (n + TS - 1) / TS;          // rows and columns past the gauges are identity against k = 0
  double q = 0.0, uk = 0.0;
  int hit = 0;
  for (int rb0 = 0; rb0 < nt; rb0 += RB) {
    const int rbn = min(RB, nt - rb0);
    const bool last = rb0 + RB >= nt;
    f32x16 acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[r][e] = 0.f;
    for (int sb = 0; sb < rb0 + rbn; ++sb) {
      __syncthreads();
      slab_fill(slab, gp, n, sb, py, px, nug, psill, a, model, [&](int i, float c0, bool at) {
        if (last) {
          uk = fma(u[i], (double)c0, uk);
          hit |= at;
        }
      });
#pragma unroll
      for (int r = 0; r < RB; ++r)
        if (r < rbn && rb0 + r >= sb) tile_stage(At[r], Ws + (size_t)(rb0 + r) * TS * np + sb * TS, np, TS);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < RB; ++r)
        if (r < rbn && rb0 + r >= sb) acc[r] = tile_mfma(At[r], slab, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int e = 0; e < 16; ++e) q = fma((double)acc[r][e], (double)acc[r][e], q);
  }
  q += __shfl_xor(q, 32, 64);                // the two row halves of the pixel's column
  __syncthreads();
  red[tid] = uk;
  hits[tid] = hit;
  __syncthreads();
  const int pi = wave * 32 + l31;
  if (lhi == 0 && p0 + pi < HW) {
    const double ukp = red[pi] + red[PT + pi];
    const double c00 = (double)psill + (double)nug;
    const double d = 1.0 - ukp;
    const double v = c00 - q + d * d / su;
    const float o = (hits[pi] | hits[PT + pi]) ? 0.f : (float)fmax(v, 0.0);
    for (int t = 0; t < R; ++t) var[(size_t)(fs + t) * HW + p0 + pi] = o;
  }
}

// ---- colsq [nsys][np] = column square-sums of W in fp64: workgroup (column tile, system), thread (c, r0) takes rows r0 (mod 8) from the
// diagonal tile down, the eight row classes are added in order
__global__ __launch_bounds__(256) void krig_colsq_kernel(const float* __restrict__ Wi, int np, double* __restrict__ colsq) {
  __shared__ double part[8][TS];
  const float* Ws = Wi + (size_t)blockIdx.y * np * np;
  const int j0 = blockIdx.x * TS;
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  double acc = 0.0;
  for (int k = j0 + r0; k < np; k += 8) {
    const double w = (double)Ws[(size_t)k * np + j0 + c];
    acc = fma(w, w, acc);
  }
  part[r0][c] = acc;
  __syncthreads();
  if (threadIdx.x < TS) {
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) t += part[r][c];
    colsq[(size_t)blockIdx.y * np + j0 + c] = t;
  }
}

// ---- LOO of frame f = f0 + s R + t from alpha, u, s and the column square-sums; NaN where there is no model or fewer than 2 gauges
__global__ __launch_bounds__(256) void krig_loo_kernel(const double* __restrict__ colsq, const double* __restrict__ sol,
                                                       const float* __restrict__ alpha, const float* __restrict__ z,
                                                       const int* __restrict__ counts, const int* __restrict__ status,
                                                       const int* __restrict__ cand, int f0, int R, int T, int cap, int np,
                                                       float* __restrict__ pred, float* __restrict__ var) {
  __shared__ double red[256];
  const int s = blockIdx.y, fs = f0 + s * R, f = fs + blockIdx.x;
  const int n = min(counts[fs], np);
  const double* u = sol + (size_t)s * (R + 1) * np;
  const double* cs = colsq + (size_t)s * np;
  const bool none = n < 2 || no_model(status[s], cand, f / T);
  const double su = sum_u(u, n, red);
  for (int i = threadIdx.x; i < cap; i += 256) {
    float pv = 0.f, vv = 0.f;
    if (i < n) {
      if (none) {
        pv = vv = __builtin_nanf("");
      } else {
        const double bii = cs[i] - u[i] * u[i] / su;
        pv = (float)((double)z[(size_t)f * cap + i] - (double)alpha[(size_t)f * cap + i] / bii);
        vv = (float)(1.0 / bii);
      }
    }
    pred[(size_t)f * cap + i] = pv;
    var[(size_t)f * cap + i] = vv;
  }
}

// ---- all-gauge IDW at the frame's own gauges with the gauge itself left out: one target gauge per thread, the shape of idw_all_kernel
__global__ __launch_bounds__(256) void idw_loo_kernel(const int* __restrict__ pix, const float* __restrict__ z, const int* __restrict__ counts,
                                                      int cap, float power, float* __restrict__ pred) {
  __shared__ int spix[PCHUNK];
  __shared__ float sz[PCHUNK];
  const int f = blockIdx.y;
  const int n = min(counts[f], cap);
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int tp = pix[(size_t)f * cap + min(t, cap - 1)];
  const int py = tp >> 16, px = tp & 0xffff;
  const float e = -0.5f * power;
  const bool square = power == 2.f;
  double num = 0.0, den = 0.0;
  for (int i0 = 0; i0 < n; i0 += PCHUNK) {
    __syncthreads();
    if (threadIdx.x < PCHUNK) {
      const bool in = i0 + (int)threadIdx.x < n;
      spix[threadIdx.x] = in ? pix[(size_t)f * cap + i0 + threadIdx.x] : 0;
      sz[threadIdx.x] = in ? z[(size_t)f * cap + i0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    const int cnt = min(PCHUNK, n - i0);
    for (int i = 0; i < cnt; ++i) {
      if (i0 + i == t) continue;
      const int g = spix[i];
      const int dy = py - (g >> 16), dx = px - (g & 0xffff);
      const int d2 = dy * dy + dx * dx;
      const float w = square ? 1.f / (float)d2 : powf((float)d2, e);
      num = fma((double)w, (double)sz[i], num);
      den += (double)w;
    }
  }
  if (t < cap) pred[(size_t)f * cap + t] = t < n ? (n < 2 ? __builtin_nanf("") : (float)(num / den)) : 0.f;
}

// ---- scores: part [F][5] = (n, sum e, sum |e|, sum e^2, sum e^2 / var) over the frame's gauges whose prediction (and variance,
// where there is one) is not NaN, e = z - pred; then the frames in order
__global__ __launch_bounds__(256) void loo_part_kernel(const float* __restrict__ z, const float* __restrict__ pred, const float* __restrict__ var,
                                                       const int* __restrict__ counts, int cap, double* __restrict__ part) {
  __shared__ double red[256];
  const int f = blockIdx.x;
  const int n = min(counts[f], cap);
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += 256) {
    const float pv = pred[(size_t)f * cap + i];
    const float vv = var != nullptr ? var[(size_t)f * cap + i] : 1.f;
    if (pv != pv || vv != vv) continue;
    const double e = (double)z[(size_t)f * cap + i] - (double)pv;
    a[0] += 1.0;
    a[1] += e;
    a[2] += fabs(e);
    a[3] += e * e;
    if (var != nullptr) a[4] += e * e / (double)vv;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double r = block_sum_d(a[k], red);
    if (threadIdx.x == 0) part[(size_t)f * 5 + k] = r;
  }
}

__global__ __launch_bounds__(256) void loo_total_kernel(const double* __restrict__ part, int F, double* __restrict__ out) {
  __shared__ double red[256];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double a = 0.0;
    for (int f = threadIdx.x; f < F; f += 256) a += part[(size_t)f * 5 + k];
    const double r = block_sum_d(a, red);
    if (threadIdx.x == 0) out[k] = r;
  }
}

}  // namespace
}  // namespace p2i

using namespace p2i;

extern "C" int p2i_krig_invert(const float* L, int nsys, int np, float* Winv, void* stream) {
  P2I_REQUIRE(L && Winv && L != Winv, "null pointer, or the inverse would overwrite the factor");
  P2I_REQUIRE(nsys > 0 && nsys <= 65535 && np > 0 && np % TS == 0 && np <= MAX_NP, "bad system shape %d x %d", nsys, np);
  hipStream_t s = (hipStream_t)stream;
  const int nt = np / TS;
  P2I_LAUNCH(krig_invdiag_kernel, dim3(nt, nsys), dim3(256), 0, s, L, np, Winv);
  if (nt > 1) P2I_LAUNCH(krig_invcol_kernel, dim3(nt - 1, nsys), dim3(256), 0, s, L, np, Winv);
  return launch_status();
}

extern "C" int p2i_krig_variance(const p2i_krig_systems* k, const float* Winv, const double* sol, int H, int W, float* var, void* stream) {
  if (int rc = krig_sys_check(k, KS_PIX | KS_COUNTS | KS_STATUS | KS_PARAMS | KS_MODEL | KS_NP, Winv && sol && var, H, W)) return rc;
  const int HW = H * W;
  P2I_LAUNCH(krig_variance_kernel, dim3(ceil_div(HW, PT), k->nsys), dim3(256), 0, (hipStream_t)stream, Winv, sol, k->pix, k->counts,
             (const int*)k->status, k->cand, k->params, k->model, k->f0, k->R, k->T, W, HW, k->cap, k->np, var);
  return launch_status();
}

extern "C" int p2i_krig_loo(const p2i_krig_systems* k, const float* Winv, const double* sol, const float* alpha, double* colsq, float* pred,
                            float* var, void* stream) {
  if (int rc = krig_sys_check(k, KS_Z | KS_COUNTS | KS_STATUS | KS_NP, Winv && sol && alpha && colsq && pred && var)) return rc;
  hipStream_t s = (hipStream_t)stream;
  P2I_LAUNCH(krig_colsq_kernel, dim3(k->np / TS, k->nsys), dim3(256), 0, s, Winv, k->np, colsq);
  P2I_LAUNCH(krig_loo_kernel, dim3(k->R, k->nsys), dim3(256), 0, s, (const double*)colsq, sol, alpha, k->z, k->counts,
             (const int*)k->status, k->cand, k->f0, k->R, k->T, k->cap, k->np, pred, var);
  return launch_status();
}

extern "C" int p2i_idw_loo(const int* pix, const float* z, const int* counts, int F, int cap, float power, float* pred, void* stream) {
  P2I_REQUIRE(pix && z && counts && pred, "null pointer");
  P2I_REQUIRE(F > 0 && F <= 65535 && cap > 0 && cap <= MAX_NP, "bad IDW shape");
  P2I_REQUIRE(power > 0.f, "IDW power must be positive");
  P2I_LAUNCH(idw_loo_kernel, dim3(ceil_div(cap, 256), F), dim3(256), 0, (hipStream_t)stream, pix, z, counts, cap, power, pred);
  return launch_status();
}

extern "C" int p2i_loo_scores(const float* z, const float* pred, const float* var, const int* counts, int F, int cap, double* part,
                              double* out, void* stream) {
  P2I_REQUIRE(z && pred && counts && part && out, "null pointer");
  P2I_REQUIRE(F > 0 && cap > 0, "bad shape");
  hipStream_t s = (hipStream_t)stream;
  P2I_LAUNCH(loo_part_kernel, dim3(F), dim3(256), 0, s, z, pred, var, counts, cap, part);
  P2I_LAUNCH(loo_total_kernel, dim3(1), dim3(256), 0, s, (const double*)part, F, out);
  return launch_status();
}
