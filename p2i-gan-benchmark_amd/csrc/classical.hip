// Classical (parameter-free) baselines: ordinary kriging in its dual form and all-gauge inverse-distance weighting, per (b, t) frame
// (DESIGN.md section 14).  Stages: point compaction -> [empirical variogram bins -> fit] -> covariance build + Cholesky factor ->
// triangular solves + dual coefficients -> pairwise-sum predictor; IDW shares the compaction and the predictor's shape.
//
// Gauges of a frame are its pixels with mask != 0 in raster order, packed as (y << 16) | x.  Systems are padded to a multiple of
// TS = 32 with identity rows / columns and zero right-hand sides, so a padded unknown is exactly 0 and never touches a result.
// Number formats: the covariance matrix and its factor are fp32 (fmaf); every long sum that feeds a result (substitutions, 1^T u,
// 1^T v, the predictor's sum over gauges, IDW's numerator and denominator) is accumulated in fp64 from fp32 terms; the variogram
// (bins and fit) is fp64 throughout.  Every sum has a fixed order (no atomics): results are identical from run to run.
#include "krig_common.h"

namespace p2i {
namespace {

constexpr int N_RANGE = 25;       // range candidates a_c = w 2^((c - 6) / 3)
constexpr int N_KAPPA = 17;       // anisotropy candidates kappa_q = 2^((q - 6) / 2) px / frame (space-time fit)
constexpr int RC = 8;            // right-hand sides fed from one covariance evaluation

// ---- compaction: one workgroup per frame.  pix / z [F][cap] (entries past the count are zero), info[f] = count (may exceed cap:
// the host refuses), info[F + f] = 1 if the frame's mask pattern differs from that of frame 0 of its sample
__global__ __launch_bounds__(256) void krig_compact_kernel(const float* __restrict__ masked, const float* __restrict__ mask, int F, int T,
                                                           int HW, int W, int cap, int* __restrict__ pix, float* __restrict__ z,
                                                           int* __restrict__ info) {
  __shared__ int wave_cnt[4];
  __shared__ int wave_diff[4];
  const int f = blockIdx.x;
  const float* m = mask + (size_t)f * HW;
  const float* m0 = mask + (size_t)(f / T) * T * HW;
  const float* xv = masked + (size_t)f * HW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int found = 0;
  bool diff = false;
  for (int base = 0; base < HW; base += 256) {
    const int p = base + threadIdx.x;
    const bool hit = p < HW && m[p] != 0.f;
    if (p < HW) diff |= (m0[p] != 0.f) != hit;
    const unsigned long long bal = __ballot(hit);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    int off = found;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    const int slot = off + before;
    if (hit && slot < cap) {
      pix[(size_t)f * cap + slot] = ((p / W) << 16) | (p % W);
      z[(size_t)f * cap + slot] = xv[p];
    }
    found += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
  for (int i = min(found, cap) + threadIdx.x; i < cap; i += 256) {
    pix[(size_t)f * cap + i] = 0;
    z[(size_t)f * cap + i] = 0.f;
  }
  const int any = __any(diff) ? 1 : 0;
  if (lane == 0) wave_diff[wave] = any;
  __syncthreads();
  if (threadIdx.x == 0) {
    info[f] = found;
    info[F + f] = wave_diff[0] | wave_diff[1] | wave_diff[2] | wave_diff[3];
  }
}

// ---- empirical variogram.  Workgroup (chunk, frame) takes the rows i = chunk (mod chunks) of the frame's pairs i < j into the
// [bin][thread] image of krig_common.h.
// part [F][chunks][n_lags][3] = (pairs, sum of (z_i - z_j)^2 / 2, sum of h)
__global__ __launch_bounds__(BIN_THREADS) void krig_bins_kernel(const int* __restrict__ pix, const float* __restrict__ z,
                                                                const int* __restrict__ counts, int cap, int n_lags, double lagw,
                                                                double* __restrict__ part) {
  VarioBins bins = vario_bins_lds();
  const int f = blockIdx.y, ch = blockIdx.x, nch = gridDim.x, tid = threadIdx.x;
  bins.clear(n_lags);
  const int n = min(counts[f], cap);
  const int* px = pix + (size_t)f * cap;
  const float* zf = z + (size_t)f * cap;
  const double hmax = (double)n_lags * lagw;
  for (int i = ch; i < n; i += nch) {
    const int pi = px[i];
    const double zi = (double)zf[i];
    for (int j = i + 1 + tid; j < n; j += BIN_THREADS) {
      const int pj = px[j];
      const int dy = (pi >> 16) - (pj >> 16), dx = (pi & 0xffff) - (pj & 0xffff);
      bins.add(sqrt((double)(dy * dy + dx * dx)), hmax, lagw, n_lags, zi, zf + j);
    }
  }
  bins.reduce(n_lags, part, (size_t)f * nch + ch);
}

// ---- fit, spatial (ST = false) and space-time (ST = true): one workgroup per sample.  Adds the chunks' partial bins in order, then
// candidate q 25 + c fits (nugget, psill) of gamma = nugget + psill g(sqrt(hbar^2 + (kappa_q u)^2) / a_c) by the count-weighted normal
// equations and fallbacks of krig_common.h; thread 0 keeps the smallest SSE (lowest q 25 + c on a tie, so that bins of u = 0 alone
// give the spatial fit with q = 0).  The spatial fit has the temporal lag u = 0 only (nu = 1, nch = its frames' chunks in order) and
// the 25 candidates of q = 0, in which kappa does not appear.
// part [B][nu][nch][n_lags][3], bins [B][nu][n_lags][3] (raw sums), cand [B] = q 25 + c (-1: degenerate), params [B][4] fp32 for the
// kriging kernels.  ST: fit [B][5] = (nugget, psill, range, kappa, sse), params = (nugget, psill, range, kappa), a harmless (0, 1, w, 1)
// when degenerate; spatial: fit [B][4] = (nugget, psill, range, sse), params = (nugget, psill, range, 0), (0, 1, w, 0) when degenerate
template <bool ST>
__global__ __launch_bounds__(ST ? 256 : 64) void krig_fit_kernel(const double* __restrict__ part, int nu, int nch, int n_lags, double lagw,
                                                                 int model, double* __restrict__ bins, double* __restrict__ fit,
                                                                 int* __restrict__ cand, float* __restrict__ params) {
  constexpr int NT = ST ? 256 : 64, NB = (ST ? MAX_TLAGS + 1 : 1) * MAX_LAGS, NC = (ST ? N_KAPPA : 1) * N_RANGE, NF = ST ? 5 : 4;
  __shared__ double sn[NB], sgam[NB], shb[NB];
  __shared__ double c_sse[NC], c_nug[NC], c_ps[NC];
  __shared__ int c_ok[NC];
  const int b = blockIdx.x, tid = threadIdx.x, nb = nu * n_lags;
  for (int e = tid; e < nb; e += NT) {
    const int u = ST ? e / n_lags : 0, k = ST ? e % n_lags : e;
    double c = 0.0, g = 0.0, h = 0.0;
    for (int p = 0; p < nch; ++p) {
      const double* q = part + ((((size_t)b * nu + u) * nch + p) * n_lags + k) * 3;
      c += q[0];
      g += q[1];
      h += q[2];
    }
    double* o = bins + ((size_t)b * nb + e) * 3;
    o[0] = c;
    o[1] = g;
    o[2] = h;
    sn[e] = c;
    sgam[e] = c > 0.0 ? g / c : 0.0;
    shb[e] = c > 0.0 ? h / c : 0.0;
  }
  __syncthreads();
  for (int cd = tid; cd < NC; cd += NT) {
    const double kap = exp2((double)(cd / N_RANGE - 6) * 0.5);
    const double a = lagw * exp2((double)(cd % N_RANGE - 6) / 3.0);
    const FitCand r = vario_fit_candidate(sn, sgam, nb, [&](int e) {
      if constexpr (!ST) return g_d(shb[e] / a, model);
      const double ku = kap * (double)(e / n_lags);
      const double d = e < n_lags ? shb[e] : sqrt(shb[e] * shb[e] + ku * ku);
      return g_d(d / a, model);
    });
    c_ok[cd] = r.ok;
    c_sse[cd] = r.sse;
    c_nug[cd] = r.nug;
    c_ps[cd] = r.ps;
  }
  __syncthreads();
  if (tid == 0) {
    int best = -1;
    for (int c = 0; c < NC; ++c)
      if (c_ok[c] && (best < 0 || c_sse[c] < c_sse[best])) best = c;
    double* o = fit + (size_t)b * NF;
    float* pf = params + (size_t)b * 4;
    cand[b] = best;
    if (best >= 0) {
      const double kap = exp2((double)(best / N_RANGE - 6) * 0.5);
      const double a = lagw * exp2((double)(best % N_RANGE - 6) / 3.0);
      o[0] = c_nug[best];
      o[1] = c_ps[best];
      o[2] = a;
      if constexpr (ST) o[3] = kap;
      o[NF - 1] = c_sse[best];
      pf[0] = (float)c_nug[best];
      pf[1] = (float)c_ps[best];
      pf[2] = (float)a;
      pf[3] = ST ? (float)kap : 0.f;
    } else {
      for (int k = 0; k < NF; ++k) o[k] = 0.0;
      pf[0] = 0.f;
      pf[1] = 1.f;
      pf[2] = (float)lagw;
      pf[3] = ST ? 1.f : 0.f;
    }
  }
}

// ---- covariance matrix of system s (gauges of frame f0 + s R), lower tiles only; identity on the padding
__global__ __launch_bounds__(256) void krig_build_kernel(const int* __restrict__ pix, const int* __restrict__ counts,
                                                         const float* __restrict__ params, int model, int f0, int R, int T, int cap, int np,
                                                         float* __restrict__ A) {
  const int s = blockIdx.z, f = f0 + s * R, b = f / T;
  const float nug = params[b * 4], psill = params[b * 4 + 1], a = params[b * 4 + 2];
  const int* px = pix + (size_t)f * cap;
  cov_tile_write(A + (size_t)s * np * np, min(counts[f], np), np, [&](int i, int j) {
    const int pi = px[i], pj = px[j];
    const int dy = (pi >> 16) - (pj >> 16), dx = (pi & 0xffff) - (pj & 0xffff);
    return cov_f(sqrtf((float)(dy * dy + dx * dx)), psill, a, model) + (i == j ? nug : 0.f);
  });
}

// ---- one panel of the right-looking Cholesky: factor the diagonal tile at k0 in LDS, then solve the rows below it against it (one
// row per thread, the row's 32 entries in registers).  A pivot that is not > 0 marks the system and is replaced by 1: the system's
// frames fall back to their gauge mean, and nothing non-finite is divided by.
__global__ __launch_bounds__(256) void krig_panel_kernel(float* __restrict__ A, int np, int k0, int* __restrict__ status) {
  __shared__ float D[TS][TS + 1];
  __shared__ int bad;
  float* As = A + (size_t)blockIdx.x * np * np;
  const int tid = threadIdx.x, c = tid & 31, r0 = tid >> 5;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) D[r0 + 8 * rr][c] = As[(size_t)(k0 + r0 + 8 * rr) * np + k0 + c];
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int j = 0; j < TS; ++j) {
    const float p = D[j][j];
    const bool ok = p > 0.f;
    const float d = ok ? sqrtf(p) : 1.f;
    __syncthreads();                                   // every thread has read the pivot
    if (tid < TS) {
      if (tid == j) {
        D[j][j] = d;
        if (!ok) bad = 1;
      } else if (tid > j) {
        D[tid][j] = D[tid][j] / d;
      }
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int i = r0 + 8 * rr;
      if (c > j && i >= c) D[i][c] = fmaf(-D[i][j], D[c][j], D[i][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int i = r0 + 8 * rr;
    if (c <= i) As[(size_t)(k0 + i) * np + k0 + c] = D[i][c];
  }
  for (int i = k0 + TS + tid; i < np; i += 256) {
    float4* row = reinterpret_cast<float4*>(As + (size_t)i * np + k0);
    float x[TS];
#pragma unroll
    for (int q = 0; q < TS / 4; ++q) {
      const float4 v = row[q];
      x[4 * q] = v.x;
      x[4 * q + 1] = v.y;
      x[4 * q + 2] = v.z;
      x[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int cc = 0; cc < TS; ++cc) {
      float acc = x[cc];
#pragma unroll
      for (int m = 0; m < cc; ++m) acc = fmaf(-x[m], D[cc][m], acc);
      x[cc] = acc / D[cc][cc];
    }
#pragma unroll
    for (int q = 0; q < TS / 4; ++q) row[q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
  }
  if (tid == 0 && bad) status[blockIdx.x] = 1;
}

// ---- trailing update after the panel at k0: tile (I, J), J <= I, of the rows / columns past the panel loses L[I][k] L[J][k]^T
__global__ __launch_bounds__(256) void krig_update_kernel(float* __restrict__ A, int np, int k0) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ float Li[TS][TS + 1], Lj[TS][TS + 1];
  float* As = A + (size_t)blockIdx.z * np * np;
  const int i0 = k0 + TS + blockIdx.y * TS, j0 = k0 + TS + blockIdx.x * TS;
  const int tid = threadIdx.x, c = tid & 31, r0 = tid >> 5;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int r = r0 + 8 * rr;
    Li[r][c] = As[(size_t)(i0 + r) * np + k0 + c];
    Lj[r][c] = As[(size_t)(j0 + r) * np + k0 + c];
  }
  __syncthreads();
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int r = r0 + 8 * rr;
    float* o = As + (size_t)(i0 + r) * np + j0 + c;
    float acc = *o;
#pragma unroll
    for (int m = 0; m < TS; ++m) acc = fmaf(-Li[r][m], Lj[c][m], acc);
    *o = acc;
  }
}

// ---- L L^T x = rhs for right-hand side q of system s: q = 0 is the ones vector, q >= 1 the values of frame f0 + s R + q - 1.
// The vector lives in LDS as fp64; per tile, wave 0 substitutes through the diagonal tile (lane = row, the solved entry handed on by
// a shuffle) and all threads then take the tile's contribution off the remaining rows.  sol [nsys][R + 1][np] fp64
__global__ __launch_bounds__(256) void krig_solve_kernel(const float* __restrict__ A, const float* __restrict__ z,
                                                         const int* __restrict__ counts, int f0, int R, int cap, int np,
                                                         double* __restrict__ sol) {
  extern __shared__ double y[];
  __shared__ float D[TS][TS + 1];
  const int s = blockIdx.y, q = blockIdx.x, f = f0 + s * R;
  const int n = min(counts[f], np);
  const float* As = A + (size_t)s * np * np;
  const int tid = threadIdx.x, c = tid & 31, r0 = tid >> 5;
  for (int i = tid; i < np; i += 256) y[i] = i < n ? (q == 0 ? 1.0 : (double)z[(size_t)(f + q - 1) * cap + i]) : 0.0;
  __syncthreads();
  for (int k0 = 0; k0 < np; k0 += TS) {                     // forward: L w = rhs
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) D[r0 + 8 * rr][c] = As[(size_t)(k0 + r0 + 8 * rr) * np + k0 + c];
    __syncthreads();
    if (tid < 64) {
      double val = y[k0 + c];
      for (int cc = 0; cc < TS; ++cc) {
        if (c == cc) val = val / (double)D[cc][cc];
        const double yc = __shfl(val, cc, 64);
        if (c > cc) val -= (double)D[c][cc] * yc;
      }
      if (tid < TS) y[k0 + c] = val;
    }
    __syncthreads();
    for (int i = k0 + TS + tid; i < np; i += 256) {
      const float4* row = reinterpret_cast<const float4*>(As + (size_t)i * np + k0);
      double acc = 0.0;
#pragma unroll
      for (int m = 0; m < TS / 4; ++m) {
        const float4 v = row[m];
        acc += (double)v.x * y[k0 + 4 * m];
        acc += (double)v.y * y[k0 + 4 * m + 1];
        acc += (double)v.z * y[k0 + 4 * m + 2];
        acc += (double)v.w * y[k0 + 4 * m + 3];
      }
      y[i] -= acc;
    }
    __syncthreads();
  }
  for (int k0 = np - TS; k0 >= 0; k0 -= TS) {               // backward: L^T x = w
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) D[r0 + 8 * rr][c] = As[(size_t)(k0 + r0 + 8 * rr) * np + k0 + c];
    __syncthreads();
    if (tid < 64) {
      double val = y[k0 + c];
      for (int cc = TS - 1; cc >= 0; --cc) {
        if (c == cc) val = val / (double)D[cc][cc];
        const double xc = __shfl(val, cc, 64);
        if (c < cc) val -= (double)D[cc][c] * xc;
      }
      if (tid < TS) y[k0 + c] = val;
    }
    __syncthreads();
    for (int i = tid; i < k0; i += 256) {
      double acc = 0.0;
#pragma unroll 8
      for (int m = 0; m < TS; ++m) acc += (double)As[(size_t)(k0 + m) * np + i] * y[k0 + m];
      y[i] -= acc;
    }
    __syncthreads();
  }
  double* o = sol + ((size_t)s * (R + 1) + q) * np;
  for (int i = tid; i < np; i += 256) o[i] = y[i];
}

// ---- dual coefficients of frame f = f0 + s R + t: m = 1^T v / 1^T u, alpha = v - m u.  A frame without gauges gives (0, 0); a
// degenerate sample (cand < 0) or a failed factorisation gives the gauge mean and alpha = 0.
__global__ __launch_bounds__(256) void krig_dual_kernel(const double* __restrict__ sol, const float* __restrict__ z,
                                                        const int* __restrict__ counts, const int* __restrict__ status,
                                                        const int* __restrict__ cand, int f0, int R, int T, int cap, int np,
                                                        float* __restrict__ alpha, float* __restrict__ mean) {
  __shared__ double red[256];
  const int s = blockIdx.y, t = blockIdx.x, fs = f0 + s * R, f = fs + t;
  const int n = min(counts[fs], np);
  const double* u = sol + (size_t)s * (R + 1) * np;
  const double* v = u + (size_t)(t + 1) * np;
  const float* zf = z + (size_t)f * cap;
  float* af = alpha + (size_t)f * cap;
  const bool fallback = n == 0 || no_model(status[s], cand, f / T);
  const double su = sum_u(u, n, red);
  double sv = 0.0, sz = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    sv += v[i];
    sz += (double)zf[i];
  }
  sv = block_sum_d(sv, red);
  sz = block_sum_d(sz, red);
  const double m = fallback ? (n > 0 ? sz / (double)n : 0.0) : sv / su;
  for (int i = threadIdx.x; i < cap; i += 256) af[i] = (!fallback && i < n) ? (float)(v[i] - m * u[i]) : 0.f;
  if (threadIdx.x == 0) mean[f] = (float)m;
}

// ---- predictor: out[f][p] = mean[f] + sum_i alpha[f][i] c0(p, i) for the frames f of set s (gauges of frame f0 + s R), one pixel per
// thread.  c0 is evaluated once per (pixel, gauge) and feeds up to RC frames of the set; blockIdx.z walks the set in groups of RC.
__global__ __launch_bounds__(256) void krig_predict_kernel(const int* __restrict__ pix, const float* __restrict__ alpha,
                                                           const float* __restrict__ mean, const int* __restrict__ counts,
                                                           const float* __restrict__ params, int model, int f0, int R, int T, int W, int HW,
                                                           int cap, float* __restrict__ out) {
  __shared__ int spix[PCHUNK];
  __shared__ float sa[RC][PCHUNK];
  const int s = blockIdx.y, fs = f0 + s * R, fg = fs + blockIdx.z * RC;
  const int nr = min(RC, R - (int)blockIdx.z * RC);
  const int n = min(counts[fs], cap);
  const int b = fs / T;
  const float nug = params[b * 4], psill = params[b * 4 + 1], a = params[b * 4 + 2];
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int py = p / W, px = p % W;
  double acc[RC];
#pragma unroll
  for (int q = 0; q < RC; ++q) acc[q] = 0.0;
  for (int i0 = 0; i0 < n; i0 += PCHUNK) {
    __syncthreads();
    if (threadIdx.x < PCHUNK) spix[threadIdx.x] = i0 + (int)threadIdx.x < n ? pix[(size_t)fs * cap + i0 + threadIdx.x] : 0;
    for (int e = threadIdx.x; e < RC * PCHUNK; e += 256) {
      const int q = e / PCHUNK, i = e % PCHUNK;
      sa[q][i] = (q < nr && i0 + i < n) ? alpha[(size_t)(fg + q) * cap + i0 + i] : 0.f;
    }
    __syncthreads();
    const int cnt = min(PCHUNK, n - i0);
    for (int i = 0; i < cnt; ++i) {
      const int g = spix[i];
      const int dy = py - (g >> 16), dx = px - (g & 0xffff);
      const int d2 = dy * dy + dx * dx;
      const double c0 = (double)(cov_f(sqrtf((float)d2), psill, a, model) + (d2 == 0 ? nug : 0.f));
#pragma unroll
      for (int q = 0; q < RC; ++q) acc[q] = fma((double)sa[q][i], c0, acc[q]);
    }
  }
  if (p < HW) {
#pragma unroll
    for (int q = 0; q < RC; ++q)
      if (q < nr) out[(size_t)(fg + q) * HW + p] = (float)((double)mean[fg + q] + acc[q]);
  }
}

// ---- all-gauge IDW of frame f: sum_i w_i z_i / sum_i w_i, w_i = h^-power; the gauge's own value on a gauge pixel; 0 without gauges
__global__ __launch_bounds__(256) void idw_all_kernel(const int* __restrict__ pix, const float* __restrict__ z, const int* __restrict__ counts,
                                                      int W, int HW, int cap, float power, float* __restrict__ out) {
  __shared__ int spix[PCHUNK];
  __shared__ float sz[PCHUNK];
  const int f = blockIdx.y;
  const int n = min(counts[f], cap);
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int py = p / W, px = p % W;
  const float e = -0.5f * power;
  const bool square = power == 2.f;
  double num = 0.0, den = 0.0;
  float hitv = 0.f;
  bool hit = false;
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
      const int g = spix[i];
      const int dy = py - (g >> 16), dx = px - (g & 0xffff);
      const int d2 = dy * dy + dx * dx;
      if (d2 == 0) {
        hit = true;
        hitv = sz[i];
      } else {
        const float w = square ? 1.f / (float)d2 : powf((float)d2, e);
        num = fma((double)w, (double)sz[i], num);
        den += (double)w;
      }
    }
  }
  if (p < HW) out[(size_t)f * HW + p] = n == 0 ? 0.f : (hit ? hitv : (float)(num / den));
}

}  // namespace
}  // namespace p2i

using namespace p2i;

// the panel / update driver over the lower tiles of nsys built systems (krig_common.h): shared with the space-time build of stkrig.hip
void p2i::krig_factor_tiles(float* L, int nsys, int np, int* status, hipStream_t s) {
  const int nt = np / TS;
  for (int k = 0; k < nt; ++k) {
    P2I_LAUNCH(krig_panel_kernel, dim3(nsys), dim3(256), 0, s, L, np, k * TS, status);
    const int rem = nt - k - 1;
    if (rem > 0) P2I_LAUNCH(krig_update_kernel, dim3(rem, rem, nsys), dim3(256), 0, s, L, np, k * TS);
  }
}

// the one variogram fit (krig_common.h): p2i_krig_fit here and p2i_stkrig_fit of stkrig.hip
void p2i::krig_fit_launch(bool st, const double* part, int B, int nu, int nch, int n_lags, double lagw, int model, double* bins,
                          double* fit, int* cand, float* params, hipStream_t s) {
  if (st)
    P2I_LAUNCH(krig_fit_kernel<true>, dim3(B), dim3(256), 0, s, part, nu, nch, n_lags, lagw, model, bins, fit, cand, params);
  else
    P2I_LAUNCH(krig_fit_kernel<false>, dim3(B), dim3(64), 0, s, part, nu, nch, n_lags, lagw, model, bins, fit, cand, params);
}

extern "C" int p2i_krig_compact(const float* masked, const float* mask, int B, int T, int H, int W, int cap, int* pix, float* z, int* info,
                                void* stream) {
  P2I_REQUIRE(masked && mask && pix && z && info, "null pointer");
  P2I_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE, "bad frame shape %d x %d x %d x %d", B, T, H, W);
  P2I_REQUIRE((long long)B * T <= 65535, "at most 65535 frames per call (got %lld)", (long long)B * T);
  if (int rc = krig_cap_check(cap)) return rc;
  P2I_LAUNCH(krig_compact_kernel, dim3(B * T), dim3(256), 0, (hipStream_t)stream, masked, mask, B * T, T, H * W, W, cap, pix, z, info);
  return launch_status();
}

extern "C" int p2i_krig_bins(const int* pix, const float* z, const int* counts, int F, int cap, int chunks, int n_lags, double lag_width,
                             double* part, void* stream) {
  P2I_REQUIRE(pix && z && counts && part, "null pointer");
  P2I_REQUIRE(F > 0 && F <= 65535 && cap > 0 && chunks > 0 && chunks <= 1024, "bad variogram shape");
  if (int rc = krig_lags_check(n_lags, lag_width)) return rc;
  P2I_LAUNCH(krig_bins_kernel, dim3(chunks, F), dim3(BIN_THREADS), 0, (hipStream_t)stream, pix, z, counts, cap, n_lags, lag_width, part);
  return launch_status();
}

extern "C" int p2i_krig_fit(const double* part, int B, int nparts, int n_lags, double lag_width, int model, double* bins, double* fit,
                            int* cand, float* params, void* stream) {
  P2I_REQUIRE(part && bins && fit && cand && params, "null pointer");
  P2I_REQUIRE(B > 0 && nparts > 0, "bad fit shape");
  if (int rc = krig_lags_check(n_lags, lag_width)) return rc;
  if (int rc = krig_model_check(model)) return rc;
  krig_fit_launch(false, part, B, 1, nparts, n_lags, lag_width, model, bins, fit, cand, params, (hipStream_t)stream);
  return launch_status();
}

extern "C" int p2i_krig_factor(const p2i_krig_systems* k, float* L, void* stream) {
  if (int rc = krig_sys_check(k, KS_PIX | KS_COUNTS | KS_PARAMS | KS_STATUS | KS_MODEL | KS_NP, L)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int nt = k->np / TS;
  P2I_LAUNCH(krig_build_kernel, dim3(nt, nt, k->nsys), dim3(256), 0, s, k->pix, k->counts, k->params, k->model, k->f0, k->R, k->T, k->cap,
             k->np, L);
  krig_factor_tiles(L, k->nsys, k->np, k->status, s);
  return launch_status();
}

extern "C" int p2i_krig_solve(const p2i_krig_systems* k, const float* L, double* sol, float* alpha, float* mean, void* stream) {
  if (int rc = krig_sys_check(k, KS_Z | KS_COUNTS | KS_STATUS | KS_NP, L && sol && alpha && mean)) return rc;
  const int R = k->R;
  P2I_REQUIRE(R + 1 <= 65535, "too many right-hand sides");
  hipStream_t s = (hipStream_t)stream;
  P2I_LAUNCH(krig_solve_kernel, dim3(R + 1, k->nsys), dim3(256), (size_t)k->np * sizeof(double), s, L, k->z, k->counts, k->f0, R, k->cap,
             k->np, sol);
  P2I_LAUNCH(krig_dual_kernel, dim3(R, k->nsys), dim3(256), 0, s, sol, k->z, k->counts, (const int*)k->status, k->cand, k->f0, R, k->T,
             k->cap, k->np, alpha, mean);
  return launch_status();
}

extern "C" int p2i_krig_predict(const p2i_krig_systems* k, const float* alpha, const float* mean, int H, int W, float* out, void* stream) {
  if (int rc = krig_sys_check(k, KS_PIX | KS_COUNTS | KS_PARAMS | KS_MODEL, alpha && mean && out, H, W)) return rc;
  const int HW = H * W, R = k->R;
  P2I_REQUIRE(ceil_div(R, RC) <= 65535, "too many frames per set");
  P2I_LAUNCH(krig_predict_kernel, dim3(ceil_div(HW, 256), k->nsys, ceil_div(R, RC)), dim3(256), 0, (hipStream_t)stream, k->pix, alpha, mean,
             k->counts, k->params, k->model, k->f0, R, k->T, W, HW, k->cap, out);
  return launch_status();
}

extern "C" int p2i_idw_all(const int* pix, const float* z, const int* counts, int F, int H, int W, int cap, float power, float* out,
                           void* stream) {
  P2I_REQUIRE(pix && z && counts && out, "null pointer");
  P2I_REQUIRE(F > 0 && F <= 65535 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE && cap > 0, "bad IDW shape");
  P2I_REQUIRE(power > 0.f, "IDW power must be positive");
  const int HW = H * W;
  P2I_LAUNCH(idw_all_kernel, dim3(ceil_div(HW, 256), F), dim3(256), 0, (hipStream_t)stream, pix, z, counts, W, HW, cap, power, out);
  return launch_status();
}
