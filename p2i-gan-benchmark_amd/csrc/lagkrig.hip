// Lagrangian space-time ordinary kriging: stkrig.hip's model with its distance measured in the frame that moves
// with the rain, d = sqrt((dy - v_y dt)^2 + (dx - v_x dt)^2 + kappa^2 dt^2), v = (v_y, v_x) in pixels per frame, one velocity per
// sample.  New here are the two ends: the velocity estimate from the gauges alone (a weighted cross-variogram score over a grid of
// candidate velocities), the variogram bins on the advected spatial distance, the covariance build and the predictor.  The middle is
// reused as it is: p2i_stkrig_fit, krig_factor_tiles, p2i_krig_solve / _invert and the leave-one-site-out kernels of stkrig_loso.hip.
//
// Number formats: the velocity estimate and the bins are fp64 throughout; K, its factor and c0 are fp32 (the velocity enters them as
// an fp32 copy); the predictor's sum over the points is fp64.  Every sum has a fixed order (no atomics).
#include "krig_common.h"

namespace p2i {
namespace {

constexpr int MAX_LAGS = 32;
constexpr int MAX_TLAGS = 7;
constexpr int BIN_THREADS = 64;
constexpr int FG = 8;             // target frames of one predictor workgroup
constexpr int VCHUNK = 128;       // gauges of the later frame staged in LDS per pass of the velocity kernel
constexpr int VPAIR = 32;         // pairs of one batch of its separable weight tables
constexpr int MAX_VHALF = 16;     // candidate grid (2 nhalf + 1)^2 <= 33 x 33
constexpr int VGRID = 2 * MAX_VHALF + 1;

// ---- velocity score.  Workgroup (chunk, sample) holds ALL candidates v = (i s, j s), index c = (i + nhalf) n + (j + nhalf), n = 2 nhalf
// + 1: thread tid takes c = tid and c = tid + blockDim.x (blockDim.x = the candidates rounded up to a wave, at most 1024; n n <= 1089).
// For every temporal lag u = 1 .. n_tlags and frame t < T - u the gauges j of frame t + u are staged in LDS VCHUNK at a time (as
// doubles), and the rows i = chunk (mod chunks) of frame t run against them:
//   w = exp(-|x_j - x_i - v u|^2 / (2 r0^2)),  W += w,  S += w (z_i - z_j)^2 / 2,  N += w where x_j != x_i
// The weight is separable over the grid, w = a[j][i'] b[j][j'] with a = exp(-(dy - i' s u)^2 / (2 r0^2)) and b the same in x, so a batch
// of VPAIR pairs costs 2 n VPAIR fp64 exponentials for the whole workgroup (tables in LDS, filled by all threads) in place of one per
// pair and candidate; a candidate then pays two LDS reads, one product and three fma per pair.
// N is the support of a candidate among the pairs of DISTINCT pixels: with gauges that stay where they are, the same-pixel pairs put
// one full-weight pair per site and frame pair into W(0) and into no fast candidate, so W cannot say which candidates are thin.
// part [B][chunks][n n][3] = (W, S, N)
__global__ __launch_bounds__(1024) void lagkrig_velocity_kernel(const int* __restrict__ pix, const float* __restrict__ z,
                                                                const int* __restrict__ counts, int T, int cap, int n_tlags, int nhalf,
                                                                double vstep, double inv2r2, double* __restrict__ part) {
  __shared__ double sy[VCHUNK], sx[VCHUNK], sz[VCHUNK];
  __shared__ double ta[VPAIR][VGRID], tb[VPAIR][VGRID];          // a[j][i'], b[j][j'] of the batch
  __shared__ double2 tg[VPAIR];                                  // ((z_i - z_j)^2 / 2, 1 where x_j != x_i else 0)
  const int b = blockIdx.y, ch = blockIdx.x, nch = gridDim.x, tid = threadIdx.x, nth = blockDim.x;
  const int n = 2 * nhalf + 1, ncand = n * n;
  int ci[2], cj[2];
  double Wv[2], Sv[2], Nv[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int c = min(tid + s * nth, ncand - 1);          // a slot past the last candidate repeats it and writes nothing
    ci[s] = c / n;
    cj[s] = c % n;
    Wv[s] = Sv[s] = Nv[s] = 0.0;
  }
  const bool two = nth < ncand;          // uniform: a second slot exists
  for (int u = 1; u <= n_tlags; ++u) {
    const double su = vstep * (double)u;
    for (int t = 0; t + u < T; ++t) {
      const int fa = b * T + t, fb = fa + u;
      const int na = min(counts[fa], cap), nb = min(counts[fb], cap);
      const int* pa = pix + (size_t)fa * cap;
      const float* za = z + (size_t)fa * cap;
      for (int j0 = 0; j0 < nb; j0 += VCHUNK) {
        const int cnt = min(VCHUNK, nb - j0);
        __syncthreads();
        for (int j = tid; j < cnt; j += nth) {
          const int pj = pix[(size_t)fb * cap + j0 + j];
          sy[j] = (double)(pj >> 16);
          sx[j] = (double)(pj & 0xffff);
          sz[j] = (double)z[(size_t)fb * cap + j0 + j];
        }
        for (int i = ch; i < na; i += nch) {
          const int pi = pa[i];
          const double yi = (double)(pi >> 16), xi = (double)(pi & 0xffff), zi = (double)za[i];
          for (int jb = 0; jb < cnt; jb += VPAIR) {
            const int pb = min(VPAIR, cnt - jb);
            __syncthreads();          // the staged gauges are written; the previous batch's tables are read
            for (int e = tid; e < 2 * pb * n; e += nth) {
              const int half = e / (pb * n), r = e - half * (pb * n), j = r / n, k = r - j * n;
              const double d = (half ? sx[jb + j] - xi : sy[jb + j] - yi) - (double)(k - nhalf) * su;
              (half ? tb : ta)[j][k] = exp(-(d * d) * inv2r2);
            }
            for (int j = tid; j < pb; j += nth) {
              const double d = zi - sz[jb + j];
              tg[j] = make_double2(0.5 * (d * d), (sy[jb + j] == yi && sx[jb + j] == xi) ? 0.0 : 1.0);
            }
            __syncthreads();
#pragma unroll 8
            for (int j = 0; j < pb; ++j) {
              const double2 g = tg[j];
              const double w0 = ta[j][ci[0]] * tb[j][cj[0]];
              Wv[0] += w0;
              Sv[0] = fma(w0, g.x, Sv[0]);
              Nv[0] = fma(w0, g.y, Nv[0]);
              if (two) {
                const double w1 = ta[j][ci[1]] * tb[j][cj[1]];
                Wv[1] += w1;
                Sv[1] = fma(w1, g.x, Sv[1]);
                Nv[1] = fma(w1, g.y, Nv[1]);
              }
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int c = tid + s * nth;
    if (c < ncand) {
      double* o = part + (((size_t)b * nch + ch) * ncand + c) * 3;
      o[0] = Wv[s];
      o[1] = Sv[s];
      o[2] = Nv[s];
    }
  }
}

// ---- velocity choice: one workgroup per sample adds the chunks' partials in order into weight [B][n n] = W(v), support [B][n n] =
// N(v) and score [B][n n] = S(v) / W(v) (+inf where W = 0); thread 0 then takes, among the candidates with N(v) >= N(0) / 2, the
// smallest score, on a tie the smaller v_y^2 + v_x^2, then the lower index.  No pair or zero variance: every score ties and v = 0 wins.
// vel [B][2] fp64 = (v_y, v_x), velf [B][2] its fp32 copy, vcand [B] the index
__global__ __launch_bounds__(256) void lagkrig_pick_kernel(const double* __restrict__ part, int nch, int nhalf, double vstep,
                                                           double* __restrict__ score, double* __restrict__ weight,
                                                           double* __restrict__ support, double* __restrict__ vel, float* __restrict__ velf, int* __restrict__ vcand) {
  const int b = blockIdx.x, n = 2 * nhalf + 1, ncand = n * n;
  double* sc = score + (size_t)b * ncand;
  double* wt = weight + (size_t)b * ncand;
  double* sp = support + (size_t)b * ncand;
  for (int c = threadIdx.x; c < ncand; c += 256) {
    double Wv = 0.0, Sv = 0.0, Nv = 0.0;
    for (int p = 0; p < nch; ++p) {
      const double* q = part + (((size_t)b * nch + p) * ncand + c) * 3;
      Wv += q[0];
      Sv += q[1];
      Nv += q[2];
    }
    wt[c] = Wv;
    sp[c] = Nv;
    sc[c] = Wv > 0.0 ? Sv / Wv : (double)INFINITY;
  }
  __syncthreads();          // the tables are this workgroup's own global writes
  if (threadIdx.x == 0) {
    const int c0 = nhalf * n + nhalf;
    const double need = 0.5 * sp[c0];
    int best = c0, bi = 0, bj = 0;          // v = 0 is always eligible
    for (int c = 0; c < ncand; ++c) {
      if (!(sp[c] >= need)) continue;
      const int i = c / n - nhalf, j = c % n - nhalf;
      const double s = sc[c], sb = sc[best];
      const int r2 = i * i + j * j, rb = bi * bi + bj * bj;
      if (s < sb || (s == sb && (r2 < rb || (r2 == rb && c < best)))) {
        best = c;
        bi = i;
        bj = j;
      }
    }
    const double vy = (double)bi * vstep, vx = (double)bj * vstep;
    vel[b * 2] = vy;
    vel[b * 2 + 1] = vx;
    velf[b * 2] = (float)vy;
    velf[b * 2 + 1] = (float)vx;
    vcand[b] = best;
  }
}

// ---- variogram bins: stkrig_bins_kernel with the advected spatial distance h = |x_j - x_i - v u| of a pair (i in frame t, j in
// frame t + u).  With v = 0 the radicand is the same exact integer and every later operation and its order are
// stkrig_bins_kernel's, so the bins are its bins bit for bit.
// part [B][n_tlags + 1][chunks][n_lags][3] = (pairs, sum of (z_i - z_j)^2 / 2, sum of h)
__global__ __launch_bounds__(BIN_THREADS) void lagkrig_bins_kernel(const int* __restrict__ pix, const float* __restrict__ z,
                                                                   const int* __restrict__ counts, const double* __restrict__ vel,
                                                                   int T, int cap, int n_lags, double lagw, double* __restrict__ part) {
  __shared__ double sg[MAX_LAGS][BIN_THREADS];
  __shared__ double sh[MAX_LAGS][BIN_THREADS];
  __shared__ unsigned sc[MAX_LAGS][BIN_THREADS];
  const int b = blockIdx.z, u = blockIdx.y, nu = gridDim.y, ch = blockIdx.x, nch = gridDim.x, tid = threadIdx.x;
  for (int k = 0; k < n_lags; ++k) {
    sg[k][tid] = 0.0;
    sh[k][tid] = 0.0;
    sc[k][tid] = 0u;
  }
  const double hmax = (double)n_lags * lagw;
  const double oy = vel[b * 2] * (double)u, ox = vel[b * 2 + 1] * (double)u;
  for (int t = 0; t + u < T; ++t) {
    const int fa = b * T + t, fb = fa + u;
    const int na = min(counts[fa], cap), nb = min(counts[fb], cap);
    const int* pa = pix + (size_t)fa * cap;
    const int* pb = pix + (size_t)fb * cap;
    const float* za = z + (size_t)fa * cap;
    const float* zb = z + (size_t)fb * cap;
    for (int i = ch; i < na; i += nch) {
      const int pi = pa[i];
      const double zi = (double)za[i];
      for (int j = (u == 0 ? i + 1 : 0) + tid; j < nb; j += BIN_THREADS) {
        const int pj = pb[j];
        const double ey = (double)((pj >> 16) - (pi >> 16)) - oy, ex = (double)((pj & 0xffff) - (pi & 0xffff)) - ox;
        const double h = sqrt(ey * ey + ex * ex);
        if (h < hmax) {
          const int k = min((int)floor(h / lagw), n_lags - 1);
          const double d = zi - (double)zb[j];
          sg[k][tid] += 0.5 * (d * d);
          sh[k][tid] += h;
          sc[k][tid] += 1u;
        }
      }
    }
  }
  __syncthreads();
  for (int k = tid; k < n_lags; k += BIN_THREADS) {
    double g = 0.0, h = 0.0, c = 0.0;
    for (int t = 0; t < BIN_THREADS; ++t) {
      g += sg[k][t];
      h += sh[k][t];
      c += (double)sc[k][t];
    }
    double* o = part + ((((size_t)b * nu + u) * nch + ch) * n_lags + k) * 3;
    o[0] = c;
    o[1] = g;
    o[2] = h;
  }
}

// ---- covariance matrix of the point set of sample s0 + s, lower tiles only; identity on the padding (stkrig_build_kernel's layout)
__global__ __launch_bounds__(256) void lagkrig_build_kernel(const int* __restrict__ stpix, const int* __restrict__ stt,
                                                            const int* __restrict__ stcounts, const float* __restrict__ params,
                                                            const float* __restrict__ velf, int model, int s0, int cap, int np,
                                                            float* __restrict__ A) {
  if (blockIdx.x > blockIdx.y) return;
  const int s = blockIdx.z, b = s0 + s;
  const int n = min(stcounts[b], np);
  const float nug = params[b * 4], psill = params[b * 4 + 1], a = params[b * 4 + 2], kap = params[b * 4 + 3];
  const float vy = velf[b * 2], vx = velf[b * 2 + 1];
  const float k2 = kap * kap;
  const int* px = stpix + (size_t)b * cap;
  const int* pt = stt + (size_t)b * cap;
  float* As = A + (size_t)s * np * np;
  const int j = blockIdx.x * TS + (threadIdx.x & 31);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int i = blockIdx.y * TS + (threadIdx.x >> 5) + 8 * rr;
    float v = i == j ? 1.f : 0.f;
    if (i < n && j < n) {
      const int pi = px[i], pj = px[j];
      const int dy = (pi >> 16) - (pj >> 16), dx = (pi & 0xffff) - (pj & 0xffff);
      v = cov_f(lag_dist((float)dy, (float)dx, (float)(pt[i] - pt[j]), vy, vx, k2), psill, a, model) + (i == j ? nug : 0.f);
    }
    As[(size_t)i * np + j] = v;
  }
}

// ---- predictor: out[b][t][p] = mean[b] + sum_i alpha[b][i] c0((t, p), i), one pixel per thread, FG target frames per workgroup
// (blockIdx.z), the points staged in LDS PCHUNK at a time.  The pixel differences of a (pixel, point) pair are taken once; each target
// frame then costs lag_dist, one cov_f and the fp64 accumulate.  Spherical: a (pixel, point, frame) triple whose squared advected
// distance reaches range^2 has c0 = 0 and is skipped before the square root.
__global__ __launch_bounds__(256) void lagkrig_predict_kernel(const int* __restrict__ stpix, const int* __restrict__ stt,
                                                              const float* __restrict__ alpha, const float* __restrict__ mean,
                                                              const int* __restrict__ stcounts, const float* __restrict__ params,
                                                              const float* __restrict__ velf, int model, int T, int W, int HW, int cap,
                                                              float* __restrict__ out) {
  __shared__ int spix[PCHUNK];
  __shared__ int st[PCHUNK];
  __shared__ float sa[PCHUNK];
  const int b = blockIdx.y, t0 = blockIdx.z * FG;
  const int nr = min(FG, T - t0);
  const int n = min(stcounts[b], cap);
  const float nug = params[b * 4], psill = params[b * 4 + 1], a = params[b * 4 + 2], kap = params[b * 4 + 3];
  const float vy = velf[b * 2], vx = velf[b * 2 + 1];
  const float k2 = kap * kap;
  const float a2 = model == 1 ? a * a : 3.0e38f;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int py = p / W, px = p % W;
  double acc[FG];
#pragma unroll
  for (int q = 0; q < FG; ++q) acc[q] = 0.0;
  for (int i0 = 0; i0 < n; i0 += PCHUNK) {
    __syncthreads();
    if (threadIdx.x < PCHUNK) {
      const bool in = i0 + (int)threadIdx.x < n;
      const size_t e = (size_t)b * cap + i0 + threadIdx.x;
      spix[threadIdx.x] = in ? stpix[e] : 0;
      st[threadIdx.x] = in ? stt[e] : 0;
      sa[threadIdx.x] = in ? alpha[e] : 0.f;
    }
    __syncthreads();
    const int cnt = min(PCHUNK, n - i0);
    for (int i = 0; i < cnt; ++i) {
      const int g = spix[i];
      const int dy = py - (g >> 16), dx = px - (g & 0xffff);
      const int d2 = dy * dy + dx * dx;
      const float fdy = (float)dy, fdx = (float)dx;
      const int dt0 = t0 - st[i];
      const double ai = (double)sa[i];
#pragma unroll
      for (int q = 0; q < FG; ++q) {
        const int dt = dt0 + q;
        const float s2 = lag_d2(fdy, fdx, (float)dt, vy, vx, k2);
        if (s2 < a2) {
          const float c0 = cov_f(sqrtf(s2), psill, a, model) + ((d2 | dt) == 0 ? nug : 0.f);
          acc[q] = fma(ai, (double)c0, acc[q]);
        }
      }
    }
  }
  if (p < HW) {
    const double m = (double)mean[b];
#pragma unroll
    for (int q = 0; q < FG; ++q)
      if (q < nr) out[((size_t)b * T + t0 + q) * HW + p] = (float)(m + acc[q]);
  }
}

}  // namespace
}  // namespace p2i

using namespace p2i;

extern "C" int p2i_lagkrig_velocity(const int* pix, const float* z, const int* counts, int B, int T, int cap, int chunks, int n_tlags,
                                    int nhalf, double vstep, double bandwidth, double* part, void* stream) {
  P2I_REQUIRE(pix && z && counts && part, "null pointer");
  P2I_REQUIRE(B > 0 && B <= 65535 && T > 0 && (long long)B * T <= 65535 && cap > 0 && chunks > 0 && chunks <= 1024, "bad velocity shape");
  P2I_REQUIRE(n_tlags >= 0 && n_tlags <= MAX_TLAGS && n_tlags < T, "n_tlags must be 0..%d and below T", MAX_TLAGS);
  P2I_REQUIRE(nhalf >= 0 && nhalf <= MAX_VHALF, "the candidate grid is at most %d x %d", 2 * MAX_VHALF + 1, 2 * MAX_VHALF + 1);
  P2I_REQUIRE(vstep > 0.0 && bandwidth > 0.0, "the velocity step and the bandwidth must be positive");
  const int n = 2 * nhalf + 1;
  const int threads = min(1024, ceil_div(n * n, 64) * 64);          // two candidates per thread beyond 1024
  P2I_LAUNCH(lagkrig_velocity_kernel, dim3(chunks, B), dim3(threads), 0, (hipStream_t)stream, pix, z, counts, T, cap, n_tlags, nhalf, vstep,
             1.0 / (2.0 * bandwidth * bandwidth), part);
  return launch_status();
}

extern "C" int p2i_lagkrig_pick(const double* part, int B, int chunks, int nhalf, double vstep, double* score, double* weight, double* support,
                                double* vel, float* velf, int* vcand, void* stream) {
  P2I_REQUIRE(part && score && weight && support && vel && velf && vcand, "null pointer");
  P2I_REQUIRE(B > 0 && B <= 65535 && chunks > 0 && chunks <= 1024, "bad velocity shape");
  P2I_REQUIRE(nhalf >= 0 && nhalf <= MAX_VHALF && vstep > 0.0, "the candidate grid is at most %d x %d with a positive step", 2 * MAX_VHALF + 1,
              2 * MAX_VHALF + 1);
  P2I_LAUNCH(lagkrig_pick_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, part, chunks, nhalf, vstep, score, weight, support, vel, velf,
             vcand);
  return launch_status();
}

extern "C" int p2i_lagkrig_bins(const int* pix, const float* z, const int* counts, const double* vel, int B, int T, int cap, int chunks,
                                int n_lags, int n_tlags, double lag_width, double* part, void* stream) {
  P2I_REQUIRE(pix && z && counts && vel && part, "null pointer");
  P2I_REQUIRE(B > 0 && B <= 65535 && T > 0 && (long long)B * T <= 65535 && cap > 0 && chunks > 0 && chunks <= 1024, "bad variogram shape");
  P2I_REQUIRE(n_lags > 0 && n_lags <= MAX_LAGS && lag_width > 0.0, "n_lags must be 1..%d with a positive lag width", MAX_LAGS);
  P2I_REQUIRE(n_tlags >= 0 && n_tlags <= MAX_TLAGS && n_tlags < T, "n_tlags must be 0..%d and below T", MAX_TLAGS);
  P2I_LAUNCH(lagkrig_bins_kernel, dim3(chunks, n_tlags + 1, B), dim3(BIN_THREADS), 0, (hipStream_t)stream, pix, z, counts, vel, T, cap, n_lags,
             lag_width, part);
  return launch_status();
}

extern "C" int p2i_lagkrig_factor(const int* stpix, const int* stt, const int* stcounts, const float* params, const float* velf, int model,
                                  int s0, int nsys, int np, int cap, float* L, int* status, void* stream) {
  P2I_REQUIRE(stpix && stt && stcounts && params && velf && L && status, "null pointer");
  P2I_REQUIRE(model == 0 || model == 1, "variogram model must be 0 (exponential) or 1 (spherical)");
  if (int rc = krig_sys_check(s0, 1, 1, nsys, np, cap)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int nt = np / TS;
  P2I_LAUNCH(lagkrig_build_kernel, dim3(nt, nt, nsys), dim3(256), 0, s, stpix, stt, stcounts, params, velf, model, s0, cap, np, L);
  krig_factor_tiles(L, nsys, np, status, s);
  return launch_status();
}

extern "C" int p2i_lagkrig_predict(const int* stpix, const int* stt, const float* alpha, const float* mean, const int* stcounts,
                                   const float* params, const float* velf, int model, int B, int T, int H, int W, int cap, float* out,
                                   void* stream) {
  P2I_REQUIRE(stpix && stt && alpha && mean && stcounts && params && velf && out, "null pointer");
  P2I_REQUIRE(model == 0 || model == 1, "variogram model must be 0 (exponential) or 1 (spherical)");
  P2I_REQUIRE(H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE, "bad frame shape");
  P2I_REQUIRE(B > 0 && B <= 65535 && T > 0 && ceil_div(T, FG) <= 65535, "bad sample shape %d x %d", B, T);
  P2I_REQUIRE(cap > 0 && cap % TS == 0 && cap <= MAX_NP, "cap must be a multiple of %d, at most %d (got %d)", TS, MAX_NP, cap);
  const int HW = H * W;
  P2I_LAUNCH(lagkrig_predict_kernel, dim3(ceil_div(HW, 256), B, ceil_div(T, FG)), dim3(256), 0, (hipStream_t)stream, stpix, stt, alpha, mean,
             stcounts, params, velf, model, T, W, HW, cap, out);
  return launch_status();
}
