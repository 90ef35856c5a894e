// Space-time ordinary kriging: every pixel of every frame of a sample from ALL gauges of ALL frames of that
// sample, one system per sample, with the metric space-time distance d = sqrt(dy^2 + dx^2 + kappa^2 dt^2) (kappa in pixels per frame)
// inside the covariance of krig_common.h.  Stages: per-frame compaction (classical.hip) -> gather into per-sample point sets ->
// [space-time variogram bins -> (kappa, range) candidate fit (classical.hip's one fit kernel, ST = true)] -> covariance build + the
// shared tiled Cholesky (classical.hip) ->
// p2i_krig_solve with the samples standing in for frames -> predictor.
//
// LAG: the bins, build and predictor kernels in the frame that moves with the rain, one velocity v = (v_y, v_x)
// in pixels per frame per sample (lagkrig.hip estimates it): d = sqrt((dy - v_y dt)^2 + (dx - v_x dt)^2 + kappa^2 dt^2).  The
// entry points run the LAG = true instantiations when they are given a velocity; the gather, the fit, the Cholesky and the solve do not
// see the distance and serve both.
//
// Number formats as in classical.hip: K, its factor and c0 are fp32 (the velocity enters them as an fp32 copy); the predictor's sum
// over the points is fp64; the variogram is fp64 throughout.  Every sum has a fixed order (no atomics).
#include "krig_common.h"

namespace p2i {
namespace {

// ---- gather: one workgroup per sample walks its T frames in order (the running offset is the exclusive scan of their counts) and
// appends each frame's gauges; stpix / stt / stz [B][cap] are zero past the count, stcounts[b] = the sum (it may exceed cap: the host
// has refused before)
__global__ __launch_bounds__(256) void stkrig_gather_kernel(const int* __restrict__ pix, const float* __restrict__ z,
                                                            const int* __restrict__ counts, int T, int fcap, int cap,
                                                            int* __restrict__ stpix, int* __restrict__ stt, float* __restrict__ stz,
                                                            int* __restrict__ stcounts) {
  const int b = blockIdx.x;
  int off = 0;
  for (int t = 0; t < T; ++t) {
    const int f = b * T + t;
    const int n = min(counts[f], fcap);
    for (int i = threadIdx.x; i < n; i += 256) {
      const int o = off + i;
      if (o < cap) {
        stpix[(size_t)b * cap + o] = pix[(size_t)f * fcap + i];
        stt[(size_t)b * cap + o] = t;
        stz[(size_t)b * cap + o] = z[(size_t)f * fcap + i];
      }
    }
    off += n;
  }
  for (int o = min(off, cap) + threadIdx.x; o < cap; o += 256) {
    stpix[(size_t)b * cap + o] = 0;
    stt[(size_t)b * cap + o] = 0;
    stz[(size_t)b * cap + o] = 0.f;
  }
  if (threadIdx.x == 0) stcounts[b] = off;
}

// ---- space-time variogram bins.  Workgroup (chunk, u, sample) takes temporal lag u: for every frame t < T - u the rows i = chunk
// (mod chunks) of frame t against the gauges j of frame t + u (j > i when u = 0, all j otherwise), binned by the SPATIAL distance.
// One temporal lag per workgroup keeps the [bin][thread] LDS image of krig_common.h (40 KiB) at its size with all 32 lags.
// LAG: the advected spatial distance h = |x_j - x_i - v u| in fp64, vel [B][2] fp64 (else null).  With v = 0 the radicand is the same
// exact integer and every later operation and its order are the same, so the bins are the LAG = false bins bit for bit.
// part [B][n_tlags + 1][chunks][n_lags][3] = (pairs, sum of (z_i - z_j)^2 / 2, sum of h)
template <bool LAG>
__global__ __launch_bounds__(BIN_THREADS) void stkrig_bins_kernel(const int* __restrict__ pix, const float* __restrict__ z,
                                                                  const int* __restrict__ counts, const double* __restrict__ vel,
                                                                  int T, int cap, int n_lags, double lagw, double* __restrict__ part) {
  VarioBins bins = vario_bins_lds();
  const int b = blockIdx.z, u = blockIdx.y, nu = gridDim.y, ch = blockIdx.x, nch = gridDim.x, tid = threadIdx.x;
  bins.clear(n_lags);
  const double hmax = (double)n_lags * lagw;
  double oy = 0.0, ox = 0.0;               // LAG: v u
  if constexpr (LAG) {
    oy = vel[b * 2] * (double)u;
    ox = vel[b * 2 + 1] * (double)u;
  }
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
        double h;
        if constexpr (LAG) {
          const double ey = (double)((pj >> 16) - (pi >> 16)) - oy, ex = (double)((pj & 0xffff) - (pi & 0xffff)) - ox;
          h = sqrt(ey * ey + ex * ex);
        } else {
          const int dy = (pi >> 16) - (pj >> 16), dx = (pi & 0xffff) - (pj & 0xffff);
          h = sqrt((double)(dy * dy + dx * dx));
        }
        bins.add(h, hmax, lagw, n_lags, zi, zb + j);
      }
    }
  }
  bins.reduce(n_lags, part, ((size_t)b * nu + u) * nch + ch);
}

// ---- covariance matrix of the point set of sample s0 + s (the tile writer of krig_common.h); LAG: lag_dist with velf [B][2] fp32
// (else null) in place of st_dist
template <bool LAG>
__global__ __launch_bounds__(256) void stkrig_build_kernel(const int* __restrict__ stpix, const int* __restrict__ stt,
                                                           const int* __restrict__ stcounts, const float* __restrict__ params,
                                                           const float* __restrict__ velf, int model, int s0, int cap, int np,
                                                           float* __restrict__ A) {
  const int s = blockIdx.z, b = s0 + s;
  const float nug = params[b * 4], psill = params[b * 4 + 1], a = params[b * 4 + 2], kap = params[b * 4 + 3];
  float vy = 0.f, vx = 0.f;
  if constexpr (LAG) {
    vy = velf[b * 2];
    vx = velf[b * 2 + 1];
  }
  const float k2 = kap * kap;
  const int* px = stpix + (size_t)b * cap;
  const int* pt = stt + (size_t)b * cap;
  cov_tile_write(A + (size_t)s * np * np, min(stcounts[b], np), np, [&](int i, int j) {
    const int pi = px[i], pj = px[j];
    const int dy = (pi >> 16) - (pj >> 16), dx = (pi & 0xffff) - (pj & 0xffff);
    float h;
    if constexpr (LAG)
      h = lag_dist((float)dy, (float)dx, (float)(pt[i] - pt[j]), vy, vx, k2);
    else
      h = st_dist(dy * dy + dx * dx, pt[i] - pt[j], k2);
    return cov_f(h, psill, a, model) + (i == j ? nug : 0.f);
  });
}

// ---- predictor: out[b][t][p] = mean[b] + sum_i alpha[b][i] c0((t, p), i), one pixel per thread, FG target frames per workgroup
// (blockIdx.z), the points staged in LDS PCHUNK at a time.  The integer pixel differences of a (pixel, point) pair are taken once.
// LAG = false: their d^2 feeds every frame of the group, each adding kappa^2 (t - t_i)^2; spherical: a pair spatially beyond the
// range adds nothing to any frame.  LAG = true: each frame takes lag_d2; spherical: a (pixel, point, frame) triple whose squared
// advected distance reaches range^2 has c0 = 0 and is skipped before the square root.
template <bool LAG>
__global__ __launch_bounds__(256) void stkrig_predict_kernel(const int* __restrict__ stpix, const int* __restrict__ stt,
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
  float vy = 0.f, vx = 0.f;
  if constexpr (LAG) {
    vy = velf[b * 2];
    vx = velf[b * 2 + 1];
  }
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
      if constexpr (!LAG)
        if ((float)d2 >= a2) continue;
      const float fdy = (float)dy, fdx = (float)dx;
      const int dt0 = t0 - st[i];
      const double ai = (double)sa[i];
#pragma unroll
      for (int q = 0; q < FG; ++q) {
        const int dt = dt0 + q;
        const auto add = [&](float h) {
          const float c0 = cov_f(h, psill, a, model) + ((d2 | dt) == 0 ? nug : 0.f);
          acc[q] = fma(ai, (double)c0, acc[q]);
        };
        if constexpr (LAG) {
          const float s2 = lag_d2(fdy, fdx, (float)dt, vy, vx, k2);
          if (s2 < a2) add(sqrtf(s2));
        } else {
          add(st_dist(d2, dt, k2));
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

extern "C" int p2i_stkrig_gather(const int* pix, const float* z, const int* counts, int B, int T, int fcap, int cap, int* stpix,
                                 int* stt, float* stz, int* stcounts, void* stream) {
  P2I_REQUIRE(pix && z && counts && stpix && stt && stz && stcounts, "null pointer");
  P2I_REQUIRE(B > 0 && T > 0 && (long long)B * T <= 65535, "bad sample shape %d x %d", B, T);
  P2I_REQUIRE(fcap > 0, "bad frame row length %d", fcap);
  if (int rc = krig_cap_check(cap)) return rc;
  P2I_LAUNCH(stkrig_gather_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pix, z, counts, T, fcap, cap, stpix, stt, stz, stcounts);
  return launch_status();
}

// The three stages that see the distance take the sample velocities (vel fp64 for the bins, velf fp32 for K and c0): NULL runs the
// LAG = false kernel, anything else the LAG = true one.
extern "C" int p2i_stkrig_bins(const int* pix, const float* z, const int* counts, const double* vel, int B, int T, int cap, int chunks,
                               int n_lags, int n_tlags, double lag_width, double* part, void* stream) {
  P2I_REQUIRE(pix && z && counts && part, "null pointer");
  P2I_REQUIRE(B > 0 && B <= 65535 && T > 0 && (long long)B * T <= 65535 && cap > 0 && chunks > 0 && chunks <= 1024, "bad variogram shape");
  if (int rc = krig_lags_check(n_lags, lag_width)) return rc;
  P2I_REQUIRE(n_tlags >= 0 && n_tlags <= MAX_TLAGS && n_tlags < T, "n_tlags must be 0..%d and below T", MAX_TLAGS);
  P2I_LAUNCH(vel ? stkrig_bins_kernel<true> : stkrig_bins_kernel<false>, dim3(chunks, n_tlags + 1, B), dim3(BIN_THREADS), 0,
             (hipStream_t)stream, pix, z, counts, vel, T, cap, n_lags, lag_width, part);
  return launch_status();
}

extern "C" int p2i_stkrig_fit(const double* part, int B, int chunks, int n_lags, int n_tlags, double lag_width, int model, double* bins,
                              double* fit, int* cand, float* params, void* stream) {
  P2I_REQUIRE(part && bins && fit && cand && params, "null pointer");
  P2I_REQUIRE(B > 0 && chunks > 0, "bad fit shape");
  if (int rc = krig_lags_check(n_lags, lag_width)) return rc;
  P2I_REQUIRE(n_tlags >= 0 && n_tlags <= MAX_TLAGS, "n_tlags must be 0..%d", MAX_TLAGS);
  if (int rc = krig_model_check(model)) return rc;
  krig_fit_launch(true, part, B, n_tlags + 1, chunks, n_lags, lag_width, model, bins, fit, cand, params, (hipStream_t)stream);
  return launch_status();
}

extern "C" int p2i_stkrig_factor(const p2i_krig_systems* k, const int* stt, const float* velf, float* L, void* stream) {
  if (int rc = krig_sys_check(k, KS_PIX | KS_COUNTS | KS_PARAMS | KS_STATUS | KS_MODEL | KS_NP, stt && L)) return rc;
  P2I_REQUIRE(k->R == 1 && k->T == 1, "a space-time system is one sample: R = T = 1");
  hipStream_t s = (hipStream_t)stream;
  const int nt = k->np / TS;
  P2I_LAUNCH(velf ? stkrig_build_kernel<true> : stkrig_build_kernel<false>, dim3(nt, nt, k->nsys), dim3(256), 0, s, k->pix, stt, k->counts,
             k->params, velf, k->model, k->f0, k->cap, k->np, L);
  krig_factor_tiles(L, k->nsys, k->np, k->status, s);
  return launch_status();
}

extern "C" int p2i_stkrig_predict(const int* stpix, const int* stt, const float* alpha, const float* mean, const int* stcounts,
                                  const float* params, const float* velf, int model, int B, int T, int H, int W, int cap, float* out,
                                  void* stream) {
  P2I_REQUIRE(stpix && stt && alpha && mean && stcounts && params && out, "null pointer");
  if (int rc = krig_frame_check(model, H, W)) return rc;
  P2I_REQUIRE(B > 0 && B <= 65535 && T > 0 && ceil_div(T, FG) <= 65535, "bad sample shape %d x %d", B, T);
  if (int rc = krig_cap_check(cap)) return rc;
  const int HW = H * W;
  P2I_LAUNCH(velf ? stkrig_predict_kernel<true> : stkrig_predict_kernel<false>, dim3(ceil_div(HW, 256), B, ceil_div(T, FG)), dim3(256), 0,
             (hipStream_t)stream, stpix, stt, alpha, mean, stcounts, params, velf, model, T, W, HW, cap, out);
  return launch_status();
}
