// Lagrangian space-time ordinary kriging: stkrig.hip's model with its distance measured in the frame that moves
// with the rain, d = sqrt((dy - v_y dt)^2 + (dx - v_x dt)^2 + kappa^2 dt^2), v = (v_y, v_x) in pixels per frame, one velocity per
// sample.  This file holds what is new in it: the velocity estimate from the gauges alone (a weighted cross-variogram score over a
// grid of candidate velocities) and the choice among the candidates.  Everything after the velocity is stkrig.hip's: its bins, build
// and predictor kernels are templates whose LAG = true instantiations take the velocity (p2i_stkrig_bins / _factor / _predict run
// them when they are given one), and p2i_stkrig_fit, krig_factor_tiles, p2i_krig_solve / _invert and the leave-one-site-out kernels of
// stkrig_loso.hip are reused as they are.
//
// Number formats: the velocity estimate is fp64 throughout; velf is its fp32 copy for K and c0.  Every sum has a fixed order (no
// atomics).
#include "krig_common.h"

namespace p2i {
namespace {

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
