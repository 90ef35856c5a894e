// Leave-one-site-out (LOSO) cross-validation of space-time ordinary kriging.  A site is the set of a sample's
// points that share a pixel (one per frame in which the pixel is a gauge, so at most T).  With A = [[K, 1], [1^T, 0]] and B = A^-1,
// the top-left block of B is W^T W - u u^T / s (W = L^-1, u = K^-1 1, s = 1^T u), and for a site S
//   B_SS = (W^T W)_SS - u_S u_S^T / s,  e_S = B_SS^-1 alpha_S,  zhat_-S = z_S - e_S,  sigma^2_-S = diag(B_SS^-1)
// (the block form of Dubrule's identity): one factorisation and one inverse per sample, no refits.  Stages: site-major point set
// (the points sorted by (pixel, frame), so that a site is a contiguous run) -> p2i_stkrig_factor / p2i_krig_solve / p2i_krig_invert
// on it, unchanged -> the band of W^T W that holds every site block -> one small fp64 system per site.
//
// Number formats: W is fp32 as the inverse leaves it; the band Gram (products of fp32 entries are exact in fp64), B_SS, its Cholesky
// and everything after it are fp64.  Every sum has a fixed order and there are no atomics: results are identical from run to run.
#include "krig_common.h"

namespace p2i {
namespace {

constexpr int GK = 32;            // rows of W staged per step of the band Gram
constexpr int PPT = MAX_NP / 256; // points per thread of the site-major gather

// ---- site-major point set: one workgroup per sample.  The frames' gauges are read frame-major into LDS; the rank of point i in
// (pixel, frame) order is the count of points j with pix_j < pix_i, or pix_j = pix_i and j < i (a pixel appears once per frame, so
// the frame-major index orders equal pixels by frame): one 64-bit compare of (pix << 12) | index, the index being below 4096.  perm[rank] = i then gives the sorted set, a site starts where the sorted
// pixel changes, and the site index is the exclusive count of starts (per-thread runs, then the 256 run totals in order).
// Outputs: stpix / stt / stz [B][cap] (zero past the count), stcounts [B], site_start [B][cap + 1] (run starts, the count from entry
// nsites on), nsites [B], psite [B][cap] (site of a sorted point, -1 past the count), back [B][cap] (t fcap + rank in frame, -1 past the
// count), fsite [B T][fcap] (site of a frame's gauge in the per-frame layout, -1 past the frame's count)
__global__ __launch_bounds__(256) void stkrig_gather_sites_kernel(const int* __restrict__ pix, const float* __restrict__ z,
                                                                  const int* __restrict__ counts, int T, int fcap, int cap,
                                                                  int* __restrict__ stpix, int* __restrict__ stt, float* __restrict__ stz,
                                                                  int* __restrict__ stcounts, int* __restrict__ site_start,
                                                                  int* __restrict__ nsites, int* __restrict__ psite, int* __restrict__ back,
                                                                  int* __restrict__ fsite) {
  __shared__ int spix[MAX_NP];
  __shared__ int sback[MAX_NP];
  __shared__ int perm[MAX_NP];
  __shared__ int scnt[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t fbase = (size_t)b * T * fcap;
  int off = 0;
  for (int t = 0; t < T; ++t) {
    const int f = b * T + t;
    const int nf = min(counts[f], fcap);
    for (int i = tid; i < fcap; i += 256) {
      const int o = off + i;
      if (i < nf && o < cap) {
        spix[o] = pix[(size_t)f * fcap + i];
        sback[o] = t * fcap + i;
      } else {
        fsite[(size_t)f * fcap + i] = -1;
      }
    }
    off += nf;
  }
  const int n = min(off, cap);
  __syncthreads();
  unsigned long long key[PPT];                  // this thread's points i = tid + 256 k in registers, as (pix << 12) | i: one compare per pair,
  int rk[PPT];                                  // and one LDS read of pix_j serves them all
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int i = tid + 256 * k;
    key[k] = ((unsigned long long)(unsigned)(i < n ? spix[i] : 0) << 12) | (unsigned)i;
    rk[k] = 0;
  }
  for (int j = 0; j < n; ++j) {
    const unsigned long long kq = ((unsigned long long)(unsigned)spix[j] << 12) | (unsigned)j;
#pragma unroll
    for (int k = 0; k < PPT; ++k) rk[k] += kq < key[k] ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < PPT; ++k)
    if (tid + 256 * k < n) perm[rk[k]] = tid + 256 * k;
  __syncthreads();
  const int per = (cap + 255) / 256;
  const int r0 = tid * per, r1 = min(cap, r0 + per);
  int starts = 0;
  for (int r = r0; r < min(r1, n); ++r) starts += (r == 0 || spix[perm[r]] != spix[perm[r - 1]]) ? 1 : 0;
  scnt[tid] = starts;
  __syncthreads();
  int sidx = -1, total = 0;                    // sidx: the site of the last start before r0
  for (int q = 0; q < 256; ++q) {
    if (q < tid) sidx += scnt[q];
    total += scnt[q];
  }
  int* ss = site_start + (size_t)b * (cap + 1);
  for (int r = r0; r < r1; ++r) {
    const size_t e = (size_t)b * cap + r;
    if (r < n) {
      const int i = perm[r], p = spix[i], bk = sback[i];
      if (r == 0 || p != spix[perm[r - 1]]) ss[++sidx] = r;
      stpix[e] = p;
      stt[e] = bk / fcap;
      stz[e] = z[fbase + bk];
      psite[e] = sidx;
      back[e] = bk;
      fsite[fbase + bk] = sidx;
    } else {
      stpix[e] = 0;
      stt[e] = 0;
      stz[e] = 0.f;
      psite[e] = -1;
      back[e] = -1;
    }
  }
  for (int g = total + tid; g <= cap; g += 256) ss[g] = n;
  if (tid == 0) {
    stcounts[b] = off;
    nsites[b] = total;
  }
}

// ---- band Gram of W: for column tile J the 32 x 32 tiles G[J][J] and G[J + 1][J] of W^T W, G[a][b] = sum_k W[k][a] W[k][b].  One
// workgroup per (J, system) walks the rows k from the diagonal tile down, GK at a time: every row is one 64-float segment (32 for the
// last J), read as float4 and staged in LDS as fp64; thread (c, r0) owns the entries (r0 + 8 rr, c) of both tiles and adds the rows in
// order.  Rows of the diagonal tile are zero right of it, so both tiles start at the same row.  The next stage's loads are in flight
// while this one computes.  LDS reads: lanes c read consecutive doubles, the row operand is a broadcast.
// gram [nsys][np / 32][2][32][32] fp64 (tile 1 of the last J is zero)
__global__ __launch_bounds__(256) void stkrig_site_gram_kernel(const float* __restrict__ Wi, int np, double* __restrict__ gram) {
  __shared__ double S[GK][2 * TS];
  const int J = blockIdx.x, nt = gridDim.x, s = blockIdx.y;
  const float* Ws = Wi + (size_t)s * np * np;
  const int j0 = J * TS;
  const bool two = J + 1 < nt;
  const int tid = threadIdx.x, c = tid & 31, r0 = tid >> 5;
  const int lr = tid >> 4, lc = (tid & 15) * 4;          // staging: rows lr and lr + 16 of the stage, columns lc .. lc + 3
  const bool ld = two || lc < TS;
  double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
  float4 nx[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
    nx[h] = ld ? *reinterpret_cast<const float4*>(Ws + (size_t)(j0 + lr + 16 * h) * np + j0 + lc) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k0 = j0; k0 < np; k0 += GK) {
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double* d = &S[lr + 16 * h][lc];
      d[0] = (double)nx[h].x;
      d[1] = (double)nx[h].y;
      d[2] = (double)nx[h].z;
      d[3] = (double)nx[h].w;
    }
    __syncthreads();
    if (k0 + GK < np && ld) {
#pragma unroll
      for (int h = 0; h < 2; ++h) nx[h] = *reinterpret_cast<const float4*>(Ws + (size_t)(k0 + GK + lr + 16 * h) * np + j0 + lc);
    }
#pragma unroll 8
    for (int k = 0; k < GK; ++k) {
      const double wc = S[k][c];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) a0[rr] = fma(S[k][r0 + 8 * rr], wc, a0[rr]);
      if (two) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) a1[rr] = fma(S[k][TS + r0 + 8 * rr], wc, a1[rr]);
      }
    }
  }
  double* g = gram + ((size_t)s * nt + J) * 2 * TS * TS;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    g[(r0 + 8 * rr) * TS + c] = a0[rr];
    g[TS * TS + (r0 + 8 * rr) * TS + c] = a1[rr];
  }
}

// ---- site solve: one workgroup per (site, system), fp64.  B_SS (m <= 32) is assembled in LDS from the Gram tiles and u, factored by
// a right-looking Cholesky (a pivot that is not > 0 gives NaN for the site), X = its factor's inverse by forward substitution (one
// column per thread), then y = X alpha_S, e_S = X^T y and sigma^2 = the column square-sums of X.  Results go through the back map into
// the per-frame layout [B T][fcap].  NaN for every point of a sample with one site, a degenerate fit or a failed factorisation.
__global__ __launch_bounds__(256) void stkrig_loso_kernel(const double* __restrict__ gram, const double* __restrict__ sol,
                                                          const float* __restrict__ alpha, const float* __restrict__ stz,
                                                          const int* __restrict__ stcounts, const int* __restrict__ site_start,
                                                          const int* __restrict__ nsites, const int* __restrict__ back,
                                                          const int* __restrict__ status, const int* __restrict__ cand, int s0, int T,
                                                          int fcap, int cap, int np, float* __restrict__ pred, float* __restrict__ var) {
  __shared__ double red[256];
  __shared__ double Bm[TS][TS + 1];
  __shared__ double Xm[TS][TS + 1];
  __shared__ double av[TS];
  __shared__ double yv[TS];
  const int s = blockIdx.y, b = s0 + s, g = blockIdx.x, tid = threadIdx.x;
  const int ns = nsites[b];
  if (g >= ns) return;
  const int n = min(stcounts[b], np);
  const int p0 = site_start[(size_t)b * (cap + 1) + g];
  const int m = site_start[(size_t)b * (cap + 1) + g + 1] - p0;
  const int* bk = back + (size_t)b * cap + p0;
  float* po = pred + (size_t)b * T * fcap;
  float* vo = var + (size_t)b * T * fcap;
  if (ns < 2 || m > TS || no_model(status[s], cand, b)) {
    for (int i = tid; i < m; i += 256) po[bk[i]] = vo[bk[i]] = __builtin_nanf("");
    return;
  }
  const double* u = sol + (size_t)s * 2 * np;
  const double su = sum_u(u, n, red);
  const int nt = np / TS;
  for (int e = tid; e < m * m; e += 256) {
    const int i = e / m, j = e % m;
    const int hi = p0 + max(i, j), lo = p0 + min(i, j);
    const int tl = lo / TS;
    const double G = gram[(((size_t)s * nt + tl) * 2 + (hi / TS - tl)) * TS * TS + (hi % TS) * TS + lo % TS];
    Bm[i][j] = G - u[p0 + i] * u[p0 + j] / su;
  }
  if (tid < m) av[tid] = (double)alpha[(size_t)b * cap + p0 + tid];
  __syncthreads();
  bool bad = false;
  for (int j = 0; j < m; ++j) {
    const double d = Bm[j][j];
    __syncthreads();                            // every thread holds the pivot before its entry becomes the factor's
    if (!(d > 0.0)) {
      bad = true;
      break;
    }
    const double l = sqrt(d);
    if (tid >= j && tid < m) Bm[tid][j] = tid == j ? l : Bm[tid][j] / l;
    __syncthreads();
    for (int e = tid; e < m * m; e += 256) {
      const int i = e / m, k = e % m;
      if (k > j && i >= k) Bm[i][k] = fma(-Bm[i][j], Bm[k][j], Bm[i][k]);
    }
    __syncthreads();
  }
  if (bad) {
    if (tid < m) po[bk[tid]] = vo[bk[tid]] = __builtin_nanf("");
    return;
  }
  if (tid < m) {
    const int c = tid;
    for (int i = 0; i < m; ++i) {
      double acc = i == c ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k) acc = fma(-Bm[i][k], Xm[k][c], acc);
      Xm[i][c] = i >= c ? acc / Bm[i][i] : 0.0;
    }
  }
  __syncthreads();
  if (tid < m) {
    double y = 0.0;
    for (int i = 0; i <= tid; ++i) y = fma(Xm[tid][i], av[i], y);
    yv[tid] = y;
  }
  __syncthreads();
  if (tid < m) {
    double e = 0.0, q = 0.0;
    for (int k = tid; k < m; ++k) {
      const double x = Xm[k][tid];
      e = fma(x, yv[k], e);
      q = fma(x, x, q);
    }
    po[bk[tid]] = (float)((double)stz[(size_t)b * cap + p0 + tid] - e);
    vo[bk[tid]] = (float)q;
  }
}

}  // namespace
}  // namespace p2i

using namespace p2i;

extern "C" int p2i_stkrig_gather_sites(const int* pix, const float* z, const int* counts, int B, int T, int fcap, int cap, int* stpix,
                                       int* stt, float* stz, int* stcounts, int* site_start, int* nsites, int* psite, int* back,
                                       int* fsite, void* stream) {
  P2I_REQUIRE(pix && z && counts && stpix && stt && stz && stcounts && site_start && nsites && psite && back && fsite, "null pointer");
  P2I_REQUIRE(B > 0 && T > 0 && (long long)B * T <= 65535, "bad sample shape %d x %d", B, T);
  P2I_REQUIRE(fcap > 0 && fcap <= MAX_NP, "bad frame row length %d", fcap);
  if (int rc = krig_cap_check(cap)) return rc;
  P2I_LAUNCH(stkrig_gather_sites_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pix, z, counts, T, fcap, cap, stpix, stt, stz, stcounts,
             site_start, nsites, psite, back, fsite);
  return launch_status();
}

extern "C" int p2i_stkrig_site_gram(const float* Winv, int nsys, int np, double* gram, void* stream) {
  P2I_REQUIRE(Winv && gram, "null pointer");
  P2I_REQUIRE(nsys > 0 && nsys <= 65535 && np > 0 && np % TS == 0 && np <= MAX_NP, "bad system shape %d x %d", nsys, np);
  P2I_LAUNCH(stkrig_site_gram_kernel, dim3(np / TS, nsys), dim3(256), 0, (hipStream_t)stream, Winv, np, gram);
  return launch_status();
}

extern "C" int p2i_stkrig_loso(const p2i_krig_systems* k, const double* gram, const double* sol, const float* alpha, const int* site_start,
                               const int* nsites, const int* back, int T, int fcap, float* pred, float* var, void* stream) {
  const unsigned reads = KS_Z | KS_COUNTS | KS_STATUS | KS_NP;
  if (int rc = krig_sys_ptrs(k, reads, gram && sol && alpha && site_start && nsites && back && pred && var)) return rc;
  P2I_REQUIRE(T > 0 && T <= TS, "a site block is at most %d frames wide (got T = %d)", TS, T);
  P2I_REQUIRE(fcap > 0 && fcap <= MAX_NP, "bad frame row length %d", fcap);
  if (int rc = krig_sys_range(k, reads)) return rc;
  P2I_REQUIRE(k->R == 1 && k->T == 1, "a space-time system is one sample: R = T = 1");
  P2I_LAUNCH(stkrig_loso_kernel, dim3(k->np, k->nsys), dim3(256), 0, (hipStream_t)stream, gram, sol, alpha, k->z, k->counts, site_start,
             nsites, back, (const int*)k->status, k->cand, k->f0, T, fcap, k->cap, k->np, pred, var);
  return launch_status();
}
