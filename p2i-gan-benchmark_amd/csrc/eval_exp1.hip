// The benchmark's exp1 scoring (reference experiments/exp1.py run_exp1, experiments/io.py) on the device; DESIGN.md section 10.
//   p2i_exp1_transform  : transform_mmhr in fp64 (exp1.py:151-159), element-wise -- the ulp check of the device pow
//   p2i_exp1_accumulate : ONE streaming pass over an aligned (pred, truth) piece of T frames: both are transformed (uint8 through
//                         the host's 256-entry table, f32 / f64 through the device pow), center-cropped to S x S, and
//                           * over the mode's selection (rank >= 0): sum|d|, sum d^2, Welford (n, mean, M2) of the truth,
//                             the 3 x k contingency counts (>= thresholds, fp64 values) and min / max / count of the f32 casts
//                             that are finite and > 0.5 (the PSS range) -> one partial per workgroup, [frame][workgroup];
//                             the caller keeps the partials of all pieces in frame order and p2i_exp1_merge folds them in
//                             that order, so the result does not depend on where the pieces were cut (deterministic);
//                           * the f32 casts of the selected values, compacted to [T][nsel] (the PSS histograms wait for the
//                             global range, known only after the last piece);
//                           * the avg_pool2d(pool, pool) f32 frames of the whole crop [T][S/pool][S/pool] (SSIM, dTSSIM).
//   p2i_exp1_hist       : per frame the two 50-bin histograms of the compacted values over the range in acc[] (edges as
//                         np.linspace(vmin, vmax, 51, dtype=float32) computes them) and the frame's PSS score + flag
//   p2i_exp1_ssim       : per frame the global SSIM of (pred_t, gt_t) and, for lags 1 and 2, SSIM(p_t, p_t-L) - SSIM(g_t, g_t-L)
//   p2i_exp1_finalize   : the per-frame series reduced in frame order and the table's numbers, out[P2I_EXP1_OUT(k)]
// Compiled with -ffp-contract=off: the linspace edges and the transform must round as numpy's separate operations do.
#include "eval_common.h"

namespace p2i {

constexpr int XK = P2I_EXP1_MAX_THR;
// stats record (doubles): the layout of acc[] and of the per-workgroup partials
enum { S_N = 0, S_ABS, S_SQ, S_GMEAN, S_GM2, S_NPSS, S_VMIN, S_VMAX, S_CNT };
constexpr int NST = S_CNT + 3 * XK;
static_assert(NST == P2I_EXP1_NSTAT, "stats layout");
constexpr int BINS = 50;

struct Thr { double v[XK]; int k; };

// a <- a (+) b is Chan et al.'s pairwise update for (n, mean, M2); sums add; the range is taken over both non-empty sides
struct Stats {
  static constexpr int WORDS = NST;
  double n, sabs, ssq, gmean, gm2, npss, vmin, vmax;
  double cnt[3 * XK];

  __device__ __forceinline__ void zero() {
    n = sabs = ssq = gmean = gm2 = npss = vmin = vmax = 0.0;
#pragma unroll
    for (int i = 0; i < 3 * XK; ++i) cnt[i] = 0.0;
  }
  __device__ __forceinline__ void merge(const Stats& b) {
    chan_merge(n, gmean, gm2, b.n, b.gmean, b.gm2);
    sabs += b.sabs;
    ssq += b.ssq;
    if (b.npss > 0.0) {
      if (npss > 0.0) {
        vmin = b.vmin < vmin ? b.vmin : vmin;
        vmax = b.vmax > vmax ? b.vmax : vmax;
      } else {
        vmin = b.vmin;
        vmax = b.vmax;
      }
      npss += b.npss;
    }
#pragma unroll
    for (int i = 0; i < 3 * XK; ++i) cnt[i] += b.cnt[i];
  }
  __device__ __forceinline__ void store(double* p) const {
    p[S_N] = n; p[S_ABS] = sabs; p[S_SQ] = ssq; p[S_GMEAN] = gmean; p[S_GM2] = gm2;
    p[S_NPSS] = npss; p[S_VMIN] = vmin; p[S_VMAX] = vmax;
#pragma unroll
    for (int i = 0; i < 3 * XK; ++i) p[S_CNT + i] = cnt[i];
  }
  static __device__ __forceinline__ Stats load(const double* p) {
    Stats s;
    s.n = p[S_N]; s.sabs = p[S_ABS]; s.ssq = p[S_SQ]; s.gmean = p[S_GMEAN]; s.gm2 = p[S_GM2];
    s.npss = p[S_NPSS]; s.vmin = p[S_VMIN]; s.vmax = p[S_VMAX];
#pragma unroll
    for (int i = 0; i < 3 * XK; ++i) s.cnt[i] = p[S_CNT + i];
    return s;
  }
  // one f32 cast joins the PSS range when it is finite and > 0.5
  __device__ __forceinline__ void pss(float v) {
    if (isfinite(v) && v > 0.5f) {
      const double d = (double)v;
      if (npss > 0.0) {
        vmin = d < vmin ? d : vmin;
        vmax = d > vmax ? d : vmax;
      } else {
        vmin = vmax = d;
      }
      npss += 1.0;
    }
  }
};

// One thread per pool x pool cell of the crop (cells of the last, partial row / column of cells when S % pool != 0 cover the
// remaining pixels but write no pooled value).  Block = 64 threads (one wave); grid (cells / 64, T).
// This kernel keeps its loose __restrict__ arguments and writes its two addresses out: it stores sel_p / sel_g inside the loop
// that loads the inputs, and run_exp1 measured 5 % slower with by-value Crop arguments (no noalias) and still 1 to 2 % slower with
// Crop views formed here from the loose arguments.  As written the unit's code object is what it was before Crop existed.
template <typename PT, typename GT>
__global__ __launch_bounds__(64) void exp1_accumulate_kernel(const PT* __restrict__ pred, int ph, int pw, int ptop, int pleft,
                                                             const GT* __restrict__ gt, int gh, int gw, int gtop, int gleft,
                                                             int S, int pool, const int* __restrict__ rank, int nsel,
                                                             const double* __restrict__ lut, Thr thr, int div3,
                                                             float* __restrict__ pool_p, float* __restrict__ pool_g,
                                                             float* __restrict__ sel_p, float* __restrict__ sel_g,
                                                             double* __restrict__ part) {
  const int cdim = (S + pool - 1) / pool, PH = S / pool;
  const int cell = blockIdx.x * 64 + threadIdx.x;
  const long long t = blockIdx.y;
  Stats s;
  s.zero();
  if (cell < cdim * cdim) {
    const int cy = cell / cdim, cx = cell - cy * cdim;
    const int y0 = cy * pool, x0 = cx * pool;
    const int y1 = min(y0 + pool, S), x1 = min(x0 + pool, S);
    const long long pbase = t * ph * pw, gbase = t * gh * gw;
    float psum = 0.f, gsum = 0.f;
    for (int y = y0; y < y1; ++y) {
      for (int x = x0; x < x1; ++x) {
        const double p = tload<PT>(pred, pbase + (long long)(ptop + y) * pw + pleft + x, lut, div3);
        const double g = tload<GT>(gt, gbase + (long long)(gtop + y) * gw + gleft + x, lut, div3);
        const float pf = (float)p, gf = (float)g;
        psum += pf;                       // avg_pool2d's row-major f32 sum over the window
        gsum += gf;
        const int r = rank[y * S + x];
        if (r >= 0 && r < nsel) {
          const double d = p - g;
          s.sabs += fabs(d);
          s.ssq += d * d;
          welford_push(s.n, s.gmean, s.gm2, g);
#pragma unroll
          for (int k = 0; k < XK; ++k)
            if (k < thr.k) {
              const bool pp = p >= thr.v[k], gg = g >= thr.v[k];
              s.cnt[3 * k + 0] += (pp && gg) ? 1.0 : 0.0;     // hits
              s.cnt[3 * k + 1] += (!pp && gg) ? 1.0 : 0.0;    // misses
              s.cnt[3 * k + 2] += (pp && !gg) ? 1.0 : 0.0;    // false alarms
            }
          s.pss(pf);
          s.pss(gf);
          sel_p[t * nsel + r] = pf;
          sel_g[t * nsel + r] = gf;
        }
      }
    }
    if (cy < PH && cx < PH) {
      const float inv = (float)(pool * pool);
      pool_p[(t * PH + cy) * PH + cx] = psum / inv;
      pool_g[(t * PH + cy) * PH + cx] = gsum / inv;
    }
  }
  __shared__ double red[64 * NST];
  block_tree<64>(s, red);
  if (threadIdx.x == 0) s.store(part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * NST);
}

// acc <- acc (+) part[0] (+) part[1] ... in a fixed order: thread i folds parts i, i + 128, ... ascending, a tree joins the threads
__global__ __launch_bounds__(128) void exp1_merge_kernel(const double* __restrict__ part, long long nparts, double* __restrict__ acc) {
  Stats s;
  s.zero();
  for (long long i = threadIdx.x; i < nparts; i += 128) {
    s.merge(Stats::load(part + i * NST));
  }
  __shared__ double red[128 * NST];
  block_tree<128>(s, red);
  if (threadIdx.x == 0) {
    Stats a = Stats::load(acc);
    a.merge(s);
    a.store(acc);
  }
}

// The PSS edges: numpy's histogram uses np.linspace(first, last, 51, dtype=float32) -- y_i = i * step + vmin in fp64 with
// step = (vmax - vmin) / 50, the last edge = vmax, each cast to f32 -- and refuses them unless strictly increasing.
// Returns false when they are not.
__device__ bool pss_edges(const double* acc, float* e) {
  const double vmin = acc[S_VMIN];
  double vmax = acc[S_VMAX];
  if (vmin == vmax) vmax = vmin + 1e-6;
  const double step = (vmax - vmin) / (double)BINS;
  for (int i = 0; i < BINS; ++i) e[i] = (float)((double)i * step + vmin);
  e[BINS] = (float)vmax;
  bool ok = true;
  for (int i = 0; i < BINS; ++i) ok = ok && (e[i] < e[i + 1]);
  return ok;
}

// np.histogram's rule: bin i holds e[i] <= x < e[i+1], x == e[50] goes to bin 49
__device__ __forceinline__ int pss_bin(float x, const float* e) {
  const float span = e[BINS] - e[0];
  int b = (int)((x - e[0]) * ((float)BINS / span));
  b = b < 0 ? 0 : (b > BINS - 1 ? BINS - 1 : b);
  while (b > 0 && x < e[b]) --b;
  while (b < BINS - 1 && x >= e[b + 1]) ++b;
  return b;
}

// one block per frame; flag[t] = 1 when both histograms are non-empty (the frame counts), score[t] its PSS;
// edges_out (51 floats + 1 status float: 1 = edges not strictly increasing) written by block 0
__global__ __launch_bounds__(256) void exp1_hist_kernel(const float* __restrict__ sel_p, const float* __restrict__ sel_g, int nsel,
                                                        const double* __restrict__ acc, double* __restrict__ score,
                                                        int* __restrict__ flag, float* __restrict__ edges_out) {
  __shared__ float e[BINS + 1];
  __shared__ int hist[2][BINS];
  __shared__ int ok_s;
  const long long t = blockIdx.x;
  if (threadIdx.x == 0) {
    ok_s = acc[S_NPSS] > 0.0 ? (int)pss_edges(acc, e) : 0;
    if (blockIdx.x == 0) {
      for (int i = 0; i <= BINS; ++i) edges_out[i] = acc[S_NPSS] > 0.0 ? e[i] : 0.f;
      edges_out[BINS + 1] = (acc[S_NPSS] > 0.0 && !ok_s) ? 1.f : 0.f;
    }
  }
  if (threadIdx.x < 2 * BINS) (&hist[0][0])[threadIdx.x] = 0;
  __syncthreads();
  const bool ok = ok_s != 0;
  for (int i = threadIdx.x; i < nsel; i += 256) {
    const float p = sel_p[t * nsel + i], g = sel_g[t * nsel + i];
    const bool vp = isfinite(p) && p > 0.5f, vg = isfinite(g) && g > 0.5f;
    // without a valid range only the emptiness of the two sides matters: count into bin 0
    if (vp) atomicAdd(&hist[0][ok ? pss_bin(p, e) : 0], 1);
    if (vg) atomicAdd(&hist[1][ok ? pss_bin(g, e) : 0], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long np_ = 0, ng = 0;
    for (int b = 0; b < BINS; ++b) { np_ += hist[0][b]; ng += hist[1][b]; }
    const bool valid = np_ > 0 && ng > 0;
    double sc = 0.0;
    if (valid && ok) {
      const double dp = (double)np_ + 1e-12, dg = (double)ng + 1e-12;
      for (int b = 0; b < BINS; ++b) {
        const double fp = (double)hist[0][b] / dp, fg = (double)hist[1][b] / dg;
        sc += fp < fg ? fp : fg;
      }
    }
    flag[t] = valid ? 1 : 0;
    score[t] = sc;
  }
}

// global SSIM of two frames of n values (exp1.py ssim2d: biased moments, c1 = 1e-4, c2 = 9e-4, + 1e-10), two passes in fp64
__device__ double ssim_pair(const float* __restrict__ a, const float* __restrict__ b, int n, double* red) {
  double sa = 0.0, sb = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { sa += (double)a[i]; sb += (double)b[i]; }
  red[threadIdx.x] = sa;
  red[256 + threadIdx.x] = sb;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { red[threadIdx.x] += red[threadIdx.x + o]; red[256 + threadIdx.x] += red[256 + threadIdx.x + o]; }
    __syncthreads();
  }
  const double ma = red[0] / (double)n, mb = red[256] / (double)n;
  __syncthreads();
  double vaa = 0.0, vbb = 0.0, vab = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double da = (double)a[i] - ma, db = (double)b[i] - mb;
    vaa += da * da;
    vbb += db * db;
    vab += da * db;
  }
  red[threadIdx.x] = vaa;
  red[256 + threadIdx.x] = vbb;
  red[512 + threadIdx.x] = vab;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[threadIdx.x] += red[threadIdx.x + o];
      red[256 + threadIdx.x] += red[256 + threadIdx.x + o];
      red[512 + threadIdx.x] += red[512 + threadIdx.x + o];
    }
    __syncthreads();
  }
  const double sig_a = red[0] / (double)n, sig_b = red[256] / (double)n, sig_ab = red[512] / (double)n;
  __syncthreads();
  const double c1 = 1e-4, c2 = 9e-4;
  const double num = (2.0 * ma * mb + c1) * (2.0 * sig_ab + c2);
  const double den = (ma * ma + mb * mb + c1) * (sig_a + sig_b + c2);
  return num / (den + 1e-10);
}

// one block per frame t of the method's whole stack: s0[t] = SSIM(p_t, g_t); dL[t] (t >= L) = SSIM(p_t, p_t-L) - SSIM(g_t, g_t-L)
__global__ __launch_bounds__(256) void exp1_ssim_kernel(const float* __restrict__ pp, const float* __restrict__ pg, int n,
                                                        double* __restrict__ s0, double* __restrict__ d1, double* __restrict__ d2) {
  __shared__ double red[3 * 256];
  const long long t = blockIdx.x;
  const float* p = pp + t * n;
  const float* g = pg + t * n;
  const double v0 = ssim_pair(p, g, n, red);
  double v1 = 0.0, v2 = 0.0;
  if (t >= 1) v1 = ssim_pair(p, p - n, n, red) - ssim_pair(g, g - n, n, red);
  if (t >= 2) v2 = ssim_pair(p, p - 2 * n, n, red) - ssim_pair(g, g - 2 * n, n, red);
  if (threadIdx.x == 0) {
    s0[t] = v0;
    d1[t] = v1;
    d2[t] = v2;
  }
}

// sum of x[i0..T) (and the count of flag[i] != 0 when flag) in a fixed order: strided per thread, then a tree
__device__ double block_sum_fixed(const double* __restrict__ x, const int* __restrict__ flag, int i0, int T, double* red, double* cnt) {
  double s = 0.0, c = 0.0;
  for (int i = i0 + (int)threadIdx.x; i < T; i += 256) {
    if (flag && !flag[i]) continue;
    s += x[i];
    c += 1.0;
  }
  red[threadIdx.x] = s;
  red[256 + threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { red[threadIdx.x] += red[threadIdx.x + o]; red[256 + threadIdx.x] += red[256 + threadIdx.x + o]; }
    __syncthreads();
  }
  const double r = red[0];
  *cnt = red[256];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void exp1_finalize_kernel(const double* __restrict__ acc, Thr thr, int T,
                                                            const double* __restrict__ score, const int* __restrict__ flag,
                                                            const float* __restrict__ edges, const double* __restrict__ s0,
                                                            const double* __restrict__ d1, const double* __restrict__ d2,
                                                            double* __restrict__ out) {
  __shared__ double red[2 * 256];
  double c;
  const double pss_sum = block_sum_fixed(score, flag, 0, T, red, &c);
  const double pss_n = c;
  const double ssim_sum = block_sum_fixed(s0, nullptr, 0, T, red, &c);
  const double d1_sum = block_sum_fixed(d1, nullptr, 1, T, red, &c);
  const double d2_sum = block_sum_fixed(d2, nullptr, 2, T, red, &c);
  if (threadIdx.x != 0) return;
  const double qnan = __builtin_nan("");
  const double n = acc[S_N];
  out[0] = acc[S_ABS] / n;                                    // MAE   (0/0 = NaN on an empty selection, as np.mean)
  out[1] = sqrt(acc[S_SQ] / n);                               // RMSE
  out[2] = pss_n > 0.0 ? pss_sum / pss_n : qnan;              // PSS
  out[3] = ssim_sum / (double)T;                              // SSIM
  out[4] = T > 1 ? d1_sum / (double)(T - 1) : qnan;           // dTSSIM lag 1
  out[5] = T > 2 ? d2_sum / (double)(T - 2) : qnan;           // dTSSIM lag 2
  out[6] = 1.0 - acc[S_SQ] / (acc[S_GM2] + 1e-10);            // NSE
  for (int k = 0; k < thr.k; ++k) {
    const long long h = (long long)acc[S_CNT + 3 * k], m = (long long)acc[S_CNT + 3 * k + 1], f = (long long)acc[S_CNT + 3 * k + 2];
    const long long cn = (long long)n - h - m - f;
    double* o = out + 7 + 4 * k;
    o[0] = (double)h / ((double)(h + m) + 1e-10);
    o[1] = (double)f / ((double)(h + f) + 1e-10);
    o[2] = (double)h / ((double)(h + m + f) + 1e-10);
    // exp1's HSS: integer numerator and denominator terms as numpy evaluates them on int64 counts
    const long long hn = 2 * (h * cn - m * f);
    const long long hd = m * m + f * f + 2 * h * cn + (m + f) * (h + cn);
    o[3] = (h + m + f + cn) > 0 ? (double)hn / ((double)hd + 1e-10) : qnan;
  }
  // status: 1 = the PSS edges are not strictly increasing while some frame needs them (np.histogram raises ValueError)
  out[7 + 4 * thr.k] = (edges[BINS + 1] != 0.f && pss_n > 0.0) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void exp1_transform_kernel(const void* __restrict__ x, int dtype, long long n, int div3,
                                                             double* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    double v;
    if (dtype == P2I_EXP1_U8) v = (double)((const uint8_t*)x)[i];
    else if (dtype == P2I_EXP1_F32) v = (double)((const float*)x)[i];
    else v = ((const double*)x)[i];
    out[i] = mmhr(v, div3);
  }
}

}  // namespace p2i

using namespace p2i;

extern "C" int p2i_exp1_transform(const void* x, int dtype, int64_t n, int divide_by_3, double* out, void* stream) {
  P2I_REQUIRE(x && out && n > 0 && eval_dtype_ok(dtype), "bad arguments");
  const long long blocks = (n + 255) / 256;
  const int nb = (int)(blocks > 4096 ? 4096 : blocks);
  P2I_LAUNCH(exp1_transform_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, dtype, (long long)n, divide_by_3, out);
  return launch_status();
}

extern "C" int p2i_exp1_workspace(int T, int S, int pool, int64_t* part_doubles) {
  P2I_REQUIRE(part_doubles && T > 0 && S > 0 && (pool == 1 || pool == 8), "bad arguments");
  const int cdim = (S + pool - 1) / pool;
  *part_doubles = (int64_t)ceil_div(cdim * cdim, 64) * T * NST;
  return P2I_OK;
}

extern "C" int p2i_exp1_accumulate(const p2i_eval_input* pred, const p2i_eval_input* truth, int T, int S, int pool, const int* rank,
                                   int nsel, const double* lut, const double* thresholds_host, int nthr, int divide_by_3,
                                   float* pool_pred, float* pool_truth, float* sel_pred, float* sel_truth, double* part,
                                   void* stream) {
  P2I_REQUIRE(input_set(pred) && input_set(truth) && rank && lut && part && pool_pred && pool_truth, "bad arguments");
  P2I_REQUIRE(eval_dtype_ok(pred->dtype) && eval_dtype_ok(truth->dtype), "unsupported dtype");
  P2I_REQUIRE(T > 0 && T <= 65535 && S > 0 && (pool == 1 || pool == 8) && S / pool > 0, "bad frame count / crop / pool");
  P2I_REQUIRE(crop_ok(pred, S, S), "crop outside the prediction");
  P2I_REQUIRE(crop_ok(truth, S, S), "crop outside the truth");
  P2I_REQUIRE(nsel >= 0 && nsel <= S * S && (nsel == 0 || (sel_pred && sel_truth)), "bad selection");
  P2I_REQUIRE(nthr >= 0 && nthr <= XK && (nthr == 0 || thresholds_host), "at most %d thresholds", XK);
  Thr thr;
  thr.k = nthr;
  for (int i = 0; i < XK; ++i) thr.v[i] = i < nthr ? thresholds_host[i] : 0.0;
  const int cdim = (S + pool - 1) / pool;
  const dim3 grid((unsigned)ceil_div(cdim * cdim, 64), (unsigned)T);
  const hipStream_t s = (hipStream_t)stream;
  dispatch2(pred, truth, [&](auto p, auto g) {
    P2I_LAUNCH((exp1_accumulate_kernel<Elem<decltype(p)>, Elem<decltype(g)>>), grid, dim3(64), 0, s, p.p, p.h, p.w, p.top, p.left, g.p,
               g.h, g.w, g.top, g.left, S, pool, rank, nsel, lut, thr, divide_by_3, pool_pred, pool_truth, sel_pred, sel_truth, part);
  });
  return launch_status();
}

extern "C" int p2i_exp1_merge(const double* part, int64_t nparts, double* acc, void* stream) {
  P2I_REQUIRE(part && acc && nparts > 0, "bad arguments");
  P2I_LAUNCH(exp1_merge_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, part, (long long)nparts, acc);
  return launch_status();
}

extern "C" int p2i_exp1_hist(const float* sel_pred, const float* sel_truth, int T, int nsel, const double* acc, double* score,
                             int* flag, float* edges, void* stream) {
  P2I_REQUIRE(acc && score && flag && edges && T > 0 && nsel >= 0 && (nsel == 0 || (sel_pred && sel_truth)), "bad arguments");
  P2I_LAUNCH(exp1_hist_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, sel_pred, sel_truth, nsel, acc, score, flag, edges);
  return launch_status();
}

extern "C" int p2i_exp1_ssim(const float* pool_pred, const float* pool_truth, int T, int npix, double* ssim, double* d1, double* d2,
                             void* stream) {
  P2I_REQUIRE(pool_pred && pool_truth && ssim && d1 && d2 && T > 0 && npix > 0, "bad arguments");
  P2I_LAUNCH(exp1_ssim_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, pool_pred, pool_truth, npix, ssim, d1, d2);
  return launch_status();
}

extern "C" int p2i_exp1_finalize(const double* acc, const double* thresholds_host, int nthr, int T, const double* score, const int* flag,
                                 const float* edges, const double* ssim, const double* d1, const double* d2, double* out, void* stream) {
  P2I_REQUIRE(acc && score && flag && edges && ssim && d1 && d2 && out && T > 0, "bad arguments");
  P2I_REQUIRE(nthr >= 0 && nthr <= XK && (nthr == 0 || thresholds_host), "at most %d thresholds", XK);
  Thr thr;
  thr.k = nthr;
  for (int i = 0; i < XK; ++i) thr.v[i] = i < nthr ? thresholds_host[i] : 0.0;
  P2I_LAUNCH(exp1_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, acc, thr, T, score, flag, edges, ssim, d1, d2, out);
  return launch_status();
}
