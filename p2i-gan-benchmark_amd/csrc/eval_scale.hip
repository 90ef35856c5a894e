// Scale-aware verification of inference outputs on the device: the fractions skill score over thresholds x neighbourhood sizes and
// the radially averaged power spectral density; DESIGN.md section 15.  Inputs are exp1's (Crop<T> / tload of eval_common.h); every
// pixel of the crop counts, there is no mask.
//   p2i_scale_fss            : one workgroup per (frame, threshold) builds the summed-area tables of the two binary crops
//                              (pred >= q, truth >= q; NaN compares false) and takes every scale's window counts c_p, c_g from four
//                              table reads per pixel; the window of size n at (y, x) covers rows y - n/2 .. y - n/2 + n - 1 and the
//                              same range of columns, pixels outside the crop count 0.  Writes per (frame, threshold) the exact
//                              integers sum c_p^2, sum c_g^2, sum c_p c_g of every scale and the truth's hit count.  Crops up to
//                              P2I_SCALE_LDS_CROP keep 16-bit tables in LDS; larger ones 32-bit tables in a caller's workspace.
//                              The same arithmetic on the same integers: the results do not depend on the path.
//   p2i_scale_fss_merge      : acc[i] += sum over frames of part[t][i] (64-bit integers: no order to fix).
//   p2i_scale_dft_rows /
//   p2i_scale_dft_cols       : the S x S DFT of a transformed crop as two dense complex products over the host's twiddle table
//                              cos, sin(2 pi m / S) indexed at (j k) mod S -- any S -- for k_x <= S/2 only (real input); the second
//                              writes psd = |F|^2 / S^2.  Plain fp64 FMAs, written as explicit fma (the unit compiles with
//                              -ffp-contract=off, so nothing else fuses).
//   p2i_scale_rings          : per frame the ring means P(r), r = rint(sqrt(k_y^2 + k_x^2)) <= S/2, from the host's ring-sorted
//                              list of half-plane bins (weight 2 for a bin whose mirror lies outside the half plane), summed in list
//                              order by one thread per ring.
//   p2i_scale_spectrum_merge : the mean of the frames' P(r) in frame order over the frames where neither field holds a NaN.
#include "eval_common.h"

namespace p2i {

constexpr int XK = P2I_EXP1_MAX_THR;
constexpr int XN = P2I_SCALE_MAX_SCALES;
constexpr int LS = P2I_SCALE_LDS_CROP;
typedef unsigned long long u64;

struct SThr { double v[XK]; int k; };
struct SScales { int n[XN]; int k; };

// elements per table row: the 16-bit LDS tables take an odd number of dwords per row, so a thread per row walks distinct banks
static inline __host__ __device__ int fss_pitch(int S, bool lds) {
  if (!lds) return S;
  int dw = (S + 1) / 2;
  if (!(dw & 1)) ++dw;
  return 2 * dw;
}

// window count from an inclusive summed-area table: rows (ylo, yhi], columns (xlo, xhi]; ylo, xlo = -1 when the window starts at 0
template <typename CT>
__device__ __forceinline__ unsigned win(const CT* tb, int pitch, int ylo, int yhi, int xlo, int xhi) {
  unsigned v = tb[yhi * pitch + xhi];
  if (ylo >= 0) v -= tb[ylo * pitch + xhi];
  if (xlo >= 0) v -= tb[yhi * pitch + xlo];
  if (ylo >= 0 && xlo >= 0) v += tb[ylo * pitch + xlo];
  return v;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// grid (T, nthr), 256 threads.  part[t][k][3 * nscales + 1]: per scale A, B, C, then the truth's hits.  The LDS path takes
// 2 * S * fss_pitch(S) 16-bit counts of dynamic LDS (65 KB at S = 128: above the default limit, raised by the entry point).
template <typename PT, typename GT, typename CT, bool LDS>
__global__ __launch_bounds__(256) void scale_fss_kernel(Crop<PT> pred, Crop<GT> gt, int S, const double* __restrict__ lut, SThr thr,
                                                        SScales sc, int div3, CT* __restrict__ ws, long long* __restrict__ part) {
  extern __shared__ double fss_lds[];
  __shared__ u64 red[4][3];
  const long long t = blockIdx.x;
  const int k = blockIdx.y;
  const int pitch = fss_pitch(S, LDS);
  const int tsz = S * pitch;
  CT* tp = LDS ? (CT*)fss_lds : ws + (t * gridDim.y + k) * 2 * (long long)tsz;
  CT* tg = tp + tsz;
  double q = 0.0;
#pragma unroll
  for (int j = 0; j < XK; ++j)
    if (j == k) q = thr.v[j];
  for (int i = threadIdx.x; i < S * S; i += 256) {
    const int y = i / S, x = i - y * S;
    const double p = pred.at(t, y, x, lut, div3), g = gt.at(t, y, x, lut, div3);
    tp[y * pitch + x] = (CT)(p >= q ? 1 : 0);
    tg[y * pitch + x] = (CT)(g >= q ? 1 : 0);
  }
  __syncthreads();
  // rows of both tables (the truth's rows follow the prediction's), then columns
  for (int r = threadIdx.x; r < 2 * S; r += 256) {
    CT* row = tp + r * pitch;
    CT s = 0;
    for (int x = 0; x < S; ++x) {
      s += row[x];
      row[x] = s;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * S; c += 256) {
    CT* col = c < S ? tp + c : tg + (c - S);
    CT s = 0;
    for (int y = 0; y < S; ++y) {
      s += col[y * pitch];
      col[y * pitch] = s;
    }
  }
  __syncthreads();
  const int rec = 3 * sc.k + 1;
  long long* out = part + (t * gridDim.y + k) * rec;
  if (threadIdx.x == 0) out[3 * sc.k] = (long long)tg[(S - 1) * pitch + (S - 1)];
  for (int si = 0; si < sc.k; ++si) {
    int n = 1;
#pragma unroll
    for (int j = 0; j < XN; ++j)
      if (j == si) n = sc.n[j];
    const int h = n / 2;
    u64 a = 0, b = 0, c = 0;
    for (int i = threadIdx.x; i < S * S; i += 256) {
      const int y = i / S, x = i - y * S;
      const int ylo = y - h - 1, yhi = min(y - h + n, S) - 1;
      const int xlo = x - h - 1, xhi = min(x - h + n, S) - 1;
      const u64 cp = win(tp, pitch, ylo, yhi, xlo, xhi), cg = win(tg, pitch, ylo, yhi, xlo, xhi);
      a += cp * cp;
      b += cg * cg;
      c += cp * cg;
    }
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) {
      red[threadIdx.x >> 6][0] = a;
      red[threadIdx.x >> 6][1] = b;
      red[threadIdx.x >> 6][2] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3)
      out[3 * si + threadIdx.x] = (long long)(red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
    __syncthreads();
  }
}

// part [T][n] -> acc[n] += column sums; one thread per column
__global__ __launch_bounds__(256) void scale_fss_merge_kernel(const long long* __restrict__ part, long long T, int n,
                                                              long long* __restrict__ acc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long long s = 0;
  for (long long t = 0; t < T; ++t) s += part[t * n + i];
  acc[i] += s;
}

constexpr int RB = 4;      // crop rows per workgroup of the row transform

// G[t][field][y][kx] = sum_x f[y][x] exp(-2 pi i x kx / S), kx < NK = S/2 + 1.  grid (T, ceil(S / RB)), 128 threads,
// LDS: RB rows of f, then cos[S], sin[S].
template <typename T>
__global__ __launch_bounds__(128) void scale_dft_rows_kernel(Crop<T> in, int S, int NK, int field, const double* __restrict__ lut,
                                                             int div3, const double* __restrict__ tw, double* __restrict__ G,
                                                             int* __restrict__ nanflag) {
  extern __shared__ double sm[];
  double* f = sm;
  double* cs = sm + RB * S;
  double* sn = cs + S;
  const long long t = blockIdx.x;
  const int y0 = blockIdx.y * RB;
  bool bad = false;
  for (int i = threadIdx.x; i < RB * S; i += 128) {
    const int r = i / S, x = i - r * S;
    const double v = y0 + r < S ? in.at(t, y0 + r, x, lut, div3) : 0.0;
    f[i] = v;
    bad = bad || (v != v);
  }
  for (int i = threadIdx.x; i < S; i += 128) {
    cs[i] = tw[i];
    sn[i] = tw[S + i];
  }
  if (bad) nanflag[t * 2 + field] = 1;
  __syncthreads();
  for (int kx = threadIdx.x; kx < NK; kx += 128) {
    double re[RB], im[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) re[r] = im[r] = 0.0;
    int idx = 0;
    for (int x = 0; x < S; ++x) {
      const double c = cs[idx], s = sn[idx];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const double v = f[r * S + x];
        re[r] = fma(v, c, re[r]);
        im[r] = fma(v, s, im[r]);
      }
      idx += kx;
      if (idx >= S) idx -= S;
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
      if (y0 + r < S) {
        double* o = G + (((t * 2 + field) * S + (y0 + r)) * NK + kx) * 2;
        o[0] = re[r];
        o[1] = -im[r];
      }
  }
}

// psd[ff][ky][kx] = |sum_y G[ff][y][kx] exp(-2 pi i y ky / S)|^2 / S^2.  grid (2 T, ceil(NK / CB)), 128 threads,
// LDS: re[S][CB], im[S][CB], cos[S], sin[S].
template <int CB>
__global__ __launch_bounds__(128) void scale_dft_cols_kernel(const double* __restrict__ G, int S, int NK, const double* __restrict__ tw,
                                                             double* __restrict__ psd) {
  extern __shared__ double sm[];
  double* gre = sm;
  double* gim = gre + S * CB;
  double* cs = gim + S * CB;
  double* sn = cs + S;
  const long long ff = blockIdx.x;
  const int k0 = blockIdx.y * CB;
  for (int i = threadIdx.x; i < S * CB; i += 128) {
    const int y = i / CB, c = i - y * CB;
    const bool in = k0 + c < NK;
    const double* g = G + ((ff * S + y) * NK + (k0 + c)) * 2;
    gre[i] = in ? g[0] : 0.0;
    gim[i] = in ? g[1] : 0.0;
  }
  for (int i = threadIdx.x; i < S; i += 128) {
    cs[i] = tw[i];
    sn[i] = tw[S + i];
  }
  __syncthreads();
  const double ss = (double)S * (double)S;
  for (int ky = threadIdx.x; ky < S; ky += 128) {
    double re[CB], im[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) re[c] = im[c] = 0.0;
    int idx = 0;
    for (int y = 0; y < S; ++y) {
      const double c = cs[idx], s = sn[idx];
#pragma unroll
      for (int j = 0; j < CB; ++j) {
        const double gr = gre[y * CB + j], gi = gim[y * CB + j];
        re[j] = fma(gr, c, re[j]);
        re[j] = fma(gi, s, re[j]);
        im[j] = fma(gi, c, im[j]);
        im[j] = fma(-gr, s, im[j]);
      }
      idx += ky;
      if (idx >= S) idx -= S;
    }
#pragma unroll
    for (int j = 0; j < CB; ++j)
      if (k0 + j < NK) psd[(ff * S + ky) * NK + (k0 + j)] = (re[j] * re[j] + im[j] * im[j]) / ss;
  }
}

// P[ff][r] = (sum over the ring's listed bins of weight * psd) / count[r]; grid (2 T), 128 threads
__global__ __launch_bounds__(128) void scale_rings_kernel(const double* __restrict__ psd, int npix, const int* __restrict__ order,
                                                          const double* __restrict__ weight, const int* __restrict__ offsets,
                                                          const double* __restrict__ count, int R, double* __restrict__ P) {
  const long long ff = blockIdx.x;
  const double* src = psd + ff * npix;
  for (int r = threadIdx.x; r < R; r += 128) {
    double s = 0.0;
    for (int i = offsets[r]; i < offsets[r + 1]; ++i) s += src[order[i]] * weight[i];
    P[ff * R + r] = s / count[r];
  }
}

// out[field][r] = mean over the frames without a NaN in either field, in frame order; out[2 R] = the frames left out
__global__ __launch_bounds__(128) void scale_spectrum_merge_kernel(const double* __restrict__ P, const int* __restrict__ flag,
                                                                   long long T, int R, double* __restrict__ out) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= 2 * R) return;
  const int field = i / R, r = i - field * R;
  double s = 0.0;
  long long n = 0;
  for (long long t = 0; t < T; ++t) {
    if (flag[2 * t] || flag[2 * t + 1]) continue;
    s += P[(t * 2 + field) * R + r];
    ++n;
  }
  out[i] = s / (double)n;
  if (i == 0) out[2 * R] = (double)(T - n);
}

}  // namespace p2i

using namespace p2i;

extern "C" int p2i_scale_fss(const p2i_eval_input* pred, const p2i_eval_input* truth, int T, int S, const double* lut,
                             const double* thresholds_host, int nthr, const int* scales_host, int nscales, int divide_by_3,
                             void* workspace, int64_t* part, void* stream) {
  P2I_REQUIRE(input_set(pred) && input_set(truth) && lut && part && thresholds_host && scales_host, "bad arguments");
  P2I_REQUIRE(eval_dtype_ok(pred->dtype) && eval_dtype_ok(truth->dtype), "unsupported dtype");
  P2I_REQUIRE(T > 0 && S > 0 && S <= P2I_SCALE_MAX_CROP, "bad frame count / crop (at most %d)", P2I_SCALE_MAX_CROP);
  P2I_REQUIRE(workspace || S <= LS, "a crop above %d needs the table workspace", LS);
  P2I_REQUIRE(crop_ok(pred, S, S), "crop outside the prediction");
  P2I_REQUIRE(crop_ok(truth, S, S), "crop outside the truth");
  P2I_REQUIRE(nthr > 0 && nthr <= XK, "1 to %d thresholds", XK);
  P2I_REQUIRE(nscales > 0 && nscales <= XN, "1 to %d scales", XN);
  SThr thr;
  thr.k = nthr;
  for (int i = 0; i < XK; ++i) thr.v[i] = i < nthr ? thresholds_host[i] : 0.0;
  SScales sc;
  sc.k = nscales;
  for (int i = 0; i < XN; ++i) {
    P2I_REQUIRE(i >= nscales || scales_host[i] >= 1, "a scale is a window size >= 1");
    // every window of size >= 2 S - 1 covers the whole crop from every pixel
    sc.n[i] = i < nscales ? (scales_host[i] < 2 * S - 1 ? scales_host[i] : 2 * S - 1) : 1;
  }
  const dim3 grid((unsigned)T, (unsigned)nthr);
  const hipStream_t s = (hipStream_t)stream;
  dispatch2(pred, truth, [&](auto p, auto g) {
    using PT = Elem<decltype(p)>;
    using GT = Elem<decltype(g)>;
    if (workspace)
      P2I_LAUNCH((scale_fss_kernel<PT, GT, uint32_t, false>), grid, dim3(256), 0, s, p, g, S, lut, thr, sc, divide_by_3,
                 (uint32_t*)workspace, (long long*)part);
    else {
      static bool raised = false;      // per dtype pair
      if (!raised) {
        (void)hipFuncSetAttribute((const void*)scale_fss_kernel<PT, GT, uint16_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  2 * LS * fss_pitch(LS, true) * (int)sizeof(uint16_t));
        raised = true;
      }
      P2I_LAUNCH((scale_fss_kernel<PT, GT, uint16_t, true>), grid, dim3(256), (size_t)2 * S * fss_pitch(S, true) * sizeof(uint16_t), s, p, g, S, lut, thr, sc, divide_by_3,
                 (uint16_t*)nullptr, (long long*)part);
    }
  });
  return launch_status();
}

extern "C" int p2i_scale_fss_merge(const int64_t* part, int64_t T, int n, int64_t* acc, void* stream) {
  P2I_REQUIRE(part && acc && T > 0 && n > 0, "bad arguments");
  P2I_LAUNCH(scale_fss_merge_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)part,
             (long long)T, n, (long long*)acc);
  return launch_status();
}

extern "C" int p2i_scale_dft_rows(const p2i_eval_input* in, int T, int S, int field, const double* lut, int divide_by_3,
                                  const double* twiddle, double* G, int* nanflag, void* stream) {
  P2I_REQUIRE(input_set(in) && lut && twiddle && G && nanflag && eval_dtype_ok(in->dtype), "bad arguments");
  P2I_REQUIRE(T > 0 && S > 0 && S <= P2I_SCALE_MAX_CROP && (field == 0 || field == 1), "bad frame count / crop / field");
  P2I_REQUIRE(crop_ok(in, S, S), "crop outside the input");
  const dim3 grid((unsigned)T, (unsigned)ceil_div(S, RB));
  const size_t lds = (size_t)(RB + 2) * S * sizeof(double);
  dispatch1(in, [&](auto x) {
    P2I_LAUNCH((scale_dft_rows_kernel<Elem<decltype(x)>>), grid, dim3(128), lds, (hipStream_t)stream, x, S, S / 2 + 1, field, lut,
               divide_by_3, twiddle, G, nanflag);
  });
  return launch_status();
}

extern "C" int p2i_scale_dft_cols(const double* G, int T, int S, const double* twiddle, double* psd, void* stream) {
  P2I_REQUIRE(G && twiddle && psd && T > 0 && S > 0 && S <= P2I_SCALE_MAX_CROP, "bad arguments");
  const int NK = S / 2 + 1;
  // four columns per workgroup while their LDS image stays under 64 KB, two above
  if (S <= 512)
    P2I_LAUNCH(scale_dft_cols_kernel<4>, dim3(2u * (unsigned)T, (unsigned)ceil_div(NK, 4)), dim3(128), (size_t)10 * S * sizeof(double),
               (hipStream_t)stream, G, S, NK, twiddle, psd);
  else
    P2I_LAUNCH(scale_dft_cols_kernel<2>, dim3(2u * (unsigned)T, (unsigned)ceil_div(NK, 2)), dim3(128), (size_t)6 * S * sizeof(double),
               (hipStream_t)stream, G, S, NK, twiddle, psd);
  return launch_status();
}

extern "C" int p2i_scale_rings(const double* psd, int T, int S, const int* order, const double* weight, const int* offsets,
                               const double* count, int R, double* P, void* stream) {
  P2I_REQUIRE(psd && order && weight && offsets && count && P && T > 0 && S > 0 && R == S / 2 + 1, "bad arguments");
  P2I_LAUNCH(scale_rings_kernel, dim3(2u * (unsigned)T), dim3(128), 0, (hipStream_t)stream, psd, S * (S / 2 + 1), order, weight, offsets,
             count, R, P);
  return launch_status();
}

extern "C" int p2i_scale_spectrum_merge(const double* P, const int* nanflag, int64_t T, int R, double* out, void* stream) {
  P2I_REQUIRE(P && nanflag && out && T > 0 && R > 0, "bad arguments");
  P2I_LAUNCH(scale_spectrum_merge_kernel, dim3((unsigned)ceil_div(2 * R, 128)), dim3(128), 0, (hipStream_t)stream, P, nanflag,
             (long long)T, R, out);
  return launch_status();
}
