// Probabilistic verification of a (prediction, variance) pair against the truth on the device; DESIGN.md section 22.  Everything is
// scored on the inputs' own 0-255 scale in fp64: mu = prediction, s2 = variance (a third cropped input, or one scalar for the
// whole piece), y = truth, predictive distribution N(mu, s2), left-censored at 0 when `censor` is set.
//   p2i_prob_accumulate : ONE pass over an aligned piece of T frames of a rows x cols crop.  A workgroup of 128 threads takes
//                         P2I_PROB_WG_PIXELS consecutive pixels of the piece (frame-major, then row-major) and writes one partial
//                         record (layout: include/p2i_hip.h).  How the record's sums are formed, all of it free of floating-point
//                         atomics and therefore the same bits on every run:
//                           * scalar fp64 sums (CRPS, e, |e|, e^2, s2, z, z^2, interval widths, per threshold p and (p - o)^2)
//                             live in registers and fold over the workgroup with block_tree;
//                           * counts (scored / skipped / zero-variance pixels, interval hits, events, sigma-bin and reliability-
//                             bin populations) are 64-bit integer LDS atomics: exact, whatever the order;
//                           * binned sums of values in [0, 1] (p per reliability bin, the fractional PIT weights) are 64-bit
//                             integer LDS atomics of rint(v * 2^32);
//                           * the unbounded binned sums (s2 and e^2 per sigma-bin) go to a private LDS row per thread
//                             ([bin][thread], pitch 129 doubles) that one thread per bin folds in thread order.
//                         The PIT weights of a censored pixel with y == 0 spread over bins 0 .. m, m = floor(P0 nb): the m full
//                         bins each take w = 1 / (nb P0) and bin m the rest.  Instead of m + 1 atomics the kernel adds w once to
//                         a prefix table at m - 1 ("every bin <= m - 1") and the rest to bin m; the host adds the prefix table's
//                         suffix sums to the histogram.
//   p2i_prob_merge      : acc[w] += the sum of word w over the records in a fixed order, one workgroup per word.
// Compiled with -ffp-contract=off: the rain-rate transform of eval_common.h and the decisions (bins, interval ends) round as the
// separate operations of tests/prob_ref.py do.
#include "eval_common.h"

namespace p2i {

constexpr int PK = P2I_EXP1_MAX_THR;
constexpr int PL = P2I_PROB_MAX_LEVELS;
constexpr int PE = P2I_PROB_MAX_EDGES;
constexpr int PS = PE + 1;                       // sigma-bins: underflow, the PE - 1 inner ones, overflow
constexpr int PNB = P2I_PROB_MAX_PIT_BINS;
constexpr int PRB = P2I_PROB_MAX_REL_BINS;
constexpr int PTH = 128;                         // threads of a workgroup
constexpr int PPT = P2I_PROB_WG_PIXELS / PTH;    // pixels per thread
constexpr int PPITCH = PTH + 1;                  // of a private row: threads of one bin and bins of one thread fall on distinct banks
typedef unsigned long long u64;
static_assert(P2I_PROB_WG_PIXELS % PTH == 0, "workgroup pixels");

enum { PF_CRPS = 0, PF_E, PF_AE, PF_E2, PF_S2, PF_Z, PF_Z2, PF_NSCALAR };
enum { PI_N = 0, PI_SKIP, PI_ZERO, PI_NSCALAR };

// offsets of the record's sections, in 64-bit words (the fp64 sections first, then the int64 ones)
struct PLayout {
  int K, L, NS, NB, RB;
  __host__ __device__ int f_w() const { return PF_NSCALAR; }
  __host__ __device__ int f_p() const { return f_w() + L; }
  __host__ __device__ int f_br() const { return f_p() + K; }
  __host__ __device__ int f_sv() const { return f_br() + K; }
  __host__ __device__ int f_se() const { return f_sv() + NS; }
  __host__ __device__ int nf() const { return f_se() + NS; }
  __host__ __device__ int i_in() const { return PI_NSCALAR; }
  __host__ __device__ int i_o() const { return i_in() + L; }
  __host__ __device__ int i_pit() const { return i_o() + K; }
  __host__ __device__ int i_pre() const { return i_pit() + NB; }
  __host__ __device__ int i_sn() const { return i_pre() + NB; }
  __host__ __device__ int i_rn() const { return i_sn() + NS; }
  __host__ __device__ int i_ro() const { return i_rn() + K * RB; }
  __host__ __device__ int i_rp() const { return i_ro() + K * RB; }
  __host__ __device__ int ni() const { return i_rp() + K * RB; }
};
constexpr int PNI_MAX = PI_NSCALAR + PL + PK + 2 * PNB + PS + 3 * PK * PRB;

struct PArgs {
  double q[PK];        // thresholds, mm/h: the observed event is transform(y) >= q
  double xq[PK];       // the same thresholds on the pixel scale: the forecast probability is Phi((mu - xq) / sigma)
  double h[PL];        // half-widths Phi^-1((1 + level) / 2)
  double edge[PE];     // ascending sigma edges
  PLayout lay;
  int nedges, censor, div3;
};

// the per-thread scalar sums; block_tree folds them
struct PRec {
  static constexpr int WORDS = PF_NSCALAR + PL + 2 * PK;
  double v[WORDS];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < WORDS; ++i) v[i] = 0.0;
  }
  __device__ __forceinline__ void merge(const PRec& b) {
#pragma unroll
    for (int i = 0; i < WORDS; ++i) v[i] += b.v[i];
  }
  __device__ __forceinline__ void store(double* p) const {
#pragma unroll
    for (int i = 0; i < WORDS; ++i) p[i] = v[i];
  }
  static __device__ __forceinline__ PRec load(const double* p) {
    PRec r;
#pragma unroll
    for (int i = 0; i < WORDS; ++i) r.v[i] = p[i];
    return r;
  }
};

constexpr double P_SQRT1_2 = 0.70710678118654752440;
constexpr double P_INV_SQRT_2PI = 0.39894228040143267794;
constexpr double P_INV_SQRT_PI = 0.56418958354775628695;
constexpr double P_FIX = 4294967296.0;           // 2^32

__device__ __forceinline__ double Phi(double x) { return 0.5 * erfc(-x * P_SQRT1_2); }
__device__ __forceinline__ double phi(double x) { return exp(-0.5 * x * x) * P_INV_SQRT_2PI; }
__device__ __forceinline__ u64 fix32(double w) { return (u64)rint(w * P_FIX); }
__device__ __forceinline__ int bin_of(double u, int nb) {
  const int b = (int)floor(u * (double)nb);      // u in [0, 1]; the lower clamp keeps an infinite input's NaN inside the table
  return b > nb - 1 ? nb - 1 : (b < 0 ? 0 : b);
}

template <typename T> __device__ __forceinline__ double raw(const T* p, long long i) { return (double)p[i]; }

// the variance input: a cropped array of dtype vdt, or (p == NULL) the scalar s0
struct PVar {
  const void* p;
  int dt, h, w, top, left;
  double s0;
  __device__ __forceinline__ double at(long long t, int y, int x) const {
    if (!p) return s0;
    const long long i = t * h * w + (long long)(top + y) * w + left + x;
    if (dt == P2I_EXP1_F64) return ((const double*)p)[i];
    if (dt == P2I_EXP1_F32) return (double)((const float*)p)[i];
    return (double)((const uint8_t*)p)[i];
  }
};

template <typename PT, typename GT>
__global__ __launch_bounds__(PTH) void prob_accumulate_kernel(Crop<PT> pred, Crop<GT> gt, PVar var, long long total, int rows, int cols,
                                                              const int* __restrict__ rank, const double* __restrict__ lut, PArgs a,
                                                              double* __restrict__ part) {
  __shared__ u64 itab[PNI_MAX];
  __shared__ double fbuf[2 * PS * PPITCH > PTH * PRec::WORDS ? 2 * PS * PPITCH : PTH * PRec::WORDS];   // private rows, then the tree
  const PLayout lay = a.lay;
  const int K = lay.K, L = lay.L, NS = lay.NS, NB = lay.NB, RB = lay.RB;
  const int tid = threadIdx.x;
  for (int i = tid; i < lay.ni(); i += PTH) itab[i] = 0;
  for (int j = 0; j < 2 * NS; ++j) fbuf[j * PPITCH + tid] = 0.0;
  __syncthreads();
  PRec s;
  s.zero();
  const int npix = rows * cols;
  const long long base = (long long)blockIdx.x * P2I_PROB_WG_PIXELS;
  const bool censor = a.censor != 0;
  long long nscored = 0, nskip = 0, nzero = 0;
  for (int it = 0; it < PPT; ++it) {
    const long long g = base + it * PTH + tid;
    if (g >= total) break;
    const long long t = g / npix;
    const int r = (int)(g - t * npix);
    if (rank && rank[r] < 0) continue;
    const int yy = r / cols, xx = r - yy * cols;
    const long long gi = gt.row(t, yy) + xx;
    const double mu = raw<PT>(pred.p, pred.row(t, yy) + xx);
    const double y = raw<GT>(gt.p, gi);
    const double s2 = var.at(t, yy, xx);
    if (mu != mu || y != y || s2 != s2 || s2 < 0.0 || (censor && y < 0.0)) {
      ++nskip;
      continue;
    }
    ++nscored;
    const double ty = tload<GT>(gt.p, gi, lut, a.div3);      // exp1's path to the observed rain rate
    const double sg = sqrt(s2);
    const double mc = (censor && mu < 0.0) ? 0.0 : mu;       // the point forecast mu'
    const double e = y - mc;
    s.v[PF_E] += e;
    s.v[PF_AE] += fabs(e);
    s.v[PF_E2] += e * e;
    s.v[PF_S2] += s2;
    int sb = 0;
#pragma unroll
    for (int j = 0; j < PE; ++j)
      if (j < a.nedges && a.edge[j] <= sg) ++sb;
    atomicAdd(&itab[lay.i_sn() + sb], (u64)1);
    fbuf[sb * PPITCH + tid] += s2;
    fbuf[(NS + sb) * PPITCH + tid] += e * e;
    if (sg > 0.0) {
      const double z = (y - mu) / sg, l = -mu / sg;
      const double Fz = Phi(z);
      double c = z * (2.0 * Fz - 1.0) + 2.0 * phi(z);
      double Fl = 0.0;
      if (censor) {
        Fl = Phi(l);
        c = -l * Fl * Fl + c - 2.0 * phi(l) * Fl - (1.0 - 0.5 * erfc(-l)) * P_INV_SQRT_PI;     // Phi(l sqrt 2) = erfc(-l) / 2
      } else {
        c = c - P_INV_SQRT_PI;
      }
      s.v[PF_CRPS] += sg * c;
      s.v[PF_Z] += z;
      s.v[PF_Z2] += z * z;
      if (censor && y == 0.0) {
        if (Fl <= 0.0) {
          atomicAdd(&itab[lay.i_pit()], fix32(1.0));
        } else {
          const int m = bin_of(Fl, NB);
          if (m > 0) atomicAdd(&itab[lay.i_pre() + m - 1], fix32((1.0 / (double)NB) / Fl));
          atomicAdd(&itab[lay.i_pit() + m], fix32((Fl - (double)m / (double)NB) / Fl));
        }
      } else {
        atomicAdd(&itab[lay.i_pit() + bin_of(Fz, NB)], fix32(1.0));
      }
    } else {
      ++nzero;
      s.v[PF_CRPS] += fabs(e);
      const double u = y < mc ? 0.0 : (y > mc ? 1.0 : 0.5);
      atomicAdd(&itab[lay.i_pit() + bin_of(u, NB)], fix32(1.0));
    }
#pragma unroll
    for (int k = 0; k < PL; ++k)
      if (k < L) {
        double lo = mu - a.h[k] * sg, hi = mu + a.h[k] * sg;
        if (censor) {
          lo = lo < 0.0 ? 0.0 : lo;
          hi = hi < 0.0 ? 0.0 : hi;
        }
        if (y >= lo && y <= hi) atomicAdd(&itab[lay.i_in() + k], (u64)1);
        s.v[PF_NSCALAR + k] += hi - lo;
      }
    const double tmc = sg > 0.0 ? 0.0 : mmhr(mc, a.div3);     // a point mass exceeds q when its rain rate does
#pragma unroll
    for (int k = 0; k < PK; ++k)
      if (k < K) {
        const double p = sg > 0.0 ? Phi((mu - a.xq[k]) / sg) : (tmc >= a.q[k] ? 1.0 : 0.0);
        const bool o = ty >= a.q[k];
        const double d = p - (o ? 1.0 : 0.0);
        s.v[PF_NSCALAR + PL + k] += p;
        s.v[PF_NSCALAR + PL + PK + k] += d * d;
        const int rb = k * RB + bin_of(p, RB);
        atomicAdd(&itab[lay.i_rn() + rb], (u64)1);
        atomicAdd(&itab[lay.i_rp() + rb], fix32(p));
        if (o) {
          atomicAdd(&itab[lay.i_o() + k], (u64)1);
          atomicAdd(&itab[lay.i_ro() + rb], (u64)1);
        }
      }
  }
  if (nscored) atomicAdd(&itab[PI_N], (u64)nscored);
  if (nskip) atomicAdd(&itab[PI_SKIP], (u64)nskip);
  if (nzero) atomicAdd(&itab[PI_ZERO], (u64)nzero);
  __syncthreads();
  const int NF = lay.nf(), NI = lay.ni();
  double* out = part + (long long)blockIdx.x * (NF + NI);
  long long* iout = (long long*)(out + NF);
  for (int i = tid; i < NI; i += PTH) iout[i] = (long long)itab[i];
  if (tid < 2 * NS) {
    double f = 0.0;
    for (int i = 0; i < PTH; ++i) f += fbuf[tid * PPITCH + i];
    out[lay.f_sv() + tid] = f;        // the e^2 section follows the s2 section
  }
  __syncthreads();
  block_tree<PTH>(s, fbuf);
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < PF_NSCALAR; ++i) out[i] = s.v[i];
#pragma unroll
    for (int k = 0; k < PL; ++k)
      if (k < L) out[lay.f_w() + k] = s.v[PF_NSCALAR + k];
#pragma unroll
    for (int k = 0; k < PK; ++k)
      if (k < K) {
        out[lay.f_p() + k] = s.v[PF_NSCALAR + PL + k];
        out[lay.f_br() + k] = s.v[PF_NSCALAR + PL + PK + k];
      }
  }
}

// acc[w] += the sum of word w over the records, in a fixed order: one workgroup of 64 threads per word, thread i adds records
// i, i + 64, ... ascending and a tree joins the threads.  Word w < nf is fp64, the rest int64.
__global__ __launch_bounds__(64) void prob_merge_kernel(const double* __restrict__ part, long long nparts, int nf, int nw,
                                                        double* __restrict__ acc) {
  __shared__ double fs[64];
  __shared__ long long is[64];
  const int w = blockIdx.x, tid = threadIdx.x;
  if (w < nf) {
    double s = 0.0;
    for (long long i = tid; i < nparts; i += 64) s += part[i * nw + w];
    fs[tid] = s;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
      if (tid < o) fs[tid] += fs[tid + o];
      __syncthreads();
    }
    if (tid == 0) acc[w] += fs[0];
  } else {
    long long s = 0;
    for (long long i = tid; i < nparts; i += 64) s += ((const long long*)part)[i * nw + w];
    is[tid] = s;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
      if (tid < o) is[tid] += is[tid + o];
      __syncthreads();
    }
    if (tid == 0) ((long long*)acc)[w] += is[0];
  }
}

static inline bool prob_layout(int nthr, int nlev, int nedges, int pit_bins, int rel_bins, PLayout* lay) {
  if (nthr < 0 || nthr > PK || nlev < 0 || nlev > PL || nedges < 0 || nedges > PE) return false;
  if (pit_bins < 1 || pit_bins > PNB || rel_bins < 1 || rel_bins > PRB) return false;
  *lay = PLayout{nthr, nlev, nedges + 1, pit_bins, rel_bins};
  return true;
}

}  // namespace p2i

using namespace p2i;

extern "C" int p2i_prob_record(int nthr, int nlevels, int nedges, int pit_bins, int rel_bins, int* nf, int* ni) {
  PLayout lay;
  P2I_REQUIRE(nf && ni && prob_layout(nthr, nlevels, nedges, pit_bins, rel_bins, &lay), "bad arguments");
  *nf = lay.nf();
  *ni = lay.ni();
  return P2I_OK;
}

extern "C" int p2i_prob_accumulate(const p2i_eval_input* pred, const p2i_eval_input* var, double var_scalar, const p2i_eval_input* truth,
                                   int64_t T, int rows, int cols, const int* rank, const double* lut, const double* thresholds_host,
                                   const double* xq_host, int nthr, const double* halfwidths_host, int nlevels, const double* edges_host,
                                   int nedges, int pit_bins, int rel_bins, int censor, int divide_by_3, double* part,
                                   int64_t part_words, void* stream) {
  P2I_REQUIRE(input_set(pred) && input_set(truth) && lut && part, "bad arguments");
  static const p2i_eval_input no_array{};
  if (!var) var = &no_array;      // as NULL data: var_scalar for every pixel
  P2I_REQUIRE(eval_dtype_ok(pred->dtype) && eval_dtype_ok(truth->dtype) && (!var->data || eval_dtype_ok(var->dtype)), "unsupported dtype");
  P2I_REQUIRE(T > 0 && rows > 0 && cols > 0 && (int64_t)rows * cols <= (int64_t)1 << 30, "bad frame count / crop");
  P2I_REQUIRE(crop_ok(pred, rows, cols), "crop outside the prediction");
  P2I_REQUIRE(crop_ok(truth, rows, cols), "crop outside the truth");
  P2I_REQUIRE(!var->data || crop_ok(var, rows, cols), "crop outside the variance");
  PArgs a;
  P2I_REQUIRE(prob_layout(nthr, nlevels, nedges, pit_bins, rel_bins, &a.lay), "at most %d thresholds, %d levels, %d edges, %d PIT bins, %d reliability bins",
              PK, PL, PE, PNB, PRB);
  P2I_REQUIRE((nthr == 0 || (thresholds_host && xq_host)) && (nlevels == 0 || halfwidths_host) && (nedges == 0 || edges_host),
              "missing host array");
  for (int i = 0; i < PK; ++i) {
    a.q[i] = i < nthr ? thresholds_host[i] : 0.0;
    a.xq[i] = i < nthr ? xq_host[i] : 0.0;
  }
  for (int i = 0; i < PL; ++i) {
    P2I_REQUIRE(i >= nlevels || halfwidths_host[i] >= 0.0, "a half-width is >= 0");
    a.h[i] = i < nlevels ? halfwidths_host[i] : 0.0;
  }
  for (int i = 0; i < PE; ++i) {
    P2I_REQUIRE(i >= nedges || i == 0 || edges_host[i] > edges_host[i - 1], "sigma edges ascend");
    a.edge[i] = i < nedges ? edges_host[i] : 0.0;
  }
  a.nedges = nedges;
  a.censor = censor ? 1 : 0;
  a.div3 = divide_by_3;
  const long long total = (long long)T * rows * cols;
  const long long nwg = (total + P2I_PROB_WG_PIXELS - 1) / P2I_PROB_WG_PIXELS;
  P2I_REQUIRE(nwg <= 0x7fffffffLL && part_words >= nwg * (a.lay.nf() + a.lay.ni()), "partial buffer too small");
  const PVar v{var->data, var->dtype, var->h, var->w, var->top, var->left, var_scalar};
  dispatch2(pred, truth, [&](auto p, auto g) {
    P2I_LAUNCH((prob_accumulate_kernel<Elem<decltype(p)>, Elem<decltype(g)>>), dim3((unsigned)nwg), dim3(PTH), 0, (hipStream_t)stream, p,
               g, v, total, rows, cols, rank, lut, a, part);
  });
  return launch_status();
}

extern "C" int p2i_prob_merge(const double* part, int64_t nparts, int nf, int ni, double* acc, void* stream) {
  P2I_REQUIRE(part && acc && nparts > 0 && nf > 0 && ni > 0, "bad arguments");
  P2I_LAUNCH(prob_merge_kernel, dim3((unsigned)(nf + ni)), dim3(64), 0, (hipStream_t)stream, part, (long long)nparts, nf, nf + ni, acc);
  return launch_status();
}
