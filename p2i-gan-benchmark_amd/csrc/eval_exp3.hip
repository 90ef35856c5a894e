// The benchmark's exp3 analysis (reference experiments/exp3.py run_exp3, experiments/io.py) on the device; DESIGN.md section 11.
//   p2i_exp3_accumulate : ONE pass over an aligned (pred, truth) piece of T frames, both transformed as in exp1 (eval_common.h)
//                         and center-cropped to S x S.  Per frame it writes
//                           * rec[t] = (n, sum (p-g)^2, truth mean, truth M2) over the selection's finite pairs (Welford per
//                             thread, Chan's fold over the workgroup in a fixed order);
//                           * rows[t][y] = the scatter pool of crop row y: pixels of the whole crop with p, g finite, g >= 0.1;
//                           * into hist[65] (when given): the 64 log-frequency bins of the prediction's finite values in [0, 32]
//                             (bin min(floor(2 p), 63)) and, last, its count of finite values.  Integer counts: exact.
//   p2i_exp3_truth_hist : the same 65 counters for every frame of a truth event
//   p2i_exp3_scan       : the inclusive prefix (int64) of a method's row counts: pool ordinal k lies in the first row whose prefix
//                         exceeds k
//   p2i_exp3_gather     : for K pool ordinals, in the order given, the (g, p) pair: binary search over the prefix for the row,
//                         then a scan of that row for the j-th kept pixel.  Called once per aligned piece; a piece writes only
//                         the ordinals that fall in its rows.
//   p2i_exp3_nse        : per event the nanmean of the clipped per-frame NSEs, and the whole-stack NSE from the frame records
//                         folded in one fixed order (strided per thread, then a tree)
// Compiled with -ffp-contract=off: the transform rounds as numpy's separate operations do (as in eval_exp1.hip).
#include "eval_common.h"

namespace p2i {

constexpr int NREC = P2I_EXP3_NREC;     // n, sum d^2, mean, M2
constexpr int LBINS = P2I_EXP3_BINS;
constexpr int NHIST = P2I_EXP3_NHIST;
static_assert(NREC == 4 && NHIST == LBINS + 1, "exp3 layout");

struct Rec {
  static constexpr int WORDS = NREC;
  double n, sq, mean, m2;
  __device__ __forceinline__ void merge(const Rec& b) {
    chan_merge(n, mean, m2, b.n, b.mean, b.m2);
    sq += b.sq;
  }
  __device__ __forceinline__ void store(double* p) const { p[0] = n; p[1] = sq; p[2] = mean; p[3] = m2; }
  static __device__ __forceinline__ Rec load(const double* p) { return Rec{p[0], p[1], p[2], p[3]}; }
};

// 1 - sum d^2 / (M2 + 1e-10) (experiments/exp3.py nse), NaN without a finite pair
__device__ __forceinline__ double rec_nse(const Rec& r) { return r.n > 0.0 ? 1.0 - r.sq / (r.m2 + 1e-10) : __builtin_nan(""); }

// the log-frequency bin of a transformed value (edges np.linspace(0, 32, 65), multiples of 0.5): -1 outside [0, 32] / not finite
__device__ __forceinline__ int lf_bin(double v) {
  if (!isfinite(v) || v < 0.0 || v > 32.0) return -1;
  const int b = (int)(v * 2.0);     // exact: v * 2 is exact and v >= 0
  return b > LBINS - 1 ? LBINS - 1 : b;
}

__device__ __forceinline__ void hist_flush(const int* h, unsigned long long* hist) {
  if ((int)threadIdx.x < NHIST && h[threadIdx.x] != 0) atomicAdd(hist + threadIdx.x, (unsigned long long)h[threadIdx.x]);
}

// One workgroup (4 waves) per frame; wave w takes crop rows w, w + 4, ...; lane l takes columns l, l + 64, ... of the row.
template <typename PT, typename GT>
__global__ __launch_bounds__(256) void exp3_accumulate_kernel(Crop<PT> pred, Crop<GT> gt, int S, const int* __restrict__ rank,
                                                              const double* __restrict__ lut, int div3, double* __restrict__ rec,
                                                              int* __restrict__ rows, unsigned long long* __restrict__ hist) {
  __shared__ int h[NHIST];
  __shared__ double red[256 * NREC];
  const long long t = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if ((int)threadIdx.x < NHIST) h[threadIdx.x] = 0;
  __syncthreads();
  Rec r{0.0, 0.0, 0.0, 0.0};
  for (int y = wave; y < S; y += 4) {
    int cnt = 0;
    for (int x0 = 0; x0 < S; x0 += 64) {
      const int x = x0 + lane;
      bool keep = false;
      if (x < S) {
        const double p = pred.at(t, y, x, lut, div3);
        const double g = gt.at(t, y, x, lut, div3);
        const bool fp = isfinite(p), fg = isfinite(g);
        keep = fp && fg && g >= 0.1;
        if (fp && fg && rank[y * S + x] >= 0) {
          const double d = p - g;
          r.sq += d * d;
          welford_push(r.n, r.mean, r.m2, g);
        }
        if (hist) {
          const int b = lf_bin(p);
          if (b >= 0) atomicAdd(&h[b], 1);
          if (fp) atomicAdd(&h[LBINS], 1);
        }
      }
      cnt += __popcll(__ballot(keep));
    }
    if (lane == 0) rows[t * S + y] = cnt;
  }
  block_tree<256>(r, red);
  if (threadIdx.x == 0) r.store(rec + t * NREC);
  if (hist) hist_flush(h, hist);
}

template <typename GT>
__global__ __launch_bounds__(256) void exp3_truth_hist_kernel(Crop<GT> gt, int S, const double* __restrict__ lut, int div3,
                                                              unsigned long long* __restrict__ hist) {
  __shared__ int h[NHIST];
  const long long t = blockIdx.x;
  if ((int)threadIdx.x < NHIST) h[threadIdx.x] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < S * S; i += 256) {
    const int y = i / S, x = i - y * S;
    const double g = gt.at(t, y, x, lut, div3);
    const int b = lf_bin(g);
    if (b >= 0) atomicAdd(&h[b], 1);
    if (isfinite(g)) atomicAdd(&h[LBINS], 1);
  }
  __syncthreads();
  hist_flush(h, hist);
}

// inclusive prefix of n int32 counts into int64, one workgroup of 1024 threads: thread i sums its contiguous chunk, a
// Hillis-Steele scan over the chunk sums gives each chunk's offset, then every thread writes its chunk's prefix
__global__ __launch_bounds__(1024) void exp3_scan_kernel(const int* __restrict__ rows, long long n, long long* __restrict__ prefix) {
  __shared__ long long s[1024];
  const long long chunk = (n + 1023) / 1024;
  const long long b0 = (long long)threadIdx.x * chunk;
  const long long b1 = b0 + chunk < n ? b0 + chunk : n;
  long long sum = 0;
  for (long long i = b0; i < b1; ++i) sum += rows[i];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const long long v = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += v;
    __syncthreads();
  }
  long long run = s[threadIdx.x] - sum;
  for (long long i = b0; i < b1; ++i) {
    run += rows[i];
    prefix[i] = run;
  }
}

template <typename PT, typename GT>
__global__ __launch_bounds__(256) void exp3_gather_kernel(Crop<PT> pred, Crop<GT> gt, int T, int S, const double* __restrict__ lut,
                                                          int div3, const long long* __restrict__ prefix, long long row0,
                                                          const long long* __restrict__ ords, int K, double* __restrict__ out_g,
                                                          double* __restrict__ out_p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K) return;
  const long long nrows = (long long)T * S;
  const long long lo = row0 > 0 ? prefix[row0 - 1] : 0;
  const long long o = ords[i];
  if (o < lo || o >= prefix[row0 + nrows - 1]) return;      // another piece's ordinal
  long long a = row0, b = row0 + nrows - 1;                  // the first row of the piece whose prefix exceeds o
  while (a < b) {
    const long long m = a + (b - a) / 2;
    if (prefix[m] > o) b = m;
    else a = m + 1;
  }
  long long j = o - (a > row0 ? prefix[a - 1] : lo);
  const long long lr = a - row0;
  const long long t = lr / S;
  const int y = (int)(lr - t * S);
  const long long prow = pred.row(t, y), grow = gt.row(t, y);
  for (int x = 0; x < S; ++x) {
    const double p = pred.at(prow, x, lut, div3);
    const double g = gt.at(grow, x, lut, div3);
    if (isfinite(p) && isfinite(g) && g >= 0.1) {
      if (j == 0) {
        out_g[i] = g;
        out_p[i] = p;
        return;
      }
      --j;
    }
  }
}

// out[0] = the whole-stack NSE from srec[0 .. T); out[1 + e] = nanmean over frames [off[e], off[e+1]) of erec of max(NSE, 0)
// (NaN where no frame is finite)
__global__ __launch_bounds__(256) void exp3_nse_kernel(const double* __restrict__ erec, const int* __restrict__ off, int E,
                                                       const double* __restrict__ srec, int T, double* __restrict__ out) {
  __shared__ double red[256 * NREC];
  Rec r{0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < T; i += 256) r.merge(Rec::load(srec + (long long)i * NREC));
  block_tree<256>(r, red);
  if (threadIdx.x == 0) out[0] = rec_nse(r);
  for (int e = threadIdx.x; e < E; e += 256) {
    double s = 0.0, c = 0.0;
    for (int f = off[e]; f < off[e + 1]; ++f) {
      const double v = rec_nse(Rec::load(erec + (long long)f * NREC));
      if (isfinite(v)) {
        s += v > 0.0 ? v : 0.0;
        c += 1.0;
      }
    }
    out[1 + e] = c > 0.0 ? s / c : __builtin_nan("");
  }
}

}  // namespace p2i

using namespace p2i;

extern "C" int p2i_exp3_accumulate(const p2i_eval_input* pred, const p2i_eval_input* truth, int T, int S, const int* rank,
                                   const double* lut, int divide_by_3, double* rec, int* rows, uint64_t* hist, void* stream) {
  P2I_REQUIRE(input_set(pred) && input_set(truth) && rank && lut && rec && rows, "bad arguments");
  P2I_REQUIRE(eval_dtype_ok(pred->dtype) && eval_dtype_ok(truth->dtype), "unsupported dtype");
  P2I_REQUIRE(T > 0 && S > 0, "bad frame count / crop");
  P2I_REQUIRE(crop_ok(pred, S, S), "crop outside the prediction");
  P2I_REQUIRE(crop_ok(truth, S, S), "crop outside the truth");
  const hipStream_t s = (hipStream_t)stream;
  dispatch2(pred, truth, [&](auto p, auto g) {
    P2I_LAUNCH((exp3_accumulate_kernel<Elem<decltype(p)>, Elem<decltype(g)>>), dim3((unsigned)T), dim3(256), 0, s, p, g, S, rank, lut,
               divide_by_3, rec, rows, (unsigned long long*)hist);
  });
  return launch_status();
}

extern "C" int p2i_exp3_truth_hist(const p2i_eval_input* truth, int T, int S, const double* lut, int divide_by_3, uint64_t* hist,
                                   void* stream) {
  P2I_REQUIRE(input_set(truth) && lut && hist && eval_dtype_ok(truth->dtype) && T > 0 && S > 0, "bad arguments");
  P2I_REQUIRE(crop_ok(truth, S, S), "crop outside the truth");
  const hipStream_t s = (hipStream_t)stream;
  dispatch1(truth, [&](auto g) {
    P2I_LAUNCH(exp3_truth_hist_kernel<Elem<decltype(g)>>, dim3((unsigned)T), dim3(256), 0, s, g, S, lut, divide_by_3,
               (unsigned long long*)hist);
  });
  return launch_status();
}

extern "C" int p2i_exp3_scan(const int* rows, int64_t n, int64_t* prefix, void* stream) {
  P2I_REQUIRE(rows && prefix && n > 0, "bad arguments");
  P2I_LAUNCH(exp3_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rows, (long long)n, (long long*)prefix);
  return launch_status();
}

extern "C" int p2i_exp3_gather(const p2i_eval_input* pred, const p2i_eval_input* truth, int T, int S, const double* lut, int divide_by_3,
                               const int64_t* prefix, int64_t row0, const int64_t* ords, int K, double* out_g, double* out_p,
                               void* stream) {
  P2I_REQUIRE(input_set(pred) && input_set(truth) && lut && prefix && ords && out_g && out_p && K > 0 && row0 >= 0, "bad arguments");
  P2I_REQUIRE(eval_dtype_ok(pred->dtype) && eval_dtype_ok(truth->dtype), "unsupported dtype");
  P2I_REQUIRE(T > 0 && S > 0, "bad frame count / crop");
  P2I_REQUIRE(crop_ok(pred, S, S), "crop outside the prediction");
  P2I_REQUIRE(crop_ok(truth, S, S), "crop outside the truth");
  const hipStream_t s = (hipStream_t)stream;
  dispatch2(pred, truth, [&](auto p, auto g) {
    P2I_LAUNCH((exp3_gather_kernel<Elem<decltype(p)>, Elem<decltype(g)>>), dim3((unsigned)ceil_div(K, 256)), dim3(256), 0, s, p, g, T, S,
               lut, divide_by_3, (const long long*)prefix, (long long)row0, (const long long*)ords, K, out_g, out_p);
  });
  return launch_status();
}

extern "C" int p2i_exp3_nse(const double* event_rec, const int* event_off, int E, const double* stack_rec, int T, double* out,
                            void* stream) {
  P2I_REQUIRE(out && E >= 0 && T >= 0 && (E == 0 || (event_rec && event_off)) && (T == 0 || stack_rec), "bad arguments");
  P2I_LAUNCH(exp3_nse_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, event_rec, event_off, E, stack_rec, T, out);
  return launch_status();
}
