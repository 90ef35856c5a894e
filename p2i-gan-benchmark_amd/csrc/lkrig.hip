// Moving-neighbourhood space-time ordinary kriging: every target is predicted from its k nearest points in the
// space-time metric, from a small system of its own, which also gives the kriging variance and, with the target's own site taken
// out of the candidates, leave-one-site-out.  The points are the per-frame arrays of p2i_krig_compact, read as they are: there is no
// per-sample limit.
//
// One wave per target, one wave per workgroup (so that __syncthreads is the wave's own LDS fence and no wave waits for another),
// TPB targets per workgroup one after the other.
//   selection  lane j holds entry j of the sorted list of the best (key, point) so far in registers; the window's candidates are
//              streamed 64 at a time, those below the k-th entry are inserted one by one (ballot for the position, one lane shift).
//              key = d2 + kappa^2 dt^2 in fp64 by one rounded product and one rounded sum; order (key, frame, raster) = (key, point).
//   system     K's lower triangle in LDS, row stride KC + 1 (lane = row: column reads and row reads are both conflict free); fp32
//              entries, left-looking Cholesky by columns with fp64 dot products; the two substitutions (right-hand sides c0 and 1)
//              in fp64 with the column's pivot broadcast from its lane.
// Every sum has a fixed order; the count of failed targets is an integer atomic.
//
// LAG: the same kernels in the frame that moves with the rain, one velocity v = (v_y, v_x) per sample (velf, fp32).
// The key becomes (e_y^2 + e_x^2) + kappa^2 dt^2 with e = (target - point) - v dt in fp64, every operation rounded once; K and c0 take
// lag_dist in place of st_dist.  Everything else, and every LAG = false instantiation, is as it was.
#include "krig_common.h"

namespace p2i {
namespace {

constexpr int LK_TPB = 8;                 // targets per workgroup
constexpr int LK_NONE = 0x7fffffff;       // the point index of an empty list entry

struct LkArgs {
  const int* pix;
  const float* z;
  const int* counts;
  const float* params;
  const int* cand;
  const double* stat;
  const float* velf;     // [B][2] = (v_y, v_x), read by the LAG kernels only (else null)
  int model, k, frames, T, fcap;
  double none;           // +inf, the key of an empty list entry: handed in by the host so that the wave-uniform threshold starts from a
                         // loaded scalar pair (as a 64-bit scalar literal the compiler's move keeps 32 bits of it)
};

__device__ __forceinline__ bool lk_before(double ka, int ia, double kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

// lane `src` (wave-uniform) of v to every lane through a scalar register: no trip through the LDS crossbar
__device__ __forceinline__ int lane_i(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ double lane_d(double v, int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

__device__ __forceinline__ double wave_sum_d(double v) {    // fixed butterfly: every lane gets the same sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- the sample's gauge mean and point count, stat [B][2] fp64: 256 threads take the points slot-strided, frame by frame, then the
// fixed tree
__global__ __launch_bounds__(256) void lkrig_stat_kernel(const float* __restrict__ z, const int* __restrict__ counts, int T, int fcap,
                                                         double* __restrict__ stat) {
  __shared__ double red[256];
  const int b = blockIdx.x;
  double s = 0.0, c = 0.0;
  for (int t = 0; t < T; ++t) {
    const int f = b * T + t;
    const int n = min(counts[f], fcap);
    for (int i = threadIdx.x; i < n; i += 256) {
      s += (double)z[(size_t)f * fcap + i];
      c += 1.0;
    }
  }
  s = block_sum_d(s, red);
  c = block_sum_d(c, red);
  if (threadIdx.x == 0) {
    stat[b * 2] = c > 0.0 ? s / c : 0.0;
    stat[b * 2 + 1] = c;
  }
}

// One target (frame t of sample b, pixel (ty, tx)) by the whole wave.  excl >= 0: the candidates at pixel code excl are left out
// (leave-one-site-out).  Returns through pred / var (all lanes alike) and m, the number of neighbours; nbr (nullable) gets the
// selection, -1 past m.  fail: 1 where a pivot was not positive.
template <int KC, bool LAG>
__device__ __forceinline__ void lk_target(const LkArgs& A, float* __restrict__ sK, int b, int t, int ty, int tx, int excl, float nug,
                                          float psill, float a, float kap, float vy, float vx, float& pred, float& var, int& fail,
                                          int* __restrict__ nbr) {
  constexpr int S = KC + 1;
  const int lane = threadIdx.x;
  const int k = A.k;
  const double kk = (double)kap * (double)kap;
  const float k2 = kap * kap;
  // ---- selection
  double ekey = A.none;
  int eidx = LK_NONE;
  double tk = A.none;            // the k-th entry: a candidate enters only before it
  int ti = LK_NONE;
  for (int ad = 0; ad <= A.frames; ++ad) {
    const double kdt = __dmul_rn(kk, (double)(ad * ad));
    if (kdt > tk) break;         // every key of this and of the farther frames is at least kdt
    for (int sgn = 0; sgn < (ad ? 2 : 1); ++sgn) {
      const int tp = sgn ? t + ad : t - ad;
      if (tp < 0 || tp >= A.T) continue;
      const size_t f = (size_t)b * A.T + tp;
      const int n = min(A.counts[f], A.fcap);
      double oy = 0.0, ox = 0.0;               // LAG: v (t - t'), one rounded product per axis
      if constexpr (LAG) {
        const double fdt = (double)(t - tp);
        oy = __dmul_rn((double)vy, fdt);
        ox = __dmul_rn((double)vx, fdt);
      }
      for (int c0 = 0; c0 < n; c0 += 64) {
        const int slot = c0 + lane;
        bool ok = slot < n;
        double ck = HUGE_VAL;
        const int ci = tp * A.fcap + slot;
        if (ok) {
          const int g = A.pix[f * A.fcap + slot];
          const int dy = ty - (g >> 16), dx = tx - (g & 0xffff);
          if constexpr (LAG) {
            const double ey = __dadd_rn((double)dy, -oy), ex = __dadd_rn((double)dx, -ox);
            ck = __dadd_rn(__dadd_rn(__dmul_rn(ey, ey), __dmul_rn(ex, ex)), kdt);
          } else {
            ck = __dadd_rn((double)(dy * dy + dx * dx), kdt);
          }
          ok = g != excl;
        }
        unsigned long long todo = __ballot(ok && lk_before(ck, ci, tk, ti));
        while (todo) {
          const int src = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const double bk = lane_d(ck, src);
          const int bi = lane_i(ci, src);
          if (!lk_before(bk, bi, tk, ti)) continue;
          const int pos = __popcll(__ballot(lk_before(ekey, eidx, bk, bi)));     // the entries before it are a prefix
          const double uk = __shfl_up(ekey, 1);
          const int ui = __shfl_up(eidx, 1);
          if (lane == pos) {
            ekey = bk;
            eidx = bi;
          } else if (lane > pos) {
            ekey = uk;
            eidx = ui;
          }
          tk = lane_d(ekey, k - 1);
          ti = lane_i(eidx, k - 1);
        }
      }
    }
  }
  const bool mine = lane < k && eidx != LK_NONE;
  const int m = __popcll(__ballot(mine));
  if (nbr != nullptr && lane < k) nbr[lane] = mine ? eidx : -1;
  fail = 0;
  if (m == 0) {                  // no candidate in the window: the sample's gauge mean
    pred = (float)A.stat[b * 2];
    var = __builtin_nanf("");
    return;
  }
  // ---- the neighbours, lane = selection rank
  int g = 0, gt = 0;
  double zi = 0.0;
  if (mine) {
    gt = eidx / A.fcap;
    const size_t e = ((size_t)b * A.T + gt) * A.fcap + (eidx - gt * A.fcap);
    g = A.pix[e];
    zi = (double)A.z[e];
  }
  const int gy = g >> 16, gx = g & 0xffff;
  float c0 = 0.f;
  if (mine) {
    const int dy = ty - gy, dx = tx - gx, dt = t - gt;
    const int d2 = dy * dy + dx * dx;
    float h;
    if constexpr (LAG)
      h = lag_dist((float)dy, (float)dx, (float)dt, vy, vx, k2);
    else
      h = st_dist(d2, dt, k2);
    c0 = cov_f(h, psill, a, A.model) + ((d2 | dt) == 0 ? nug : 0.f);
  }
  const bool at_gauge = lane_d(ekey, 0) == 0.0;      // key 0: the same pixel in the same frame (kappa > 0)
  __syncthreads();               // the previous target's reads of sK are done
  for (int j = 0; j < m; ++j) {
    const int pj = lane_i(g, j), tj = lane_i(gt, j);
    if (mine && lane >= j) {
      const int dy = gy - (pj >> 16), dx = gx - (pj & 0xffff);
      float h;
      if constexpr (LAG)
        h = lag_dist((float)dy, (float)dx, (float)(gt - tj), vy, vx, k2);
      else
        h = st_dist(dy * dy + dx * dx, gt - tj, k2);
      sK[lane * S + j] = cov_f(h, psill, a, A.model) + (lane == j ? nug : 0.f);
    }
  }
  __syncthreads();
  // ---- K = L L^T, column by column, lane = row
  double rinv = 0.0;
  for (int j = 0; j < m; ++j) {
    double s = 0.0;
    if (mine && lane >= j) {
      s = (double)sK[lane * S + j];
      for (int c = 0; c < j; ++c) s = fma(-(double)sK[lane * S + c], (double)sK[j * S + c], s);
    }
    const float d = (float)lane_d(s, j);
    if (!(d > 0.f)) {
      fail = 1;
      break;
    }
    const float l = sqrtf(d);
    if (mine && lane >= j) sK[lane * S + j] = lane == j ? l : (float)s / l;
    double r = (double)(1.f / l);            // 1 / L_jj to fp64 by one Newton step, kept by lane j for the substitutions
    r = r * fma(-(double)l, r, 2.0);
    if (lane == j) rinv = r;
    __syncthreads();
  }
  if (fail) {                    // the mean of the selected values
    pred = (float)(wave_sum_d(zi) / (double)m);
    var = __builtin_nanf("");
    return;
  }
  // ---- L y = (c0, 1), then L^T (a, u) = y
  double y = mine ? (double)c0 : 0.0, w = mine ? 1.0 : 0.0;
  for (int j = 0; j < m; ++j) {
    const double rj = lane_d(rinv, j);
    const double yj = lane_d(y, j) * rj, wj = lane_d(w, j) * rj;
    if (lane == j) {
      y = yj;
      w = wj;
    } else if (mine && lane > j) {
      const double l = (double)sK[lane * S + j];
      y = fma(-l, yj, y);
      w = fma(-l, wj, w);
    }
  }
  for (int j = m - 1; j >= 0; --j) {
    const double rj = lane_d(rinv, j);
    const double yj = lane_d(y, j) * rj, wj = lane_d(w, j) * rj;
    if (lane == j) {
      y = yj;
      w = wj;
    } else if (lane < j) {
      const double l = (double)sK[j * S + lane];
      y = fma(-l, yj, y);
      w = fma(-l, wj, w);
    }
  }
  const double sa = wave_sum_d(y), su = wave_sum_d(w);
  const double mu = (sa - 1.0) / su;
  const double lam = y - mu * w;             // 0 on the lanes past m
  const double zh = wave_sum_d(lam * zi);
  const double lc = wave_sum_d(lam * (double)c0);
  const double v = ((double)psill + (double)nug) - lc - mu;
  pred = (float)zh;
  var = at_gauge ? 0.f : (float)fmax(v, 0.0);
}

// parameters of sample b; returns 0 for a sample whose targets take a rule and no system (out0 / var0 hold it)
__device__ __forceinline__ int lk_sample(const LkArgs& A, int b, float& nug, float& psill, float& a, float& kap, float& out0) {
  nug = A.params[b * 4];
  psill = A.params[b * 4 + 1];
  a = A.params[b * 4 + 2];
  kap = A.params[b * 4 + 3];
  if (!(A.stat[b * 2 + 1] > 0.0)) {          // no gauge at all: zeros
    out0 = 0.f;
    return 0;
  }
  if (A.cand != nullptr && A.cand[b] < 0) {  // degenerate fit: the gauge mean
    out0 = (float)A.stat[b * 2];
    return 0;
  }
  return 1;
}

template <int KC, bool LAG>
__global__ __launch_bounds__(64) void lkrig_predict_kernel(LkArgs A, int W, int HW, float* __restrict__ out, float* __restrict__ var,
                                                           int* __restrict__ status, int* __restrict__ nbr) {
  __shared__ float sK[KC * (KC + 1)];
  const int b = blockIdx.z, t = blockIdx.y;
  float nug, psill, a, kap, out0 = 0.f;
  const int live = lk_sample(A, b, nug, psill, a, kap, out0);
  float vy = 0.f, vx = 0.f;
  if constexpr (LAG) {
    vy = A.velf[b * 2];
    vx = A.velf[b * 2 + 1];
  }
  int failed = 0;
  for (int q = 0; q < LK_TPB; ++q) {
    const int p = blockIdx.x * LK_TPB + q;
    if (p >= HW) break;
    const size_t o = ((size_t)b * A.T + t) * HW + p;
    int* nb = nbr != nullptr ? nbr + o * A.k : nullptr;
    float pr = out0, vr = __builtin_nanf("");
    if (live) {
      int fail;
      lk_target<KC, LAG>(A, sK, b, t, p / W, p % W, -1, nug, psill, a, kap, vy, vx, pr, vr, fail, nb);
      failed += fail;
    } else if (nb != nullptr && (int)threadIdx.x < A.k) {
      nb[threadIdx.x] = -1;
    }
    if (threadIdx.x == 0) {
      out[o] = pr;
      if (var != nullptr) var[o] = vr;
    }
  }
  if (threadIdx.x == 0 && failed) atomicAdd(status + b, failed);
}

// the points as targets, each without the candidates at its own pixel; pred / var [B T][fcap], 0 past the frame's count
template <int KC, bool LAG>
__global__ __launch_bounds__(64) void lkrig_loso_kernel(LkArgs A, float* __restrict__ pred, float* __restrict__ var, int* __restrict__ status) {
  __shared__ float sK[KC * (KC + 1)];
  const int b = blockIdx.z, t = blockIdx.y;
  const size_t f = (size_t)b * A.T + t;
  const int n = min(A.counts[f], A.fcap);
  float nug, psill, a, kap, out0 = 0.f;
  const int live = lk_sample(A, b, nug, psill, a, kap, out0);
  float vy = 0.f, vx = 0.f;
  if constexpr (LAG) {
    vy = A.velf[b * 2];
    vx = A.velf[b * 2 + 1];
  }
  int failed = 0;
  for (int q = 0; q < LK_TPB; ++q) {
    const int i = blockIdx.x * LK_TPB + q;
    if (i >= A.fcap) break;
    float pr = 0.f, vr = 0.f;
    if (i < n) {
      pr = vr = __builtin_nanf("");
      if (live) {
        const int g = A.pix[f * A.fcap + i];
        int fail;
        lk_target<KC, LAG>(A, sK, b, t, g >> 16, g & 0xffff, g, nug, psill, a, kap, vy, vx, pr, vr, fail, nullptr);
        failed += fail;
        if (vr != vr && !fail) pr = vr;      // no candidate left: no score
      }
    }
    if (threadIdx.x == 0) {
      pred[f * A.fcap + i] = pr;
      var[f * A.fcap + i] = vr;
    }
  }
  if (threadIdx.x == 0 && failed) atomicAdd(status + b, failed);
}

int lk_check(const LkArgs& A, int B) {
  P2I_REQUIRE(A.pix && A.z && A.counts && A.params && A.stat, "null pointer");
  P2I_REQUIRE(A.model == 0 || A.model == 1, "variogram model must be 0 (exponential) or 1 (spherical)");
  P2I_REQUIRE(A.k >= 1 && A.k <= 64, "k must be 1..64 (got %d)", A.k);
  P2I_REQUIRE(B > 0 && B <= 65535 && A.T > 0 && A.T <= 65535, "bad sample shape %d x %d", B, A.T);
  P2I_REQUIRE(A.frames >= 0 && A.frames < A.T, "the temporal half-window must be 0..T - 1 (got %d)", A.frames);
  P2I_REQUIRE(A.fcap > 0 && A.fcap <= MAX_NP, "fcap must be 1..%d (got %d)", MAX_NP, A.fcap);
  return P2I_OK;
}

}  // namespace
}  // namespace p2i

using namespace p2i;

// velf [B][2] fp32 = (v_y, v_x) per sample runs the LAG = true kernels, NULL the LAG = false ones
extern "C" int p2i_lkrig_predict(const int* pix, const float* z, const int* counts, const float* params, const int* cand, int model, int k,
                                 int frames, int B, int T, int H, int W, int fcap, double* stat, float* out, float* var, int* status,
                                 int* nbr, const float* velf, void* stream) {
  const LkArgs A{pix, z, counts, params, cand, stat, velf, model, k, frames, T, fcap, HUGE_VAL};
  if (int rc = lk_check(A, B)) return rc;
  P2I_REQUIRE(out && status, "null pointer");
  P2I_REQUIRE(H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE, "bad frame shape");
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  P2I_LAUNCH(lkrig_stat_kernel, dim3(B), dim3(256), 0, s, z, counts, T, fcap, stat);
  const auto kernel = k <= 32 ? (velf ? lkrig_predict_kernel<32, true> : lkrig_predict_kernel<32, false>)
                              : (velf ? lkrig_predict_kernel<64, true> : lkrig_predict_kernel<64, false>);
  P2I_LAUNCH(kernel, dim3(ceil_div(HW, LK_TPB), T, B), dim3(64), 0, s, A, W, HW, out, var, status, nbr);
  return launch_status();
}

extern "C" int p2i_lkrig_loso(const int* pix, const float* z, const int* counts, const float* params, const int* cand, int model, int k,
                              int frames, int B, int T, int fcap, double* stat, float* pred, float* var, int* status, const float* velf,
                              void* stream) {
  const LkArgs A{pix, z, counts, params, cand, stat, velf, model, k, frames, T, fcap, HUGE_VAL};
  if (int rc = lk_check(A, B)) return rc;
  P2I_REQUIRE(pred && var && status, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  P2I_LAUNCH(lkrig_stat_kernel, dim3(B), dim3(256), 0, s, z, counts, T, fcap, stat);
  const auto kernel = k <= 32 ? (velf ? lkrig_loso_kernel<32, true> : lkrig_loso_kernel<32, false>)
                              : (velf ? lkrig_loso_kernel<64, true> : lkrig_loso_kernel<64, false>);
  P2I_LAUNCH(kernel, dim3(ceil_div(fcap, LK_TPB), T, B), dim3(64), 0, s, A, pred, var, status);
  return launch_status();
}
