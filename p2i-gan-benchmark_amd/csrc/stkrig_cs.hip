// Conditional simulation of space-time ordinary kriging (include/p2i_stcs.h): members whose noise is coherent
// in time.  A member of a sample is an unconditional Gaussian field U with the space-time covariance C(sqrt(dy^2 + dx^2 + kappa^2
// dt^2)), drawn by circulant embedding on the St x Sy x Sx = (e_t T) x (e H) x (e W) torus, plus the space-time kriging of the residual
// z - U at the sample's points:
//   lambda = Re DFT3(b), A = sqrt(lambda+ / (St Sy Sx)), Y = DFT3(A xi)[:T, :H, :W], U_2q = Re Y, U_2q+1 = Im Y
//   r = z - U(t_i, p_i), v = K^-1 r = W^T (W r), mu = u^T r / s, alpha = v - mu u, Z(t, p) = U(t, p) + mu + sum_i alpha_i c0((t, p), i)
// xi is krig_cs.h's (cell = (l Sy + j) Sx + k, one stream id per sample).  The transform runs corner-only and axis by axis: along k and
// along j per temporal frequency l by krig_cs.h's plane products on v_mfma_f32_32x32x2_f32, into a complex workspace P2
// [pair][re, im][St][H][W]; along l by a bandwidth kernel on the vector unit.  Number formats as in krig_cs.hip: fp64 spectrum, fp32
// amplitude, noise, transforms and predictor, fp64 conditioning sums on the fp32 W.  Every sum has a fixed order and there are no
// atomics.
#include "krig_cs.h"
#include "p2i_stcs.h"

namespace p2i {
namespace {

constexpr int STCS_MAX_ST = P2I_STCS_MAX_ST;   // temporal side of the torus: a row of cosines in LDS as fp64
constexpr int TG = 16;                         // frames whose accumulators a thread of stage 3 keeps (2 TG registers)
constexpr int CBS = 2;                         // 32-member tiles of alpha per workgroup of the predictor: M <= 64

// ---- spectrum, pass 1: row (l, j) of the base b[l][j][k] = C(sqrt(dj^2 + dk^2 + kappa^2 dl^2)) + nugget [dl = dj = dk = 0] of sample
// b, cosine-transformed along k.  tw = cos(2 pi m / St), m < St, then cos(2 pi m / Sy), m < Sy, then cos(2 pi m / Sx), m < Sx.
__global__ __launch_bounds__(256) void stcs_spec_rows_kernel(const float* __restrict__ params, const int* __restrict__ cand, int model,
                                                             int St, int Sy, int Sx, const double* __restrict__ tw,
                                                             double* __restrict__ tmp) {
  __shared__ double row[CS_MAX_S];
  __shared__ double cx[CS_MAX_S];
  const int b = blockIdx.z, l = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  if (cand != nullptr && cand[b] < 0) return;
  const double nug = (double)params[b * 4], psill = (double)params[b * 4 + 1], a = (double)params[b * 4 + 2], kap = (double)params[b * 4 + 3];
  const int dj = min(j, Sy - j), dl = min(l, St - l);
  const double t2 = kap * kap * (double)(dl * dl);
  for (int k = tid; k < Sx; k += 256) {
    const int dk = min(k, Sx - k);
    const int d2 = dj * dj + dk * dk;
    row[k] = psill * (1.0 - g_d(sqrt((double)d2 + t2) / a, model)) + ((d2 | dl) == 0 ? nug : 0.0);
    cx[k] = tw[St + Sy + k];
  }
  __syncthreads();
  for (int kp = tid; kp < Sx; kp += 256) {
    double acc = 0.0;
    int idx = 0;
    for (int k = 0; k < Sx; ++k) {
      acc = fma(row[k], cx[idx], acc);
      idx += kp;
      if (idx >= Sx) idx -= Sx;
    }
    tmp[(((size_t)b * St + l) * Sy + j) * Sx + kp] = acc;
  }
}

// ---- spectrum, pass 2: out[plane][j'][k'] = sum_j cos(2 pi j j' / Sy) in[plane][j][k'] of plane = b St + l, one thread per k'
__global__ __launch_bounds__(256) void stcs_spec_cols_kernel(const int* __restrict__ cand, int St, int Sy, int Sx,
                                                             const double* __restrict__ tw, const double* __restrict__ in,
                                                             double* __restrict__ out) {
  __shared__ double cy[CS_MAX_S];
  const int plane = blockIdx.z, jp = blockIdx.x, tid = threadIdx.x;
  if (cand != nullptr && cand[plane / St] < 0) return;
  for (int j = tid; j < Sy; j += 256) cy[j] = tw[St + j];
  __syncthreads();
  const int kp = blockIdx.y * 256 + tid;
  if (kp >= Sx) return;
  const double* t = in + (size_t)plane * Sy * Sx + kp;
  double acc = 0.0;
  int idx = 0;
  for (int j = 0; j < Sy; ++j) {
    acc = fma(cy[idx], t[(size_t)j * Sx], acc);
    idx += jp;
    if (idx >= Sy) idx -= Sy;
  }
  out[((size_t)plane * Sy + jp) * Sx + kp] = acc;
}

// ---- spectrum, pass 3: lam[b][l'][c] = sum_l cos(2 pi l l' / St) in[b][l][c] over the plane's cells c, one thread per cell
__global__ __launch_bounds__(256) void stcs_spec_time_kernel(const int* __restrict__ cand, int St, int cells, const double* __restrict__ tw,
                                                             const double* __restrict__ in, double* __restrict__ lam) {
  __shared__ double ct[STCS_MAX_ST];
  const int b = blockIdx.z, lp = blockIdx.y, tid = threadIdx.x;
  if (cand != nullptr && cand[b] < 0) return;
  for (int l = tid; l < St; l += 256) ct[l] = tw[l];
  __syncthreads();
  const int c = blockIdx.x * 256 + tid;
  if (c >= cells) return;
  const double* t = in + (size_t)b * St * cells + c;
  double acc = 0.0;
  int idx = 0;
  for (int l = 0; l < St; ++l) {
    acc = fma(ct[idx], t[(size_t)l * cells], acc);
    idx += lp;
    if (idx >= St) idx -= St;
  }
  lam[((size_t)b * St + lp) * cells + c] = acc;
}

// ---- fields, stage 1: plane l of unit (sample b, pair q) = u0 + blockIdx.x / St: P[unit][l] [2][Sy][W] = (A[b][l] xi[l]) F_Sx[:, :W]
__global__ __launch_bounds__(256) void stcs_fields1_kernel(const float* __restrict__ amp, const long long* __restrict__ streams,
                                                           const float* __restrict__ tx, unsigned seed_lo, unsigned seed_hi, int u0,
                                                           int npairs, int St, int Sy, int Sx, int W, float* __restrict__ P) {
  __shared__ float Gr[TS][A_LD];
  __shared__ float Gi[TS][A_LD];
  const int ul = blockIdx.x / St, l = blockIdx.x % St, unit = u0 + ul, b = unit / npairs, q = unit % npairs;
  const unsigned long long st = (unsigned long long)streams[b];
  const size_t plane = (size_t)Sy * Sx;
  cs_stage1_tile(Gr, Gi, amp + ((size_t)b * St + l) * plane, tx, seed_lo, seed_hi, (unsigned)l * (unsigned)plane, (unsigned)q, (unsigned)st,
                 (unsigned)(st >> 32), blockIdx.y * TS, blockIdx.z * PT + (threadIdx.x >> 6) * TS, Sy, Sx, W,
                 P + (size_t)blockIdx.x * 2 * Sy * W);
}

// ---- fields, stage 2: P2[unit] [2][St][H][W]: plane l = F_Sy[:H, :] P[unit][l]
__global__ __launch_bounds__(256) void stcs_fields2_kernel(const float* __restrict__ P, const float* __restrict__ ty, int St, int Sy, int H,
                                                           int W, float* __restrict__ P2) {
  const int ul = blockIdx.x / St, l = blockIdx.x % St;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int h0 = blockIdx.y * TS, w0 = blockIdx.z * PT + wave * TS;
  if (w0 >= W) return;
  f32x16 yr, yi;
  cs_stage2_tile(P + (size_t)blockIdx.x * 2 * Sy * W, ty, h0, w0, Sy, H, W, yr, yi);
  if (w0 + l31 < W) {
    const size_t HW = (size_t)H * W;
    float* o = P2 + ((size_t)ul * 2 * St + l) * HW + w0 + l31;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int h = h0 + acc_row(e, lhi);
      if (h < H) {
        o[(size_t)h * W] = yr[e];
        o[(size_t)St * HW + (size_t)h * W] = yi[e];
      }
    }
  }
}

// ---- fields, stage 3: Y[t] = sum_l (cos - i sin)(2 pi t l / St) P2[l] of the frames t0 .. t0 + TG - 1 of unit u0 + blockIdx.z, one
// pixel per thread, l in order, fmaf; tt [2][St][T] = cos, sin of 2 pi (t l mod St) / St (uniform across the workgroup).  Re is member
// 2q, Im member 2q + 1 (dropped when M is odd and it is the last) of ens [B][T][M][HW].
__global__ __launch_bounds__(256) void stcs_fields3_kernel(const float* __restrict__ P2, const float* __restrict__ tt, int u0, int npairs,
                                                           int M, int T, int St, int HW, float* __restrict__ ens) {
  const int ul = blockIdx.z, unit = u0 + ul, b = unit / npairs, q = unit % npairs, t0 = blockIdx.y * TG;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const float* re = P2 + (size_t)ul * 2 * St * HW + p;
  const float* im = re + (size_t)St * HW;
  float yr[TG], yi[TG];
#pragma unroll
  for (int g = 0; g < TG; ++g) yr[g] = yi[g] = 0.f;
  for (int l = 0; l < St; ++l) {
    const float vr = re[(size_t)l * HW], vi = im[(size_t)l * HW];
    const float* c = tt + (size_t)l * T;
    const float* s = c + (size_t)St * T;
#pragma unroll
    for (int g = 0; g < TG; ++g) {
      const int t = min(t0 + g, T - 1);             // frames past T are computed against a clamped address and not stored
      const float cs = c[t], sn = s[t];
      yr[g] = fmaf(vi, sn, fmaf(vr, cs, yr[g]));
      yi[g] = fmaf(-vr, sn, fmaf(vi, cs, yi[g]));
    }
  }
  const bool has_im = 2 * q + 1 < M;
#pragma unroll
  for (int g = 0; g < TG; ++g) {
    if (t0 + g < T) {
      float* o = ens + (((size_t)b * T + t0 + g) * M + 2 * q) * HW + p;
      o[0] = yr[g];
      if (has_im) o[HW] = yi[g];
    }
  }
}

// ---- conditional members of frame t = blockIdx.z of sample s on a tile of PT pixels: D = alpha c0 on the slab core of krig_mfma.h
// with A = alpha (m = member, up to CBS 32-row tiles), K = point, c0 from the space-time slab_fill.  The epilogue adds U (read from the
// buffer it writes) and mu; a point of this frame is written as its z; a sample without a model is written as NaN.  One frame per
// workgroup: keeping the staged alpha tiles for 2 or 4 frames of the same pixels measured 6 % and 21 % slower.
__global__ __launch_bounds__(256, 2) void stcs_predict_kernel(const float* __restrict__ alpha, const float* __restrict__ mu,
                                                              const int* __restrict__ pix, const int* __restrict__ stt,
                                                              const float* __restrict__ z, const int* __restrict__ counts,
                                                              const int* __restrict__ status, const int* __restrict__ cand,
                                                              const float* __restrict__ params, int model, int f0, int T, int M, int W,
                                                              int HW, int cap, int np, float* ens) {
  __shared__ float slab[TS][SLAB_LD];
  __shared__ float At[CBS][TS][A_LD];
  __shared__ int hit[PT];
  const int s = blockIdx.y, b = f0 + s, t = blockIdx.z;
  const int n = min(counts[b], np);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int p0 = blockIdx.x * PT;
  float* out = ens + ((size_t)b * T + t) * M * HW;
  if (n == 0 || no_model(status[s], cand, b)) {       // NaN
    if (tid < PT && p0 + tid < HW)
      for (int c = 0; c < M; ++c) out[(size_t)c * HW + p0 + tid] = __builtin_nanf("");
    return;
  }
  const float nug = params[b * 4], psill = params[b * 4 + 1], a = params[b * 4 + 2], kap = params[b * 4 + 3];
  const float k2 = kap * kap;
  const float* al = alpha + (size_t)s * M * cap;
  const float* ms = mu + (size_t)s * M;
  const int* gp = pix + (size_t)b * cap;
  const int* gt = stt + (size_t)b * cap;
  const int bp = tid & (PT - 1);
  const int p = min(p0 + bp, HW - 1);
  const int py = p / W, px = p % W;
  if (tid < PT) hit[tid] = -1;
  f32x16 acc[CBS];
#pragma unroll
  for (int r = 0; r < CBS; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[r][e] = 0.f;
  const int nt = (n + TS - 1) / TS;
  for (int sb = 0; sb < nt; ++sb) {
    __syncthreads();
    slab_fill(slab, gp, gt, n, sb, py, px, t, nug, psill, a, k2, model, [&](int i, float, bool at) {
      if (at) hit[bp] = i;                         // the points of one frame are distinct pixels: one writer per pixel
    });
#pragma unroll
    for (int r = 0; r < CBS; ++r)
      if (r * TS < M) tile_stage(At[r], al + (size_t)(r * TS) * cap + sb * TS, cap, M - r * TS);     // a tile past M is never read
    __syncthreads();
#pragma unroll
    for (int r = 0; r < CBS; ++r)
      if (r * TS < M) acc[r] = tile_mfma(At[r], slab, acc[r]);
  }
  const int pi = wave * 32 + l31;
  if (p0 + pi < HW) {
    const int h = hit[pi];
#pragma unroll
    for (int r = 0; r < CBS; ++r) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int col = r * TS + acc_row(e, lhi);
        if (col < M) {
          float* o = out + (size_t)col * HW + p0 + pi;
          *o = h >= 0 ? z[(size_t)b * cap + h] : (*o + ms[col]) + acc[r][e];
        }
      }
    }
  }
}

}  // namespace
}  // namespace p2i

using namespace p2i;

static inline int stcs_torus_check(int St, int Sy, int Sx) {
  P2I_REQUIRE(St > 0 && St <= STCS_MAX_ST, "embedding torus: %d temporal cells, must be in 1..%d", St, STCS_MAX_ST);
  P2I_REQUIRE(Sy > 0 && Sx > 0 && Sy <= CS_MAX_S && Sx <= CS_MAX_S, "embedding torus %d x %d: sides must be in 1..%d", Sy, Sx, CS_MAX_S);
  return P2I_OK;
}

static inline int stcs_frames_check(int M, int T, int H, int W) {
  P2I_REQUIRE(T > 0 && T <= STCS_MAX_ST, "frames per sample must be in 1..%d (got %d)", STCS_MAX_ST, T);
  return cs_members_check(M, H, W);
}

extern "C" int p2i_stcs_abi_version(void) { return 1; }

extern "C" int p2i_stcs_spectrum(const float* params, const int* cand, int model, int B, int St, int Sy, int Sx, const double* twiddle,
                                 double* work, float* amp, double* clip, void* stream) {
  P2I_REQUIRE(params && twiddle && work && amp && clip, "null pointer");
  if (int rc = krig_model_check(model)) return rc;
  if (int rc = stcs_torus_check(St, Sy, Sx)) return rc;
  P2I_REQUIRE(B > 0 && (long long)B * St <= 65535, "bad batch %d", B);
  hipStream_t s = (hipStream_t)stream;
  const int cells = Sy * Sx;
  double* w0 = work;
  double* w1 = work + (size_t)B * St * cells;
  P2I_LAUNCH(stcs_spec_rows_kernel, dim3(Sy, St, B), dim3(256), 0, s, params, cand, model, St, Sy, Sx, twiddle, w0);
  P2I_LAUNCH(stcs_spec_cols_kernel, dim3(Sy, ceil_div(Sx, 256), B * St), dim3(256), 0, s, cand, St, Sy, Sx, twiddle, (const double*)w0, w1);
  P2I_LAUNCH(stcs_spec_time_kernel, dim3(ceil_div(cells, 256), St, B), dim3(256), 0, s, cand, St, cells, twiddle, (const double*)w1, w0);
  P2I_LAUNCH(cs_spec_amp_kernel, dim3(B), dim3(256), 0, s, cand, St * Sy, Sx, (const double*)w0, amp, clip);
  return launch_status();
}

extern "C" int p2i_stcs_noise(uint64_t seed, int64_t stream_id, int q0, int npairs, int St, int Sy, int Sx, float* xi, void* stream) {
  P2I_REQUIRE(xi, "null pointer");
  if (int rc = stcs_torus_check(St, Sy, Sx)) return rc;
  P2I_REQUIRE(q0 >= 0 && npairs > 0 && npairs <= 65535, "bad member pairs %d + %d", q0, npairs);
  const uint64_t st = (uint64_t)stream_id;
  const int n = St * Sy * Sx;
  P2I_LAUNCH(cs_noise_kernel, dim3(ceil_div(n, 256), npairs), dim3(256), 0, (hipStream_t)stream, (unsigned)seed, (unsigned)(seed >> 32),
             (unsigned)st, (unsigned)(st >> 32), q0, n, xi);
  return launch_status();
}

extern "C" int p2i_stcs_fields(const float* amp, const int64_t* streams, const float* tx, const float* ty, const float* tt, uint64_t seed,
                               int u0, int nunits, int M, int T, int H, int W, int St, int Sy, int Sx, int stages, float* P, float* P2,
                               float* ens, void* stream) {
  P2I_REQUIRE(amp && streams && tx && ty && tt && P && P2 && ens, "null pointer");
  if (int rc = stcs_torus_check(St, Sy, Sx)) return rc;
  P2I_REQUIRE(M >= 1 && M <= CS_MAX_M, "members must be in 1..%d (got %d)", CS_MAX_M, M);
  P2I_REQUIRE(T > 0 && H > 0 && W > 0 && T <= St && H <= Sy && W <= Sx, "sample %d x %d x %d does not fit the torus %d x %d x %d", T, H, W, St,
              Sy, Sx);
  P2I_REQUIRE(u0 >= 0 && nunits > 0 && nunits <= 65535, "bad unit range %d + %d", u0, nunits);
  P2I_REQUIRE(stages >= 1 && stages <= P2I_STCS_STAGES_ALL, "stages must be a non-empty subset of %d (got %d)", P2I_STCS_STAGES_ALL, stages);
  hipStream_t s = (hipStream_t)stream;
  const int npairs = (M + 1) / 2;
  if (stages & 1)
    P2I_LAUNCH(stcs_fields1_kernel, dim3(nunits * St, ceil_div(Sy, TS), ceil_div(W, PT)), dim3(256), 0, s, amp, (const long long*)streams, tx,
             (unsigned)seed, (unsigned)(seed >> 32), u0, npairs, St, Sy, Sx, W, P);
  if (stages & 2)
    P2I_LAUNCH(stcs_fields2_kernel, dim3(nunits * St, ceil_div(H, TS), ceil_div(W, PT)), dim3(256), 0, s, (const float*)P, ty, St, Sy, H, W, P2);
  if (stages & 4)
    P2I_LAUNCH(stcs_fields3_kernel, dim3(ceil_div(H * W, 256), ceil_div(T, TG), nunits), dim3(256), 0, s, (const float*)P2, tt, u0, npairs, M, T,
             St, H * W, ens);
  return launch_status();
}

static inline int stcs_sys_check(const p2i_krig_systems* k, unsigned reads, bool own) {
  if (int rc = krig_sys_check(k, reads, own)) return rc;
  P2I_REQUIRE(k->R == 1 && k->T == 1, "a space-time system is one sample: R = T = 1");
  return P2I_OK;
}

extern "C" int p2i_stcs_weights(const p2i_krig_systems* k, const int* stt, const float* Winv, const double* sol, const float* ens, int M,
                                int T, int H, int W, float* alpha, float* mu, void* stream) {
  if (int rc = stcs_sys_check(k, KS_PIX | KS_Z | KS_COUNTS | KS_STATUS | KS_NP, stt && Winv && sol && ens && alpha && mu)) return rc;
  if (int rc = stcs_frames_check(M, T, H, W)) return rc;
  const int np = k->np;
  const int nc = np <= 1024 ? 4 : 2;                            // r and y, 2 nc np fp64: 128 KiB at np = 4096
  const size_t lds = (size_t)2 * nc * np * sizeof(double);
  static bool raised = false;
  if (!raised) {
    (void)hipFuncSetAttribute((const void*)cs_weights_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    raised = true;
  }
  P2I_LAUNCH(cs_weights_kernel<true>, dim3(ceil_div(M, nc), k->nsys), dim3(256), lds, (hipStream_t)stream, Winv, sol, k->pix, stt, k->z,
             k->counts, (const int*)k->status, k->cand, ens, k->f0, 1, 1, T, M, W, H * W, k->cap, np, nc, alpha, mu);
  return launch_status();
}

extern "C" int p2i_stcs_predict(const p2i_krig_systems* k, const int* stt, const float* alpha, const float* mu, int M, int T, int H, int W,
                                float* ens, void* stream) {
  if (int rc = stcs_sys_check(k, KS_PIX | KS_Z | KS_COUNTS | KS_STATUS | KS_PARAMS | KS_MODEL | KS_NP, stt && alpha && mu && ens)) return rc;
  if (int rc = stcs_frames_check(M, T, H, W)) return rc;
  const int HW = H * W;
  P2I_LAUNCH(stcs_predict_kernel, dim3(ceil_div(HW, PT), k->nsys, T), dim3(256), 0, (hipStream_t)stream, alpha, mu, k->pix, stt, k->z,
             k->counts, (const int*)k->status, k->cand, k->params, k->model, k->f0, T, M, W, HW, k->cap, k->np, ens);
  return launch_status();
}
