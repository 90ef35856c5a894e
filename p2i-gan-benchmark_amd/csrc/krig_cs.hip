// Conditional simulation of ordinary kriging: ensemble members that carry the variogram's texture and honour
// every gauge.  A member is an unconditional Gaussian field U with the covariance of the model, drawn by circulant embedding on the
// (e H) x (e W) torus, plus the kriging of the residual z - U(gauges):
//   lambda = Re DFT2(b), A = sqrt(lambda+ / (Sy Sx)), Y = DFT2(A xi), U_2q = Re Y[:H, :W], U_2q+1 = Im Y[:H, :W]
//   r = z - U(x), v = K^-1 r = W^T (W r), mu = u^T r / s, alpha = v - mu u, Z(p) = U(p) + mu + sum_i alpha_i c0(p, i)
// xi is counter-based (Philox4x32-10, Box-Muller): a member is a function of (seed, stream, member, variogram, gauges) only.
// Number formats: the spectrum is fp64; the noise, both DFT products and the predictor run in fp32 on v_mfma_f32_32x32x2_f32 (a k-ordered
// fmaf chain per output); W is fp32 and the conditioning sums (W r, W^T y, u^T r) are fp64.  Every sum has a fixed order and there are
// no atomics: results are identical from run to run.
#include "krig_cs.h"

namespace p2i {
namespace {

constexpr int CB = 4;             // 32-column tiles of alpha per workgroup of the predictor (section 16's row-block balance)

// ---- spectrum, pass 1: row j of the base b[j][k] = C(sqrt(dj^2 + dk^2)) + nugget [dj = dk = 0] of sample b, cosine-transformed
// along k: tmp[b][j][k'] = sum_k b[j][k] cos(2 pi k k' / Sx).  tw = cos(2 pi m / Sy), m < Sy, then cos(2 pi m / Sx), m < Sx.
__global__ __launch_bounds__(256) void cs_spec_rows_kernel(const float* __restrict__ params, const int* __restrict__ cand, int model, int Sy,
                                                           int Sx, const double* __restrict__ tw, double* __restrict__ tmp) {
  __shared__ double row[CS_MAX_S];
  __shared__ double cx[CS_MAX_S];
  const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  if (cand != nullptr && cand[b] < 0) return;
  const double nug = (double)params[b * 4], psill = (double)params[b * 4 + 1], a = (double)params[b * 4 + 2];
  const int dj = min(j, Sy - j);
  for (int k = tid; k < Sx; k += 256) {
    const int dk = min(k, Sx - k);
    const int d2 = dj * dj + dk * dk;
    row[k] = psill * (1.0 - g_d(sqrt((double)d2) / a, model)) + (d2 == 0 ? nug : 0.0);
    cx[k] = tw[Sy + k];
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
    tmp[((size_t)b * Sy + j) * Sx + kp] = acc;
  }
}

// ---- spectrum, pass 2: lam[b][j'][k'] = sum_j cos(2 pi j j' / Sy) tmp[b][j][k'], one thread per k'
__global__ __launch_bounds__(256) void cs_spec_cols_kernel(const int* __restrict__ cand, int Sy, int Sx, const double* __restrict__ tw,
                                                           const double* __restrict__ tmp, double* __restrict__ lam) {
  __shared__ double cy[CS_MAX_S];
  const int b = blockIdx.z, jp = blockIdx.x, tid = threadIdx.x;
  if (cand != nullptr && cand[b] < 0) return;
  for (int j = tid; j < Sy; j += 256) cy[j] = tw[j];
  __syncthreads();
  const int kp = blockIdx.y * 256 + tid;
  if (kp >= Sx) return;
  const double* t = tmp + (size_t)b * Sy * Sx + kp;
  double acc = 0.0;
  int idx = 0;
  for (int j = 0; j < Sy; ++j) {
    acc = fma(cy[idx], t[(size_t)j * Sx], acc);
    idx += jp;
    if (idx >= Sy) idx -= Sy;
  }
  lam[((size_t)b * Sy + jp) * Sx + kp] = acc;
}

// ---- fields, stage 1: P = (A xi) F_Sx[:, :W] of member pair q of frame f0 + fl, on a tile of 32 torus rows x 128 columns (one
// 32-column MFMA tile per wave): krig_cs.h's plane product on the frame's torus.
__global__ __launch_bounds__(256) void cs_fields1_kernel(const float* __restrict__ amp, const long long* __restrict__ streams,
                                                         const float* __restrict__ tx, unsigned seed_lo, unsigned seed_hi, int f0, int T,
                                                         int npairs, int Sy, int Sx, int W, float* __restrict__ P) {
  __shared__ float Gr[TS][A_LD];
  __shared__ float Gi[TS][A_LD];
  const int fp = blockIdx.x, fl = fp / npairs, q = fp % npairs, f = f0 + fl, b = f / T;
  const unsigned long long st = (unsigned long long)streams[f];
  cs_stage1_tile(Gr, Gi, amp + (size_t)b * Sy * Sx, tx, seed_lo, seed_hi, 0u, (unsigned)q, (unsigned)st, (unsigned)(st >> 32),
                 blockIdx.y * TS, blockIdx.z * PT + (threadIdx.x >> 6) * TS, Sy, Sx, W, P + (size_t)fp * 2 * Sy * W);
}

// ---- fields, stage 2: Y = F_Sy[:H, :] P on a tile of 32 rows x 128 columns of the frame (krig_cs.h's plane product).  Y_re is
// member 2q, Y_im member 2q + 1 (dropped when M is odd and it is the last).
__global__ __launch_bounds__(256) void cs_fields2_kernel(const float* __restrict__ P, const float* __restrict__ ty, int f0, int npairs, int M,
                                                         int Sy, int H, int W, float* __restrict__ ens) {
  const int fp = blockIdx.x, fl = fp / npairs, q = fp % npairs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int h0 = blockIdx.y * TS, w0 = blockIdx.z * PT + wave * TS;
  if (w0 >= W) return;
  f32x16 yr, yi;
  cs_stage2_tile(P + (size_t)fp * 2 * Sy * W, ty, h0, w0, Sy, H, W, yr, yi);
  if (w0 + l31 < W) {
    const size_t HW = (size_t)H * W;
    float* o = ens + ((size_t)(f0 + fl) * M + 2 * q) * HW + w0 + l31;
    const bool odd = 2 * q + 1 < M;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int h = h0 + acc_row(e, lhi);
      if (h < H) {
        o[(size_t)h * W] = yr[e];
        if (odd) o[HW + (size_t)h * W] = yi[e];
      }
    }
  }
}

// ---- conditional members of system s on a tile of PT pixels: D = alpha c0 on the slab core of krig_mfma.h with A = alpha (m = column:
// frame t = col / M, member col % M of the system), K = gauge; a wave holds CB column tiles, blockIdx.z walks the column groups.  Per
// 32-gauge slab the c0 slab is filled next to the group's alpha tiles (zeros past the columns); c0 is evaluated once per (pixel,
// gauge) for up to 32 CB outputs.  The epilogue adds U (read from the buffer it writes) and mu; a gauge pixel is written as the
// frame's z there; a system without a model is written as NaN.
__global__ __launch_bounds__(256, 2) void cs_predict_kernel(const float* __restrict__ alpha, const float* __restrict__ mu,
                                                            const int* __restrict__ pix, const float* __restrict__ z,
                                                            const int* __restrict__ counts, const int* __restrict__ status,
                                                            const int* __restrict__ cand, const float* __restrict__ params, int model,
                                                            int f0, int R, int T, int M, int W, int HW, int cap, int np, float* ens) {
  __shared__ float slab[TS][SLAB_LD];
  __shared__ float At[CB][TS][A_LD];
  __shared__ int hit[PT];
  const int s = blockIdx.y, fs = f0 + s * R, b = fs / T, ncols = R * M, cg = blockIdx.z * CB * TS;
  const int n = min(counts[fs], np);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int p0 = blockIdx.x * PT;
  float* out = ens + (size_t)fs * M * HW;
  if (n == 0 || no_model(status[s], cand, b)) {       // NaN
    if (tid < PT && p0 + tid < HW)
      for (int c = cg; c < min(cg + CB * TS, ncols); ++c) out[(size_t)c * HW + p0 + tid] = __builtin_nanf("");
    return;
  }
  const float nug = params[b * 4], psill = params[b * 4 + 1], a = params[b * 4 + 2];
  const float* al = alpha + (size_t)s * ncols * cap;
  const float* ms = mu + (size_t)s * ncols;
  const int* gp = pix + (size_t)fs * cap;
  const int bp = tid & (PT - 1);
  const int p = min(p0 + bp, HW - 1);
  const int py = p / W, px = p % W;
  if (tid < PT) hit[tid] = -1;
  f32x16 acc[CB];
#pragma unroll
  for (int r = 0; r < CB; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[r][e] = 0.f;
  const int nt = (n + TS - 1) / TS;
  for (int sb = 0; sb < nt; ++sb) {
    __syncthreads();
    slab_fill(slab, gp, n, sb, py, px, nug, psill, a, model, [&](int i, float, bool at) {
      if (at) hit[bp] = i;                         // gauge pixels are distinct: one writer per pixel
    });
#pragma unroll
    for (int r = 0; r < CB; ++r) tile_stage(At[r], al + (size_t)(cg + r * TS) * cap + sb * TS, cap, ncols - (cg + r * TS));
    __syncthreads();
#pragma unroll
    for (int r = 0; r < CB; ++r)
      if (cg + r * TS < ncols) acc[r] = tile_mfma(At[r], slab, acc[r]);
  }
  const int pi = wave * 32 + l31;
  if (p0 + pi < HW) {
    const int h = hit[pi];
#pragma unroll
    for (int r = 0; r < CB; ++r) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int col = cg + r * TS + acc_row(e, lhi);
        if (col < ncols) {
          float* o = out + (size_t)col * HW + p0 + pi;
          *o = h >= 0 ? z[(size_t)(fs + col / M) * cap + h] : (*o + ms[col]) + acc[r][e];
        }
      }
    }
  }
}

}  // namespace
}  // namespace p2i

using namespace p2i;

static inline int cs_torus_check(int Sy, int Sx) {
  P2I_REQUIRE(Sy > 0 && Sx > 0 && Sy <= CS_MAX_S && Sx <= CS_MAX_S, "embedding torus %d x %d: sides must be in 1..%d", Sy, Sx, CS_MAX_S);
  return P2I_OK;
}

extern "C" int p2i_krig_cs_spectrum(const float* params, const int* cand, int model, int B, int Sy, int Sx, const double* twiddle,
                                    double* work, float* amp, double* clip, void* stream) {
  P2I_REQUIRE(params && twiddle && work && amp && clip, "null pointer");
  if (int rc = krig_model_check(model)) return rc;
  if (int rc = cs_torus_check(Sy, Sx)) return rc;
  P2I_REQUIRE(B > 0 && B <= 65535, "bad batch %d", B);
  hipStream_t s = (hipStream_t)stream;
  double* tmp = work;
  double* lam = work + (size_t)B * Sy * Sx;
  P2I_LAUNCH(cs_spec_rows_kernel, dim3(Sy, B), dim3(256), 0, s, params, cand, model, Sy, Sx, twiddle, tmp);
  P2I_LAUNCH(cs_spec_cols_kernel, dim3(Sy, ceil_div(Sx, 256), B), dim3(256), 0, s, cand, Sy, Sx, twiddle, (const double*)tmp, lam);
  P2I_LAUNCH(cs_spec_amp_kernel, dim3(B), dim3(256), 0, s, cand, Sy, Sx, (const double*)lam, amp, clip);
  return launch_status();
}

extern "C" int p2i_krig_cs_noise(uint64_t seed, int64_t stream_id, int q0, int npairs, int Sy, int Sx, float* xi, void* stream) {
  P2I_REQUIRE(xi, "null pointer");
  if (int rc = cs_torus_check(Sy, Sx)) return rc;
  P2I_REQUIRE(q0 >= 0 && npairs > 0 && npairs <= 65535, "bad member pairs %d + %d", q0, npairs);
  const uint64_t st = (uint64_t)stream_id;
  P2I_LAUNCH(cs_noise_kernel, dim3(ceil_div(Sy * Sx, 256), npairs), dim3(256), 0, (hipStream_t)stream, (unsigned)seed, (unsigned)(seed >> 32),
             (unsigned)st, (unsigned)(st >> 32), q0, Sy * Sx, xi);
  return launch_status();
}

extern "C" int p2i_krig_cs_fields(const float* amp, const int64_t* streams, const float* tx, const float* ty, uint64_t seed, int f0,
                                  int nframes, int T, int M, int H, int W, int Sy, int Sx, float* P, float* ens, void* stream) {
  P2I_REQUIRE(amp && streams && tx && ty && P && ens, "null pointer");
  if (int rc = cs_torus_check(Sy, Sx)) return rc;
  P2I_REQUIRE(H > 0 && W > 0 && H <= Sy && W <= Sx, "frame %d x %d does not fit the torus %d x %d", H, W, Sy, Sx);
  P2I_REQUIRE(M >= 1 && M <= CS_MAX_M, "members must be in 1..%d (got %d)", CS_MAX_M, M);
  P2I_REQUIRE(f0 >= 0 && nframes > 0 && T > 0 && nframes <= 65535, "bad frame range %d + %d", f0, nframes);
  hipStream_t s = (hipStream_t)stream;
  const int npairs = (M + 1) / 2;
  P2I_LAUNCH(cs_fields1_kernel, dim3(nframes * npairs, ceil_div(Sy, TS), ceil_div(W, PT)), dim3(256), 0, s, amp, (const long long*)streams,
             tx, (unsigned)seed, (unsigned)(seed >> 32), f0, T, npairs, Sy, Sx, W, P);
  P2I_LAUNCH(cs_fields2_kernel, dim3(nframes * npairs, ceil_div(H, TS), ceil_div(W, PT)), dim3(256), 0, s, (const float*)P, ty, f0, npairs,
             M, Sy, H, W, ens);
  return launch_status();
}

extern "C" int p2i_krig_cs_weights(const p2i_krig_systems* k, const float* Winv, const double* sol, const float* ens, int M, int H, int W,
                                   float* alpha, float* mu, void* stream) {
  if (int rc = krig_sys_check(k, KS_PIX | KS_Z | KS_COUNTS | KS_STATUS | KS_NP, Winv && sol && ens && alpha && mu)) return rc;
  if (int rc = cs_members_check(M, H, W)) return rc;
  const int np = k->np;
  const int nc = np <= 1024 ? 4 : (np <= 2048 ? 2 : 1);
  const size_t lds = (size_t)2 * nc * np * sizeof(double);      // at most 64 KiB
  static bool raised = false;
  if (!raised) {
    (void)hipFuncSetAttribute((const void*)cs_weights_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    raised = true;
  }
  P2I_LAUNCH(cs_weights_kernel<false>, dim3(ceil_div(k->R * M, nc), k->nsys), dim3(256), lds, (hipStream_t)stream, Winv, sol, k->pix,
             (const int*)nullptr, k->z, k->counts, (const int*)k->status, k->cand, ens, k->f0, k->R, k->T, 1, M, W, H * W, k->cap, np, nc,
             alpha, mu);
  return launch_status();
}

extern "C" int p2i_krig_cs_predict(const p2i_krig_systems* k, const float* alpha, const float* mu, int M, int H, int W, float* ens,
                                   void* stream) {
  if (int rc = krig_sys_check(k, KS_PIX | KS_Z | KS_COUNTS | KS_STATUS | KS_PARAMS | KS_MODEL | KS_NP, alpha && mu && ens)) return rc;
  if (int rc = cs_members_check(M, H, W)) return rc;
  const int HW = H * W;
  P2I_LAUNCH(cs_predict_kernel, dim3(ceil_div(HW, PT), k->nsys, ceil_div(k->R * M, CB * TS)), dim3(256), 0, (hipStream_t)stream, alpha, mu,
             k->pix, k->z, k->counts, (const int*)k->status, k->cand, k->params, k->model, k->f0, k->R, k->T, M, W, HW, k->cap, k->np, ens);
  return launch_status();
}
