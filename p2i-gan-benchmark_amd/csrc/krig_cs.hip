// Conditional simulation of ordinary kriging: ensemble members that carry the variogram's texture and honour
// every gauge.  A member is an unconditional Gaussian field U with the covariance of the model, drawn by circulant embedding on the
// (e H) x (e W) torus, plus the kriging of the residual z - U(gauges):
//   lambda = Re DFT2(b), A = sqrt(lambda+ / (Sy Sx)), Y = DFT2(A xi), U_2q = Re Y[:H, :W], U_2q+1 = Im Y[:H, :W]
//   r = z - U(x), v = K^-1 r = W^T (W r), mu = u^T r / s, alpha = v - mu u, Z(p) = U(p) + mu + sum_i alpha_i c0(p, i)
// xi is counter-based (Philox4x32-10, Box-Muller): a member is a function of (seed, stream, member, variogram, gauges) only.
// Number formats: the spectrum is fp64; the noise, both DFT products and the predictor run in fp32 on v_mfma_f32_32x32x2_f32 (a k-ordered
// fmaf chain per output); W is fp32 and the conditioning sums (W r, W^T y, u^T r) are fp64.  Every sum has a fixed order and there are
// no atomics: results are identical from run to run.
#include "krig_mfma.h"

namespace p2i {
namespace {

constexpr int CS_MAX_S = 512;      // side of the embedding torus: a row of it in LDS as fp64
constexpr int CS_MAX_M = 64;       // members per frame
constexpr int WU = 8;              // loads of W a thread of the weights kernel keeps in flight
constexpr int CB = 4;             // 32-column tiles of alpha per workgroup of the predictor (section 16's row-block balance)

// ---- Philox4x32-10 (Salmon et al. 2011): the first two output words of counter (c0, c1, c2, c3) under key (k0, k1)
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned& r0,
                                              unsigned& r1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r0 = c0;
  r1 = c1;
}

// the complex standard normal xi of torus cell idx = j Sx + k, member pair q, frame id `stream`: Box-Muller on (r0, r1), the
// logarithm through log1p in the upper half of r0 where u1 -> 1
__device__ __forceinline__ float2 cs_xi(unsigned seed_lo, unsigned seed_hi, unsigned idx, unsigned q, unsigned st_lo, unsigned st_hi) {
  unsigned r0, r1;
  philox4x32_10(idx, q, st_lo, st_hi, seed_lo, seed_hi, r0, r1);
  const float sc = 2.3283064365386963e-10f;      // 2^-32
  const float l = r0 < 0x80000000u ? logf((float)(r0 + 1u) * sc) : log1pf(-((float)(0xFFFFFFFFu - r0) * sc));
  const float rad = sqrtf(-2.f * l);
  float sn, cs;
  sincospif(2.f * ((float)r1 * sc), &sn, &cs);
  return make_float2(rad * cs, rad * sn);
}

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

// ---- spectrum, pass 3: the clip share rho = sum max(-lam, 0) / sum |lam| and the amplitude A = sqrt(lam+ / (Sy Sx)) with
// lam+ = max(lam, 0) sum lam / sum max(lam, 0).  A degenerate fitted sample gets A = 0 and rho = NaN.
__global__ __launch_bounds__(256) void cs_spec_amp_kernel(const int* __restrict__ cand, int Sy, int Sx, const double* __restrict__ lam,
                                                          float* __restrict__ amp, double* __restrict__ clip) {
  __shared__ double red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = Sy * Sx;
  const double* l = lam + (size_t)b * n;
  float* o = amp + (size_t)b * n;
  if (cand != nullptr && cand[b] < 0) {
    for (int i = tid; i < n; i += 256) o[i] = 0.f;
    if (tid == 0) clip[b] = __builtin_nan("");
    return;
  }
  double pos = 0.0, neg = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double v = l[i];
    pos += fmax(v, 0.0);
    neg += fmax(-v, 0.0);
  }
  pos = block_sum_d(pos, red);
  neg = block_sum_d(neg, red);
  const double scale = (pos - neg) / pos / (double)n;
  for (int i = tid; i < n; i += 256) o[i] = (float)sqrt(fmax(l[i], 0.0) * scale);
  if (tid == 0) clip[b] = neg / (pos + neg);
}

// ---- the noise of the definition on its own: xi [npairs][Sy][Sx][2]
__global__ __launch_bounds__(256) void cs_noise_kernel(unsigned seed_lo, unsigned seed_hi, unsigned st_lo, unsigned st_hi, int q0, int n,
                                                       float* __restrict__ xi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float2 v = cs_xi(seed_lo, seed_hi, (unsigned)i, (unsigned)(q0 + blockIdx.y), st_lo, st_hi);
  reinterpret_cast<float2*>(xi)[(size_t)blockIdx.y * n + i] = v;
}

// ---- fields, stage 1: P = (A xi) F_Sx[:, :W] of member pair q of frame f0 + fl, on a tile of 32 torus rows x 128 columns (one
// 32-column MFMA tile per wave).  Per 32-wide slab of the k axis all threads draw G = A xi [32][32] into LDS (4 cells each; G never
// touches HBM) and the waves multiply it with the twiddles tx [2][Sx][W] (cos, sin of 2 pi k w / Sx) read as the B operand:
// P_re = G_re cos + G_im sin, P_im = G_im cos - G_re sin.  Rows and k past the torus are zeros; columns past W are not stored.
__global__ __launch_bounds__(256) void cs_fields1_kernel(const float* __restrict__ amp, const long long* __restrict__ streams,
                                                         const float* __restrict__ tx, unsigned seed_lo, unsigned seed_hi, int f0, int T,
                                                         int npairs, int Sy, int Sx, int W, float* __restrict__ P) {
  __shared__ float Gr[TS][A_LD];
  __shared__ float Gi[TS][A_LD];
  const int fp = blockIdx.x, fl = fp / npairs, q = fp % npairs, f = f0 + fl, b = f / T;
  const unsigned long long st = (unsigned long long)streams[f];
  const unsigned st_lo = (unsigned)st, st_hi = (unsigned)(st >> 32);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int j0 = blockIdx.y * TS, w0 = blockIdx.z * PT + wave * TS;
  const int wc = min(w0 + l31, W - 1);
  const float* ab = amp + (size_t)b * Sy * Sx;
  f32x16 pr, pi;
#pragma unroll
  for (int e = 0; e < 16; ++e) pr[e] = pi[e] = 0.f;
  for (int k0 = 0; k0 < Sx; k0 += TS) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = (tid >> 5) + 8 * e, c = tid & 31;
      const int j = j0 + r, k = k0 + c;
      float gr = 0.f, gi = 0.f;
      if (j < Sy && k < Sx) {
        const float2 xi = cs_xi(seed_lo, seed_hi, (unsigned)(j * Sx + k), (unsigned)q, st_lo, st_hi);
        const float a = ab[(size_t)j * Sx + k];
        gr = a * xi.x;
        gi = a * xi.y;
      }
      Gr[r][c] = gr;
      Gi[r][c] = gi;
    }
    __syncthreads();
    if (w0 < W) {
#pragma unroll 4
      for (int kk = 0; kk < TS / 2; ++kk) {
        const int kc = min(k0 + 2 * kk + lhi, Sx - 1);       // past the torus G is 0
        const float cs = tx[(size_t)kc * W + wc], sn = tx[(size_t)(Sx + kc) * W + wc];
        const float ar = Gr[l31][2 * kk + lhi], ai = Gi[l31][2 * kk + lhi];
        pr = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, cs, pr, 0, 0, 0);
        pr = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, sn, pr, 0, 0, 0);
        pi = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, cs, pi, 0, 0, 0);
        pi = __builtin_amdgcn_mfma_f32_32x32x2f32(-ar, sn, pi, 0, 0, 0);
      }
    }
  }
  if (w0 + l31 < W) {
    float* o = P + (size_t)fp * 2 * Sy * W + w0 + l31;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = j0 + acc_row(e, lhi);
      if (j < Sy) {
        o[(size_t)j * W] = pr[e];
        o[(size_t)(Sy + j) * W] = pi[e];
      }
    }
  }
}

// ---- fields, stage 2: Y = F_Sy[:H, :] P on a tile of 32 rows x 128 columns of the frame; both operands come straight from memory
// (ty [2][Sy][H]: cos, sin of 2 pi j h / Sy, as the A operand; P as the B operand).  Y_re = cos P_re + sin P_im is member 2q,
// Y_im = cos P_im - sin P_re member 2q + 1 (dropped when M is odd and it is the last).
__global__ __launch_bounds__(256) void cs_fields2_kernel(const float* __restrict__ P, const float* __restrict__ ty, int f0, int npairs, int M,
                                                         int Sy, int H, int W, float* __restrict__ ens) {
  const int fp = blockIdx.x, fl = fp / npairs, q = fp % npairs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  const int h0 = blockIdx.y * TS, w0 = blockIdx.z * PT + wave * TS;
  if (w0 >= W) return;
  const int hc = min(h0 + l31, H - 1), wc = min(w0 + l31, W - 1);
  const float* Pr = P + (size_t)fp * 2 * Sy * W + wc;
  const float* Pi = Pr + (size_t)Sy * W;
  f32x16 yr, yi;
#pragma unroll
  for (int e = 0; e < 16; ++e) yr[e] = yi[e] = 0.f;
  for (int jb = 0; jb < Sy; jb += 2) {
    const int j = jb + lhi, jc = min(j, Sy - 1);
    const float ac = j < Sy ? ty[(size_t)jc * H + hc] : 0.f;
    const float as = j < Sy ? ty[(size_t)(Sy + jc) * H + hc] : 0.f;
    const float br = Pr[(size_t)jc * W], bi = Pi[(size_t)jc * W];
    yr = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, br, yr, 0, 0, 0);
    yr = __builtin_amdgcn_mfma_f32_32x32x2f32(as, bi, yr, 0, 0, 0);
    yi = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, bi, yi, 0, 0, 0);
    yi = __builtin_amdgcn_mfma_f32_32x32x2f32(-as, br, yi, 0, 0, 0);
  }
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

// ---- conditioning weights of nc columns (frame t = col / M, member col % M) of system s: r = z - U(gauges), y = W r (a wave per row,
// lanes along the row, a fixed shuffle tree), v = W^T y (a thread per column of W, rows in order; W holds explicit zeros above its
// diagonal), mu = u^T r / s, alpha = v - mu u; all fp64 on the fp32 W.  LDS: r and y, [nc][np] fp64 each.  A system without a model
// gets alpha = 0 and mu = 0 (the predictor writes NaN there).
__global__ __launch_bounds__(256) void cs_weights_kernel(const float* __restrict__ Wi, const double* __restrict__ sol,
                                                         const int* __restrict__ pix, const float* __restrict__ z,
                                                         const int* __restrict__ counts, const int* __restrict__ status,
                                                         const int* __restrict__ cand, const float* __restrict__ ens, int f0, int R, int T,
                                                         int M, int W, int HW, int cap, int np, int nc, float* __restrict__ alpha,
                                                         float* __restrict__ mu) {
  extern __shared__ double sm[];
  __shared__ double red[256];
  constexpr int NC = 4;
  double* rr = sm;
  double* yy = sm + (size_t)nc * np;
  const int s = blockIdx.y, fs = f0 + s * R, ncols = R * M, c0 = blockIdx.x * nc;
  const int n = min(counts[fs], np);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* al = alpha + (size_t)s * ncols * cap;
  float* ms = mu + (size_t)s * ncols;
  if (n == 0 || no_model(status[s], cand, fs / T)) {
    for (int c = 0; c < nc && c0 + c < ncols; ++c) {
      for (int i = tid; i < cap; i += 256) al[(size_t)(c0 + c) * cap + i] = 0.f;
      if (tid == 0) ms[c0 + c] = 0.f;
    }
    return;
  }
  const double* u = sol + (size_t)s * (R + 1) * np;
  const float* Ws = Wi + (size_t)s * np * np;
  const int* gp = pix + (size_t)fs * cap;
  const double su = sum_u(u, n, red);
  double muc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    muc[c] = 0.0;
    if (c < nc) {
      const bool valid = c0 + c < ncols;
      const int col = min(c0 + c, ncols - 1);
      const float* zf = z + (size_t)(fs + col / M) * cap;
      const float* uf = ens + ((size_t)fs * M + col) * HW;
      double ur = 0.0;
      for (int i = tid; i < n; i += 256) {
        const int g = gp[i];
        const double r = valid ? (double)zf[i] - (double)uf[(g >> 16) * W + (g & 0xffff)] : 0.0;
        rr[(size_t)c * np + i] = r;
        ur = fma(u[i], r, ur);
      }
      muc[c] = block_sum_d(ur, red) / su;
    }
  }
  __syncthreads();
  for (int i = wave; i < n; i += 4) {                       // y = W r
    double acc[NC] = {0.0, 0.0, 0.0, 0.0};
    const float* wr = Ws + (size_t)i * np;
    for (int k0 = lane; k0 <= i; k0 += 64 * WU) {          // WU loads in flight, then their products in the row's order
      float a[WU];
#pragma unroll
      for (int q = 0; q < WU; ++q) a[q] = k0 + 64 * q <= i ? wr[k0 + 64 * q] : 0.f;
#pragma unroll
      for (int q = 0; q < WU; ++q) {
        const int k = k0 + 64 * q;
        if (k <= i) {
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (c < nc) acc[c] = fma((double)a[q], rr[(size_t)c * np + k], acc[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < nc) {
        double v = acc[c];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) yy[(size_t)c * np + i] = v;
      }
    }
  }
  __syncthreads();
  for (int kb = 0; kb < cap; kb += 256) {                   // v = W^T y, alpha = v - mu u; zeros past the count
    const int k = kb + tid;
    double acc[NC] = {0.0, 0.0, 0.0, 0.0};
    if (k < n) {
      const float* wc = Ws + (size_t)kb * np + k;
      int i = kb;
      for (; i + WU <= n; i += WU, wc += (size_t)WU * np) {    // WU loads in flight, then their products in row order
        float a[WU];
#pragma unroll
        for (int q = 0; q < WU; ++q) a[q] = wc[(size_t)q * np];
#pragma unroll
        for (int q = 0; q < WU; ++q)
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (c < nc) acc[c] = fma((double)a[q], yy[(size_t)c * np + i + q], acc[c]);
      }
      for (; i < n; ++i, wc += np) {
        const double a = (double)*wc;
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < nc) acc[c] = fma(a, yy[(size_t)c * np + i], acc[c]);
      }
    }
    if (k < cap) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc && c0 + c < ncols) al[(size_t)(c0 + c) * cap + k] = k < n ? (float)(acc[c] - muc[c] * u[k]) : 0.f;
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc && c0 + c < ncols) ms[c0 + c] = (float)muc[c];
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

static inline int cs_members_check(int M, int H, int W) {
  P2I_REQUIRE(M >= 1 && M <= CS_MAX_M, "members must be in 1..%d (got %d)", CS_MAX_M, M);
  P2I_REQUIRE(H > 0 && W > 0 && H <= CS_MAX_S && W <= CS_MAX_S, "bad frame shape");
  return P2I_OK;
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
    (void)hipFuncSetAttribute((const void*)cs_weights_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    raised = true;
  }
  P2I_LAUNCH(cs_weights_kernel, dim3(ceil_div(k->R * M, nc), k->nsys), dim3(256), lds, (hipStream_t)stream, Winv, sol, k->pix, k->z,
             k->counts, (const int*)k->status, k->cand, ens, k->f0, k->R, k->T, M, W, H * W, k->cap, np, nc, alpha, mu);
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
