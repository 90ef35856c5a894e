// What the conditional simulations share (krig_cs.hip: per frame on a 2-D torus; stkrig_cs.hip: per sample on a
// 3-D torus, section 26): the counter-based noise, the two complex DFT products of a torus plane on v_mfma_f32_32x32x2_f32 and the
// conditioning weights.  A torus cell is one unsigned index: j Sx + k in 2-D, (l Sy + j) Sx + k in 3-D; the plane products take the
// index of the plane's first cell.
#pragma once
#include "krig_mfma.h"

namespace p2i {
namespace {

constexpr int CS_MAX_S = 512;      // side of the embedding torus: a row of it in LDS as fp64
constexpr int CS_MAX_M = 64;       // members per frame
constexpr int WU = 8;              // loads of W a thread of the weights kernel keeps in flight

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

// the complex standard normal xi of torus cell idx, member pair q, id `stream` (a frame's in 2-D, a sample's in 3-D): Box-Muller on
// (r0, r1), the logarithm through log1p in the upper half of r0 where u1 -> 1
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

// ---- the noise of the definition on its own: xi [npairs][n cells][2]
__global__ __launch_bounds__(256) void cs_noise_kernel(unsigned seed_lo, unsigned seed_hi, unsigned st_lo, unsigned st_hi, int q0, int n,
                                                       float* __restrict__ xi) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float2 v = cs_xi(seed_lo, seed_hi, (unsigned)i, (unsigned)(q0 + blockIdx.y), st_lo, st_hi);
  reinterpret_cast<float2*>(xi)[(size_t)blockIdx.y * n + i] = v;
}

// ---- spectrum, last pass over the Sy x Sx cells of a sample (the 3-D torus passes St Sy for Sy): the clip share rho = sum max(-lam, 0) /
// sum |lam| and the amplitude A = sqrt(lam+ / (Sy Sx)) with lam+ = max(lam, 0) sum lam / sum max(lam, 0).  A degenerate fitted sample gets A = 0 and rho = NaN.
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

// ---- stage 1 of a torus plane [Sy][Sx] whose first cell is cell0: P = (A xi) F_Sx[:, :W] of member pair q on the workgroup's tile
// of 32 torus rows from j0 x 128 columns (the wave's 32 from w0), into Po [2][Sy][W].  Per 32-wide slab of the k axis all threads
// draw G = A xi [32][32] into LDS (4 cells each; G never touches HBM) and the waves multiply it with the twiddles tx [2][Sx][W] (cos,
// sin of 2 pi k w / Sx) read as the B operand: P_re = G_re cos + G_im sin, P_im = G_im cos - G_re sin.  Rows and k past the torus are
// zeros; columns past W are not stored.  ab: the plane's amplitude.
__device__ __forceinline__ void cs_stage1_tile(float (*Gr)[A_LD], float (*Gi)[A_LD], const float* __restrict__ ab,
                                               const float* __restrict__ tx, unsigned seed_lo, unsigned seed_hi, unsigned cell0, unsigned q,
                                               unsigned st_lo, unsigned st_hi, int j0, int w0, int Sy, int Sx, int W,
                                               float* __restrict__ Po) {
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wc = min(w0 + l31, W - 1);
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
        const float2 xi = cs_xi(seed_lo, seed_hi, cell0 + (unsigned)(j * Sx + k), q, st_lo, st_hi);
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
    float* o = Po + w0 + l31;
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

// ---- stage 2 of a plane: Y = F_Sy[:H, :] P on the wave's tile of 32 rows from h0 x 32 columns from w0 < W; both operands come
// straight from memory (ty [2][Sy][H]: cos, sin of 2 pi j h / Sy, as the A operand; Pp [2][Sy][W] as the B operand).
// yr = cos P_re + sin P_im, yi = cos P_im - sin P_re; the caller stores the rows and columns inside the frame.
__device__ __forceinline__ void cs_stage2_tile(const float* __restrict__ Pp, const float* __restrict__ ty, int h0, int w0, int Sy, int H,
                                               int W, f32x16& yr, f32x16& yi) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, lhi = lane >> 5;
  const int hc = min(h0 + l31, H - 1), wc = min(w0 + l31, W - 1);
  const float* Pr = Pp + wc;
  const float* Pi = Pr + (size_t)Sy * W;
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
}

// ---- conditioning weights of nc columns of system s: r = z - U(points), y = W r (a wave per row, lanes along the row, a fixed
// shuffle tree), v = W^T y (a thread per column of W, rows in order; W holds explicit zeros above its diagonal), mu = u^T r / s,
// alpha = v - mu u; all fp64 on the fp32 W.  LDS: r and y, [nc][np] fp64 each.  A system without a model gets alpha = 0 and mu = 0
// (the predictor writes NaN there).
// ST = false: a system is R frames of one gauge set, column = frame t = col / M, member col % M; z and U of frame fs + t.
// ST = true: a system is one sample (R = T = 1 in the descriptor, TF frames), column = member; point i lies in frame stt[i] of the
// sample, so its residual is z_i - U_m(stt_i, pix_i), ens [samples][TF][M][HW].
template <bool ST>
__global__ __launch_bounds__(256) void cs_weights_kernel(const float* __restrict__ Wi, const double* __restrict__ sol,
                                                         const int* __restrict__ pix, const int* __restrict__ stt,
                                                         const float* __restrict__ z, const int* __restrict__ counts,
                                                         const int* __restrict__ status, const int* __restrict__ cand,
                                                         const float* __restrict__ ens, int f0, int R, int T, int TF, int M, int W, int HW,
                                                         int cap, int np, int nc, float* __restrict__ alpha, float* __restrict__ mu) {
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
  const int* gt = ST ? stt + (size_t)fs * cap : nullptr;
  const double su = sum_u(u, n, red);
  double muc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    muc[c] = 0.0;
    if (c < nc) {
      const bool valid = c0 + c < ncols;
      const int col = min(c0 + c, ncols - 1);
      const float* zf = z + (size_t)(fs + (ST ? 0 : col / M)) * cap;
      const float* uf = ST ? ens + ((size_t)fs * TF * M + col) * HW : ens + ((size_t)fs * M + col) * HW;
      double ur = 0.0;
      for (int i = tid; i < n; i += 256) {
        const int g = gp[i];
        const size_t at = (ST ? (size_t)gt[i] * M * HW : (size_t)0) + (size_t)((g >> 16) * W + (g & 0xffff));
        const double r = valid ? (double)zf[i] - (double)uf[at] : 0.0;
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

}  // namespace
}  // namespace p2i

static inline int cs_members_check(int M, int H, int W) {
  P2I_REQUIRE(M >= 1 && M <= p2i::CS_MAX_M, "members must be in 1..%d (got %d)", p2i::CS_MAX_M, M);
  P2I_REQUIRE(H > 0 && W > 0 && H <= p2i::CS_MAX_S && W <= p2i::CS_MAX_S, "bad frame shape");
  return P2I_OK;
}
