// STDK (spatio-temporal DeepKriging) baseline: Wendland bases, visible-point selection and the 100-100-100-1 MLP over every
// (sample, frame, pixel) row -- models/stdk.py:149-186 of the reference, without materialising its [rows, K_s + K_t + 79 T]
// feature tensor.  Layer 1 is split by its three input blocks (pixel / frame / sample: DESIGN.md section 8):
//   h1[(b,t,p)] = relu(P[p] + Q[b,t]),  P = phi_s W1s^T,  Q[b,t] = phi_t[t] W1t^T + z[b] W1z^T + b1
// so the per-row work is two 100 x 100 layers and the head, done on v_mfma_f32_16x16x4_f32 (exact f32) with the layer outputs kept
// in registers.  Hidden width 100 is padded to 112 = 7 x 16 (pads are zero throughout).
//
// Register layout of a wave's 16 rows ("transposed" products): every layer computes H_out^T = W H_in^T, so the MFMA's A operand is
// a weight fragment (from LDS) and its B operand the previous layer's accumulator, with no lane movement.  Lane l holds the hidden
// units n = 16 m + 4 (l >> 4) + v (m < 7 tiles, v < 4 registers) of row l & 15; the k order of a product is permuted accordingly.
#include "common.h"

namespace p2i {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HID = 100;       // hidden width of the reference's DKMLP
constexpr int HP = 112;        // padded to 7 tiles of 16
constexpr int NT = 7;
constexpr int WS = 116;        // LDS row stride of a [112][112] weight image: the transposed reads are conflict-free
constexpr int ROWS_WG = 64;    // pixels per workgroup (4 waves x 16)

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ---- bases: phi[i][k] = wendland(|pos_i - knot_k| / theta_k), pos_i = (i / W, i % W); knots as (y, x) float pairs
__global__ __launch_bounds__(256) void stdk_basis_kernel(const float* __restrict__ knots, const float* __restrict__ theta, int K, int H,
                                                         int W, float* __restrict__ phi) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)H * W * K) return;
  const int k = (int)(e % K);
  const int i = (int)(e / K);
  const float dy = (float)(i / W) - knots[2 * k], dx = (float)(i % W) - knots[2 * k + 1];
  const float d = __fsqrt_rn(dy * dy + dx * dx) / theta[k];      // integer coordinates: the squared distance is exact
  float out = 0.f;
  if (d <= 1.f) {
    const float a = 1.f - d, a2 = a * a, a6 = a2 * a2 * a2;
    out = a6 * (35.f * (d * d) + 18.f * d + 3.f) / 3.f;
  }
  phi[e] = out;
}

// ---- visible points of one (b, t) frame: mask != 0 pixels in raster order, then mask == 0 pixels in raster order, first k of them
__global__ __launch_bounds__(256) void stdk_select_kernel(const float* __restrict__ x, const float* __restrict__ mask, int HW, int k,
                                                          int* __restrict__ idx, float* __restrict__ z) {
  __shared__ int wave_cnt[4];
  const int bt = blockIdx.x;
  const float* m = mask + (size_t)bt * HW;
  const float* xv = x + (size_t)bt * HW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int found = 0;                                        // uniform over the workgroup
  for (int pass = 0; pass < 2 && found < k; ++pass) {
    for (int base = 0; base < HW && found < k; base += 256) {
      const int p = base + threadIdx.x;
      const bool hit = p < HW && ((m[p] != 0.f) == (pass == 0));
      const unsigned long long bal = __ballot(hit);
      const int before = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wave_cnt[wave] = __popcll(bal);
      __syncthreads();
      int off = found;
      for (int w = 0; w < wave; ++w) off += wave_cnt[w];
      const int slot = off + before;
      if (hit && slot < k) {
        idx[(size_t)bt * k + slot] = p;
        z[(size_t)bt * k + slot] = xv[p];
      }
      found += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
      __syncthreads();
    }
  }
}

// ---- small strided GEMM (layer 1 and its weight gradient): C[s][i][j] = sum_{k in split s} A[i*ai + k*ak] B[k*bk + j*bj] for
// j < Nv (0 for Nv <= j < N).  One thread per output, k ascending: run-to-run identical.
__global__ __launch_bounds__(256) void stdk_gemm_kernel(const float* __restrict__ A, long long ai, long long ak, const float* __restrict__ B,
                                                        long long bk, long long bj, float* __restrict__ C, long long ldc, long long split_stride,
                                                        int M, int N, int Nv, int K, int kchunk) {
  const int j = blockIdx.x * 16 + (threadIdx.x & 15);
  const int i = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= M || j >= N) return;
  const int s = blockIdx.z;
  float acc = 0.f;
  if (j < Nv) {
    const int k1 = min(K, (s + 1) * kchunk);
    for (int k = s * kchunk; k < k1; ++k) acc = fmaf(A[i * ai + k * ak], B[k * bk + j * bj], acc);
  }
  C[s * split_stride + i * ldc + j] = acc;
}

// Q[b][t][n] = Zt[t][n] + Zb[b][n] + b1[n] (n < 100; padded rows of 112)
__global__ __launch_bounds__(256) void stdk_q_kernel(const float* __restrict__ zt, const float* __restrict__ zb, const float* __restrict__ b1,
                                                     int B, int T, float* __restrict__ q) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * T * HP) return;
  const int n = e % HP, bt = e / HP, t = bt % T, b = bt / T;
  q[e] = n < HID ? (zt[t * HP + n] + zb[b * HP + n]) + b1[n] : 0.f;
}

// dQ [B][T][100] -> dQt [T][100] (sum over b), dQb [B][100] (sum over t), db1 [100] (sum over b then t), fixed order
__global__ __launch_bounds__(256) void stdk_q_reduce_kernel(const float* __restrict__ dq, int B, int T, float* __restrict__ dqt,
                                                            float* __restrict__ dqb, float* __restrict__ db1) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < T * HID) {
    const int t = e / HID, n = e % HID;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dq[((size_t)b * T + t) * HID + n];
    dqt[e] = s;
  } else if (e < (T + B) * HID) {
    const int b = e / HID - T, n = e % HID;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += dq[((size_t)b * T + t) * HID + n];
    dqb[b * HID + n] = s;
  } else if (e < (T + B + 1) * HID) {
    const int n = e - (T + B) * HID;
    float s = 0.f;
    for (int t = 0; t < T; ++t) {
      float st = 0.f;
      for (int b = 0; b < B; ++b) st += dq[((size_t)b * T + t) * HID + n];
      s += st;
    }
    db1[n] = s;
  }
}

// [100][100] row-major weight -> zero-padded [112][WS] LDS image
__device__ __forceinline__ void load_w(float* s, const float* __restrict__ w) {
  for (int e = threadIdx.x; e < HP * WS; e += blockDim.x) {
    const int n = e / WS, k = e - n * WS;
    s[e] = (n < HID && k < HID) ? w[n * HID + k] : 0.f;
  }
}
__device__ __forceinline__ void load_v(float* s, const float* __restrict__ v) {
  for (int e = threadIdx.x; e < HP; e += blockDim.x) s[e] = e < HID ? v[e] : 0.f;
}

// h1 of row (bt, p) in the register layout: x[m][v] = relu(P[p][n] + Q[bt][n]), n = 16 m + 4 g + v
__device__ __forceinline__ void layer1(const float* __restrict__ P, const float* __restrict__ Q, int bt, int p, bool valid, int g,
                                       f32x4 (&x)[NT]) {
#pragma unroll
  for (int m = 0; m < NT; ++m) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(Q + (size_t)bt * HP + 16 * m + 4 * g);
    f32x4 pv = {0.f, 0.f, 0.f, 0.f};
    if (valid) pv = *reinterpret_cast<const f32x4*>(P + (size_t)p * HP + 16 * m + 4 * g);
#pragma unroll
    for (int v = 0; v < 4; ++v) x[m][v] = fmaxf(pv[v] + q[v], 0.f);
  }
}

// y^T = W x^T (+ bias, relu): A = W[16 nt + r][16 m + 4 g + v] (TRANS: W^T, i.e. W[16 m + 4 g + v][16 nt + r]), B = x[m][v]
template <bool TRANS>
__device__ __forceinline__ void layer(const float* sw, const f32x4 (&x)[NT], int r, int g, f32x4 (&y)[NT]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) y[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < NT; ++m) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float a = TRANS ? sw[(16 * m + 4 * g + v) * WS + 16 * nt + r] : sw[(16 * nt + r) * WS + 16 * m + 4 * g + v];
        y[nt] = mfma4(a, x[m][v], y[nt]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);      // one k tile at a time: hoisting all 196 weight reads costs ~200 VGPRs (spills in the backward)
  }
}
__device__ __forceinline__ void bias_relu(f32x4 (&y)[NT], const float* sb, int g) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int v = 0; v < 4; ++v) y[nt][v] = fmaxf(y[nt][v] + sb[16 * nt + 4 * g + v], 0.f);
}

struct MlpSmem {
  float w2[HP * WS], w3[HP * WS], b2[HP], b3[HP], w4[HP];
};

// ---- forward: y[bt][p] = head(relu(W3 relu(W2 h1 + b2) + b3)).  grid (ceil(HW / 64), bt splits), 4 waves of 16 pixels each.
__global__ __launch_bounds__(256) void stdk_mlp_fwd_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                           const float* __restrict__ w2, const float* __restrict__ b2,
                                                           const float* __restrict__ w3, const float* __restrict__ b3,
                                                           const float* __restrict__ w4, const float* __restrict__ b4, int HW, int BT,
                                                           int bt_per, float* __restrict__ y) {
  __shared__ MlpSmem sm;
  load_w(sm.w2, w2); load_w(sm.w3, w3);
  load_v(sm.b2, b2); load_v(sm.b3, b3); load_v(sm.w4, w4);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int p = blockIdx.x * ROWS_WG + wave * 16 + r;
  const bool valid = p < HW;
  const float bias4 = b4[0];
  const int bt0 = blockIdx.y * bt_per, bt1 = min(BT, bt0 + bt_per);
  for (int bt = bt0; bt < bt1; ++bt) {
    f32x4 h1[NT], h2[NT];
    layer1(P, Q, bt, p, valid, g, h1);
    layer<false>(sm.w2, h1, r, g, h2);
    bias_relu(h2, sm.b2, g);
    layer<false>(sm.w3, h2, r, g, h1);
    bias_relu(h1, sm.b3, g);
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
      for (int v = 0; v < 4; ++v) s = fmaf(sm.w4[16 * m + 4 * g + v], h1[m][v], s);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (g == 0 && valid) y[(size_t)bt * HW + p] = s + bias4;
  }
}

__device__ __forceinline__ void store_rows(float* __restrict__ dst, size_t row, bool valid, int g, const f32x4 (&x)[NT]) {
  if (!valid) return;
#pragma unroll
  for (int m = 0; m < NT; ++m) *reinterpret_cast<f32x4*>(dst + row * HP + 16 * m + 4 * g) = x[m];
}

// ---- backward: recompute h1..h3 of the tile, then g3 = d/d(pre-activation 3), g2, g1.  Stores h1, h2, h3, g2, g3 (rows x 112) for
// the weight-gradient pass, dP partials [split][HW][100] (sum over this split's frames, in registers) and dQ partials
// [HW / 16 wave tiles][BT][100] (sum over the wave's 16 pixels, lane shuffles in a fixed order).
__global__ __launch_bounds__(256) void stdk_mlp_bwd_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                           const float* __restrict__ w2, const float* __restrict__ b2,
                                                           const float* __restrict__ w3, const float* __restrict__ b3,
                                                           const float* __restrict__ w4, const float* __restrict__ dy, int HW, int BT,
                                                           int bt_per, float* __restrict__ h1s, float* __restrict__ h2s,
                                                           float* __restrict__ h3s, float* __restrict__ g2s, float* __restrict__ g3s,
                                                           float* __restrict__ dp_part, float* __restrict__ dq_part) {
  __shared__ MlpSmem sm;
  load_w(sm.w2, w2); load_w(sm.w3, w3);
  load_v(sm.b2, b2); load_v(sm.b3, b3); load_v(sm.w4, w4);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int p = blockIdx.x * ROWS_WG + wave * 16 + r;
  const bool valid = p < HW;
  const int tile = blockIdx.x * 4 + wave;
  const int bt0 = blockIdx.y * bt_per, bt1 = min(BT, bt0 + bt_per);
  f32x4 dp[NT];
#pragma unroll
  for (int m = 0; m < NT; ++m) dp[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int bt = bt0; bt < bt1; ++bt) {
    const size_t row = (size_t)bt * HW + p;
    f32x4 h1[NT], h2[NT], t[NT];
    layer1(P, Q, bt, p, valid, g, h1);
    store_rows(h1s, row, valid, g, h1);
    layer<false>(sm.w2, h1, r, g, h2);
    bias_relu(h2, sm.b2, g);
    store_rows(h2s, row, valid, g, h2);
    layer<false>(sm.w3, h2, r, g, t);
    bias_relu(t, sm.b3, g);
    store_rows(h3s, row, valid, g, t);
    const float d = valid ? dy[row] : 0.f;
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
      for (int v = 0; v < 4; ++v) t[m][v] = t[m][v] > 0.f ? d * sm.w4[16 * m + 4 * g + v] : 0.f;    // g3
    store_rows(g3s, row, valid, g, t);
    f32x4 u[NT];
    layer<true>(sm.w3, t, r, g, u);                                                                // W3^T g3
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
      for (int v = 0; v < 4; ++v) u[m][v] = h2[m][v] > 0.f ? u[m][v] : 0.f;                       // g2
    store_rows(g2s, row, valid, g, u);
    layer<true>(sm.w2, u, r, g, t);                                                                // W2^T g2
#pragma unroll
    for (int m = 0; m < NT; ++m) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        float v1 = h1[m][v] > 0.f ? t[m][v] : 0.f;                                                 // g1
        dp[m][v] += v1;
        v1 += __shfl_xor(v1, 1, 64);
        v1 += __shfl_xor(v1, 2, 64);
        v1 += __shfl_xor(v1, 4, 64);
        v1 += __shfl_xor(v1, 8, 64);
        t[m][v] = v1;
      }
      const int n = 16 * m + 4 * g;
      if (r == 0 && n < HID) *reinterpret_cast<f32x4*>(dq_part + ((size_t)tile * BT + bt) * HID + n) = t[m];
    }
  }
  if (!valid) return;
#pragma unroll
  for (int m = 0; m < NT; ++m) {
    const int n = 16 * m + 4 * g;
    if (n < HID) *reinterpret_cast<f32x4*>(dp_part + ((size_t)blockIdx.y * HW + p) * HID + n) = dp[m];
  }
}

// ---- weight gradients of layers 2..4 from the stored rows: part[chunk] = sum over the chunk's rows of g^T [h | 1]
// (wave w: output rows 16 w .. 16 w + 15; column 100 of h is taken as 1, so column 100 of the product is the bias gradient).
// HEAD (layer 4): g is dy (one output row).  part layout: [chunk][nout * 100 weights, then nout biases].
template <bool HEAD>
__global__ __launch_bounds__(448) void stdk_wgrad_kernel(const float* __restrict__ gsrc, const float* __restrict__ h, long long nrows,
                                                         int chunk_rows, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int nout = HEAD ? 1 : HID;
  const long long r0 = (long long)blockIdx.x * chunk_rows;
  const long long r1 = min(nrows, r0 + chunk_rows);
  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long rb = r0; rb < r1; rb += 4) {
    const long long row = rb + g;
    const bool in = row < r1;
    float a = 0.f;
    if (in) a = HEAD ? (r == 0 ? gsrc[row] : 0.f) : gsrc[row * HP + 16 * w + r];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int k = 16 * j + r;
      const float b = in ? (k == HID ? 1.f : h[row * HP + k]) : 0.f;
      acc[j] = mfma4(a, b, acc[j]);
    }
  }
  float* out = part + (size_t)blockIdx.x * (nout * HID + nout);
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int k = 16 * j + r;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int n = 16 * w + 4 * g + v;
      if (n >= nout) continue;
      if (k < HID) out[n * HID + k] = acc[j][v];
      else if (k == HID) out[nout * HID + n] = acc[j][v];
    }
  }
}

int gemm(const float* A, long long ai, long long ak, const float* B, long long bk, long long bj, float* C, long long ldc, long long split_stride,
         int M, int N, int Nv, int K, int splits, hipStream_t s) {
  const int kchunk = ceil_div(K > 0 ? K : 1, splits);
  P2I_LAUNCH(stdk_gemm_kernel, dim3(ceil_div(N, 16), ceil_div(M, 16), splits), dim3(256), 0, s, A, ai, ak, B, bk, bj, C, ldc, split_stride,
             M, N, Nv, K, kchunk);
  return launch_status();
}

}  // namespace
}  // namespace p2i
using namespace p2i;

extern "C" int p2i_stdk_basis(const float* knots, const float* theta, int K, int H, int W, float* phi, void* stream) {
  P2I_REQUIRE(knots && theta && phi, "null pointer");
  P2I_REQUIRE(K > 0 && H > 0 && W > 0 && (long long)H * W * K < (1ll << 31), "bad basis shape");
  const long long n = (long long)H * W * K;
  P2I_LAUNCH(stdk_basis_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, (hipStream_t)stream, knots, theta, K, H, W, phi);
  return launch_status();
}

extern "C" int p2i_stdk_select(const float* masked, const float* mask, int BT, int HW, int k, int* idx, float* z, void* stream) {
  P2I_REQUIRE(masked && mask && idx && z, "null pointer");
  P2I_REQUIRE(BT > 0 && k > 0 && HW >= k, "stdk_select needs H*W >= k (%d < %d)", HW, k);
  P2I_LAUNCH(stdk_select_kernel, dim3(BT), dim3(256), 0, (hipStream_t)stream, masked, mask, HW, k, idx, z);
  return launch_status();
}

extern "C" int p2i_stdk_layer1_fwd(const float* phi_s, const float* phi_t, const float* z, const float* w1, const float* b1, int B, int T,
                                   int HW, int Ks, int Kt, int Kz, float* P, float* zt, float* zb, float* Q, void* stream) {
  P2I_REQUIRE(phi_s && phi_t && z && w1 && b1 && P && zt && zb && Q, "null pointer");
  P2I_REQUIRE(B > 0 && T > 0 && HW > 0 && Ks > 0 && Kt > 0 && Kz > 0, "bad layer-1 shape");
  hipStream_t s = (hipStream_t)stream;
  const long long F = (long long)Ks + Kt + Kz;
  if (int e = gemm(phi_s, Ks, 1, w1, 1, F, P, HP, 0, HW, HP, HID, Ks, 1, s)) return e;
  if (int e = gemm(phi_t, Kt, 1, w1 + Ks, 1, F, zt, HP, 0, T, HP, HID, Kt, 1, s)) return e;
  if (int e = gemm(z, Kz, 1, w1 + Ks + Kt, 1, F, zb, HP, 0, B, HP, HID, Kz, 1, s)) return e;
  P2I_LAUNCH(stdk_q_kernel, dim3(ceil_div(B * T * HP, 256)), dim3(256), 0, s, zt, zb, b1, B, T, Q);
  return launch_status();
}

extern "C" int p2i_stdk_mlp_fwd(const float* P, const float* Q, const float* w2, const float* b2, const float* w3, const float* b3,
                                const float* w4, const float* b4, int HW, int BT, float* y, void* stream) {
  P2I_REQUIRE(P && Q && w2 && b2 && w3 && b3 && w4 && b4 && y, "null pointer");
  P2I_REQUIRE(HW > 0 && BT > 0, "bad MLP shape");
  const int gx = ceil_div(HW, ROWS_WG);
  const int splits = min(BT, max(1, ceil_div(2048, gx)));
  const int bt_per = ceil_div(BT, splits);
  P2I_LAUNCH(stdk_mlp_fwd_kernel, dim3(gx, ceil_div(BT, bt_per)), dim3(256), 0, (hipStream_t)stream, P, Q, w2, b2, w3, b3, w4, b4, HW, BT,
             bt_per, y);
  return launch_status();
}

// bt splits of the backward grid and row chunks of the weight-gradient pass (the partial buffers are sized from these)
static int bwd_bt_per(int HW, int BT) { return ceil_div(BT, min(BT, max(1, ceil_div(1024, ceil_div(HW, ROWS_WG))))); }
static int bwd_splits(int HW, int BT) { return ceil_div(BT, bwd_bt_per(HW, BT)); }     // every split owns >= 1 frame; together all
static int wgrad_chunk_rows(long long nrows) { return (int)max(256ll, (ceil_div64(nrows, 1024) + 3) / 4 * 4); }

extern "C" int p2i_stdk_bwd_workspace(int HW, int BT, int64_t* sizes4) {
  P2I_REQUIRE(sizes4 && HW > 0 && BT > 0, "bad MLP shape");
  const long long nrows = (long long)BT * HW;
  const long long chunks = ceil_div64(nrows, wgrad_chunk_rows(nrows));
  sizes4[0] = 5 * nrows * HP;                                              // h1, h2, h3, g2, g3 rows
  sizes4[1] = (long long)bwd_splits(HW, BT) * HW * HID;                    // dP partials
  sizes4[2] = (long long)ceil_div(HW, ROWS_WG) * 4 * BT * HID;             // dQ partials
  sizes4[3] = chunks * (2 * (HID * HID + HID) + HID + 1);                  // weight-gradient partials
  return P2I_OK;
}

extern "C" int p2i_stdk_mlp_bwd(const float* P, const float* Q, const float* w2, const float* b2, const float* w3, const float* b3,
                                const float* w4, const float* dy, int HW, int BT, float* rows5, float* dp_part, float* dq_part,
                                float* wpart, float* dP, float* dQ, float* dw2, float* db2, float* dw3, float* db3, float* dw4, float* db4,
                                void* stream) {
  P2I_REQUIRE(P && Q && w2 && b2 && w3 && b3 && w4 && dy && rows5 && dp_part && dq_part && wpart, "null pointer");
  P2I_REQUIRE(dP && dQ && dw2 && db2 && dw3 && db3 && dw4 && db4, "null pointer");
  P2I_REQUIRE(HW > 0 && BT > 0, "bad MLP shape");
  hipStream_t s = (hipStream_t)stream;
  const int gx = ceil_div(HW, ROWS_WG);
  const int bt_per = bwd_bt_per(HW, BT), splits = bwd_splits(HW, BT);
  const long long nrows = (long long)BT * HW;
  const size_t plane = (size_t)nrows * HP;
  float* h1s = rows5;
  float* h2s = rows5 + plane;
  float* h3s = rows5 + 2 * plane;
  float* g2s = rows5 + 3 * plane;
  float* g3s = rows5 + 4 * plane;
  P2I_LAUNCH(stdk_mlp_bwd_kernel, dim3(gx, splits), dim3(256), 0, s, P, Q, w2, b2, w3, b3, w4, dy, HW, BT, bt_per, h1s, h2s, h3s, g2s, g3s,
             dp_part, dq_part);
  if (int e = launch_status()) return e;
  const int chunk_rows = wgrad_chunk_rows(nrows);
  const int chunks = (int)ceil_div64(nrows, chunk_rows);
  const size_t big = (size_t)chunks * (HID * HID + HID);
  P2I_LAUNCH(stdk_wgrad_kernel<false>, dim3(chunks), dim3(448), 0, s, g3s, h2s, nrows, chunk_rows, wpart);
  P2I_LAUNCH(stdk_wgrad_kernel<false>, dim3(chunks), dim3(448), 0, s, g2s, h1s, nrows, chunk_rows, wpart + big);
  P2I_LAUNCH(stdk_wgrad_kernel<true>, dim3(chunks), dim3(64), 0, s, dy, h3s, nrows, chunk_rows, wpart + 2 * big);
  if (int e = launch_status()) return e;
  // outputs are accumulated into by det_reduce: zero first
  for (auto& zb : {std::make_pair(dP, (size_t)HW * HID), std::make_pair(dQ, (size_t)BT * HID), std::make_pair(dw2, (size_t)HID * HID),
                   std::make_pair(db2, (size_t)HID), std::make_pair(dw3, (size_t)HID * HID), std::make_pair(db3, (size_t)HID),
                   std::make_pair(dw4, (size_t)HID), std::make_pair(db4, (size_t)1)})
    if (hipError_t e = memset_async(zb.first, 0, zb.second * sizeof(float), s)) { set_error("memset: %s", hipGetErrorString(e)); return (int)e; }
  if (int e = det_reduce(dp_part, HW * HID, splits, 1, (long long)HW * HID, DetSegs{{dP, nullptr, nullptr, nullptr}, {HW * HID, 0, 0, 0}}, s)) return e;
  if (int e = det_reduce(dq_part, BT * HID, gx * 4, 1, (long long)BT * HID, DetSegs{{dQ, nullptr, nullptr, nullptr}, {BT * HID, 0, 0, 0}}, s)) return e;
  const int per = HID * HID + HID;
  if (int e = det_reduce(wpart, per, chunks, 1, per, DetSegs{{dw3, db3, nullptr, nullptr}, {HID * HID, HID, 0, 0}}, s)) return e;
  if (int e = det_reduce(wpart + big, per, chunks, 1, per, DetSegs{{dw2, db2, nullptr, nullptr}, {HID * HID, HID, 0, 0}}, s)) return e;
  return det_reduce(wpart + 2 * big, HID + 1, chunks, 1, HID + 1, DetSegs{{dw4, db4, nullptr, nullptr}, {HID, 1, 0, 0}}, s);
}

extern "C" int p2i_stdk_layer1_bwd(const float* phi_s, const float* phi_t, const float* z, const float* dP, const float* dQ, int B, int T,
                                   int HW, int Ks, int Kt, int Kz, float* dqt, float* dqb, float* part, int splits, float* dw1, float* db1,
                                   void* stream) {
  P2I_REQUIRE(phi_s && phi_t && z && dP && dQ && dqt && dqb && part && dw1 && db1, "null pointer");
  P2I_REQUIRE(B > 0 && T > 0 && HW > 0 && Ks > 0 && Kt > 0 && Kz > 0 && splits > 0, "bad layer-1 shape");
  hipStream_t s = (hipStream_t)stream;
  const long long F = (long long)Ks + Kt + Kz;
  P2I_LAUNCH(stdk_q_reduce_kernel, dim3(ceil_div((T + B + 1) * HID, 256)), dim3(256), 0, s, dQ, B, T, dqt, dqb, db1);
  if (int e = launch_status()) return e;
  const long long ps = HID * F;          // part: [splits][100][F], every element written by one of the three products
  if (int e = gemm(dP, 1, HID, phi_s, Ks, 1, part, F, ps, HID, Ks, Ks, HW, splits, s)) return e;
  if (int e = gemm(dqt, 1, HID, phi_t, Kt, 1, part + Ks, F, ps, HID, Kt, Kt, T, splits, s)) return e;
  if (int e = gemm(dqb, 1, HID, z, Kz, 1, part + Ks + Kt, F, ps, HID, Kz, Kz, B, splits, s)) return e;
  if (hipError_t e = memset_async(dw1, 0, (size_t)ps * sizeof(float), s)) { set_error("memset: %s", hipGetErrorString(e)); return (int)e; }
  return det_reduce(part, (int)ps, splits, 1, ps, DetSegs{{dw1, nullptr, nullptr, nullptr}, {(int)ps, 0, 0, 0}}, s);
}
