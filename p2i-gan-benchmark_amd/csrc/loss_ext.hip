// The reference's alternative training objectives (modules/losses.py) beyond ReconstructionLoss / gan_loss: the legacy rain-rate
// transform (:51-53), weighted L1 (:56-65), row softmax with temperature (:68-73), KL batchmean (:76-80), forward temporal
// difference (:83-85), MaxPool2d(5, 4, 2) (:88-91), temporal-difference matching (:94-109), the shock map (:112-137) and the shock
// loss (:140-162), each with its gradient.  All tensors fp32 and contiguous.  Every cross-workgroup sum is a set of workgroup
// partials added in workgroup order by det_reduce (common.h); every backward pass is a gather with a fixed order of additions, so
// two runs give the same bits.  Max-pool ties: the first maximal element of the window in raster order takes the gradient; a NaN
// wins every scan (`v > m || v != v`), so a window that holds one pools to NaN and its last NaN in raster order is the argmax (torch).
#include "common.h"

namespace p2i {

static inline int ext_grid(long long n, int per_block, int cap) {
  long long g = (n + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int V> struct Vec;
template <> struct Vec<1> { float v[1]; };
template <> struct alignas(16) Vec<4> { float v[4]; };
template <int V> __device__ __forceinline__ Vec<V> vload(const float* p) { return *reinterpret_cast<const Vec<V>*>(p); }
template <int V> __device__ __forceinline__ void vstore(float* p, const Vec<V>& x) { *reinterpret_cast<Vec<V>*>(p) = x; }

// ---------------------------------------------------------------- transform (losses.py:51-53): 0.036 * 10^((x*255/3)*0.0625)
__device__ __forceinline__ float legacy_rate(float x) {
  const float e = (x * 255.0f / 3.0f) * 0.0625f;
  return 0.036f * exp2f(e * 3.3219280948873623f);            // 10^e
}
template <int V, bool BWD>
__global__ __launch_bounds__(256) void transform_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ out,
                                                        long long nv) {
  const float slope = 2.302585092994046f * (255.0f / 3.0f) * 0.0625f;      // d/dx of the exponent, times ln 10
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    const Vec<V> a = vload<V>(x + i * V);
    Vec<V> g, r;
    if (BWD) g = vload<V>(dy + i * V);
#pragma unroll
    for (int k = 0; k < V; ++k) r.v[k] = BWD ? g.v[k] * legacy_rate(a.v[k]) * slope : legacy_rate(a.v[k]);
    vstore<V>(out + i * V, r);
  }
}

// ---------------------------------------------------------------- forward difference (losses.py:83-85) over dim 1
// fwd: out[b][t] = x[b][t+1] - x[b][t], t < T-1.  bwd: dx[b][t] = dy[b][t-1] (t >= 1) - dy[b][t] (t <= T-2).  inner = V * iv elements.
template <int V>
__global__ __launch_bounds__(256) void fdiff_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, int T, long long iv,
                                                        long long nv) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    const long long row = i / iv, b = row / (T - 1);               // output row (b, t) is input row b*T + t = row + b
    const float* p = x + (i + b * iv) * V;
    const Vec<V> lo = vload<V>(p), hi = vload<V>(p + iv * V);
    Vec<V> r;
#pragma unroll
    for (int k = 0; k < V; ++k) r.v[k] = hi.v[k] - lo.v[k];
    vstore<V>(out + i * V, r);
  }
}
template <int V>
__global__ __launch_bounds__(256) void fdiff_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int T, long long iv,
                                                        long long nv) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    const long long row = i / iv, b = row / T;
    const int t = (int)(row - b * T);
    const float* p = dy + (i - b * iv) * V;                        // dy row (b, t) = b*(T-1) + t
    Vec<V> r;
#pragma unroll
    for (int k = 0; k < V; ++k) r.v[k] = 0.f;
    if (t >= 1) {
      const Vec<V> a = vload<V>(p - iv * V);
#pragma unroll
      for (int k = 0; k < V; ++k) r.v[k] += a.v[k];
    }
    if (t <= T - 2) {
      const Vec<V> a = vload<V>(p);
#pragma unroll
      for (int k = 0; k < V; ++k) r.v[k] -= a.v[k];
    }
    vstore<V>(dx + i * V, r);
  }
}

// ---------------------------------------------------------------- weighted L1 (losses.py:56-65)
__device__ __forceinline__ float wl1_weight(float y) {
  const float a = 0.50f, b = 5.14f, c = 0.12f, xmax = 0.70f;
  return (y > xmax) ? (a * expf(b * xmax) + c) : (a * expf(b * y) + c);
}
template <int V>
__global__ __launch_bounds__(256) void wl1_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, long long nv,
                                                      float inv_n, float* __restrict__ part) {
  __shared__ float red[16];
  float acc = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    const Vec<V> p = vload<V>(pred + i * V), y = vload<V>(tgt + i * V);
#pragma unroll
    for (int k = 0; k < V; ++k) acc += wl1_weight(y.v[k]) * fabsf(p.v[k] - y.v[k]);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc * inv_n;
}
template <int V>
__global__ __launch_bounds__(256) void wl1_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                      const float* __restrict__ gout, float* __restrict__ dpred, long long nv, float inv_n) {
  const float g = gout[0] * inv_n;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    const Vec<V> p = vload<V>(pred + i * V), y = vload<V>(tgt + i * V);
    Vec<V> r;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float d = p.v[k] - y.v[k];
      r.v[k] = d > 0.f ? g * wl1_weight(y.v[k]) : (d < 0.f ? -g * wl1_weight(y.v[k]) : 0.f);      // sign(0) = 0
    }
    vstore<V>(dpred + i * V, r);
  }
}

// ---------------------------------------------------------------- row softmax with temperature (losses.py:68-73)
// one workgroup per row of L elements: max, sum, write
__global__ __launch_bounds__(1024) void softmax_t_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int L, float inv_temp) {
  __shared__ float red[16];
  const float* xr = x + (size_t)blockIdx.x * L;
  float* yr = y + (size_t)blockIdx.x * L;
  float m = -INFINITY;
  for (int i = threadIdx.x; i < L; i += blockDim.x) m = fmaxf(m, xr[i] * inv_temp);
  m = block_max(m, red);
  float s = 0.f;
  for (int i = threadIdx.x; i < L; i += blockDim.x) s += expf(xr[i] * inv_temp - m);
  s = block_sum(s, red);
  const float inv = 1.f / s;
  for (int i = threadIdx.x; i < L; i += blockDim.x) yr[i] = expf(xr[i] * inv_temp - m) * inv;
}
// dx = y * (dy - sum(dy * y)) / temperature
__global__ __launch_bounds__(1024) void softmax_t_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx,
                                                             int L, float inv_temp) {
  __shared__ float red[16];
  const size_t o = (size_t)blockIdx.x * L;
  float dot = 0.f;
  for (int i = threadIdx.x; i < L; i += blockDim.x) dot += y[o + i] * dy[o + i];
  dot = block_sum(dot, red);
  for (int i = threadIdx.x; i < L; i += blockDim.x) dx[o + i] = y[o + i] * (dy[o + i] - dot) * inv_temp;
}

// ---------------------------------------------------------------- KL, batchmean (losses.py:76-80): sum xlogy(q, q) - q log p, / B
template <int V>
__global__ __launch_bounds__(256) void kl_fwd_kernel(const float* __restrict__ p, const float* __restrict__ q, long long nv, float inv_b,
                                                     float* __restrict__ part) {
  __shared__ float red[16];
  float acc = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    const Vec<V> a = vload<V>(p + i * V), b = vload<V>(q + i * V);
#pragma unroll
    for (int k = 0; k < V; ++k) acc += (b.v[k] == 0.f ? 0.f : b.v[k] * logf(b.v[k])) - b.v[k] * logf(a.v[k]);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc * inv_b;
}
template <int V>
__global__ __launch_bounds__(256) void kl_bwd_kernel(const float* __restrict__ p, const float* __restrict__ q, const float* __restrict__ gout,
                                                     float* __restrict__ dp, long long nv, float inv_b) {
  const float g = -gout[0] * inv_b;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    const Vec<V> a = vload<V>(p + i * V), b = vload<V>(q + i * V);
    Vec<V> r;
#pragma unroll
    for (int k = 0; k < V; ++k) r.v[k] = g * b.v[k] / a.v[k];
    vstore<V>(dp + i * V, r);
  }
}

// ---------------------------------------------------------------- MaxPool2d(5, stride 4, padding 2) (losses.py:88-91)
// max over the valid part of the window (padding is -inf) and the plane index h*W + w of its first maximal element in raster order;
// a NaN replaces whatever the scan holds, so the window's last NaN wins
__device__ __forceinline__ float spool_window(const float* __restrict__ plane, int H, int W, int oh, int ow, int& arg) {
  const int h0 = max(4 * oh - 2, 0), h1 = min(4 * oh + 2, H - 1), w0 = max(4 * ow - 2, 0), w1 = min(4 * ow + 2, W - 1);
  float m = plane[h0 * W + w0];
  arg = h0 * W + w0;
  for (int h = h0; h <= h1; ++h)
    for (int w = w0; w <= w1; ++w) {
      const float v = plane[h * W + w];
      if (v > m || v != v) { m = v; arg = h * W + w; }
    }
  return m;
}
__global__ __launch_bounds__(256) void spool_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, int* __restrict__ idx,
                                                        long long total, int H, int W, int Ho, int Wo) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ow = (int)(i % Wo), oh = (int)((i / Wo) % Ho);
    const long long n = i / ((long long)Wo * Ho);
    int arg;
    out[i] = spool_window(x + n * H * W, H, W, oh, ow, arg);
    if (idx) idx[i] = arg;
  }
}
// gather: dx[n][h][w] = scale * sum over the (up to 2 x 2) windows that cover (h, w) and whose argmax it is of dout
__global__ __launch_bounds__(256) void spool_bwd_kernel(const int* __restrict__ idx, const float* __restrict__ dout,
                                                        const float* __restrict__ scale, float* __restrict__ dx, long long total, int H,
                                                        int W, int Ho, int Wo) {
  const float sc = scale ? scale[0] : 1.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int w = (int)(i % W), h = (int)((i / W) % H);
    const long long n = i / ((long long)W * H);
    const int me = h * W + w;
    const int oh0 = h < 2 ? 0 : (h + 1) / 4, oh1 = min((h + 2) / 4, Ho - 1);       // 4 oh - 2 <= h <= 4 oh + 2
    const int ow0 = w < 2 ? 0 : (w + 1) / 4, ow1 = min((w + 2) / 4, Wo - 1);
    float acc = 0.f;
    for (int oh = oh0; oh <= oh1; ++oh)
      for (int ow = ow0; ow <= ow1; ++ow) {
        const long long o = (n * Ho + oh) * Wo + ow;
        if (idx[o] == me) acc += dout[o];
      }
    dx[i] = acc * sc;
  }
}

// ---------------------------------------------------------------- temporal-difference matching (losses.py:94-109)
// thread = one pooled position of one (b, t) plane, t < T - 1: the three pools, the term, and for the backward pass the argmax of
// the pred_diff window with coef = d mean / d P(pred_diff)
__global__ __launch_bounds__(256) void tdm_fwd_kernel(const float* __restrict__ pd, const float* __restrict__ td, const float* __restrict__ tr,
                                                      long long total, int Tm1, int H, int W, int Ho, int Wo, float beta, float eps,
                                                      float inv_count, float* __restrict__ part, float* __restrict__ coef,
                                                      int* __restrict__ idx) {
  __shared__ float red[16];
  float acc = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ow = (int)(i % Wo), oh = (int)((i / Wo) % Ho);
    const long long n = i / ((long long)Wo * Ho), b = n / Tm1;
    int ap, at;
    const float P = spool_window(pd + n * H * W, H, W, oh, ow, ap);
    const float Q = spool_window(td + n * H * W, H, W, oh, ow, at);
    const float base = spool_window(tr + (n + b) * H * W, H, W, oh, ow, at);      // true[b][t]: plane b*T + t
    const float wgt = 1.0f / (1.0f + beta * base + eps);
    const float d = P - Q;
    acc += d * d * wgt;
    if (coef) { coef[i] = 2.f * d * wgt * inv_count; idx[i] = ap; }
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc * inv_count;
}

// ---------------------------------------------------------------- shock map / shock loss (losses.py:112-162)
struct ShockArgs {
  int N, H, W;          // planes and their size as stored
  int Hp, Wp;           // the map's size: H / pool, W / pool (floor)
  int pool, m;          // max_pool2d(pool, pool) ahead of the map; border_ignore
  float beta, eps;
};
constexpr int STW = 32, STH = 8;                 // map pixels per workgroup tile; the staged tile has a halo of 1

__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }   // n >= 2, -1 <= i <= n

__device__ __forceinline__ float pooled_at(const float* __restrict__ plane, int W, int py, int px, int pool) {
  const float* p = plane + (size_t)(py * pool) * W + px * pool;
  float m = p[0];
  for (int i = 0; i < pool; ++i)
    for (int j = 0; j < pool; ++j) {
      const float v = p[i * W + j];
      if (v > m || v != v) m = v;                                              // fmaxf would drop a NaN
    }
  return m;
}
// stage the (STH + 2) x (STW + 2) pooled, reflect-padded tile whose interior starts at map pixel (ty0, tx0)
__device__ __forceinline__ void shock_stage(float (*t)[STW + 2], const float* __restrict__ plane, const ShockArgs& a, int ty0, int tx0) {
  for (int i = threadIdx.x; i < (STH + 2) * (STW + 2); i += STW * STH) {
    const int ly = i / (STW + 2), lx = i - ly * (STW + 2);
    const int gy = ty0 + ly - 1, gx = tx0 + lx - 1;
    float v = 0.f;
    if (gy <= a.Hp && gx <= a.Wp) v = pooled_at(plane, a.W, reflect1(gy, a.Hp), reflect1(gx, a.Wp), a.pool);
    t[ly][lx] = v;
  }
}
// Sobel / 8 (kx, ky = kx^T) and the 5-point Laplacian at the tile's interior pixel (ly, lx)
__device__ __forceinline__ void shock_stencils(const float (*t)[STW + 2], int ly, int lx, float& gx, float& gy, float& lap) {
  const float v00 = t[ly][lx], v01 = t[ly][lx + 1], v02 = t[ly][lx + 2];
  const float v10 = t[ly + 1][lx], v11 = t[ly + 1][lx + 1], v12 = t[ly + 1][lx + 2];
  const float v20 = t[ly + 2][lx], v21 = t[ly + 2][lx + 1], v22 = t[ly + 2][lx + 2];
  gx = ((v00 - v02) + 2.f * (v10 - v12) + (v20 - v22)) * 0.125f;
  gy = ((v00 - v20) + 2.f * (v01 - v21) + (v02 - v22)) * 0.125f;
  lap = (v01 + v10 + v12 + v21) - 4.f * v11;
}
// MODE 0: out = shock_map(x).  MODE 1: out = relu(|shock(pool(y))| - |shock(pool(x))|) cropped by m (x = pred, y = true).
// MODE 2 / 3: out = three planes [3][N][Hp][Wp] of g * ds/dgx, g * ds/dgy, g * ds/dlap of x's map, with g = dout (MODE 2) or the
// loss's gradient to x's map, -dout * [|s_y| > |s_x|] * sign(s_x) inside the crop and 0 in the ignored border (MODE 3).
template <int MODE>
__global__ __launch_bounds__(STW * STH) void shock_tile_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ dout, float* __restrict__ out, const ShockArgs a) {
  constexpr bool LOSS = (MODE == 1 || MODE == 3);
  __shared__ float tx[STH + 2][STW + 2];
  __shared__ float ty[LOSS ? STH + 2 : 1][STW + 2];
  const int n = blockIdx.z, ty0 = blockIdx.y * STH, tx0 = blockIdx.x * STW;
  const size_t plane = (size_t)n * a.H * a.W;
  shock_stage(tx, x + plane, a, ty0, tx0);
  if constexpr (LOSS) shock_stage(ty, y + plane, a, ty0, tx0);
  __syncthreads();
  const int lx = threadIdx.x % STW, ly = threadIdx.x / STW;
  const int qy = ty0 + ly, qx = tx0 + lx;
  if (qy >= a.Hp || qx >= a.Wp) return;
  float gx, gy, lap;
  shock_stencils(tx, ly, lx, gx, gy, lap);
  const float th = tanhf(a.beta * lap), gr = sqrtf(gx * gx + gy * gy + a.eps);
  const float sx = th * gr;
  const size_t q = ((size_t)n * a.Hp + qy) * a.Wp + qx;
  if constexpr (MODE == 0) { out[q] = sx; return; }
  float g = 0.f;
  if constexpr (LOSS) {
    float hx, hy, hl;
    shock_stencils(ty, ly, lx, hx, hy, hl);
    const float sy = tanhf(a.beta * hl) * sqrtf(hx * hx + hy * hy + a.eps);
    const float d = fabsf(sy) - fabsf(sx);
    const int Hc = a.Hp - 2 * a.m, Wc = a.Wp - 2 * a.m, cy = qy - a.m, cx = qx - a.m;
    const bool inside = cy >= 0 && cy < Hc && cx >= 0 && cx < Wc;
    const size_t c = ((size_t)n * Hc + cy) * Wc + cx;
    if constexpr (MODE == 1) {
      if (inside) out[c] = d <= 0.f ? 0.f : d;                                 // relu; a NaN difference stays NaN
      return;
    }
    if (inside && !(d <= 0.f)) g = sx > 0.f ? -dout[c] : (sx < 0.f ? dout[c] : 0.f);  // relu'(0) = 0, relu'(NaN) = 1, sign(0) = 0
  } else {
    g = dout[q];
  }
  const size_t np = (size_t)a.N * a.Hp * a.Wp;
  const float gt = g * th / gr;
  out[q] = gt * gx;
  out[np + q] = gt * gy;
  out[2 * np + q] = g * a.beta * (1.f - th * th) * gr;
}

// Backward gather, thread = one stored pixel (h, w).  When pooled, only the first maximal element (or last NaN) of its pool window goes on (the
// others and the dropped trailing rows / columns get 0).  Its map pixel p then adds, over every padded position i that the reflect
// padding maps to p (p itself, -1 for p == 1, n for p == n - 2) and every tap d, the coefficient of the output pixel i - d times the
// tap's weight: the transposed stencils, border rows and columns counted as often as the padding repeats them.
__global__ __launch_bounds__(256) void shock_gather_kernel(const float* __restrict__ x, const float* __restrict__ coef, float* __restrict__ dx,
                                                           long long total, const ShockArgs a) {
  const size_t np = (size_t)a.N * a.Hp * a.Wp;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int w = (int)(i % a.W), h = (int)((i / a.W) % a.H);
    const long long n = i / ((long long)a.W * a.H);
    const int py = h / a.pool, px = w / a.pool;
    bool mine = py < a.Hp && px < a.Wp;
    if (mine && a.pool > 1) {
      const float* p = x + n * a.H * a.W + (size_t)(py * a.pool) * a.W + px * a.pool;
      float m = p[0];
      int arg = 0;
      for (int r = 0; r < a.pool; ++r)
        for (int c = 0; c < a.pool; ++c) {
          const float v = p[r * a.W + c];
          if (v > m || v != v) { m = v; arg = r * a.pool + c; }
        }
      mine = arg == (h - py * a.pool) * a.pool + (w - px * a.pool);
    }
    float acc = 0.f;
    if (mine) {
      const float* c0 = coef + n * a.Hp * a.Wp;
#pragma unroll
      for (int sy = 0; sy < 3; ++sy) {
        const int iy = sy == 0 ? py : (sy == 1 ? -1 : a.Hp);
        if (!(sy == 0 || (sy == 1 && py == 1) || (sy == 2 && py == a.Hp - 2))) continue;
#pragma unroll
        for (int sx = 0; sx < 3; ++sx) {
          const int ix = sx == 0 ? px : (sx == 1 ? -1 : a.Wp);
          if (!(sx == 0 || (sx == 1 && px == 1) || (sx == 2 && px == a.Wp - 2))) continue;
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dxx = -1; dxx <= 1; ++dxx) {
              const int qy = iy - dy, qx = ix - dxx;
              if (qy < 0 || qy >= a.Hp || qx < 0 || qx >= a.Wp) continue;
              const size_t q = (size_t)qy * a.Wp + qx;
              const float kx = (dxx == 0 ? 0.f : (dxx < 0 ? 0.125f : -0.125f)) * (dy == 0 ? 2.f : 1.f);
              const float ky = (dy == 0 ? 0.f : (dy < 0 ? 0.125f : -0.125f)) * (dxx == 0 ? 2.f : 1.f);
              const float kl = (dy == 0 && dxx == 0) ? -4.f : ((dy == 0 || dxx == 0) ? 1.f : 0.f);
              if (dxx != 0) acc += kx * c0[q];
              if (dy != 0) acc += ky * c0[np + q];
              if (dy == 0 || dxx == 0) acc += kl * c0[2 * np + q];
            }
        }
      }
    }
    dx[i] = acc;
  }
}

// out[0] = sum of nb workgroup partials, in workgroup order
static int ext_reduce1(const float* part, int nb, float* out, hipStream_t s) {
  if (hipError_t e = memset_async(out, 0, sizeof(float), s)) { set_error("memset: %s", hipGetErrorString(e)); return (int)e; }
  return det_reduce(part, 1, nb, 0, 1, DetSegs{{out, nullptr, nullptr, nullptr}, {1, 0, 0, 0}}, s);
}
static int shock_args(ShockArgs& a, int N, int H, int W, int pool, int border, float beta, float eps) {
  P2I_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && pool >= 1 && border >= 0, "bad shock-map shape");
  a.N = N; a.H = H; a.W = W; a.pool = pool; a.m = border; a.beta = beta; a.eps = eps;
  a.Hp = H / pool; a.Wp = W / pool;
  P2I_REQUIRE(a.Hp >= 2 && a.Wp >= 2, "shock map: the reflect padding needs a (pooled) height and width of at least 2");
  P2I_REQUIRE(a.Hp - 2 * border >= 1 && a.Wp - 2 * border >= 1, "shock loss: border_ignore leaves nothing");
  P2I_REQUIRE((long long)N * H * W < (1ll << 31), "shock map: more than 2^31 elements");
  return P2I_OK;
}
static inline dim3 shock_grid(const ShockArgs& a) { return dim3(ceil_div(a.Wp, STW), ceil_div(a.Hp, STH), a.N); }

}  // namespace p2i
using namespace p2i;

#define EXT_VEC(n, ...) (((n) % 4 == 0) && aligned16_all(__VA_ARGS__))
template <typename... P> static inline bool aligned16_all(P... p) { return (aligned16(p) && ...); }

extern "C" int p2i_loss_transform_fwd(const float* x, float* y, int64_t n, void* stream) {
  P2I_REQUIRE(x && y && n > 0, "bad arguments");
  if (EXT_VEC(n, x, y)) P2I_LAUNCH(transform_kernel<4, false>, dim3(ext_grid(n / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
      x, nullptr, y, n / 4);
  else P2I_LAUNCH(transform_kernel<1, false>, dim3(ext_grid(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, x, nullptr, y, n);
  return launch_status();
}
extern "C" int p2i_loss_transform_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream) {
  P2I_REQUIRE(x && dy && dx && n > 0, "bad arguments");
  if (EXT_VEC(n, x, dy, dx)) P2I_LAUNCH(transform_kernel<4, true>, dim3(ext_grid(n / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
      x, dy, dx, n / 4);
  else P2I_LAUNCH(transform_kernel<1, true>, dim3(ext_grid(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, n);
  return launch_status();
}

extern "C" int p2i_fdiff_fwd(const float* x, float* out, int B, int T, int64_t inner, void* stream) {
  P2I_REQUIRE(x && out && B > 0 && T >= 2 && inner > 0, "forward difference needs T >= 2");
  const int64_t n = (int64_t)B * (T - 1) * inner;
  if (EXT_VEC(inner, x, out)) P2I_LAUNCH(fdiff_fwd_kernel<4>, dim3(ext_grid(n / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
      x, out, T, inner / 4, n / 4);
  else P2I_LAUNCH(fdiff_fwd_kernel<1>, dim3(ext_grid(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, x, out, T, inner, n);
  return launch_status();
}
extern "C" int p2i_fdiff_bwd(const float* dy, float* dx, int B, int T, int64_t inner, void* stream) {
  P2I_REQUIRE(dy && dx && B > 0 && T >= 2 && inner > 0, "forward difference needs T >= 2");
  const int64_t n = (int64_t)B * T * inner;
  if (EXT_VEC(inner, dy, dx)) P2I_LAUNCH(fdiff_bwd_kernel<4>, dim3(ext_grid(n / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
      dy, dx, T, inner / 4, n / 4);
  else P2I_LAUNCH(fdiff_bwd_kernel<1>, dim3(ext_grid(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, dy, dx, T, inner, n);
  return launch_status();
}

extern "C" int p2i_wl1_fwd(const float* pred, const float* target, float* out1, int64_t n, void* stream) {
  P2I_REQUIRE(pred && target && out1 && n > 0, "bad arguments");
  const bool vec = EXT_VEC(n, pred, target);
  const int nb = ext_grid(vec ? n / 4 : n, 256 * 4, 512);
  const DetWs ws = det_take((size_t)nb, 0);
  P2I_REQUIRE(ws.part, "no deterministic-reduction scratch registered (p2i_det_workspace)");
  if (vec) P2I_LAUNCH(wl1_fwd_kernel<4>, dim3(nb), dim3(256), 0, (hipStream_t)stream, pred, target, n / 4, 1.f / (float)n, ws.part);
  else P2I_LAUNCH(wl1_fwd_kernel<1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, pred, target, n, 1.f / (float)n, ws.part);
  return ext_reduce1(ws.part, nb, out1, (hipStream_t)stream);
}
extern "C" int p2i_wl1_bwd(const float* pred, const float* target, const float* gout, float* dpred, int64_t n, void* stream) {
  P2I_REQUIRE(pred && target && gout && dpred && n > 0, "bad arguments");
  if (EXT_VEC(n, pred, target, dpred)) P2I_LAUNCH(wl1_bwd_kernel<4>, dim3(ext_grid(n / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
      pred, target, gout, dpred, n / 4, 1.f / (float)n);
  else P2I_LAUNCH(wl1_bwd_kernel<1>, dim3(ext_grid(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, pred, target, gout, dpred, n, 1.f / (float)n);
  return launch_status();
}

extern "C" int p2i_softmax_t_fwd(const float* x, float* y, int rows, int L, float temperature, void* stream) {
  P2I_REQUIRE(x && y && rows > 0 && L > 0 && temperature != 0.f, "bad arguments");
  P2I_LAUNCH(softmax_t_fwd_kernel, dim3(rows), dim3(L >= 1024 ? 1024 : 256), 0, (hipStream_t)stream, x, y, L, 1.f / temperature);
  return launch_status();
}
extern "C" int p2i_softmax_t_bwd(const float* y, const float* dy, float* dx, int rows, int L, float temperature, void* stream) {
  P2I_REQUIRE(y && dy && dx && rows > 0 && L > 0 && temperature != 0.f, "bad arguments");
  P2I_LAUNCH(softmax_t_bwd_kernel, dim3(rows), dim3(L >= 1024 ? 1024 : 256), 0, (hipStream_t)stream, y, dy, dx, L, 1.f / temperature);
  return launch_status();
}

extern "C" int p2i_kl_fwd(const float* p, const float* q, float* out1, int64_t n, int B, void* stream) {
  P2I_REQUIRE(p && q && out1 && n > 0 && B > 0, "bad arguments");
  const bool vec = EXT_VEC(n, p, q);
  const int nb = ext_grid(vec ? n / 4 : n, 256 * 4, 512);
  const DetWs ws = det_take((size_t)nb, 0);
  P2I_REQUIRE(ws.part, "no deterministic-reduction scratch registered (p2i_det_workspace)");
  if (vec) P2I_LAUNCH(kl_fwd_kernel<4>, dim3(nb), dim3(256), 0, (hipStream_t)stream, p, q, n / 4, 1.f / (float)B, ws.part);
  else P2I_LAUNCH(kl_fwd_kernel<1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, p, q, n, 1.f / (float)B, ws.part);
  return ext_reduce1(ws.part, nb, out1, (hipStream_t)stream);
}
extern "C" int p2i_kl_bwd(const float* p, const float* q, const float* gout, float* dp, int64_t n, int B, void* stream) {
  P2I_REQUIRE(p && q && gout && dp && n > 0 && B > 0, "bad arguments");
  if (EXT_VEC(n, p, q, dp)) P2I_LAUNCH(kl_bwd_kernel<4>, dim3(ext_grid(n / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream,
      p, q, gout, dp, n / 4, 1.f / (float)B);
  else P2I_LAUNCH(kl_bwd_kernel<1>, dim3(ext_grid(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, p, q, gout, dp, n, 1.f / (float)B);
  return launch_status();
}

extern "C" int p2i_spool_fwd(const float* x, float* out, int* idx, int N, int H, int W, void* stream) {
  P2I_REQUIRE(x && out && N > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "bad arguments");
  const int Ho = (H - 1) / 4 + 1, Wo = (W - 1) / 4 + 1;
  const long long total = (long long)N * Ho * Wo;
  P2I_LAUNCH(spool_fwd_kernel, dim3(ext_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, out, idx, total, H, W, Ho, Wo);
  return launch_status();
}
extern "C" int p2i_spool_bwd(const int* idx, const float* dout, const float* scale, float* dx, int N, int H, int W, void* stream) {
  P2I_REQUIRE(idx && dout && dx && N > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "bad arguments");
  const int Ho = (H - 1) / 4 + 1, Wo = (W - 1) / 4 + 1;
  const long long total = (long long)N * H * W;
  P2I_LAUNCH(spool_bwd_kernel, dim3(ext_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, idx, dout, scale, dx, total, H, W, Ho, Wo);
  return launch_status();
}

extern "C" int p2i_tdm_fwd(const float* pred_diff, const float* true_diff, const float* truth, float beta, float eps, float* out1,
                           float* coef, int* idx, int B, int Tm1, int H, int W, void* stream) {
  P2I_REQUIRE(pred_diff && true_diff && truth && out1 && (!coef == !idx), "bad arguments");
  P2I_REQUIRE(B > 0 && Tm1 > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "bad shape");
  const int Ho = (H - 1) / 4 + 1, Wo = (W - 1) / 4 + 1;
  const long long total = (long long)B * Tm1 * Ho * Wo;
  const int nb = ext_grid(total, 256, 512);
  const DetWs ws = det_take((size_t)nb, 0);
  P2I_REQUIRE(ws.part, "no deterministic-reduction scratch registered (p2i_det_workspace)");
  P2I_LAUNCH(tdm_fwd_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, pred_diff, true_diff, truth, total, Tm1, H, W, Ho, Wo, beta, eps,
             1.f / (float)total, ws.part, coef, idx);
  return ext_reduce1(ws.part, nb, out1, (hipStream_t)stream);
}

extern "C" int p2i_shock_map_fwd(const float* x, float* out, int N, int H, int W, float beta, float eps, void* stream) {
  P2I_REQUIRE(x && out, "null pointer");
  ShockArgs a;
  if (int e = shock_args(a, N, H, W, 1, 0, beta, eps)) return e;
  P2I_LAUNCH(shock_tile_kernel<0>, shock_grid(a), dim3(STW * STH), 0, (hipStream_t)stream, x, nullptr, nullptr, out, a);
  return launch_status();
}
extern "C" int p2i_shock_map_bwd(const float* x, const float* dout, float* dx, float* scratch, int N, int H, int W, float beta, float eps,
                                 void* stream) {
  P2I_REQUIRE(x && dout && dx && scratch, "null pointer");
  ShockArgs a;
  if (int e = shock_args(a, N, H, W, 1, 0, beta, eps)) return e;
  const long long total = (long long)N * H * W;
  P2I_LAUNCH(shock_tile_kernel<2>, shock_grid(a), dim3(STW * STH), 0, (hipStream_t)stream, x, nullptr, dout, scratch, a);
  P2I_LAUNCH(shock_gather_kernel, dim3(ext_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, scratch, dx, total, a);
  return launch_status();
}
extern "C" int p2i_shock_loss_fwd(const float* pred, const float* truth, float* out, int N, int H, int W, int pool, int border, float beta,
                                  float eps, void* stream) {
  P2I_REQUIRE(pred && truth && out, "null pointer");
  ShockArgs a;
  if (int e = shock_args(a, N, H, W, pool, border, beta, eps)) return e;
  P2I_LAUNCH(shock_tile_kernel<1>, shock_grid(a), dim3(STW * STH), 0, (hipStream_t)stream, pred, truth, nullptr, out, a);
  return launch_status();
}
extern "C" int p2i_shock_loss_bwd(const float* pred, const float* truth, const float* dout, float* dpred, float* scratch, int N, int H,
                                  int W, int pool, int border, float beta, float eps, void* stream) {
  P2I_REQUIRE(pred && truth && dout && dpred && scratch, "null pointer");
  ShockArgs a;
  if (int e = shock_args(a, N, H, W, pool, border, beta, eps)) return e;
  const long long total = (long long)N * H * W;
  P2I_LAUNCH(shock_tile_kernel<3>, shock_grid(a), dim3(STW * STH), 0, (hipStream_t)stream, pred, truth, dout, scratch, a);
  P2I_LAUNCH(shock_gather_kernel, dim3(ext_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, pred, scratch, dpred, total, a);
  return launch_status();
}
