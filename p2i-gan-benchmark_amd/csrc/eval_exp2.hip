// The benchmark's exp2 comparison renders (reference experiments/exp2.py run_exp2 / _save_combo_gif, run_exp2_paper_zarr) on the
// device; DESIGN.md section 12.
//   p2i_exp2_index   : the first n frames of a raw event [T, H, W], center-cropped to S x S, transformed as in exp1
//                      (eval_common.h) and looked up in the colour table's 142 fp64 bounds (held in LDS):
//                      index = clip(searchsorted_right(bounds, v) - 1, 0, 140), decided by fp64 >= compares; NaN -> P2I_EXP2_BAD.
//                      One 4-byte word of the output per lane, one packed store; the output needs no alignment.
//   p2i_exp2_compose : index panels [P, n, S, S] -> GIF canvases [n, Hc, pitch] of palette indices.  Under everything lies the
//                      event's static chrome [Hc, pitch] (titles, colour bar: rasterised once on the host); panel p covers the
//                      S*zoom square at (oy, ox + p * step), every source pixel magnified zoom x zoom.  A gauge panel (bit p of
//                      gauge_bits) is the background index plus one disc per mask point in the order given, coloured by the
//                      panel's own index at that point; where discs overlap the later point wins.  No atomics: every pixel
//                      scans the point list (staged through LDS) and keeps its last hit.  16 canvas pixels per lane, one
//                      16-byte store; pitch is a multiple of 16.
// The disc rule (integers, in doubled canvas coordinates so that pixel and cell centers are whole numbers): point (py, px) has
// its center at (cy, cx) = ((2 py + 1) zoom, (2 px + 1) zoom); canvas pixel (y, x) of the panel lies at (2 y + 1, 2 x + 1);
// d2 = (2 y + 1 - cy)^2 + (2 x + 1 - cx)^2.  With R = 3 zoom: d2 <= (R - 2)^2 is the disc's face, (R - 2)^2 < d2 <= R^2 its
// one-pixel edge ring.  At zoom 1 a disc is the point's pixel with the 8 pixels around it as edge.
// Compiled with -ffp-contract=off: the transform rounds as numpy's separate operations do (as in eval_exp1.hip).
#include "eval_common.h"

namespace p2i {

constexpr int NB = P2I_EXP2_NBOUNDS;      // 142 bounds, 141 colours
constexpr int BAD = P2I_EXP2_BAD;
constexpr int PCHUNK = 512;               // mask points staged per LDS round
static_assert(NB == 142 && BAD == NB - 1, "exp2 layout");

// np.digitize(v, bounds) - 1 clipped to [0, NB - 2]: the number of bounds <= v by bisection on fp64 compares
__device__ __forceinline__ int bound_index(const double* b, double v) {
  if (v != v) return BAD;
  int lo = 0, hi = NB;                    // bounds[i] <= v for i < lo, bounds[i] > v for i >= hi
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (v >= b[m]) lo = m + 1;
    else hi = m;
  }
  const int i = lo - 1;
  return i < 0 ? 0 : (i > NB - 2 ? NB - 2 : i);
}

template <typename T>
__global__ __launch_bounds__(256) void exp2_index_kernel(Crop<T> x, int S, long long total, const double* __restrict__ bounds,
                                                         const double* __restrict__ lut, int div3, uint8_t* __restrict__ out) {
  __shared__ double b[NB];
  if ((int)threadIdx.x < NB) b[threadIdx.x] = bounds[threadIdx.x];
  __syncthreads();
  // a lane owns one 4-byte word of the output's memory: with the output `shift` bytes past a word boundary, lane q covers
  // outputs [4 q - shift, 4 q - shift + 4), clipped to [0, total).  A whole word is one packed store; the clipped words of a
  // misaligned head and of the tail are byte stores
  const int shift = (int)((uintptr_t)out & 3u);
  const long long q0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4 - shift;
  const long long o0 = q0 < 0 ? 0 : q0;
  const long long o1 = q0 + 4 < total ? q0 + 4 : total;
  if (o0 >= o1) return;
  const long long ss = (long long)S * S;
  uint32_t pack = 0;
  const int cnt = (int)(o1 - o0);
  for (int j = 0; j < cnt; ++j) {
    const long long o = o0 + j;
    const long long t = o / ss;
    const int r = (int)(o - t * ss);
    const int y = r / S, xx = r - y * S;
    const double v = x.at(t, y, xx, lut, div3);
    pack |= (uint32_t)bound_index(b, v) << (8 * j);
  }
  if (cnt == 4) {
    *reinterpret_cast<uint32_t*>(out + o0) = pack;       // o0 == q0, and out + q0 is on a word boundary
  } else {
    for (int j = 0; j < cnt; ++j) out[o0 + j] = (uint8_t)(pack >> (8 * j));
  }
}

// grid (pitch / 16 / 64 rounded up, Hc, n); lane -> 16 consecutive canvas pixels of row blockIdx.y of frame blockIdx.z
__global__ __launch_bounds__(64) void exp2_compose_kernel(const uint8_t* __restrict__ panels, int P, int n, int S, int zoom,
                                                          unsigned gauge_bits, const int* __restrict__ points, int K,
                                                          const uint8_t* __restrict__ chrome, int Hc, int pitch, int oy, int ox,
                                                          int step, int bg, int edge, uint8_t* __restrict__ out) {
  __shared__ int pts[PCHUNK * 2];
  const int t = blockIdx.z, y = blockIdx.y;
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * 16;
  const bool live = x0 < pitch;
  const int side = S * zoom;
  const int ry = y - oy;
  const bool in_rows = ry >= 0 && ry < side;
  uint8_t px[16];
  int hit[16];                     // gauge pixels: -1 none, else 2 * k + (1 if edge)
  bool gauge_px[16];
  if (live) {
    const uint4 c = *reinterpret_cast<const uint4*>(chrome + (long long)y * pitch + x0);
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      px[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
      hit[j] = -1;
      gauge_px[j] = false;
    }
    if (in_rows) {
      const int sy = ry / zoom;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int rx = x0 + j - ox;
        if (rx < 0) continue;
        const int p = rx / step, cx = rx - p * step;
        if (p >= P || cx >= side) continue;
        if ((gauge_bits >> p) & 1u) {
          px[j] = (uint8_t)bg;
          gauge_px[j] = true;
        } else {
          px[j] = panels[(((long long)p * n + t) * S + sy) * S + cx / zoom];
        }
      }
    }
  }
  // every lane of the workgroup walks the point list together (the LDS rounds have barriers); only rows that cross a gauge
  // panel need it, which is uniform over the workgroup's row
  if (gauge_bits != 0u && in_rows) {
    const int R = 3 * zoom, r_out = R * R, r_in = (R - 2) * (R - 2);
    const int Y2 = 2 * ry + 1;
    for (int k0 = 0; k0 < K; k0 += PCHUNK) {
      const int kc = K - k0 < PCHUNK ? K - k0 : PCHUNK;
      __syncthreads();
      for (int i = threadIdx.x; i < kc * 2; i += 64) pts[i] = points[(long long)k0 * 2 + i];
      __syncthreads();
      if (!live) continue;
      for (int k = 0; k < kc; ++k) {
        const int dy = Y2 - (2 * pts[2 * k] + 1) * zoom;
        const int dy2 = dy * dy;
        if (dy2 > r_out) continue;
        const int cx2 = (2 * pts[2 * k + 1] + 1) * zoom;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          if (!gauge_px[j]) continue;
          const int rx = x0 + j - ox;
          const int dx = 2 * (rx % step) + 1 - cx2;
          const int d2 = dy2 + dx * dx;
          if (d2 <= r_out) hit[j] = 2 * (k0 + k) + (d2 > r_in ? 1 : 0);
        }
      }
    }
    if (live) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (hit[j] < 0) continue;
        if (hit[j] & 1) {
          px[j] = (uint8_t)edge;
        } else {
          const int k = hit[j] >> 1;
          const int p = (x0 + j - ox) / step;
          const int pr = points[2 * k], pc = points[2 * k + 1];
          if ((unsigned)pr >= (unsigned)S || (unsigned)pc >= (unsigned)S) continue;      // never read outside the panel
          const uint8_t c = panels[(((long long)p * n + t) * S + pr) * S + pc];
          if (c != BAD) px[j] = c;               // a NaN observation has a transparent face: the background shows
        }
      }
    }
  }
  if (live) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j >> 2] |= (uint32_t)px[j] << (8 * (j & 3));
    *reinterpret_cast<uint4*>(out + ((long long)t * Hc + y) * pitch + x0) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace p2i

using namespace p2i;

extern "C" int p2i_exp2_index(const p2i_eval_input* in, int T, int S, int n, const double* bounds, const double* lut, int divide_by_3,
                              uint8_t* out, void* stream) {
  P2I_REQUIRE(input_set(in) && bounds && lut && out && eval_dtype_ok(in->dtype), "bad arguments");
  P2I_REQUIRE(S > 0 && n > 0 && n <= T, "bad frame count / crop");
  P2I_REQUIRE(crop_ok(in, S, S), "crop outside the input");
  const long long total = (long long)n * S * S;
  const long long blocks = (total + (long long)((uintptr_t)out & 3u) + 1023) / 1024;
  P2I_REQUIRE(blocks <= 0x7fffffffLL, "too many pixels for one launch");
  const hipStream_t s = (hipStream_t)stream;
  dispatch1(in, [&](auto x) {
    P2I_LAUNCH(exp2_index_kernel<Elem<decltype(x)>>, dim3((unsigned)blocks), dim3(256), 0, s, x, S, total, bounds, lut, divide_by_3, out);
  });
  return launch_status();
}

extern "C" int p2i_exp2_compose(const uint8_t* panels, int P, int n, int S, int zoom, unsigned gauge_bits, const int* points, int K,
                                const uint8_t* chrome, int Hc, int pitch, int oy, int ox, int step, int bg, int edge, uint8_t* out,
                                void* stream) {
  P2I_REQUIRE(panels && chrome && out && (K == 0 || points), "bad arguments");
  P2I_REQUIRE(P >= 1 && P <= 32 && n >= 1 && n <= 65535 && S >= 1 && zoom >= 1 && K >= 0, "bad panel count / frames / zoom");
  P2I_REQUIRE((long long)S * zoom <= 1 << 20 && step >= S * zoom, "bad panel step");
  P2I_REQUIRE(Hc >= 1 && Hc <= 65535 && pitch >= 16 && pitch % 16 == 0, "bad canvas (the pitch is a multiple of 16)");
  P2I_REQUIRE(oy >= 0 && ox >= 0 && oy + S * zoom <= Hc && (long long)ox + (long long)(P - 1) * step + S * zoom <= pitch,
              "panels outside the canvas");
  P2I_REQUIRE(P == 32 || (gauge_bits >> P) == 0u, "gauge bit beyond the panels");
  P2I_REQUIRE(bg >= 0 && bg < 256 && edge >= 0 && edge < 256, "bad palette index");
  P2I_REQUIRE((((uintptr_t)out | (uintptr_t)chrome) & 15u) == 0, "canvas is not 16-byte aligned");
  P2I_LAUNCH(exp2_compose_kernel, dim3((unsigned)ceil_div(pitch / 16, 64), (unsigned)Hc, (unsigned)n), dim3(64), 0, (hipStream_t)stream,
             panels, P, n, S, zoom, gauge_bits, points, K, chrome, Hc, pitch, oy, ox, step, bg, edge, out);
  return launch_status();
}
