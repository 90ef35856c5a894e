// Object-based verification of inference outputs on the device: connected-component labelling of thresholded rain frames and the
// integer moments of every object, for SAL (Wernli et al. 2008) and the object population; DESIGN.md section 23.  Inputs are exp1's
// (Crop<T> / tload of eval_common.h); every pixel of the crop counts, there is no mask.  Everything written is an integer:
//   Q = rint(R * 2^24) of the transformed pixel R (mm/h, 0 .. 200): Q < 2^32, and with y, x < 2^10 over at most 2^20 pixels every
//   sum below (area, sum Q, sum Q y, sum Q x) stays under 200 * 2^24 * 2^10 * 2^20 < 2^62.  Integer sums have no order, so the
//   results do not depend on the grid, the path or the run.
//   p2i_objects_quantize : per (frame, field) once: Q of every crop pixel, the level bits (bit j: R >= threshold j; bit nthr:
//                          R >= R* = max(factor * Rmax, floor) with Rmax the crop's own maximum; NaN compares false and has Q = 0),
//                          and the record sum Q, sum Q y, sum Q x over all pixels, max Q, NaN flag.
//   p2i_objects_label    : per (frame, field, level) the canonical labels: a pixel of an object holds the smallest raster index
//                          y * S + x of the object's pixels, any other pixel all ones.  Union-find with atomic-min links (Komura
//                          2015; Playne & Hawick 2018): a link always points from a larger index to a smaller one, so the root is
//                          the minimum whatever the execution order.  Crops up to P2I_OBJECTS_LDS_CROP take one workgroup each with
//                          16-bit labels in pitched LDS rows; larger ones label P2I_OBJECTS_TILE^2 tiles in LDS, write 32-bit labels
//                          to the caller's workspace, unite across the tile borders there and flatten once.
//   p2i_objects_count    : per (frame, field, level) the number of objects, their total area and sum Q, sum Q y, sum Q x over them.
//   p2i_objects_scan     : the exclusive prefix of the counts (the object table's offsets) and their total.
//   p2i_objects_fill     : the compact object table, six int64 per object (label, area, sum Q, max Q, sum Q y, sum Q x) in ascending
//                          label order.  Moments are added with 64-bit integer atomics: in LDS slots while a record's objects fit
//                          them, in the (zeroed) table otherwise.  Destroys the labels.
#include "eval_common.h"

namespace p2i {

constexpr int OXK = P2I_EXP1_MAX_THR;
constexpr int OLS = P2I_OBJECTS_LDS_CROP;
constexpr int OTILE = P2I_OBJECTS_TILE;
constexpr int OSLOTS = 1024;      // LDS accumulation slots of the fill (5 x 8 bytes each)
constexpr int OSTRIP = 8;         // consecutive pixels per thread in the fill
typedef unsigned long long u64;

struct OThr { double v[OXK]; int k; };

// 16-bit elements per LDS row: an odd number of dwords, so a column walk meets distinct banks
static inline __host__ __device__ constexpr int obj_pitch(int tile) {
  int dw = (tile + 1) / 2;
  if (!(dw & 1)) ++dw;
  return 2 * dw;
}

__device__ __forceinline__ u64 owave_sum(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// thread 0 gets the workgroup's sums of N values per thread; red: N * 4 words of LDS.  Every thread calls it.
template <int N> __device__ __forceinline__ void oblock_sum(u64 (&v)[N], u64* red) {
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = owave_sum(v[j]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) red[(threadIdx.x >> 6) * N + j] = v[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = red[j] + red[N + j] + red[2 * N + j] + red[3 * N + j];
  }
  __syncthreads();
}

// exclusive prefix of v over the 256 threads, and their total; ws: 4 words of LDS.  Every thread calls it.
__device__ __forceinline__ u64 oblock_scan(u64 v, u64* ws, u64& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  u64 inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const u64 up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  u64 before = 0;
  for (int j = 0; j < wv; ++j) before += ws[j];
  total = ws[0] + ws[1] + ws[2] + ws[3];
  __syncthreads();
  return before + inc - v;
}

// grid (T), 256 threads; field 0 = prediction, 1 = truth.  q, bits: [T][2][S * S]; rec: [T][2][5]
template <typename T>
__global__ __launch_bounds__(256) void objects_quantize_kernel(Crop<T> in, int S, int field, const double* __restrict__ lut, OThr thr,
                                                               double factor, double floor_, int div3, uint32_t* __restrict__ q,
                                                               uint16_t* __restrict__ bits, long long* __restrict__ rec) {
  __shared__ u64 red[4 * 5];
  __shared__ double rmax[4];
  const long long t = blockIdx.x;
  const long long base = (t * 2 + field) * (long long)S * S;
  u64 s[5] = {0, 0, 0, 0, 0};      // sum Q, sum Q y, sum Q x, then NaN pixels and a spare word
  double rm = 0.0;
  for (int i = threadIdx.x; i < S * S; i += 256) {
    const int y = i / S, x = i - y * S;
    const double r = in.at(t, y, x, lut, div3);
    const bool nan = r != r;
    const unsigned qq = nan ? 0u : (unsigned)(long long)rint(r * 16777216.0);
    unsigned b = 0;
#pragma unroll
    for (int j = 0; j < OXK; ++j)
      if (j < thr.k && r >= thr.v[j]) b |= 1u << j;
    q[base + i] = qq;
    bits[base + i] = (uint16_t)b;
    s[0] += qq;
    s[1] += (u64)qq * (unsigned)y;
    s[2] += (u64)qq * (unsigned)x;
    s[3] += nan ? 1 : 0;
    if (r > rm) rm = r;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_down(rm, o, 64);
    if (other > rm) rm = other;
  }
  if ((threadIdx.x & 63) == 0) rmax[threadIdx.x >> 6] = rm;
  s[4] = 0;
  oblock_sum<5>(s, red);      // its barriers publish rmax as well
  // max Q = rint(Rmax * 2^24): rint is monotonic, so the maximum of the Q is the Q of the maximum
  rm = fmax(fmax(rmax[0], rmax[1]), fmax(rmax[2], rmax[3]));
  if (threadIdx.x == 0) {
    long long* o = rec + (t * 2 + field) * 5;
    o[0] = (long long)s[0];
    o[1] = (long long)s[1];
    o[2] = (long long)s[2];
    o[3] = (long long)rint(rm * 16777216.0);
    o[4] = s[3] ? 1 : 0;
  }
  const double rstar = fmax(factor * rm, floor_);
  for (int i = threadIdx.x; i < S * S; i += 256) {
    const int y = i / S, x = i - y * S;
    const double r = in.at(t, y, x, lut, div3);
    if (r >= rstar) bits[base + i] |= (uint16_t)(1u << thr.k);      // the thread's own element of the first pass
  }
}

// ---- union-find on 16-bit labels in LDS: a label is the pitched position of a pixel's parent ----
__device__ __forceinline__ unsigned find16(const volatile uint16_t* lab, unsigned p) {
  unsigned n;
  while ((n = lab[p]) != p) p = n;
  return p;
}

// lab[i] = min(lab[i], v) through a compare-and-swap of the dword that holds it; returns the old lab[i]
__device__ __forceinline__ unsigned min16(unsigned* lab32, unsigned i, unsigned v) {
  unsigned* w = lab32 + (i >> 1);
  const unsigned sh = (i & 1) * 16;
  unsigned old = *(volatile unsigned*)w;
  for (;;) {
    const unsigned cur = (old >> sh) & 0xffffu;
    if (cur <= v) return cur;
    const unsigned prev = atomicCAS(w, old, (old & ~(0xffffu << sh)) | (v << sh));
    if (prev == old) return cur;
    old = prev;
  }
}

__device__ __forceinline__ void unite16(unsigned* lab32, unsigned a, unsigned b) {
  const volatile uint16_t* lab = (const volatile uint16_t*)lab32;
  for (;;) {
    a = find16(lab, a);
    b = find16(lab, b);
    if (a == b) return;
    if (a < b) {
      const unsigned c = a;
      a = b;
      b = c;
    }
    const unsigned old = min16(lab32, a, b);      // link the larger root under the smaller
    if (old == a) return;
    a = old;      // a had a parent by then: it may have been replaced by b, so old and b are united next
  }
}

// ---- the same on 32-bit labels in global memory: a label is the raster index of a pixel's parent ----
__device__ __forceinline__ unsigned gload(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ unsigned find32(const unsigned* lab, unsigned p) {
  unsigned n;
  while ((n = gload(lab + p)) != p) p = n;
  return p;
}

__device__ __forceinline__ void unite32(unsigned* lab, unsigned a, unsigned b) {
  for (;;) {
    a = find32(lab, a);
    b = find32(lab, b);
    if (a == b) return;
    if (a < b) {
      const unsigned c = a;
      a = b;
      b = c;
    }
    const unsigned old = atomicMin(lab + a, b);
    if (old == a) return;
    a = old;
  }
}

// grid (ntfl * tiles^2), 256 threads, tiles = ceil(S / TILE); tfl = (frame * 2 + field) * nlev + level.  Labels the tile's pixels
// among themselves and writes labels[tfl][y][x] = the raster index of the tile-local root (all ones off the level's mask).  A tile's
// raster order is the crop's, so the local minimum is the smallest raster index of the local component.
template <typename LT, int TILE>
__global__ __launch_bounds__(256) void objects_label_kernel(const uint16_t* __restrict__ bits, int S, int nlev, int conn8,
                                                            LT* __restrict__ labels) {
  constexpr int PITCH = obj_pitch(TILE);
  constexpr unsigned NONE = 0xffffu;
  __shared__ unsigned lab32[TILE * PITCH / 2];
  volatile uint16_t* lab = (volatile uint16_t*)lab32;
  const int tiles = (S + TILE - 1) / TILE;
  const int tile = blockIdx.x % (tiles * tiles);
  const long long tfl = blockIdx.x / (tiles * tiles);
  const int level = (int)(tfl % nlev);
  const long long tf = tfl / nlev;
  const int y0 = (tile / tiles) * TILE, x0 = (tile % tiles) * TILE;
  const int th = min(TILE, S - y0), tw = min(TILE, S - x0);
  const uint16_t* b = bits + tf * S * S;
  LT* out = labels + tfl * S * S;
  for (int i = threadIdx.x; i < th * tw; i += 256) {
    const int ly = i / tw, lx = i - ly * tw;
    const unsigned pos = ly * PITCH + lx;
    lab[pos] = (uint16_t)(((b[(y0 + ly) * S + x0 + lx] >> level) & 1) ? pos : NONE);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < th * tw; i += 256) {
    const int ly = i / tw, lx = i - ly * tw;
    const unsigned pos = ly * PITCH + lx;
    if (lab[pos] == NONE) continue;
    if (lx > 0 && lab[pos - 1] != NONE) unite16(lab32, pos, pos - 1);
    if (ly > 0) {
      if (lab[pos - PITCH] != NONE) unite16(lab32, pos, pos - PITCH);
      else if (conn8) {      // with the pixel above set, its own left neighbour test ties both diagonals to it
        if (lx > 0 && lab[pos - PITCH - 1] != NONE) unite16(lab32, pos, pos - PITCH - 1);
        if (lx + 1 < tw && lab[pos - PITCH + 1] != NONE) unite16(lab32, pos, pos - PITCH + 1);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < th * tw; i += 256) {
    const int ly = i / tw, lx = i - ly * tw;
    const unsigned pos = ly * PITCH + lx;
    LT v = (LT)~(LT)0;
    if (lab[pos] != NONE) {
      const unsigned r = find16(lab, pos);
      const unsigned ry = r / PITCH, rx = r - ry * PITCH;
      v = (LT)((y0 + ry) * S + x0 + rx);
    }
    out[(y0 + ly) * S + x0 + lx] = v;
  }
}

// grid (ntfl * ceil(S^2 / 256)), 256 threads: unites every set pixel with its set backward neighbours (left, and above: left, mid,
// right) that lie in another tile
__global__ __launch_bounds__(256) void objects_merge_kernel(unsigned* __restrict__ labels, int S, int conn8) {
  const int per = (S * S + 255) / 256;
  const long long tfl = blockIdx.x / per;
  const int i = (blockIdx.x % per) * 256 + threadIdx.x;
  if (i >= S * S) return;
  const int y = i / S, x = i - y * S;
  const int my = y % OTILE, mx = x % OTILE;
  if (my != 0 && mx != 0 && mx != OTILE - 1) return;
  unsigned* lab = labels + tfl * S * S;
  if (lab[i] == 0xffffffffu) return;      // whether a pixel is set never changes
  if (mx == 0 && x > 0 && lab[i - 1] != 0xffffffffu) unite32(lab, i, i - 1);
  if (y > 0) {
    if (my == 0 && lab[i - S] != 0xffffffffu) unite32(lab, i, i - S);
    if (conn8) {
      if (x > 0 && (my == 0 || mx == 0) && lab[i - S - 1] != 0xffffffffu) unite32(lab, i, i - S - 1);
      if (x + 1 < S && (my == 0 || mx == OTILE - 1) && lab[i - S + 1] != 0xffffffffu) unite32(lab, i, i - S + 1);
    }
  }
}

// grid (ceil(n / 256)): every set pixel takes its root.  A concurrent writer only replaces a parent by its root.
__global__ __launch_bounds__(256) void objects_flatten_kernel(unsigned* __restrict__ labels, long long n, int S) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  const long long ss = (long long)S * S;
  unsigned* lab = labels + (g / ss) * ss;
  const unsigned i = (unsigned)(g % ss);
  if (gload(lab + i) == 0xffffffffu) return;
  const unsigned r = find32(lab, i);
  __hip_atomic_store(lab + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ntfl), 256 threads.  lev[tfl][5] = objects, area, sum Q, sum Q y, sum Q x over the level's set pixels; counts[tfl] = objects
template <typename LT>
__global__ __launch_bounds__(256) void objects_count_kernel(const LT* __restrict__ labels, const uint32_t* __restrict__ q, int S, int nlev,
                                                            long long* __restrict__ lev, long long* __restrict__ counts) {
  __shared__ u64 red[4 * 5];
  const long long tfl = blockIdx.x;
  const LT* lab = labels + tfl * S * S;
  const uint32_t* qq = q + (tfl / nlev) * S * S;
  u64 s[5] = {0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < S * S; i += 256) {
    const LT v = lab[i];
    if (v == (LT)~(LT)0) continue;
    const int y = i / S, x = i - y * S;
    const u64 w = qq[i];
    s[0] += v == (LT)i ? 1 : 0;
    s[1] += 1;
    s[2] += w;
    s[3] += w * (unsigned)y;
    s[4] += w * (unsigned)x;
  }
  oblock_sum<5>(s, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 5; ++j) lev[tfl * 5 + j] = (long long)s[j];
    counts[tfl] = (long long)s[0];
  }
}

// one workgroup of 256: offsets[i] = counts[0] + .. + counts[i - 1], offsets[n] = the total
__global__ __launch_bounds__(256) void objects_scan_kernel(const long long* __restrict__ counts, long long n,
                                                           long long* __restrict__ offsets) {
  __shared__ u64 ws[4];
  u64 carry = 0;
  for (long long b = 0; b < n; b += 256) {
    const long long i = b + threadIdx.x;
    const u64 v = i < n ? (u64)counts[i] : 0;
    u64 total;
    const u64 ex = oblock_scan(v, ws, total);
    if (i < n) offsets[i] = (long long)(carry + ex);
    carry += total;
  }
  if (threadIdx.x == 0) offsets[n] = (long long)carry;
}

// one object's moments of a run of pixels into its slot: area, sum Q, max Q, sum Q y, sum Q x
__device__ __forceinline__ void oflush(u64* dst, u64 area, u64 sq, u64 mq, u64 sy, u64 sx) {
  atomicAdd(dst + 0, area);
  atomicAdd(dst + 1, sq);
  atomicMax(dst + 2, mq);
  atomicAdd(dst + 3, sy);
  atomicAdd(dst + 4, sx);
}

// grid (ntfl), 256 threads.  Roots are ranked in raster order (a thread takes OSTRIP consecutive pixels, a workgroup pass 256 strips);
// the root's label is replaced by its rank under the top bit, which every pixel of the object then finds through its label.
template <typename LT>
__global__ __launch_bounds__(256) void objects_fill_kernel(LT* __restrict__ labels, const uint32_t* __restrict__ q, int S, int nlev,
                                                           const long long* __restrict__ offsets, long long rows,
                                                           long long* __restrict__ table) {
  constexpr LT NONE = (LT)~(LT)0;
  constexpr LT FLAG = (LT)((LT)1 << (8 * sizeof(LT) - 1));
  __shared__ u64 slots[OSLOTS * 5];
  __shared__ u64 ws[4];
  const long long tfl = blockIdx.x;
  const long long off = offsets[tfl];
  const long long n = offsets[tfl + 1] - off;
  if (n <= 0 || off < 0 || off + n > rows) return;      // uniform over the workgroup
  LT* lab = labels + tfl * S * S;
  const uint32_t* qq = q + (tfl / nlev) * S * S;
  const int npix = S * S;
  u64 carry = 0;
  for (int b = 0; b < npix; b += 256 * OSTRIP) {
    const int i0 = b + threadIdx.x * OSTRIP;
    u64 mine = 0;
    for (int j = 0; j < OSTRIP; ++j)
      if (i0 + j < npix && lab[i0 + j] == (LT)(i0 + j)) ++mine;
    u64 total;
    u64 rank = carry + oblock_scan(mine, ws, total);
    for (int j = 0; j < OSTRIP; ++j)
      if (i0 + j < npix && lab[i0 + j] == (LT)(i0 + j)) {
        table[(off + (long long)rank) * 6] = i0 + j;
        lab[i0 + j] = (LT)(FLAG | (LT)rank);
        ++rank;
      }
    carry += total;
  }
  const bool in_lds = n <= OSLOTS;
  if (in_lds)
    for (int i = threadIdx.x; i < (int)n * 5; i += 256) slots[i] = 0;
  __syncthreads();
  u64* gdst = (u64*)table + off * 6 + 1;
  for (int b = 0; b < npix; b += 256 * OSTRIP) {
    const int i0 = b + threadIdx.x * OSTRIP;
    long long cur = -1;
    u64 area = 0, sq = 0, mq = 0, sy = 0, sx = 0;
    for (int j = 0; j < OSTRIP; ++j) {
      const int i = i0 + j;
      if (i >= npix) break;
      const LT v = lab[i];
      if (v == NONE) continue;
      const long long rank = (long long)(LT)(((v & FLAG) ? v : lab[v]) & (LT)~FLAG);
      if (rank != cur) {
        if (cur >= 0) {
          if (in_lds) oflush(slots + cur * 5, area, sq, mq, sy, sx);
          else oflush(gdst + cur * 6, area, sq, mq, sy, sx);
        }
        cur = rank;
        area = sq = mq = sy = sx = 0;
      }
      const int y = i / S, x = i - y * S;
      const u64 w = qq[i];
      area += 1;
      sq += w;
      mq = w > mq ? w : mq;
      sy += w * (unsigned)y;
      sx += w * (unsigned)x;
    }
    if (cur >= 0) {
      if (in_lds) oflush(slots + cur * 5, area, sq, mq, sy, sx);
      else oflush(gdst + cur * 6, area, sq, mq, sy, sx);
    }
  }
  if (in_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < (int)n * 5; i += 256) gdst[(i / 5) * 6 + i % 5] = slots[i];
  }
}

static inline bool objects_sizes_ok(int T, int S, int nlev) {
  return T > 0 && S > 0 && S <= P2I_OBJECTS_MAX_CROP && nlev > 0 && nlev <= OXK + 1;
}

}  // namespace p2i

using namespace p2i;

extern "C" int p2i_objects_quantize(const p2i_eval_input* in, int T, int S, int field, const double* lut, const double* thresholds_host,
                                    int nthr, double sal_factor, double sal_floor, int divide_by_3, uint32_t* q, uint16_t* bits,
                                    int64_t* rec, void* stream) {
  P2I_REQUIRE(input_set(in) && lut && thresholds_host && q && bits && rec && eval_dtype_ok(in->dtype), "bad arguments");
  P2I_REQUIRE(T > 0 && S > 0 && S <= P2I_OBJECTS_MAX_CROP && (field == 0 || field == 1), "bad frame count / crop / field");
  P2I_REQUIRE(crop_ok(in, S, S), "crop outside the input");
  P2I_REQUIRE(nthr > 0 && nthr <= OXK, "1 to %d thresholds", OXK);
  P2I_REQUIRE(sal_factor > 0.0 && sal_factor <= 1.0 && sal_floor >= 0.0, "the relative level takes a factor in (0, 1] and a floor >= 0");
  OThr thr;
  thr.k = nthr;
  for (int i = 0; i < OXK; ++i) thr.v[i] = i < nthr ? thresholds_host[i] : 0.0;
  dispatch1(in, [&](auto x) {
    P2I_LAUNCH((objects_quantize_kernel<Elem<decltype(x)>>), dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, x, S, field, lut, thr,
               sal_factor, sal_floor, divide_by_3, q, bits, (long long*)rec);
  });
  return launch_status();
}

extern "C" int p2i_objects_label(const uint16_t* bits, int T, int S, int nlev, int connectivity, int wide, void* labels, void* stream) {
  P2I_REQUIRE(bits && labels && objects_sizes_ok(T, S, nlev), "bad arguments");
  P2I_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity is 4 or 8");
  P2I_REQUIRE(wide || S <= OLS, "a crop above %d needs the 32-bit label workspace", OLS);
  const long long ntfl = (long long)T * 2 * nlev;
  const int conn8 = connectivity == 8;
  const hipStream_t s = (hipStream_t)stream;
  if (!wide) {
    P2I_REQUIRE(ntfl < (1LL << 31), "too many frames in one launch");
    P2I_LAUNCH((objects_label_kernel<uint16_t, OLS>), dim3((unsigned)ntfl), dim3(256), 0, s, bits, S, nlev, conn8, (uint16_t*)labels);
    return launch_status();
  }
  const long long tiles = ceil_div(S, OTILE), per = ((long long)S * S + 255) / 256;
  P2I_REQUIRE(ntfl * tiles * tiles < (1LL << 31) && ntfl * per < (1LL << 31), "too many frames in one launch");
  P2I_LAUNCH((objects_label_kernel<uint32_t, OTILE>), dim3((unsigned)(ntfl * tiles * tiles)), dim3(256), 0, s, bits, S, nlev, conn8,
             (uint32_t*)labels);
  if (tiles > 1) {
    P2I_LAUNCH(objects_merge_kernel, dim3((unsigned)(ntfl * per)), dim3(256), 0, s, (unsigned*)labels, S, conn8);
    P2I_LAUNCH(objects_flatten_kernel, dim3((unsigned)(ntfl * per)), dim3(256), 0, s, (unsigned*)labels, ntfl * S * S, S);
  }
  return launch_status();
}

extern "C" int p2i_objects_count(const void* labels, int wide, const uint32_t* q, int T, int S, int nlev, int64_t* lev, int64_t* counts,
                                 void* stream) {
  P2I_REQUIRE(labels && q && lev && counts && objects_sizes_ok(T, S, nlev), "bad arguments");
  const dim3 grid((unsigned)(T * 2 * nlev));
  if (wide)
    P2I_LAUNCH(objects_count_kernel<uint32_t>, grid, dim3(256), 0, (hipStream_t)stream, (const uint32_t*)labels, q, S, nlev,
               (long long*)lev, (long long*)counts);
  else {
    P2I_REQUIRE(S <= OLS, "16-bit labels hold a crop of at most %d", OLS);
    P2I_LAUNCH(objects_count_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)labels, q, S, nlev,
               (long long*)lev, (long long*)counts);
  }
  return launch_status();
}

extern "C" int p2i_objects_scan(const int64_t* counts, int64_t n, int64_t* offsets, void* stream) {
  P2I_REQUIRE(counts && offsets && n > 0, "bad arguments");
  P2I_LAUNCH(objects_scan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const long long*)counts, (long long)n, (long long*)offsets);
  return launch_status();
}

extern "C" int p2i_objects_fill(void* labels, int wide, const uint32_t* q, int T, int S, int nlev, const int64_t* offsets, int64_t rows,
                                int64_t* table, void* stream) {
  P2I_REQUIRE(labels && q && offsets && objects_sizes_ok(T, S, nlev) && rows >= 0, "bad arguments");
  if (rows == 0) return P2I_OK;
  P2I_REQUIRE(table, "no object table");
  const dim3 grid((unsigned)(T * 2 * nlev));
  if (wide)
    P2I_LAUNCH(objects_fill_kernel<uint32_t>, grid, dim3(256), 0, (hipStream_t)stream, (uint32_t*)labels, q, S, nlev,
               (const long long*)offsets, (long long)rows, (long long*)table);
  else {
    P2I_REQUIRE(S <= OLS, "16-bit labels hold a crop of at most %d", OLS);
    P2I_LAUNCH(objects_fill_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream, (uint16_t*)labels, q, S, nlev,
               (const long long*)offsets, (long long)rows, (long long*)table);
  }
  return launch_status();
}
