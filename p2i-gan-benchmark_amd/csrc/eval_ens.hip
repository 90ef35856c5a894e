// Ensemble verification on the device; DESIGN.md section 25, ABI: include/p2i_ens.h.  M members and a truth on the inputs' own 0-255
// scale, every statistic in fp64.  The members reach a kernel as one by-value table (pointer, dtype, extent, crop origin and frame
// stride per member), so one kernel reads members of mixed dtypes: the dtype branch is uniform over the wave.
//   p2i_ens_points    : a workgroup of 64 threads takes P2I_ENS_WG_PIXELS consecutive points, a thread one point at a time.  The
//                       thread forms the point's M box values (coalesced along pixels at box size 1) into ITS column of an LDS
//                       image [n][64] (n = M rounded up to a power of two, padded with +inf), sorts the column in place with a
//                       bitonic network (uniform control flow, no registers holding members: nothing spills at M = 64) and reads
//                       every score off the sorted column, so the record is a function of the member SET.  Sums are formed as in
//                       eval_prob.hip: scalar fp64 sums in registers folded by block_tree, counts and the rank histogram as 64-bit
//                       integer LDS atomics (exact in any order), the per-sigma-bin sums from per-point LDS slots that one thread
//                       per bin folds in point order.  The rank weight 2^32 / (k + 1) over bins b .. b + k is added as differences
//                       (+ at b, - at b + k + 1): three atomics however many members tie.
//   p2i_ens_energy    : one workgroup of 256 threads per frame.  Tiles of 64 pixels of all M + 1 fields go to LDS (a pixel that is
//                       unselected or not finite anywhere is zeroed in every field and so adds exactly 0), each thread owns up to
//                       9 of the (M + 1) M / 2 field pairs and accumulates fma(d, d, acc) over the pixels in order.  Direct
//                       differences rather than a Gram matrix on the MFMA pipe: |a|^2 + |b|^2 - 2 a.b cancels for near members
//                       and can turn negative, a chain of squares cannot, and identical members give exactly 0; the fp64 work is
//                       small next to the loads.
//   p2i_ens_variogram : one workgroup of 256 threads per (frame, offset), a thread strides over the pixels, a fixed tree joins.
// No floating-point atomics anywhere: two runs give the same bits.  Compiled with -ffp-contract=off, as the other eval units.
#include "eval_common.h"
#include "p2i_ens.h"

namespace p2i {

constexpr int EM = P2I_ENS_MAX_MEMBERS;
constexpr int EK = P2I_EXP1_MAX_THR;
constexpr int EE = P2I_PROB_MAX_EDGES;
constexpr int ES_ = EE + 1;                      // sigma-bins
constexpr int EO = P2I_ENS_MAX_OFFSETS;
constexpr int ETH = 64;                          // threads of a points workgroup
constexpr int EPT = P2I_ENS_WG_PIXELS / ETH;     // points per thread
constexpr int GTH = 256;                         // threads of an energy / variogram workgroup
constexpr int ETILE = 64;                        // pixels of an energy tile
constexpr int EPITCH = ETILE + 1;
constexpr int EPP = ((EM + 1) * EM / 2 + GTH - 1) / GTH;   // field pairs per thread
typedef unsigned long long u64;
static_assert(P2I_ENS_WG_PIXELS % ETH == 0 && 2 * ES_ <= ETH, "workgroup shape");

enum { EF_CRPS = 0, EF_CRPSF, EF_E, EF_AE, EF_E2, EF_S2, EF_NSCALAR };
enum { EI_N = 0, EI_SKIP, EI_NSCALAR };

struct ELayout {
  int M, K, NS;
  __host__ __device__ int f_p() const { return EF_NSCALAR; }
  __host__ __device__ int f_br() const { return f_p() + K; }
  __host__ __device__ int f_sv() const { return f_br() + K; }
  __host__ __device__ int f_se() const { return f_sv() + NS; }
  __host__ __device__ int nf() const { return f_se() + NS; }
  __host__ __device__ int i_o() const { return EI_NSCALAR; }
  __host__ __device__ int i_rk() const { return i_o() + K; }
  __host__ __device__ int i_sn() const { return i_rk() + M + 2; }
  __host__ __device__ int i_rn() const { return i_sn() + NS; }
  __host__ __device__ int i_ro() const { return i_rn() + K * (M + 1); }
  __host__ __device__ int ni() const { return i_ro() + K * (M + 1); }
};
constexpr int ENI_MAX = EI_NSCALAR + EK + EM + 2 + ES_ + 2 * EK * (EM + 1);

// the members (and, in slot M, nothing: the truth travels apart) as the kernels read them
struct EMembers {
  const void* p[EM];
  long long fs[EM];      // frame stride in elements
  int dt[EM], h[EM], w[EM], top[EM], left[EM];
};
struct ETruth {
  const void* p;
  int dt, h, w, top, left;
};
struct EPArgs {
  double xq[EK], edge[EE];
  ELayout lay;
  int nedges;
};
struct EOffsets { int dy[EO], dx[EO]; };

struct ERec {
  static constexpr int WORDS = EF_NSCALAR + 2 * EK;
  double v[WORDS];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < WORDS; ++i) v[i] = 0.0;
  }
  __device__ __forceinline__ void merge(const ERec& b) {
#pragma unroll
    for (int i = 0; i < WORDS; ++i) v[i] += b.v[i];
  }
  __device__ __forceinline__ void store(double* p) const {
#pragma unroll
    for (int i = 0; i < WORDS; ++i) p[i] = v[i];
  }
  static __device__ __forceinline__ ERec load(const double* p) {
    ERec r;
#pragma unroll
    for (int i = 0; i < WORDS; ++i) r.v[i] = p[i];
    return r;
  }
};

__device__ __forceinline__ double eload(const void* p, int dt, long long i) {
  if (dt == P2I_EXP1_F64) return ((const double*)p)[i];
  if (dt == P2I_EXP1_F32) return (double)((const float*)p)[i];
  return (double)((const uint8_t*)p)[i];
}
__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and +-inf

// element offset of crop pixel (y, x) of frame t
#define E_MEMBER_AT(mem, m, t, y, x) ((t) * (mem).fs[m] + (long long)((mem).top[m] + (y)) * (mem).w[m] + (mem).left[m] + (x))
#define E_TRUTH_AT(gt, t, y, x) ((t) * (long long)(gt).h * (gt).w + (long long)((gt).top + (y)) * (gt).w + (gt).left + (x))

__global__ __launch_bounds__(ETH) void ens_points_kernel(EMembers mem, ETruth gt, EPArgs a, long long total, int cols, int box, int brows,
                                                         int bcols, int npad, const int* __restrict__ rank, double* __restrict__ part) {
  extern __shared__ double dyn[];                // the members' image [npad][ETH], then block_tree's buffer
  __shared__ u64 itab[ENI_MAX];
  __shared__ u64 qtab[EM + 1];                   // floor(2^32 / (k + 1))
  __shared__ double ps2[P2I_ENS_WG_PIXELS], pe2[P2I_ENS_WG_PIXELS];
  __shared__ int psb[P2I_ENS_WG_PIXELS];
  const ELayout lay = a.lay;
  const int M = lay.M, K = lay.K, NS = lay.NS;
  const int tid = threadIdx.x;
  for (int i = tid; i < lay.ni(); i += ETH) itab[i] = 0;
  for (int i = tid; i <= M; i += ETH) qtab[i] = 0x100000000ull / (u64)(i + 1);
  for (int it = 0; it < EPT; ++it) psb[it * ETH + tid] = -1;
  __syncthreads();
  ERec s;
  s.zero();
  double* col = dyn + tid;
  const double dM = (double)M, den = 2.0 * dM * dM, denf = 2.0 * dM * (dM - 1.0), dM1 = dM - 1.0;
  const long long npts = (long long)brows * bcols;
  const long long base = (long long)blockIdx.x * P2I_ENS_WG_PIXELS;
  long long nscored = 0, nskip = 0;
  for (int it = 0; it < EPT; ++it) {
    const int sl = it * ETH + tid;
    const long long g = base + sl;
    if (g >= total) break;
    const long long t = g / npts;
    const int r = (int)(g - t * npts);
    const int by = r / bcols, bx = r - by * bcols;
    const int y0 = by * box, x0 = bx * box;
    int cnt = 0;
    double sum = 0.0;
    for (int dy = 0; dy < box; ++dy)
      for (int dx = 0; dx < box; ++dx)
        if (!rank || rank[(y0 + dy) * cols + x0 + dx] >= 0) {
          ++cnt;
          sum += eload(gt.p, gt.dt, E_TRUTH_AT(gt, t, y0 + dy, x0 + dx));
        }
    if (cnt == 0) continue;                      // no selected pixel: no point
    const double dcnt = (double)cnt;
    const double y = sum / dcnt;
    bool bad = !finite64(y);
    for (int m = 0; m < M; ++m) {
      const void* p = mem.p[m];
      const int dt = mem.dt[m];
      double sm = 0.0;
      for (int dy = 0; dy < box; ++dy)
        for (int dx = 0; dx < box; ++dx)
          if (!rank || rank[(y0 + dy) * cols + x0 + dx] >= 0) sm += eload(p, dt, E_MEMBER_AT(mem, m, t, y0 + dy, x0 + dx));
      const double v = sm / dcnt;
      bad = bad || !finite64(v);
      col[m * ETH] = v;
    }
    if (bad) {
      ++nskip;
      continue;
    }
    ++nscored;
    for (int m = M; m < npad; ++m) col[m * ETH] = __builtin_huge_val();
    // bitonic network over the thread's column: npad / 2 independent compare-exchanges per stage
    for (int k = 2; k <= npad; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1)
        for (int hh = 0; hh < (npad >> 1); ++hh) {
          const int i = ((hh & ~(j - 1)) << 1) | (hh & (j - 1)), l = i | j;
          const double u = col[i * ETH], v = col[l * ETH];
          const bool up = (i & k) == 0;
          if ((u > v) == up) {
            col[i * ETH] = v;
            col[l * ETH] = u;
          }
        }
    double sx = 0.0, sa = 0.0, sw = 0.0;
    int b = 0, k = 0, c[EK];
#pragma unroll
    for (int q = 0; q < EK; ++q) c[q] = 0;
    for (int i = 0; i < M; ++i) {
      const double x = col[i * ETH];
      sx += x;
      sa += fabs(x - y);
      sw += (double)(2 * i - M + 1) * x;
      b += x < y ? 1 : 0;
      k += x == y ? 1 : 0;
#pragma unroll
      for (int q = 0; q < EK; ++q) c[q] += (q < K && x >= a.xq[q]) ? 1 : 0;
    }
    const double mean = sx / dM, am = sa / dM, S = 2.0 * sw;
    double ss = 0.0;
    for (int i = 0; i < M; ++i) {
      const double d = col[i * ETH] - mean;
      ss += d * d;
    }
    const double s2 = M > 1 ? ss / dM1 : 0.0;
    const double e = mean - y;
    s.v[EF_CRPS] += am - S / den;
    if (M > 1) s.v[EF_CRPSF] += am - S / denf;
    s.v[EF_E] += e;
    s.v[EF_AE] += fabs(e);
    s.v[EF_E2] += e * e;
    s.v[EF_S2] += s2;
    const u64 q = qtab[k], rem = 0x100000000ull - q * (u64)(k + 1);
    atomicAdd(&itab[lay.i_rk() + b], q + rem);
    if (rem) atomicAdd(&itab[lay.i_rk() + b + 1], (u64)0 - rem);
    atomicAdd(&itab[lay.i_rk() + b + k + 1], (u64)0 - q);
    const double sg = sqrt(s2);
    int sb = 0;
#pragma unroll
    for (int j = 0; j < EE; ++j)
      if (j < a.nedges && a.edge[j] <= sg) ++sb;
    atomicAdd(&itab[lay.i_sn() + sb], (u64)1);
    psb[sl] = sb;
    ps2[sl] = s2;
    pe2[sl] = e * e;
#pragma unroll
    for (int j = 0; j < EK; ++j)
      if (j < K) {
        const double p = (double)c[j] / dM;
        const bool o = y >= a.xq[j];
        const double d = p - (o ? 1.0 : 0.0);
        s.v[EF_NSCALAR + j] += p;
        s.v[EF_NSCALAR + EK + j] += d * d;
        atomicAdd(&itab[lay.i_rn() + j * (M + 1) + c[j]], (u64)1);
        if (o) {
          atomicAdd(&itab[lay.i_o() + j], (u64)1);
          atomicAdd(&itab[lay.i_ro() + j * (M + 1) + c[j]], (u64)1);
        }
      }
  }
  if (nscored) atomicAdd(&itab[EI_N], (u64)nscored);
  if (nskip) atomicAdd(&itab[EI_SKIP], (u64)nskip);
  __syncthreads();
  const int NF = lay.nf(), NI = lay.ni();
  double* out = part + (long long)blockIdx.x * (NF + NI);
  long long* iout = (long long*)(out + NF);
  for (int i = tid; i < NI; i += ETH) iout[i] = (long long)itab[i];
  if (tid < 2 * NS) {
    const int bin = tid < NS ? tid : tid - NS;
    const double* src = tid < NS ? ps2 : pe2;
    double f = 0.0;
    for (int i = 0; i < P2I_ENS_WG_PIXELS; ++i)
      if (psb[i] == bin) f += src[i];
    out[lay.f_sv() + tid] = f;         // the e^2 section follows the s2 section
  }
  block_tree<ETH>(s, dyn);             // its first barrier follows every thread's last use of the image
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < EF_NSCALAR; ++i) out[i] = s.v[i];
#pragma unroll
    for (int j = 0; j < EK; ++j)
      if (j < K) {
        out[lay.f_p() + j] = s.v[EF_NSCALAR + j];
        out[lay.f_br() + j] = s.v[EF_NSCALAR + EK + j];
      }
  }
}

// fixed-order sum of one double per thread over the workgroup's GTH threads; every thread calls it; the result is in red[0]
__device__ __forceinline__ void tree_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = GTH / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
}

__global__ __launch_bounds__(GTH) void ens_energy_kernel(EMembers mem, ETruth gt, int M, int rows, int cols, const int* __restrict__ rank,
                                                         double* __restrict__ out) {
  __shared__ double tile[(EM + 1) * EPITCH];     // field m (the truth is field M), pixel p at m * EPITCH + p
  __shared__ double red[GTH];
  __shared__ int dcount;
  const long long t = blockIdx.x;
  const int tid = threadIdx.x;
  const int N1 = M + 1, npairs = N1 * M / 2, npix = rows * cols;
  int pi[EPP], pj[EPP];
  double acc[EPP];
#pragma unroll
  for (int k = 0; k < EPP; ++k) {
    int q = tid + k * GTH, i = 0;
    pi[k] = pj[k] = -1;
    acc[k] = 0.0;
    if (q < npairs) {
      while (q >= M - i) {                       // row i holds the pairs (i, i + 1 .. M)
        q -= M - i;
        ++i;
      }
      pi[k] = i;
      pj[k] = i + 1 + q;
    }
  }
  if (tid == 0) dcount = 0;
  int d = 0;
  for (int p0 = 0; p0 < npix; p0 += ETILE) {
    __syncthreads();                             // the previous tile is read
    for (int e = tid; e < N1 * ETILE; e += GTH) {
      const int m = e >> 6, p = e & (ETILE - 1), r = p0 + p;
      double v = __builtin_nan("");              // outside the frame or unselected: the column is dropped below
      if (r < npix && (!rank || rank[r] >= 0)) {
        const int yy = r / cols, xx = r - yy * cols;
        v = m < M ? eload(mem.p[m], mem.dt[m], E_MEMBER_AT(mem, m, t, yy, xx)) : eload(gt.p, gt.dt, E_TRUTH_AT(gt, t, yy, xx));
      }
      tile[m * EPITCH + p] = v;
    }
    __syncthreads();
    if (tid < ETILE) {
      bool ok = true;
      for (int m = 0; m < N1; ++m) ok = ok && finite64(tile[m * EPITCH + tid]);
      if (ok) ++d;
      else
        for (int m = 0; m < N1; ++m) tile[m * EPITCH + tid] = 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPP; ++k)
      if (pi[k] >= 0) {
        const double* u = tile + pi[k] * EPITCH;
        const double* v = tile + pj[k] * EPITCH;
        double s = acc[k];
        for (int p = 0; p < ETILE; ++p) {
          const double dl = u[p] - v[p];
          s = fma(dl, dl, s);
        }
        acc[k] = s;
      }
  }
  if (d) atomicAdd(&dcount, d);
  double to_truth = 0.0, between = 0.0;
#pragma unroll
  for (int k = 0; k < EPP; ++k)
    if (pi[k] >= 0) {
      const double dist = sqrt(acc[k]);          // a sum of squares: never negative, exactly 0 for identical fields
      if (pj[k] == M) to_truth += dist;
      else between += dist;
    }
  tree_sum(to_truth, red);
  const double st = red[0];
  tree_sum(between, red);
  if (tid == 0) {
    const double dM = (double)M, t1 = st / dM, pairs = 2.0 * red[0];
    out[t * 4 + 0] = (double)dcount;
    out[t * 4 + 1] = t1 - pairs / (2.0 * dM * dM);
    out[t * 4 + 2] = M > 1 ? t1 - pairs / (2.0 * dM * (dM - 1.0)) : __builtin_nan("");
    out[t * 4 + 3] = t1;
  }
}

__global__ __launch_bounds__(GTH) void ens_variogram_kernel(EMembers mem, ETruth gt, EOffsets off, int M, int nof, int rows, int cols,
                                                            const int* __restrict__ rank, double* __restrict__ out) {
  __shared__ double red[GTH];
  const long long t = blockIdx.x / nof;
  const int o = blockIdx.x - (int)(t * nof), tid = threadIdx.x;
  const int dy = off.dy[o], dx = off.dx[o], npix = rows * cols;
  const double dM = (double)M;
  double V = 0.0, n = 0.0;
  for (int r = tid; r < npix; r += GTH) {
    const int ya = r / cols, xa = r - ya * cols, yb = ya + dy, xb = xa + dx;
    if (yb < 0 || yb >= rows || xb < 0 || xb >= cols) continue;
    if (rank && (rank[r] < 0 || rank[yb * cols + xb] < 0)) continue;
    const double va = eload(gt.p, gt.dt, E_TRUTH_AT(gt, t, ya, xa)), vb = eload(gt.p, gt.dt, E_TRUTH_AT(gt, t, yb, xb));
    bool ok = finite64(va) && finite64(vb);
    double sm = 0.0;
    for (int m = 0; m < M; ++m) {
      const void* p = mem.p[m];
      const int dt = mem.dt[m];
      const double ua = eload(p, dt, E_MEMBER_AT(mem, m, t, ya, xa)), ub = eload(p, dt, E_MEMBER_AT(mem, m, t, yb, xb));
      ok = ok && finite64(ua) && finite64(ub);
      sm += sqrt(fabs(ua - ub));
    }
    if (ok) {
      const double dl = sqrt(fabs(va - vb)) - sm / dM;
      V += dl * dl;
      n += 1.0;
    }
  }
  tree_sum(V, red);
  const double sv = red[0];
  tree_sum(n, red);
  if (tid == 0) {
    out[((long long)blockIdx.x) * 2] = sv;
    out[((long long)blockIdx.x) * 2 + 1] = red[0];
  }
}

static inline bool ens_layout(int M, int nthr, int nedges, ELayout* lay) {
  if (M < 1 || M > EM || nthr < 0 || nthr > EK || nedges < 0 || nedges > EE) return false;
  *lay = ELayout{M, nthr, nedges + 1};
  return true;
}

// the checks every entry point shares, and the kernels' tables; returns before any HIP call
static int ens_inputs(const p2i_eval_input* members, int M, int64_t frame_stride, const p2i_eval_input* truth, int64_t T, int rows,
                      int cols, EMembers* mem, ETruth* gt) {
  P2I_REQUIRE(members && input_set(truth), "bad arguments");
  P2I_REQUIRE(M >= 1 && M <= EM, "1 to %d members", EM);
  for (int m = 0; m < M; ++m) P2I_REQUIRE(members[m].data, "bad arguments");
  P2I_REQUIRE(eval_dtype_ok(truth->dtype), "unsupported dtype");
  for (int m = 0; m < M; ++m) P2I_REQUIRE(eval_dtype_ok(members[m].dtype), "unsupported dtype");
  P2I_REQUIRE(T > 0 && rows > 0 && cols > 0 && (int64_t)rows * cols <= (int64_t)1 << 30, "bad frame count / crop");
  for (int m = 0; m < M; ++m) P2I_REQUIRE(crop_ok(&members[m], rows, cols), "crop outside member %d", m);
  P2I_REQUIRE(crop_ok(truth, rows, cols), "crop outside the truth");
  P2I_REQUIRE(frame_stride >= 0, "bad frame stride");
  bool own = true, same = true;
  for (int m = 0; m < M; ++m) {
    own = own && (frame_stride == 0 || frame_stride == (int64_t)members[m].h * members[m].w);
    same = same && members[m].dtype == members[0].dtype && members[m].h == members[0].h && members[m].w == members[0].w;
  }
  P2I_REQUIRE(own || (same && frame_stride >= (int64_t)members[0].h * members[0].w),
              "a frame stride other than h * w needs members of one dtype, h and w, and is at least h * w");
  for (int m = 0; m < EM; ++m) {
    const p2i_eval_input* in = &members[m < M ? m : 0];
    mem->p[m] = in->data;
    mem->fs[m] = frame_stride ? frame_stride : (long long)in->h * in->w;
    mem->dt[m] = in->dtype;
    mem->h[m] = in->h;
    mem->w[m] = in->w;
    mem->top[m] = in->top;
    mem->left[m] = in->left;
  }
  *gt = ETruth{truth->data, truth->dtype, truth->h, truth->w, truth->top, truth->left};
  return P2I_OK;
}

}  // namespace p2i

using namespace p2i;

extern "C" int p2i_ens_abi_version(void) { return 1; }

extern "C" int p2i_ens_record(int M, int nthr, int nedges, int* nf, int* ni) {
  ELayout lay;
  P2I_REQUIRE(nf && ni && ens_layout(M, nthr, nedges, &lay), "bad arguments");
  *nf = lay.nf();
  *ni = lay.ni();
  return P2I_OK;
}

extern "C" int p2i_ens_points(const p2i_eval_input* members, int M, int64_t frame_stride, const p2i_eval_input* truth, int64_t T, int rows,
                              int cols, int box, const int* rank, const double* xq_host, int nthr, const double* edges_host, int nedges,
                              double* part, int64_t part_words, void* stream) {
  EMembers mem;
  ETruth gt;
  P2I_REQUIRE(part, "bad arguments");
  if (int rc = ens_inputs(members, M, frame_stride, truth, T, rows, cols, &mem, &gt)) return rc;
  EPArgs a;
  P2I_REQUIRE(ens_layout(M, nthr, nedges, &a.lay), "at most %d thresholds and %d edges", EK, EE);
  P2I_REQUIRE((nthr == 0 || xq_host) && (nedges == 0 || edges_host), "missing host array");
  P2I_REQUIRE(box >= 1 && box <= rows && box <= cols, "a box size lies in 1 .. min(rows, cols)");
  for (int i = 0; i < EK; ++i) a.xq[i] = i < nthr ? xq_host[i] : 0.0;
  for (int i = 0; i < EE; ++i) {
    P2I_REQUIRE(i >= nedges || i == 0 || edges_host[i] > edges_host[i - 1], "sigma edges ascend");
    a.edge[i] = i < nedges ? edges_host[i] : 0.0;
  }
  a.nedges = nedges;
  const int brows = rows / box, bcols = cols / box;
  const long long total = (long long)T * brows * bcols;
  const long long nwg = (total + P2I_ENS_WG_PIXELS - 1) / P2I_ENS_WG_PIXELS;
  P2I_REQUIRE(nwg <= 0x7fffffffLL && part_words >= nwg * (a.lay.nf() + a.lay.ni()), "partial buffer too small");
  const int npad = pow2_ceil(M);
  const size_t image = (size_t)npad * ETH, tree = (size_t)ETH * ERec::WORDS;
  P2I_LAUNCH(ens_points_kernel, dim3((unsigned)nwg), dim3(ETH), (image > tree ? image : tree) * sizeof(double), (hipStream_t)stream, mem,
             gt, a, total, cols, box, brows, bcols, npad, rank, part);
  return launch_status();
}

extern "C" int p2i_ens_energy(const p2i_eval_input* members, int M, int64_t frame_stride, const p2i_eval_input* truth, int64_t T, int rows,
                              int cols, const int* rank, double* out, void* stream) {
  EMembers mem;
  ETruth gt;
  P2I_REQUIRE(out, "bad arguments");
  if (int rc = ens_inputs(members, M, frame_stride, truth, T, rows, cols, &mem, &gt)) return rc;
  P2I_REQUIRE(T <= 0x7fffffffLL, "too many frames");
  P2I_LAUNCH(ens_energy_kernel, dim3((unsigned)T), dim3(GTH), 0, (hipStream_t)stream, mem, gt, M, rows, cols, rank, out);
  return launch_status();
}

extern "C" int p2i_ens_variogram(const p2i_eval_input* members, int M, int64_t frame_stride, const p2i_eval_input* truth, int64_t T,
                                 int rows, int cols, const int* rank, const int* offsets_host, int nof, double* out, void* stream) {
  EMembers mem;
  ETruth gt;
  P2I_REQUIRE(out && offsets_host, "bad arguments");
  P2I_REQUIRE(nof >= 1 && nof <= EO, "1 to %d offsets", EO);
  if (int rc = ens_inputs(members, M, frame_stride, truth, T, rows, cols, &mem, &gt)) return rc;
  EOffsets off;
  for (int i = 0; i < EO; ++i) {
    off.dy[i] = i < nof ? offsets_host[2 * i] : 0;
    off.dx[i] = i < nof ? offsets_host[2 * i + 1] : 0;
    P2I_REQUIRE(i >= nof || off.dy[i] || off.dx[i], "an offset is not (0, 0)");
  }
  P2I_REQUIRE(T * nof <= 0x7fffffffLL, "too many frames");
  P2I_LAUNCH(ens_variogram_kernel, dim3((unsigned)(T * nof)), dim3(GTH), 0, (hipStream_t)stream, mem, gt, off, M, nof, rows, cols, rank,
             out);
  return launch_status();
}
