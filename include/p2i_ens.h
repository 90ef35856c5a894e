/* libp2i_hip: ensemble verification (csrc/eval_ens.hip, p2igan_bench/evaluation/ensemble.py).
 *
 * A header of its own, next to p2i_hip.h: the v4 ABI of p2i_hip.h is frozen (its tests pin the number of its names and
 * p2i_abi_version), so a new unit's entry points are declared here, versioned by p2i_ens_abi_version, implemented in the same
 * libp2i_hip.so and bound through a table of their own (_hip.ENS_SIGNATURES).  Errors go through p2i_last_error; every argument
 * check returns P2I_EINVAL before the first HIP call.
 *
 * An ensemble is M members, 1 <= M <= P2I_ENS_MAX_MEMBERS, scored against one truth on the inputs' own 0-255 scale, in fp64.
 * The members travel as a HOST array of M p2i_eval_input descriptors (DEVICE arrays of P2I_EXP1_U8 / _F32 / _F64, each with its
 * own extent and crop origin; dtypes may differ) and one frame_stride in elements: member m's frame t starts at
 * data_m + t * frame_stride.  frame_stride 0 means every member's own h * w (M separate [T][h][w] arrays); the members of one
 * [T][M][h][w] array pass data_m = base + m * h * w and frame_stride M * h * w.  A non-zero stride that is not a member's h * w
 * needs all members to share dtype, h and w and must be >= h * w.  The truth is [T][h][w].  rank [rows * cols] int32 (DEVICE) selects
 * the crop's pixels with rank >= 0; NULL selects every pixel.
 *
 * p2i_ens_points: one piece of T frames at box size `box` >= 1.  A point is one of the (rows / box) x (cols / box) boxes anchored at
 *   the crop's top-left (remainder rows / columns are left out; box 1: a pixel).  The value of the truth and of each member at a
 *   point is the mean over the box's selected pixels, summed in raster order; a box without a selected pixel is no point; a point
 *   where the truth or a member is not finite is skipped (counted).  With x(0) <= ... <= x(M-1) the sorted members and y the truth:
 *     a = (1/M) sum |x(i) - y|,  S = 2 sum_i (2 i - M + 1) x(i)  (= sum_i sum_j |x_i - x_j|),
 *     CRPS = a - S / (2 M^2),  CRPS_fair = a - S / (2 M (M - 1))  (0 is stored for M = 1),
 *     xbar = (sum x(i)) / M,  s2 = sum (x(i) - xbar)^2 / (M - 1)  (0 for M = 1),  e = xbar - y,
 *     rank: b = #{x_i < y}, k = #{x_i == y}; the weight 2^32 is spread over bins b .. b + k of an (M + 1)-bin histogram, each
 *       floor(2^32 / (k + 1)) and bin b the remainder too,
 *     per pixel threshold xq (HOST array, <= P2I_EXP1_MAX_THR): c = #{x_i >= xq}, p = c / M, o = [y >= xq],
 *     the sigma-bin of sqrt(s2): the number of edges (HOST array, ascending, <= P2I_PROB_MAX_EDGES) that are <= it.
 *   One record per P2I_ENS_WG_PIXELS consecutive points (frame-major, then row-major), nf fp64 words then ni int64 words as bits:
 *     fp64 : sum CRPS, sum CRPS_fair, sum e, sum |e|, sum e^2, sum s2, [K] sum p, [K] sum (p - o)^2, [NS] sum s2 per sigma-bin,
 *            [NS] sum e^2 per sigma-bin                                                     (K = nthr, NS = nedges + 1)
 *     int64: points scored, points skipped, [K] count of o, [M + 2] the rank histogram AS DIFFERENCES (its running sum over the
 *            first M + 1 words is the histogram), [NS] points per sigma-bin, [K][M + 1] points per member count c, [K][M + 1]
 *            those with o.
 *   Records add word by word, so p2i_prob_merge folds them.  No floating-point atomics: two runs give the same bits, and the
 *   record does not depend on the members' order.  part_words >= records * (nf + ni).
 * p2i_ens_record: (nf, ni) for (M, nthr, nedges).
 * p2i_ens_energy: per frame, over the d selected pixels that are finite in the truth and in every member (box size 1):
 *   out[t] = (d, ES, ES_fair, (1/M) sum_i |X_i - y|),  ES = (1/M) sum_i |X_i - y| - 1/(2 M^2) sum_i sum_j |X_i - X_j|  (Euclidean
 *   norms over the d pixels; ES_fair has 1/(2 M (M - 1)) and is NaN for M = 1).  Squared distances are fp64 fma chains on the direct
 *   differences: identical members give exactly 0.  One workgroup per frame, sums in a fixed order.
 * p2i_ens_variogram: per frame and offset o = (dy, dx) (HOST array [nof][2], <= P2I_ENS_MAX_OFFSETS, not (0, 0)), over the pixel pairs
 *   (a, a + o) inside the crop with both pixels valid (as for the energy score):
 *   out[t][o] = (V_o, n_o),  V_o = sum (sqrt|y_a - y_b| - (1/M) sum_m sqrt|X_m(a) - X_m(b)|)^2,  n_o the number of pairs.
 */
#ifndef P2I_ENS_H
#define P2I_ENS_H
#include "p2i_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P2I_ENS_MAX_MEMBERS 64
#define P2I_ENS_MAX_OFFSETS 16
#define P2I_ENS_WG_PIXELS 256

int p2i_ens_abi_version(void);
int p2i_ens_record(int M, int nthr, int nedges, int* nf, int* ni);
int p2i_ens_points(const p2i_eval_input* members, int M, int64_t frame_stride, const p2i_eval_input* truth, int64_t T, int rows,
                   int cols, int box, const int* rank, const double* xq_host, int nthr, const double* edges_host, int nedges,
                   double* part, int64_t part_words, void* stream);
int p2i_ens_energy(const p2i_eval_input* members, int M, int64_t frame_stride, const p2i_eval_input* truth, int64_t T, int rows,
                   int cols, const int* rank, double* out, void* stream);
int p2i_ens_variogram(const p2i_eval_input* members, int M, int64_t frame_stride, const p2i_eval_input* truth, int64_t T, int rows,
                      int cols, const int* rank, const int* offsets_host, int nof, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* P2I_ENS_H */
