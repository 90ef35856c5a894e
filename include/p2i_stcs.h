/* libp2i_hip: conditional simulation of space-time ordinary kriging (csrc/stkrig_cs.hip,
 * SpaceTimeKrigingGenerator.forward_simulation of p2igan_bench/models/classical.py).
 *
 * A header of its own, next to p2i_hip.h, as p2i_ens.h is: the v4 ABI of p2i_hip.h is frozen, so this unit's entry points are declared
 * here, versioned by p2i_stcs_abi_version, implemented in the same libp2i_hip.so and bound through a table of their own
 * (_hip.STCS_SIGNATURES).  Errors go through p2i_last_error; every argument check returns P2I_EINVAL before the first HIP call.
 *
 * A sample is T frames of H x W pixels; its members are drawn on the torus St x Sy x Sx >= T x H x W (St <= P2I_STCS_MAX_ST,
 * Sy, Sx <= P2I_STCS_MAX_SIDE) and conditioned on all its space-time points.  All pointers are DEVICE pointers.
 *
 * p2i_stcs_spectrum: amp [B][St][Sy][Sx] fp32 = sqrt(lambda+ / (St Sy Sx)) and clip [B] fp64 (the clipped share of the spectrum; NaN
 *   and amp = 0 for a sample with cand[b] < 0; cand may be NULL) of b[l][j][k] = C(sqrt(dj^2 + dk^2 + kappa^2 dl^2)) + nugget at the
 *   origin, from params [B][4] = (nugget, psill, range, kappa), in fp64.  twiddle: cos(2 pi m / St), m < St, then cos(2 pi m / Sy),
 *   m < Sy, then cos(2 pi m / Sx), m < Sx, fp64.  work: 2 B St Sy Sx fp64.  B St <= 65535.
 * p2i_stcs_noise: xi [npairs][St][Sy][Sx][2] fp32, the complex standard normal of the member pairs q0 .. q0 + npairs - 1 of the sample
 *   with id stream_id: Box-Muller of Philox4x32-10 of counter (cell = (l Sy + j) Sx + k, q, stream low, stream high) under key (seed
 *   low, seed high).
 * p2i_stcs_fields: the unconditional members of the units u0 .. u0 + nunits - 1 into ens [B][T][M][H W]; unit = b npairs + q with
 *   npairs = (M + 1) / 2: DFT3(amp[b] xi)[:T, :H, :W] of pair q of sample b with xi of (seed, streams[b], q); member 2q is its real
 *   part, member 2q + 1 its imaginary part (dropped for the last pair of an odd M).  tx [2][Sx][W], ty [2][Sy][H], tt [2][St][T]: cos,
 *   sin of 2 pi (a b mod S) / S, fp32.  Workspaces: P 2 nunits St Sy W fp32, P2 2 nunits St H W fp32.  nunits <= 65535.
 *   stages: P2I_STCS_STAGES_ALL, or a subset of the three transforms (bit 0: along k into P, bit 1: along j into P2, bit 2: along l into
 *   ens) that reads what an earlier call left in the workspaces: for timing and testing a stage on its own.
 * p2i_stcs_weights: k describes the chunk's samples as systems (stpix, stz, stcounts of p2i_stkrig_gather; R = T = 1), stt [B][cap]
 *   their points' frames, Winv the inverses of the chunk's factors, sol [nsys][2][np] fp64 (row 0: K^-1 1).  alpha [nsys][M][cap],
 *   mu [nsys][M]: the kriging of the residuals z_i - U_m(stt_i, stpix_i), U read from ens; T is the frames per sample.
 * p2i_stcs_predict: ens[b][t][m] = U + mu_m + sum_i alpha_m,i c0((t, p), i) in place, c0 the space-time predictor's expression; a
 *   point's own (frame, pixel) is written as its z; NaN in every member of every frame of a sample without points, with a degenerate
 *   fit (cand[b] < 0) or with status != 0.
 */
#ifndef P2I_STCS_H
#define P2I_STCS_H
#include "p2i_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P2I_STCS_MAX_ST 128
#define P2I_STCS_MAX_SIDE 512
#define P2I_STCS_MAX_MEMBERS 64
#define P2I_STCS_STAGES_ALL 7

int p2i_stcs_abi_version(void);
int p2i_stcs_spectrum(const float* params, const int* cand, int model, int B, int St, int Sy, int Sx, const double* twiddle, double* work,
                      float* amp, double* clip, void* stream);
int p2i_stcs_noise(uint64_t seed, int64_t stream_id, int q0, int npairs, int St, int Sy, int Sx, float* xi, void* stream);
int p2i_stcs_fields(const float* amp, const int64_t* streams, const float* tx, const float* ty, const float* tt, uint64_t seed, int u0,
                    int nunits, int M, int T, int H, int W, int St, int Sy, int Sx, int stages, float* P, float* P2, float* ens,
                    void* stream);
int p2i_stcs_weights(const p2i_krig_systems* k, const int* stt, const float* Winv, const double* sol, const float* ens, int M, int T, int H,
                     int W, float* alpha, float* mu, void* stream);
int p2i_stcs_predict(const p2i_krig_systems* k, const int* stt, const float* alpha, const float* mu, int M, int T, int H, int W, float* ens,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* P2I_STCS_H */
