/* p2i_hip.h — C ABI of libp2i_hip.so, the MI355X (gfx950) kernel library under the P2I-GAN hot path.
 *
 * The reference (NTU-CompHydroMet-Lab/P2I-GAN-benchmark) is pure Python on PyTorch: the
 * arithmetic of its hot path is reached through ATen call sites (F.conv2d, nn.Conv3d, cdist,
 * topk, max_pool2d, Upsample, spectral_norm, kl_div, Adam).  Each entry point below replaces one
 * group of those call sites; the file:line next to it is the reference code it stands in for
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding a maintainer
 * of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to contiguous fp32 (or int32 where stated); the caller
 *    (PyTorch) owns all memory including workspaces; the library never allocates or frees;
 *  - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*), never syncs;
 *  - state kept by the library: none that a result depends on.  Per calling THREAD it remembers the tile plan of the last
 *    conv / wgrad launch (p2i_conv_last_plan / p2i_wgrad_last_plan, diagnostics), nothing that a later call reads: what a
 *    convolution call computes stands in its argument list.  Tuning switches (P2I_* environment variables): the engine on/off switches
 *    (P2I_CONV_X6C, P2I_CONV_X6C_FUSED, P2I_X6C_KSPLIT, P2I_CONV_V4, P2I_CONV_CK16, P2I_CONV_KG27, P2I_DGRAD_FUSED, P2I_DGRAD_PAIR,
 *    P2I_C1_FAST, P2I_O1_FWD, P2I_WGRAD_X4, P2I_WGRAD_WINDOW) are read ONCE per process; the per-launch choices that the parity
 *    tests flip inside one process (P2I_X6C_MIN_WG, P2I_X6C_MIN_WG_LOW, P2I_X6C_TILE, P2I_X6C_TPS, P2I_X6C_PC, P2I_X6P_NPW, P2I_X6P_TN1,
 *    P2I_X6C_STAGGER, P2I_X6C_FUSED_KSPLIT, P2I_WGRAD_X6, P2I_WGRAD_X6_PC, P2I_WGRAD_X6_S4) are read on EVERY call;
 *  - aliasing: an output may alias the epilogue operand of the same call that is read element-for-element at the position it is
 *    written (y == residual, dx == dx_add, dx == mask_y): every kernel reads it before it writes that element, and the split-K
 *    launches of the bf16-split kernels (which zero-fill the destination first) are not chosen for an aliased call.  No other
 *    overlap between inputs and outputs is allowed;
 *  - return value: 0 on success, negative P2I_E* on a rejected argument, positive = hipError_t
 *    of a failed launch.  Nothing throws across the ABI;
 *  - activations are NC(T)HW; a 2-D tensor is the T == 1 case of the 5-D one.
 */
#ifndef P2I_HIP_H
#define P2I_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2I_OK 0
#define P2I_EINVAL (-1)   /* bad shape / unsupported configuration */
#define P2I_ELDS (-2)     /* tile configuration does not fit LDS */

/* activation codes shared by the conv epilogue and its backward prologue */
#define P2I_ACT_NONE 0
#define P2I_ACT_RELU 1
#define P2I_ACT_LEAKY 2   /* negative slope 0.2 (p2igan.py:122-139) */
#define P2I_ACT_TANH 3

int p2i_abi_version(void);
const char* p2i_last_error(void);

/* ------------------------------------------------------------------ convolution engine
 * Replaces F.conv2d / nn.Conv3d forward + convolution_backward (deconv_pytorch.py:103-109,
 * layer.py:390,402-407, p2igan.py:120-142).  Weights are consumed in PACKED form
 * Wp[tap][k_channel][m_channel_padded] (m padded to a multiple of 32, produced by the
 * p2i_*_pack / p2i_doconv_fold entry points), so that the MFMA A-operand rows are contiguous.
 *
 * p2i_conv_fwd :  y = act(conv(x, W) + bias) + residual
 * p2i_conv_dgrad: dx = conv_transpose(dy * act'(y), W) + dx_add   (Wd = pack with roles swapped;
 *                 dx_add, dx-shaped or NULL, fuses the skip-path gradient of a residual block;
 *                 mask_y (dx-shaped or NULL): dx is finally multiplied by mask_act'(mask_y), the
 *                 derivative of the activation that produced this layer's INPUT, so the next
 *                 dgrad/wgrad up the chain consume a ready gradient and need no prologue)
 * p2i_conv_wgrad: dWp[tap][cin][cout_pad] += sum_pixels x * (dy * act'(y))   (atomic fp32 adds, or slices
 *                 summed in order with a scratch `ws`; caller zeroes dWp), db[cout] += sum dy*act'(y) when db != NULL.
 * dims: x (B,Cin,Ti,Hi,Wi), y (B,Cout,To,Ho,Wo); kernel (kt,kh,kw); stride (st,sh,sw);
 * padding (pt,ph,pw).  bias / residual / y_act may be NULL.
 * Limits (refused with P2I_EINVAL / P2I_ELDS and a p2i_last_error message, never answered wrongly): kt*kh*kw <= 27;
 * p2i_conv_wgrad: kh*kw <= 9, and the x patch of its smallest pixel tile (16 output positions, 64 channels) has to fit 160 KB
 * of LDS ("wgrad tile does not fit LDS": strides far above 3).  Extents of 1 on any axis, any padding and strides 1..3 are
 * covered by tests/test_conv_sweep_gpu.py.
 */
typedef struct {
  int B, Cin, Cout;
  int Ti, Hi, Wi;
  int To, Ho, Wo;
  int kt, kh, kw;
  int st, sh, sw;
  int pt, ph, pw;
} p2i_conv_desc;

/* What the bf16-split pipe of a forward / data-gradient call may use.  `sp` == NULL, or a descriptor whose three pointers are all
 * NULL, keeps the call on the fp32-MFMA kernels (and the single-channel kernels of conv_c1.hip).  Otherwise, with a contraction
 * width K % 16 == 0 (K = Cin for fwd, Cout for dgrad; M the other one) and enough output tiles to fill the chip, these layers are
 * computed on the bf16 matrix pipe with fp32 accuracy (conv_x6c.hip):
 *   - 3x3 stride-1 pad-1 2-D layers, forward and data gradient;
 *   - 3x3x3 pad-1 layers with spatial stride 1 and t stride 1 or 2 (the 27 taps as three t slices of nine), forward and data
 *     gradient (one launch per t-parity class);
 *   - the data gradient of 3x3 / 3x3x3 layers with stride (1,2,2) and even input height / width: the four input-parity classes
 *     of the destination fused in one workgroup (patch_gemm_x6c_kernel<8,1,true,.>).
 * Every fp32 operand is split exactly into three bf16 terms and six v_mfma_f32_32x32x16_bf16 products are accumulated in fp32
 * (the dropped products are <= 2^-23 |a b| each, below the rounding of an fp32 fma chain).  Every other layer runs on the
 * fp32-MFMA kernels exactly as with sp == NULL, and launches no split; the choice is the library's (p2i_x6c_would_take tells it,
 * 1 / 0, for a geometry and, for a forward call, an epilogue activation, so that callers can skip splitting stacks no layer needs).
 * The weights' split comes from ONE of two places, w_split first when both are set:
 *   - w_split: split a weight tensor -- or a whole stack of same-shape packed tensors [n][ntaps][K][pad32(M)], passed as ntaps =
 *     n * taps -- ONCE per weight update (p2i_x6_split / p2i_x6_split_batched; wb: 3 * ntaps * K * Mpad uint16, image
 *     Wb[plane][ntaps][K/8][Mpad][8]); w_split = wb + layer * taps * K * Mpad (uint16 elements: plane 0 of that layer) and
 *     w_split_taps = the image's total tap count (refused when smaller than the layer's);
 *   - w_scratch: 3*ntaps*K*pad32(M) uint16 of caller-owned scratch that the call overwrites with the split of its `wp`.
 * src_planes: the call's source (x / dy) as the pre-split bf16 planes of p2i_x6_split_planes; read instead of the fp32 tensor by
 * the 32-channel tiles with whole-chunk stages, ignored by every other tile and engine (an experiment, measured and not adopted:
 * tools/presplit_probe.py).  A p2i_conv_dgrad call with the act'(y) prologue (y_act != NULL) ignores `sp`.
 * Layers with too few output tiles for 256 CUs whose epilogue is linear (no activation) run with the channel chunks split over two
 * workgroups per tile that add their partial sums into the zeroed destination (P2I_X6C_KSPLIT=0 disables).  P2I_X6C_MIN_WG (read
 * per call) overrides the tile-count thresholds (default: 200 workgroups for a tile variant to be preferred, 64 for the smallest
 * tile as the last resort). */
typedef struct p2i_conv_split {
  const uint16_t* w_split;    /* plane 0 of THIS layer inside a pre-split image (p2i_x6_split / _batched), or NULL */
  uint16_t*       w_scratch;  /* else: 3*ntaps*K*pad32(M) uint16 the call may overwrite with the split, or NULL */
  const void*     src_planes; /* pre-split source of p2i_x6_split_planes, or NULL; read only by the tiles that can */
  int             w_split_taps; /* total taps of the image w_split lies in; read only with w_split */
} p2i_conv_split;

int p2i_conv_fwd(const p2i_conv_desc* d, const float* x, const float* wp, const p2i_conv_split* sp, const float* bias,
                 const float* residual, float* y, int act, void* stream);
int p2i_conv_dgrad(const p2i_conv_desc* d, const float* dy, const float* y_act, int act, const float* wp_d,
                   const p2i_conv_split* sp, const float* dx_add, const float* mask_y, int mask_act, float* dx, void* stream);
/* `ws`: caller-owned scratch of ws_floats floats, or NULL.  When it holds every workgroup's partial tile (<= 256 * kh*kw * Cin *
 * pad32(Cout) floats, 37.7 MB for the generator's 3x3 C->C layers) the partial tiles are stored and summed by a second kernel
 * instead of being added with float atomics: faster, and bit-reproducible.  ws == NULL or too small: the atomic path.
 * With a sufficient scratch, 3x3 pad-1 2-D layers and 3x3x3 pad-1 layers with t stride <= 2 (three t slices), spatial stride 1,
 * whose Cin and Cout are multiples of 64, Ho % 4 == 0, Wo % 16 == 0, called without act'(y) prologue (the generator's DO-Conv stack,
 * the discriminators' 256 -> 256 and 128 -> 128 layers) are computed on the bf16 matrix pipe with fp32 accuracy (wgrad_x6.hip: x
 * and dy split exactly into three bf16 terms each, six MFMA products per fp32 product, transposed LDS reads), dbias included
 * (summed from the staged dy tiles, added atomically); same result contract, same slices + reduce.  P2I_WGRAD_X6=0 (read per
 * call) keeps the fp32-MFMA kernel. */
int p2i_conv_wgrad(const p2i_conv_desc* d, const float* x, const float* dy, const float* y_act, int act, float* dwp,
                   float* dbias, float* ws, int64_t ws_floats, void* stream);
/* The weight split behind p2i_conv_split.w_split.  It is exact -- hi + mid + lo == w, each term w's remainder truncated to its
 * upper 16 bits -- for +-0 and every normal float32 whose remainders stay normal (pinned bit for bit for binary exponents
 * -60 .. 60 by tests/test_weightprep_gpu.py); a subnormal w loses its last bits (1e-40: the remainder's significant bits fall in
 * the lower half-word). */
int p2i_x6_split(const float* wp, uint16_t* wb, int ntaps, int K, int Mpad, void* stream);
/* the same for n <= 24 packed tensors of different shapes in one launch (wb[i]: 3 * ntaps[i] * K[i] * Mpad[i] uint16 each): the
 * discriminators' layers after p2i_weight_pack_batched */
int p2i_x6_split_batched(const float* const* wp, uint16_t* const* wb, const int* ntaps, const int* K, const int* Mpad, int n,
                         void* stream);
int p2i_x6c_would_take(const p2i_conv_desc* d, int dgrad, int act);
/* tile plan {MB, NPIX, WAVES_M, CK, NT, KG} of the calling thread's most recent fwd/dgrad launch: names the
 * patch_gemm_dma_kernel<MB,NPIX,WAVES_M,CK,NT,KG> instance (NT = -1: the prologue kernel
 * patch_gemm_kernel<MB,NPIX,WAVES_M,CK>; KG = 7: patch_gemm_x6c_kernel<8, MB/32, false, TPS>, fields {MB = 32 or 64, 256, ksplit,
 * 16, TPS = taps per pipeline stage (3 or 9), 7}; KG = 8: the fused strided data gradient patch_gemm_x6c_kernel<8, 1, true, TPS>,
 * fields {32, 256, ksplit, 16, TPS, 8}; KG = 3: o1_fwd_kernel (single output channel), fields {1, 64, 8, 1, 9, 3}; KG > 10: the f32
 * fused strided data gradient patch_gemm_fused_kernel with KG - 10 parity classes per workgroup; KG = 4: the single-input-channel
 * data gradient c1_dgrad_kernel / c1_dgrad_fast_kernel, fields {1, 256, 1, 1, taps, 4})
 * so that bench.py's roofline can be matched to rocprofv3 rows */
int p2i_conv_last_plan(int* out6);
/* Host only, no device work: the multiplier the planners hand the kernels for an index division, floor(n / d) ==
 * (uint64_t(n) * *magic) >> 32 for every 0 <= n < 65536.  It exists for 2 <= d < 65536 only; any other d (d = 1 in particular:
 * 2^32 + 1 does not fit 32 bits) is refused with P2I_EINVAL.  The planners stage a patch axis of extent 1 with extent 2, so no
 * convolution geometry that the descriptor check accepts asks for d = 1. */
int p2i_fast_div_magic(int d, uint32_t* magic);
/* same for the most recent p2i_conv_wgrad: {kind (0 wgrad_kernel<64>, 1 wgrad_dma_kernel<64,NTAP,Y4,CB>, 2 c1_wgrad_kernel,
 * 3 wgrad_x6_kernel), NTAP (wgrad_x6: 9 * kt taps in one launch), Y4, CB} */
int p2i_wgrad_last_plan(int* out4);

/* ------------------------------------------------------------------ weight preparation
 * p2i_doconv_fold_fwd: DoW = einsum('ims,ois->oim', D + D_diag, W.reshape(O/g, I, 9)) with the
 *   reference's memory reinterpretation to (O, I/g, 3, 3) (deconv_pytorch.py:111-127), written
 *   densely (zeros outside the group) in both packed layouts: wp_f[9][I][Opad] for p2i_conv_fwd
 *   and wp_d[9][O][Ipad] for p2i_conv_dgrad.  ksz==1: DoW = W.reshape (no D).  `identity_rep`>0
 *   adds the `+ x.repeat_interleave(rep, dim=1)` skip of p2igan.py:79 as a centre-tap identity; that skip exists for a 3x3
 *   layer with I * rep == O only, anything else is refused with P2I_EINVAL.
 * p2i_doconv_fold_bwd: dW, dD from the packed weight gradient produced by p2i_conv_wgrad.
 * The library holds ONE kernel family per operation, the batched one (blockIdx.z = layer): every single-layer entry point of this
 *   and the next section is a batch of one of the same kernels, so a layer gives the same bits alone as in a list -- except the
 *   spectral-norm unpack's dot product, whose number of partial sums follows the largest layer of the batch.  3x3, groups 1, no
 *   identity skip, O and I multiples of 32 take the tile kernels of the *_batched fold; every other layer the per-layer generic ones.
 * Every fold, pack, unpack and spectral-norm entry point of this and the next section, and the weight split p2i_x6_split /
 * p2i_x6_split_batched, are swept over their shapes -- exactly, on integer-valued inputs, wherever the operation allows it -- by
 * tests/test_weightprep_gpu.py (cases: tests/weightprep_cases.py).
 */
int p2i_doconv_fold_fwd(const float* W, const float* D, const float* D_diag, int O, int I, int groups,
                        int ksz, int identity_rep, float* wp_f, float* wp_d, void* stream);
int p2i_doconv_fold_bwd(const float* dwp_f, const float* W, const float* D, const float* D_diag,
                        int O, int I, int groups, int ksz, float* dW, float* dD, void* stream);

/* The same fold / fold backward for n <= 16 layers of ONE shape (3x3, groups 1, O and I multiples of 32: the generator's
 * residual stack has 8 per level) in one / two launches; arrays of n HOST entries holding device pointers. */
int p2i_doconv_fold_fwd_batched(const float* const* W, const float* const* D, const float* const* D_diag, int n, int O, int I,
                                float* const* wp_f, float* const* wp_d, void* stream);
int p2i_doconv_fold_bwd_batched(const float* const* dwp_f, const float* const* W, const float* const* D,
                                const float* const* D_diag, int n, int O, int I, float* const* dW, float* const* dD,
                                void* stream);

/* Plain (O, I, ntaps) weights <-> packed.  scale_ptr (device scalar, may be NULL) divides: used
 * for the spectral-norm weight = weight_orig / sigma. */
int p2i_weight_pack(const float* w, int O, int I, int ntaps, const float* inv_div_ptr,
                    float* wp_f, float* wp_d, void* stream);
/* dw[o][i][tap] = dwp_f[tap][i][o] / sigma  - (sum(dwp_f .* w)/sigma^2) * u[o] * v[i*ntaps+tap]
 * (gradient through torch.nn.utils.spectral_norm's `weight / sigma`); sigma_ptr NULL => plain unpack. */
int p2i_weight_unpack_grad(const float* dwp_f, int O, int I, int ntaps, const float* w_orig,
                           const float* sigma_ptr, const float* u, const float* v, float* scratch,
                           float* dw, void* stream);

/* p2i_weight_pack / p2i_weight_unpack_grad for n <= 16 layers of different shapes in one launch each (arrays of n HOST
 * entries).  The caller zeroes padded pack outputs (pad32(O) != O or pad32(I) != I); `dots`: n floats of device scratch.
 * accumulate != 0: dw += ... (the discriminator's second backward pass of a D step adds to the first one's gradient:
 * train.py:264-283 calls D twice before loss_d.backward()); 0: dw = ... */
int p2i_weight_pack_batched(const float* const* w, const int* O, const int* I, const int* ntaps, const float* const* inv_div,
                            float* const* wp_f, float* const* wp_d, int n, void* stream);
int p2i_weight_unpack_grad_batched(const float* const* dwp_f, const int* O, const int* I, const int* ntaps,
                                   const float* const* w_orig, const float* const* sigma, const float* const* u,
                                   const float* const* v, float* dots, float* const* dw, int n, int accumulate, void* stream);

/* ------------------------------------------------------------------ spectral norm
 * One power iteration of torch.nn.utils.spectral_norm (call sites layer.py:402-407,
 * p2igan.py:141): v <- normalize(W^T u), u <- normalize(W v), sigma = u^T W v, eps 1e-12.
 * training==0: sigma only from the stored u, v.  W is (O, K) row-major.  scratch >= O + K + 4 floats.
 * A batch of one of p2i_spectral_norm_batched's kernels: no sum crosses a workgroup, nothing is atomic and nothing needs zeroing,
 * so two calls on the same inputs give the same bits.
 */
int p2i_spectral_norm(const float* w, int O, int K, float* u, float* v, int training, float* sigma,
                      float* scratch, void* stream);

/* The same power iteration for n <= 16 layers at once (blockIdx.z = layer): 4 launches for the whole discriminator instead
 * of 4 per layer.  Arrays of n HOST entries holding device pointers / sizes; scratch[i] >= O[i] + K[i] + 4 floats. */
int p2i_spectral_norm_batched(const float* const* w, const int* O, const int* K, float* const* u, float* const* v,
                              int training, float* const* sigma, float* const* scratch, float* const* u_snap,
                              float* const* v_snap, int n, void* stream);   /* u_snap / v_snap (may be NULL): copies of the
                              updated u, v for the backward pass (training only) */

/* ------------------------------------------------------------------ generator glue
 * AttentionBlock x2 (layer.py:296-304, 318-322): per pixel relu(x + x*(Wx+b)) over the T=16 vector. */
int p2i_attn_fwd(const float* x, const float* w0, const float* b0, const float* w1, const float* b1,
                 float* out, int B, int T, int HW, void* stream);
int p2i_attn_bwd(const float* x, const float* w0, const float* b0, const float* w1, const float* b1,
                 const float* dout, float* dw0, float* db0, float* dw1, float* db1,
                 int B, int T, int HW, void* stream);

/* Gauge-point IDW (layer.py:324-361 + 259-293 + 246-256): nonzero(mask>0) in (t,y,x) order,
 * 4-NN by torch.cdist's fp32 formula (|a|^2+|b|^2-2ab as an fma chain), torch.topk's
 * partial-sort selection, w = 1/(d+tau)^2 normalised (+1e-12).  grid_[xyz] are the
 * torch.linspace(0,1,n) tables.  Work buffers (caller-allocated):
 *   pt_pos  int32 [B*Q]  flat (t,y,x) index of each point;  pt_count int32 [B] ; frame_count int32[B*T]
 *   row_start int32 [B*T*(H+1)]  first point of frame t in a row >= y (lets the scan skip, exactly, the
 *             frames / rows that cannot beat the current 4th-nearest distance)
 *   sel_idx int32 [B*Q*4] (indices into the point list), sel_w float [B*Q*4]  (saved for backward)
 * Empty mask => zeros (layer.py:330-332).  0 < N < 4 points in a sample is an error in the reference (torch.topk with k > N
 * raises, layer.py:282).  The library is enqueue-only and cannot raise without a device sync: it writes ZEROS for that sample
 * (out, sel_idx, sel_w; p2i_idw_bwd then gives a zero gradient), other samples of the batch are unaffected, and pt_count[b]
 * holds the count for a caller that wants the reference's error (the Python wrapper: P2I_IDW_STRICT=1, one host sync).
 * Pinned by tests/test_ops_gpu.py::test_idw_fewer_than_four_points_gives_zeros_or_raises.
 * amb == NULL: one kernel scans the points of every voxel in index order, as the reference does.  With the work buffer `amb` the
 * same result comes from a two-pass search (round 3; what ops.idw_fwd calls).  The reference's scan order matters only where the 4th and 5th smallest
 * computed distances of a voxel are EQUAL (which tied point is kept depends on the heap's history); everywhere else the set of
 * selected points is the four nearest, whatever the order.  Pass 1 searches outwards from the voxel (own frame and rows first:
 * ~10 % of the distance evaluations of the index-order scan) and lists the voxels it finds tied; pass 2 replays the reference's
 * scan for those only (3-4 % with one gauge mask shared by all frames).  Ties among the four selected points permute equal
 * weights in the 4-term output sum (<= 1 ulp of the output; sel_idx / sel_w order may differ there).
 * Round 4: pass 2 first DECIDES a listed voxel from the points within its (now known) 4th distance D, met in index order -- the
 * reference's heap holds the four smallest values seen so far, so the first four points with d <= D stay unless a point with d < D
 * follows them (idw.hip, IDW_CONSIDER_FIXED) -- and only the voxels where one does (~7 %) take the full replay, from a second list.
 * Those shares are a gauge mask's.  Whole-frame masks (the loader's nowcasting / fi / stin types) tie far more often -- the two
 * in-frame neighbours of a voxel are equidistant -- and the same passes carry them; read from the device counters on an MI355X
 * (tests/test_idw_regimes_gpu.py, shares of Q = T*H*W voxels as listed / left to the full replay): 16 x 32 x 32 nowcasting keep 4
 * 0.497 / 0.127, fi stride 6 0.532 / 0.181, fi stride 3 0.506 / 0.139, stin keep 4 block 4 0.235 / 0.095; 16 x 48 x 48 fi stride 3
 * 0.558 / 0.189.  The replay's grid covers Q / 8 voxels per sample and loops beyond that.
 *   amb int32 [B*(2Q+2+ceil(Q/256))]: per sample the number of listed voxels, the lists of pass 1's workgroups (256 slots each) and
 *       their lengths / prefix sums; behind the B samples' blocks the second list, per sample [count, voxels ...] (work buffer). */
int p2i_idw_fwd(const float* vals_src, const float* mask, const float* grid_x, const float* grid_y,
                const float* grid_z, float* out, int32_t* pt_pos, int32_t* pt_count, int32_t* frame_count,
                int32_t* row_start, float* pt_xyzn, int32_t* sel_idx, float* sel_w, int32_t* amb, int B, int T, int H, int W,
                float tau, void* stream);
/* Backward: dvals_src[pt_pos[j]] = sum over the voxels that selected point j of dout * sel_w, every other entry 0 (values enter the
 * output linearly; the weights are data).  Float atomics by default; with a scratch registered through p2i_det_workspace the same
 * scatter in 64-bit fixed point, scaled from the largest FINITE |dout| of the call: bit-equal from run to run and exact up to the
 * conversion of each product and one final rounding.  In both modes a NaN / Inf in dout arrives as NaN / Inf at the four selected
 * points of its voxel, as the reference's autograd gives it, and changes no other entry (in fixed point such products bypass the
 * integer accumulators as float atomics; finite inputs are untouched by that path, bit for bit).
 * Pinned by tests/test_idw_regimes_gpu.py. */
int p2i_idw_bwd(const float* dout, const int32_t* pt_pos, const int32_t* pt_count, const int32_t* sel_idx,
                const float* sel_w, float* dvals_src, int B, int T, int H, int W, void* stream);

/* DownsampleDuplicateChannels (layer.py:205-214): 2x2 max-pool then duplicate every channel. */
int p2i_pooldup_fwd(const float* x, float* y, int B, int C, int H, int W, void* stream);
int p2i_pooldup_bwd(const float* x, const float* dy, float* dx, int B, int C, int H, int W, void* stream);

/* UPPos front half (layer.py:392-396): u = bilinear_x2(x, align_corners=True) * 2*sigmoid(pos); bias == NULL: no epilogue, `act`
 * is not read.  With a bias, the rest of UPPos behind it: u = act(bilinear_x2(v) * 2*sigmoid(pos) + bias[c]).  The modulation is ONE factor per
 * pixel for all channels and the upsampling acts on every channel alike, so the 1x1 projection (layer.py:390,397) commutes with
 * both: relu(W (up(h) * s) + b) == relu(up(W h) * s + b).  The build projects at the LOW resolution (a quarter of the positions,
 * v = W h through p2i_conv_fwd) and finishes here; equal to the reference's order up to fp32 rounding of the reordered sums. */
int p2i_upmod_fwd(const float* x, const float* pos, const float* bias, int act, float* u, int B, int C, int S, int S2w /*in W*/, void* stream);
int p2i_upmod_bwd(const float* x, const float* pos, const float* du, float* dx, float* dpos,
                  int B, int C, int S, int S2w, void* stream);

/* ------------------------------------------------------------------ discriminator tail
 * p2igan.py:165-173: mean over T' of out3d, bilinear (align_corners=False) to out2d's size,
 * fused = sigmoid(alpha2d)*out2d + that. */
int p2i_dtail_fwd(const float* out2d, const float* out3d, const float* alpha2d, float* fused,
                  int B, int H2, int W2, int T3, int H3, int W3, void* stream);
int p2i_dtail_bwd(const float* out2d, const float* alpha2d, const float* dfused, float* dout2d,
                  float* dout3d, float* dalpha2d, int B, int H2, int W2, int T3, int H3, int W3, void* stream);

/* ------------------------------------------------------------------ losses
 * ReconstructionLoss (losses.py:38-48,56-85): out[0]=pool (weighted L1), out[1]=reg (KL of
 * temporal-difference softmaxes, batchmean), out[2]=pool+k1*reg; dpred = d out[2]/d pred.
 * scratch >= B*(T-1)*HW + 4096 floats. */
int p2i_recloss(const float* pred, const float* target, float k1_alpha, float* out3, float* dpred,
                float* scratch, int B, int T, int HW, void* stream);
/* Hinge / lsgan / nsgan losses (losses.py:210-226) with gradients; loss_type 0 hinge, 1 lsgan (MSE to the label), 2 nsgan
 * (nn.BCELoss on the raw logits, losses.py:201-202: any logit outside [0,1] is an error in torch; here *loss comes back NaN
 * and the Python wrapper raises).  mode: 0 = discriminator (0.5*(L(real)+L(fake)), train.py:266-283), 1 = generator
 * (hinge: -mean * weight; otherwise L(logits, real_label) * weight, train.py:301-308). */
int p2i_gan_loss(const float* logits_a, const float* logits_b, int n, int loss_type, int mode,
                 float weight, float real_label, float fake_label, float* loss, float* dlogits_a,
                 float* dlogits_b, void* stream);

/* ---- the reference's other objectives (losses.py:51-162).  fp32, contiguous.  Scalar results (out1) are sums of
 * workgroup partials added in a fixed order: they need the scratch of p2i_det_workspace.  gout: DEVICE pointer to the upstream
 * gradient of a scalar result.  Every backward pass is a gather (no atomics); max-pool ties go to the first maximal element of
 * the window in raster order, and a window that holds a NaN pools to NaN with its LAST NaN in raster order as the argmax (both
 * torch's rules; the 5/4/2 pool and the shock loss's pool alike).
 * p2i_loss_transform_fwd / _bwd: y = 0.036 * 10^((x*255/3)*0.0625) (losses.py:51-53; NOT metric.py's transform); dx = dy * dy/dx.
 * p2i_fdiff_fwd / _bwd: out[b][t] = x[b][t+1] - x[b][t] over dim 1 of [B][T][inner] (losses.py:83-85); T >= 2.
 * p2i_wl1_fwd / _bwd: mean(w(target) * |pred - target|), w = 0.5 exp(5.14 min(target, 0.7)) + 0.12 (losses.py:56-65); sign(0) = 0.
 * p2i_softmax_t_fwd / _bwd: y = softmax(x / temperature) over each of `rows` rows of L elements, the row maximum subtracted
 *   (losses.py:68-73); dx from y and dy.
 * p2i_kl_fwd / _bwd: out1 = sum(xlogy(q, q) - q log p) / B = F.kl_div(p.log(), q, 'batchmean') (losses.py:76-80); dp = -gout q / (p B).
 * p2i_spool_fwd / _bwd: MaxPool2d(5, stride 4, padding 2) on N planes of H x W (losses.py:88-91; padding is -inf), output
 *   ((H-1)/4+1) x ((W-1)/4+1); idx (may be NULL) = plane index h*W + w of each window's argmax.  _bwd: dx = scale[0] (DEVICE, may
 *   be NULL: 1) * the sum of dout over the up to four windows whose argmax the pixel is.
 * p2i_tdm_fwd: out1 = mean((P(pred_diff) - P(true_diff))^2 / (1 + beta P(true[:, :-1]) + eps)), P = the pool above
 *   (losses.py:94-109); pred_diff / true_diff [B][Tm1][H][W], truth [B][Tm1 + 1][H][W].  coef, idx (both or neither): d out1 / d
 *   P(pred_diff) and P(pred_diff)'s argmax; the backward pass is p2i_spool_bwd(idx, coef, gout).
 * p2i_shock_map_fwd / _bwd: s = tanh(beta lap) sqrt(gx^2 + gy^2 + eps) on N planes, gx / gy / lap = Sobel / 8 and the 5-point
 *   Laplacian under reflect padding of 1 (losses.py:112-137); H, W >= 2.  scratch: 3 N H W floats.
 * p2i_shock_loss_fwd / _bwd: out [N][Hp - 2 border][Wp - 2 border] = relu(|s(P truth)| - |s(P pred)|) cropped by border, P =
 *   max_pool2d(pool, pool), Hp = H / pool (floor) (losses.py:140-162); one kernel, no map is written.  _bwd: dpred from dout in two
 *   kernels (map-gradient coefficients, then the transposed-stencil gather routed through the pool argmax); relu'(0) = 0,
 *   sign(0) = 0; a NaN difference stays NaN in out and passes the relu's gradient (torch); scratch: 3 N Hp Wp floats. */
int p2i_loss_transform_fwd(const float* x, float* y, int64_t n, void* stream);
int p2i_loss_transform_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
int p2i_fdiff_fwd(const float* x, float* out, int B, int T, int64_t inner, void* stream);
int p2i_fdiff_bwd(const float* dy, float* dx, int B, int T, int64_t inner, void* stream);
int p2i_wl1_fwd(const float* pred, const float* target, float* out1, int64_t n, void* stream);
int p2i_wl1_bwd(const float* pred, const float* target, const float* gout, float* dpred, int64_t n, void* stream);
int p2i_softmax_t_fwd(const float* x, float* y, int rows, int L, float temperature, void* stream);
int p2i_softmax_t_bwd(const float* y, const float* dy, float* dx, int rows, int L, float temperature, void* stream);
int p2i_kl_fwd(const float* p, const float* q, float* out1, int64_t n, int B, void* stream);
int p2i_kl_bwd(const float* p, const float* q, const float* gout, float* dp, int64_t n, int B, void* stream);
int p2i_spool_fwd(const float* x, float* out, int* idx, int N, int H, int W, void* stream);
int p2i_spool_bwd(const int* idx, const float* dout, const float* scale, float* dx, int N, int H, int W, void* stream);
int p2i_tdm_fwd(const float* pred_diff, const float* true_diff, const float* truth, float beta, float eps, float* out1,
                float* coef, int* idx, int B, int Tm1, int H, int W, void* stream);
int p2i_shock_map_fwd(const float* x, float* out, int N, int H, int W, float beta, float eps, void* stream);
int p2i_shock_map_bwd(const float* x, const float* dout, float* dx, float* scratch, int N, int H, int W, float beta, float eps,
                      void* stream);
int p2i_shock_loss_fwd(const float* pred, const float* truth, float* out, int N, int H, int W, int pool, int border, float beta,
                       float eps, void* stream);
int p2i_shock_loss_bwd(const float* pred, const float* truth, const float* dout, float* dpred, float* scratch, int N, int H,
                       int W, int pool, int border, float beta, float eps, void* stream);

/* ------------------------------------------------------------------ optimiser
 * torch.optim.Adam step on flat fp32 buffers (train.py:125-136): no weight decay, no amsgrad. */
int p2i_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
             float beta2, float eps, int step, void* stream);

/* ------------------------------------------------------------------ batch assembly
 * Loader post-processing on the device (sti_dataset.py:209,223-224; train.py:468-473): frames = u8/255,
 * masks = (mask_u8 != 0), masked = frames*masks, all (B,T,1,H,W) fp32.  mask_u8 has mask_numel elements:
 * H*W (one gauge map for all frames and samples: `stis`/`sti`), T*H*W or B*T*H*W. */
int p2i_assemble_batch(const uint8_t* frames_u8, const uint8_t* mask_u8, int64_t mask_numel, float* frames,
                       float* masked, float* masks, int B, int T, int H, int W, void* stream);

/* ------------------------------------------------------------------ sliding-window inference (infer.py:188-262)
 * Window w of an event (L frames of HW floats) = frames w*step .. w*step+win-1, frames past the end repeat the last one
 * (infer.py:219-227).  p2i_window_gather builds windows w0 .. w0+nw-1 of up to two tensors (masked frames and masks) as
 * (nw, win, HW); p2i_window_mean turns the generator's predictions for ALL nwin windows, (nwin, win, HW), into the event:
 * out[l] = max(0, scale * mean over the windows that hold frame l) (the repeated copies are not counted, infer.py:229-245). */
int p2i_window_gather(const float* a, const float* b /*may be NULL*/, float* wa, float* wb, int L, int64_t HW, int w0, int nw, int win,
                      int step, void* stream);
int p2i_window_mean(const float* pred_windows, float* out, int L, int64_t HW, int nwin, int win, int step, float scale, void* stream);

/* ------------------------------------------------------------------ evaluation metrics
 * metrics/metric.py on the device.  p2i_metrics_pointwise (one pass over pred/target, n elements): sums2[0] += sum|d|,
 * sums2[1] += sum d^2 with d = T(pred) - T(target), T(x) = 10^(x/16)*0.036 when apply_transform (RegressionMetrics.update
 * :42-52); counts[k*4 + {0 hits, 1 misses, 2 false alarms, 3 correct negatives}] += ... for T(pred), T(target) >=
 * thresholds[k] (CategoricalMetrics.update :92-111; always transformed); bits (may be NULL): byte plane, bit k =
 * T(pred)>=thr[k], bit 4+k = T(target)>=thr[k], the input of p2i_metrics_fss.  thresholds/scales are HOST arrays (<= 4).
 * p2i_metrics_fss (FractionalSkillScoreMetric.update :152-170): num/den[k*ns + s] += sum over the avg_pool2d(kernel s,
 * stride 1, padding s/2) fraction fields of (fp-ft)^2 and fp^2+ft^2; the caller divides by N*ho*wo (ho = H+2*(s/2)-s+1).
 * Scales are 1..64; more than 4 thresholds or scales, a scale outside that range and n or N <= 0 are refused with P2I_EINVAL.
 * Counts, bit plane, the integer regression sums and the power-of-two FSS sums are compared exactly over sizes, block
 * boundaries and grid-stride trips by tests/test_metric_kernels_gpu.py (cases: tests/metric_cases.py). */
int p2i_metrics_pointwise(const float* pred, const float* target, int64_t n, const float* thresholds_host, int nt,
                          int apply_transform, float* sums2, unsigned long long* counts, uint8_t* bits, void* stream);
int p2i_metrics_fss(const uint8_t* bits, int N, int H, int W, int nt, const int* scales_host, int ns, float* num, float* den,
                    void* stream);

/* Same update with the step counter kept on the device: step_dev[0] is incremented by the call and the bias
 * corrections are derived from it there (coef2: 2 floats of scratch), so that the launch can be captured in a hipGraph
 * and replayed every training step. */
int p2i_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                 float eps, int32_t* step_dev, float* coef2, void* stream);

/* small helpers on the same stream */
int p2i_axpy(float* y, const float* x, float a, int64_t n, void* stream);        /* y += a*x */
int p2i_add2(float* out, const float* a, const float* b, int64_t n, void* stream);   /* out = a + b (the skip x_4 + res1, p2igan.py:95) */
int p2i_zero(float* p, int64_t n, void* stream);                                     /* memset 0 on the stream */
/* out = dy * act'(y) for a saved post-activation tensor y (may alias dy): ReLU / LeakyReLU(0.2) / tanh backward */
int p2i_act_bwd(const float* dy, const float* y, int act, float* out, int64_t n, void* stream);
int p2i_bias_grad(const float* dy, const float* y_act, int act, float* db, int B, int C, int64_t inner, void* stream);
/* both in one pass: out = dy * act'(y) and db[c] += its sum over samples and positions (db zeroed by the caller; inner % 4 == 0) */
int p2i_act_bwd_bias(const float* dy, const float* y, int act, float* out, float* db, int B, int C, int64_t inner, void* stream);

/* ---- Native step sequencer: launch tapes (round 4).
 * Replaces the per-launch host work of the reference's step and inference loops -- scripts/train.py:240-326 (one G+D iteration),
 * scripts/infer.py:217-241 (one window batch) -- which on this build is ~400 kernel launches + ~400 other calls issued one by one
 * through the binding (7.1 ms of host time per step, whatever the batch).  Between p2i_tape_begin and p2i_tape_end every kernel
 * launch, memset and stream dependency this library enqueues ON THE CALLING THREAD is also appended to a tape (the calls execute as
 * usual, or are captured if the stream is capturing); p2i_tape_replay re-enqueues the recorded operations with the recorded
 * arguments in one call.  Rules:
 *   - the tape holds HOST memory only (opaque handle, freed by p2i_tape_free); every device buffer it names is the caller's and
 *     must still be alive, at the same address, when it is replayed (the Python engine records inside a private memory pool);
 *   - operations recorded on `origin_stream` are replayed on the origin stream given to p2i_tape_replay (the caller's current
 *     stream); operations on other streams (side streams) are replayed on those same streams;
 *   - cross-stream dependencies must be expressed through p2i_event_record / p2i_event_wait (slots 0..255 of a per-thread table
 *     of events without timing) to be seen by a tape; enqueue-only like everything else, no synchronisation;
 *   - host-side values baked into kernel arguments are replayed as recorded (use p2i_adam_dev, whose step counter lives on the
 *     device). */
/* ---- Pre-split source planes (round 4, EXPERIMENT: measured, not used by the engine -- DESIGN.md section 7).  p2i_x6_split_planes:
 * fp32 activations (B, C, P) (P = frames x pixels, C % 8 == 0) -> their exact 3-way bf16 split as planes [plane][b][C/8][P][8]
 * (3 * B * C * P bf16, caller-owned).  A forward / data-gradient call given them as p2i_conv_split.src_planes reads its source from
 * these planes instead of splitting the fp32 tensor in the kernel (32-channel tiles with whole-chunk stages; any other tile ignores
 * them); the same deconv_pytorch.py:103-109 convolution, bit-equal results
 * (tests/test_ops_gpu.py::test_presplit_source_planes_are_bit_equal). */
int p2i_x6_split_planes(const float* x, void* planes, int B, int C, int64_t P, void* stream);

/* ---- Run-to-run reproducibility (round 4).  The step's small cross-workgroup sums (bias / position / attention-weight / alpha
 * gradients, spectral-norm dot products, the 1 -> 32 layer's weight gradient, the IDW backward scatter) are float atomics by
 * default: their order, hence their rounding, changes from run to run (the reference on CPU is deterministic).  With a scratch
 * registered here they are summed in a fixed order instead (the workgroups store their partials, one more small launch adds them
 * in workgroup order; bias gradients ride in the weight-gradient slices; the IDW scatter runs in 64-bit fixed point).  part: >= 65 536
 * floats (the Python binding gives 128 MB: pieces are handed out round-robin and must not be reused while an earlier kernel may
 * still run); counters: >= 1 024 unsigned, zero-initialised (reserved).
 * Process-wide (one GPU per process); part == NULL unregisters. */
int p2i_det_workspace(float* part, int64_t part_floats, unsigned* counters, int n_counters);
int p2i_event_record(int slot, void* stream);
int p2i_event_wait(int slot, void* stream);
int p2i_tape_begin(void* origin_stream);
int p2i_tape_end(void** tape_out);
/* counts4: kernels, memsets, event operations, distinct streams */
int p2i_tape_info(const void* tape, int* counts4);
int p2i_tape_replay(const void* tape, void* origin_stream);
int p2i_tape_free(void* tape);

/* ---- STDK baseline (spatio-temporal DeepKriging, reference models/stdk.py).  The reference builds a
 * [B*T*H*W, K_s + K_t + 79 T] feature tensor and runs nn.Linear x 4 over it (stdk.py:149-186); here layer 1 is split by its input
 * blocks -- P = phi_s W1s^T [HW][112], Q[b][t] = phi_t[t] W1t^T + z[b] W1z^T + b1 [B*T][112] (columns >= 100 are zero) -- and the
 * other three layers run fused over the rows (b, t, p) without writing anything but y.  Weights are the reference's nn.Linear
 * tensors as they are: w1 [100][K_s + K_t + Kz], w2 / w3 [100][100], w4 [1][100].
 * p2i_stdk_basis: phi[i][k] = Wendland-C2(|pos_i - knot_k| / theta_k) (stdk.py:26-35, 188-276) for the H x W grid pos_i = (i / W, i % W);
 *   knots [K][2] as (y, x) floats (the temporal basis is H = T, W = 1 with knots (t, 0)).
 * p2i_stdk_select: per (b, t) frame the first k of [pixels with mask != 0 in raster order, then pixels with mask == 0 in raster
 *   order] -> idx [BT][k] (int32), z [BT][k] = masked[idx] (replaces topk(mask, k, sorted=False) + gather, stdk.py:143-147, 173-175,
 *   under the build's tie rule); HW >= k.
 * p2i_stdk_layer1_fwd: P, zt [T][112], zb [B][112] (scratch), Q.  p2i_stdk_mlp_fwd: y [BT][HW].
 * p2i_stdk_bwd_workspace: floats needed by p2i_stdk_mlp_bwd's four scratch buffers (rows5, dp_part, dq_part, wpart).
 * p2i_stdk_mlp_bwd: from dy [BT][HW]: dP [HW][100] (sum over b, t), dQ [BT][100] (sum over p) and the gradients of layers 2..4;
 *   all cross-workgroup sums are partials added in a fixed order (run-to-run identical).
 * p2i_stdk_layer1_bwd: dw1 [100][F] and db1 from dP, dQ; dqt [T][100], dqb [B][100] scratch, part [splits][100][F] scratch. */
int p2i_stdk_basis(const float* knots, const float* theta, int K, int H, int W, float* phi, void* stream);
int p2i_stdk_select(const float* masked, const float* mask, int BT, int HW, int k, int* idx, float* z, void* stream);
int p2i_stdk_layer1_fwd(const float* phi_s, const float* phi_t, const float* z, const float* w1, const float* b1, int B, int T, int HW,
                        int Ks, int Kt, int Kz, float* P, float* zt, float* zb, float* Q, void* stream);
int p2i_stdk_mlp_fwd(const float* P, const float* Q, const float* w2, const float* b2, const float* w3, const float* b3, const float* w4,
                     const float* b4, int HW, int BT, float* y, void* stream);
int p2i_stdk_bwd_workspace(int HW, int BT, int64_t* sizes4);
int p2i_stdk_mlp_bwd(const float* P, const float* Q, const float* w2, const float* b2, const float* w3, const float* b3, const float* w4,
                     const float* dy, int HW, int BT, float* rows5, float* dp_part, float* dq_part, float* wpart, float* dP, float* dQ,
                     float* dw2, float* db2, float* dw3, float* db3, float* dw4, float* db4, void* stream);
int p2i_stdk_layer1_bwd(const float* phi_s, const float* phi_t, const float* z, const float* dP, const float* dQ, int B, int T, int HW,
                        int Ks, int Kt, int Kz, float* dqt, float* dqb, float* part, int splits, float* dw1, float* db1, void* stream);

/* ---- exp1 scoring (reference experiments/exp1.py run_exp1 + experiments/io.py).  Inputs are DEVICE arrays
 * of dtype P2I_EXP1_U8 / _F32 / _F64, contiguous [T][h][w]; every statistic is fp64.  transform_mmhr(x) = clip(10^min(max(x,
 * 0.001) [/3] / 16, 38) * 0.036, 0, 200) (exp1.py:151-159); uint8 values go through lut[256] (computed on the host by numpy).
 * An input travels as ONE descriptor, p2i_eval_input (a HOST struct, read during the call only): the array, its dtype code, its
 * frame extent h x w and the origin (top, left) of the crop the call reads from every frame; each input has its own extent and
 * origin, the crop's size is the call's (S x S, or rows x cols).  A NULL descriptor or NULL data is refused like a NULL array.  This
 * and every later evaluation unit take their inputs this way.
 * p2i_exp1_transform: out[i] = transform_mmhr(x[i]) (fp64; the check of the device pow).
 * p2i_exp1_workspace: doubles of `part` that p2i_exp1_accumulate needs for T frames of an S x S crop.
 * p2i_exp1_accumulate: one aligned piece of T frames; the crop is [top, top + S) x [left, left + S) of each input; rank[S*S]
 *   (int32) is the pixel's position in the mode's selection or -1.  part[T][workgroups][P2I_EXP1_NSTAT] gets per workgroup: n,
 *   sum|d|, sum d^2, the truth's Welford (mean, M2), the count / min / max of the f32 casts that are finite and > 0.5, and per
 *   threshold (HOST array, <= P2I_EXP1_MAX_THR) hits / misses / false alarms.  Writes the avg_pool2d(pool) f32 frames of the
 *   whole crop, pool_*[T][S/pool][S/pool] (pool 1 or 8), and the selected f32 casts, sel_*[T][nsel].
 * p2i_exp1_merge: acc[P2I_EXP1_NSTAT] (+)= part[0 .. nparts) in a fixed order (the partials of a method's pieces, in frame order).
 * p2i_exp1_hist: per frame t the 50-bin histograms of sel_pred / sel_truth over the range in acc (np.histogram's edges and bin
 *   rule): flag[t] = both non-empty, score[t] = sum min(p / (sum p + 1e-12), g / (sum g + 1e-12)); edges[52] = the 51 edges + a
 *   status (1: not strictly increasing).
 * p2i_exp1_ssim: ssim[t] = SSIM(pred_t, truth_t); d1[t] (t >= 1), d2[t] (t >= 2) = SSIM(p_t, p_t-L) - SSIM(g_t, g_t-L), for the
 *   method's whole stack of T pooled frames of npix values.
 * p2i_exp1_finalize: out[P2I_EXP1_NOUT(nthr)] = MAE, RMSE, PSS, SSIM, DTSSIM_L1, DTSSIM_L2, NSE, per threshold POD, FAR, CSI, HSS,
 *   then a status (1: np.histogram would raise "Too many bins for data range"). */
#define P2I_EXP1_U8 0
#define P2I_EXP1_F32 1
#define P2I_EXP1_F64 2
#define P2I_EXP1_MAX_THR 8
#define P2I_EXP1_NSTAT (8 + 3 * P2I_EXP1_MAX_THR)
#define P2I_EXP1_NOUT(nthr) (8 + 4 * (nthr))
typedef struct { const void* data; int dtype, h, w, top, left; } p2i_eval_input;   /* [T][h][w] of P2I_EXP1_U8/_F32/_F64, crop origin (top, left) */
int p2i_exp1_transform(const void* x, int dtype, int64_t n, int divide_by_3, double* out, void* stream);
int p2i_exp1_workspace(int T, int S, int pool, int64_t* part_doubles);
int p2i_exp1_accumulate(const p2i_eval_input* pred, const p2i_eval_input* truth, int T, int S, int pool, const int* rank, int nsel,
                        const double* lut, const double* thresholds_host, int nthr, int divide_by_3, float* pool_pred, float* pool_truth,
                        float* sel_pred, float* sel_truth, double* part, void* stream);
int p2i_exp1_merge(const double* part, int64_t nparts, double* acc, void* stream);
int p2i_exp1_hist(const float* sel_pred, const float* sel_truth, int T, int nsel, const double* acc, double* score, int* flag,
                  float* edges, void* stream);
int p2i_exp1_ssim(const float* pool_pred, const float* pool_truth, int T, int npix, double* ssim, double* d1, double* d2, void* stream);
int p2i_exp1_finalize(const double* acc, const double* thresholds_host, int nthr, int T, const double* score, const int* flag,
                      const float* edges, const double* ssim, const double* d1, const double* d2, double* out, void* stream);

/* ---- exp3 analysis (reference experiments/exp3.py run_exp3 + experiments/io.py).  Inputs are DEVICE arrays
 * as for exp1 (p2i_eval_input descriptors, the same transform and uint8 table); statistics are fp64, counts are integers.
 * p2i_exp3_accumulate: one aligned piece of T frames, crops [top, top + S) x [left, left + S); rank[S*S] >= 0 marks the mode's
 *   selection.  Writes rec[T][P2I_EXP3_NREC] = per frame (n, sum (p-g)^2, truth mean, truth M2) over the selection's finite
 *   pairs; rows[T][S] (int32) = per crop row the scatter pool: pixels of the whole crop with p and g finite and g >= 0.1; and, when
 *   hist is not NULL, adds the prediction's counts to hist[P2I_EXP3_NHIST]: 64 bins of np.linspace(0, 32, 65) over the finite
 *   values in [0, 32] (bin min(floor(2 x), 63)), then the count of finite values.
 * p2i_exp3_truth_hist: adds the same P2I_EXP3_NHIST counts of T truth frames to hist.
 * p2i_exp3_scan: prefix[i] = rows[0] + ... + rows[i] (int64), i < n: the inclusive prefix of a method's row counts.
 * p2i_exp3_gather: for i < K, the pool ordinal ords[i] (int64) of a method: when it falls in this piece's rows [row0, row0 + T*S)
 *   of the method's prefix, out_g[i] / out_p[i] = the transformed truth / prediction of that pool pixel (raster order); other
 *   entries are left as they are.
 * p2i_exp3_nse: out[0] = the NSE of the fold of stack_rec[0 .. T) (fixed order; NaN when empty); out[1 + e], e < E = nanmean of
 *   max(NSE, 0) over the frames event_off[e] .. event_off[e+1] - 1 of event_rec (event_off: DEVICE int32 [E + 1]). */
#define P2I_EXP3_NREC 4
#define P2I_EXP3_BINS 64
#define P2I_EXP3_NHIST (P2I_EXP3_BINS + 1)
int p2i_exp3_accumulate(const p2i_eval_input* pred, const p2i_eval_input* truth, int T, int S, const int* rank, const double* lut,
                        int divide_by_3, double* rec, int* rows, uint64_t* hist, void* stream);
int p2i_exp3_truth_hist(const p2i_eval_input* truth, int T, int S, const double* lut, int divide_by_3, uint64_t* hist, void* stream);
int p2i_exp3_scan(const int* rows, int64_t n, int64_t* prefix, void* stream);
int p2i_exp3_gather(const p2i_eval_input* pred, const p2i_eval_input* truth, int T, int S, const double* lut, int divide_by_3,
                    const int64_t* prefix, int64_t row0, const int64_t* ords, int K, double* out_g, double* out_p, void* stream);
int p2i_exp3_nse(const double* event_rec, const int* event_off, int E, const double* stack_rec, int T, double* out, void* stream);

/* ---- exp2 comparison renders (reference experiments/exp2.py run_exp2 / _save_combo_gif / run_exp2_paper_zarr; DESIGN.md section
 * 12).  Inputs are DEVICE arrays as for exp1 (p2i_eval_input descriptors, the same transform and uint8 table).
 * p2i_exp2_index: out[n][S][S] (uint8, any alignment) = the colour index of the first n of the input's T frames' crop [top, top + S) x [left,
 *   left + S): clip(searchsorted_right(bounds, transform_mmhr(x)) - 1, 0, 140) over the P2I_EXP2_NBOUNDS fp64 bounds (DEVICE,
 *   ascending), decided by fp64 >= compares; NaN -> P2I_EXP2_BAD.
 * p2i_exp2_compose: out[n][Hc][pitch] (uint8; pitch a multiple of 16, out and chrome 16-byte aligned) = chrome[Hc][pitch] with
 *   panel p of panels[P][n][S][S] magnified zoom x zoom (nearest) at rows [oy, oy + S zoom), columns [ox + p step, ox + p step +
 *   S zoom).  Panel p with bit p of gauge_bits set is instead the index bg plus one disc per point of points[K][2] (DEVICE int32
 *   (row, column), each inside [0, S)), in the order given, the later point on top: in doubled coordinates d2 = (2 y + 1 - (2 row
 *   + 1) zoom)^2 + (2 x + 1 - (2 column + 1) zoom)^2 of panel pixel (y, x); with R = 3 zoom, d2 <= (R - 2)^2 takes the panel's
 *   own index at the point (bg where that is P2I_EXP2_BAD), (R - 2)^2 < d2 <= R^2 takes the index edge. */
#define P2I_EXP2_NBOUNDS 142
#define P2I_EXP2_BAD 141
int p2i_exp2_index(const p2i_eval_input* in, int T, int S, int n, const double* bounds, const double* lut, int divide_by_3,
                   uint8_t* out, void* stream);
int p2i_exp2_compose(const uint8_t* panels, int P, int n, int S, int zoom, unsigned gauge_bits, const int* points, int K,
                     const uint8_t* chrome, int Hc, int pitch, int oy, int ox, int step, int bg, int edge, uint8_t* out, void* stream);

/* ---- classical baselines: ordinary kriging (dual form, global neighbourhood) and all-gauge IDW per (b, t) frame (DESIGN.md
 * section 14; no counterpart in the reference).  F = B T frames of H x W (both <= 16384, F <= 65535).  The gauges of a frame are its
 * pixels with mask != 0 in raster order; cap (a multiple of 32, <= 4096) is the row length of every per-gauge array.  Covariance
 * C(h) = psill (1 - g(h / a)), model 0: g(r) = 1 - exp(-r), model 1: g(r) = 1.5 r - 0.5 r^3 (r < 1), 1 beyond; params [B][4] fp32 =
 * (nugget, psill, range a, unused) per sample.  A "system" s of a call is the gauge set of frame f0 + s R, with R = 1 (one system
 * per frame) or R = T and f0 a multiple of T (one system per sample whose frames share their mask, R + 1 right-hand sides); systems
 * are padded to np (a multiple of 32, <= cap) with identity rows and zero right-hand sides.  All sums run in a fixed order.
 * p2i_krig_compact: pix [F][cap] (int32 (y << 16) | x), z [F][cap] = masked there (both zero past the count), info [2 F]: info[f] =
 *   the frame's gauge count (it may exceed cap: only the first cap gauges are stored, the caller refuses), info[F + f] = 1 if the
 *   frame's mask pattern differs from that of its sample's first frame.
 * p2i_krig_bins: fp64 partial variogram bins part [F][chunks][n_lags][3] = (pairs, sum (z_i - z_j)^2 / 2, sum h) over the pairs
 *   i < j of a frame with h < n_lags lag_width, bin min(floor(h / lag_width), n_lags - 1); n_lags <= 32.
 * p2i_krig_fit: per sample (nparts = T chunks partials each, added in order): bins [B][n_lags][3] (the sums), then for the 25 range
 *   candidates a_c = lag_width 2^((c - 6) / 3) the count-weighted least squares (nugget, psill) of gamma(h) = nugget + psill g(h / a)
 *   over the non-empty bins' means (nugget < 0: nugget = 0 and psill alone; psill not > 0: invalid); fit [B][4] fp64 = (nugget, psill,
 *   range, weighted SSE) of the smallest SSE (lowest c on a tie), cand [B] its index or -1 (degenerate sample: no valid candidate),
 *   params [B][4] the fp32 copy for the calls below.
 * p2i_krig_factor: L [nsys][np][np] fp32 (lower triangle) = the Cholesky factor of K = [C(|x_i - x_j|)] + nugget I; status[s] is set
 *   to 1 where a pivot is not > 0 (the caller zeroes it beforehand).
 * p2i_krig_solve: K u = 1 and K v = z_f for the R frames of each system (sol [nsys][R + 1][np] fp64 scratch), then mean[f] = 1^T v /
 *   1^T u and alpha [F][cap] = v - mean u (zero past the count).  A frame without gauges gets (0, 0); a frame of a degenerate sample
 *   (cand[b] < 0; cand may be NULL) or of a system with status != 0 gets its gauge mean and alpha = 0.
 * p2i_krig_predict: out [F][H W] = mean[f] + sum_i alpha[f][i] (C(|p - x_i|) + nugget [p = x_i]) for the frames f0 .. f0 + nsys R.
 * p2i_idw_all: out [F][H W] = sum_i w_i z_i / sum_i w_i, w_i = |p - x_i|^-power; z_i on a gauge pixel; 0 for a frame without gauges. */
int p2i_krig_compact(const float* masked, const float* mask, int B, int T, int H, int W, int cap, int* pix, float* z, int* info,
                     void* stream);
/* A chunk of nsys systems of one call, stated once for the nine dense stages below (ABI v3).  A stage refuses a NULL field among those
 * it reads ("null pointer"); one it does not read may be NULL, and so may cand wherever it is read.  Reads, besides f0, R, T, nsys, cap
 * (all nine) and np (all but p2i_krig_predict, whose nsys is its number of sets):
 *   p2i_krig_factor, p2i_stkrig_factor: pix, counts, params, model, status     p2i_krig_predict: pix, counts, params, model
 *   p2i_krig_solve, p2i_krig_loo, p2i_stkrig_loso: z, counts, status, cand     p2i_krig_variance: pix, counts, params, model, status, cand
 *   p2i_krig_cs_weights: pix, z, counts, status, cand                          p2i_krig_cs_predict: every field
 * The space-time stages take samples for frames: pix = stpix, z = stz, counts = stcounts, R = T = 1, f0 = the first sample. */
typedef struct p2i_krig_systems {
  const int* pix;      /* [rows][cap] (y << 16) | x */
  const float* z;      /* [rows][cap] */
  const int* counts;   /* p2i_krig_compact's info / p2i_stkrig_gather's stcounts */
  const float* params; /* [samples][4] */
  const int* cand;     /* [samples] or NULL (fixed parameters) */
  int* status;         /* [nsys] of THIS chunk */
  int model, f0, R, T, nsys, np, cap;
} p2i_krig_systems;
int p2i_krig_bins(const int* pix, const float* z, const int* counts, int F, int cap, int chunks, int n_lags, double lag_width,
                  double* part, void* stream);
int p2i_krig_fit(const double* part, int B, int nparts, int n_lags, double lag_width, int model, double* bins, double* fit, int* cand,
                 float* params, void* stream);
int p2i_krig_factor(const p2i_krig_systems* sys, float* L, void* stream);
int p2i_krig_solve(const p2i_krig_systems* sys, const float* L, double* sol, float* alpha, float* mean, void* stream);
int p2i_krig_predict(const p2i_krig_systems* sys, const float* alpha, const float* mean, int H, int W, float* out, void* stream);
int p2i_idw_all(const int* pix, const float* z, const int* counts, int F, int H, int W, int cap, float power, float* out, void* stream);

/* ---- kriging variance and leave-one-out (LOO) cross-validation of the classical baselines (no counterpart in
 * the reference).  Symbols, systems (f0, R, T, nsys, np, cap) and the frame rules are those of the block above; W = L^-1, u = K^-1 1
 * (row 0 of each system's sol), s = 1^T u, c0(p, i) = C(|p - x_i|) + nugget [p = x_i], c00 = psill + nugget.
 * p2i_krig_invert: Winv [nsys][np][np] fp32 = the inverse of each system's factor L (lower triangular, zeros above, identity on the
 *   padding), by 32-wide tiles; Winv must not alias L.
 * p2i_krig_variance: var [F][H W] = max(0, c00 - |W k(p)|^2 + (1 - u^T k(p))^2 / s), k(p) = [c0(p, i)]_i, written to the R frames of
 *   each system; exactly 0 on a gauge pixel; NaN everywhere for a system without gauges, with status != 0 or of a degenerate sample
 *   (cand[b] < 0; cand may be NULL).  sol, status as left by p2i_krig_solve / p2i_krig_factor for the same (f0, R, nsys, np).
 * p2i_krig_loo: colsq [nsys][np] fp64 (scratch) = the column square-sums of Winv; then for gauge i of each of the systems' frames
 *   B_ii = colsq_i - u_i^2 / s, pred [F][cap] = z_i - alpha_i / B_ii, var [F][cap] = 1 / B_ii; NaN for a frame with fewer than 2
 *   gauges, of a degenerate sample or of a system with status != 0; 0 past the frame's count.
 * p2i_idw_loo: pred [F][cap] = sum_{j != i} w_j z_j / sum_{j != i} w_j, w_j = |x_i - x_j|^-power (fp32 weights, fp64 sums); NaN with
 *   fewer than 2 gauges; 0 past the count.
 * p2i_loo_scores: out [5] fp64 = (n, sum e, sum |e|, sum e^2, sum e^2 / var) with e = z - pred over the entries i < counts[f] whose
 *   pred (and var, unless var is NULL: then out[4] = 0) is not NaN; part [F][5] fp64 is scratch.  Fixed order. */
int p2i_krig_invert(const float* L, int nsys, int np, float* Winv, void* stream);
int p2i_krig_variance(const p2i_krig_systems* sys, const float* Winv, const double* sol, int H, int W, float* var, void* stream);
int p2i_krig_loo(const p2i_krig_systems* sys, const float* Winv, const double* sol, const float* alpha, double* colsq, float* pred,
                 float* var, void* stream);
int p2i_idw_loo(const int* pix, const float* z, const int* counts, int F, int cap, float power, float* pred, void* stream);
int p2i_loo_scores(const float* z, const float* pred, const float* var, const int* counts, int F, int cap, double* part, double* out,
                   void* stream);

/* ---- conditional simulation of ordinary kriging (no counterpart in the reference): M ensemble members per
 * frame that carry the variogram's texture and equal z at every gauge.  Symbols, systems (f0, R, T, nsys, np, cap) and the frame
 * rules are those of the two blocks above.  The unconditional fields live on the torus Sy x Sx = (e H) x (e W), both <= 512.
 * p2i_krig_cs_spectrum: per sample b, in fp64 from the fp32 params: base[j][k] = C(sqrt(dj^2 + dk^2)) + nugget [dj = dk = 0], dj =
 *   min(j, Sy - j), dk = min(k, Sx - k); lambda = Re DFT2(base) as two cosine products over twiddle [Sy + Sx] fp64 (DEVICE, computed
 *   on the host: cos(2 pi m / Sy), m < Sy, then cos(2 pi m / Sx), m < Sx); amp [B][Sy][Sx] fp32 = sqrt(max(lambda, 0) (sum lambda /
 *   sum max(lambda, 0)) / (Sy Sx)); clip [B] fp64 = sum max(-lambda, 0) / sum |lambda|.  work: 2 B Sy Sx fp64 of scratch.  A
 *   degenerate sample (cand[b] < 0; cand may be NULL) gets amp = 0 and clip = NaN.
 * p2i_krig_cs_noise: xi [npairs][Sy][Sx][2] fp32, the complex standard normal of torus cell j Sx + k and member pair q0 + q: with
 *   (r0, r1, ., .) = Philox4x32-10 of counter (j Sx + k, q0 + q, stream_id low, high) under key (seed low, high): rho^2 = -2 ln((r0 +
 *   1) 2^-32), taken as -2 log1p(-(2^32 - 1 - r0) 2^-32) for r0 >= 2^31; xi = rho (cos, sin)(2 pi r1 2^-32).
 * p2i_krig_cs_fields: for the frames f0 .. f0 + nframes - 1 and every pair q < (M + 1) / 2: Y = DFT2(amp[f / T] xi)[:H, :W] with
 *   xi of (seed, streams[f], q) drawn in the loader, as two products on v_mfma_f32_32x32x2_f32 over tx [2][Sx][W] and ty [2][Sy][H]
 *   fp32 (cos, then sin, of 2 pi k w / Sx and 2 pi j h / Sy; DEVICE, rounded from fp64 on the host); ens [F][M][H W]: member 2q = Re
 *   Y, member 2q + 1 = Im Y (dropped past M).  P: nframes ((M + 1) / 2) 2 Sy W fp32 of scratch.  streams [F] int64.
 * p2i_krig_cs_weights: for column c = t M + m of system s (frame fs + t, member m; ens holds U there): r = z - U(gauges), v = Winv^T
 *   (Winv r), mu [nsys][R M] = u^T r / s, alpha [nsys][R M][cap] = v - mu u (0 past the count), sums in fp64.  sol, status, Winv as
 *   left by p2i_krig_solve / p2i_krig_factor / p2i_krig_invert for the same (f0, R, nsys, np).  No model: alpha = 0, mu = 0.
 * p2i_krig_cs_predict: ens[fs + t][m][p] = U + mu + sum_i alpha_i c0(p, i), in place, as an MFMA product of alpha with c0 evaluated
 *   once per (pixel, gauge) for all columns of the system; a gauge pixel is written as the frame's z there; NaN everywhere for a
 *   system without gauges, with status != 0 or of a degenerate sample.  1 <= M <= 64. */
int p2i_krig_cs_spectrum(const float* params, const int* cand, int model, int B, int Sy, int Sx, const double* twiddle, double* work,
                         float* amp, double* clip, void* stream);
int p2i_krig_cs_noise(uint64_t seed, int64_t stream_id, int q0, int npairs, int Sy, int Sx, float* xi, void* stream);
int p2i_krig_cs_fields(const float* amp, const int64_t* streams, const float* tx, const float* ty, uint64_t seed, int f0, int nframes,
                       int T, int M, int H, int W, int Sy, int Sx, float* P, float* ens, void* stream);
int p2i_krig_cs_weights(const p2i_krig_systems* sys, const float* Winv, const double* sol, const float* ens, int M, int H, int W,
                        float* alpha, float* mu, void* stream);
int p2i_krig_cs_predict(const p2i_krig_systems* sys, const float* alpha, const float* mu, int M, int H, int W, float* ens, void* stream);

/* ---- space-time ordinary kriging (no counterpart in the reference): every pixel of every frame of a sample
 * from all gauges of all frames of that sample, one system per sample.  Point i of a sample has pixel (y_i, x_i), frame t_i and value
 * z_i; the points are the frames' gauges as p2i_krig_compact leaves them, frame-major.  Distance d = sqrt(dy^2 + dx^2 + kappa^2
 * dt^2), kappa > 0 in pixels per frame, inside the covariance of the classical block; params [B][4] fp32 = (nugget, psill, range a,
 * kappa) per sample.  pix / z / counts are p2i_krig_compact's per-frame arrays with row length fcap; cap (a multiple of 32, <= 4096)
 * is the row length of the per-sample arrays; systems are padded to np (a multiple of 32, <= cap).  All sums run in a fixed order.
 * vel / velf: NULL here; the sample velocities of the Lagrangian block below otherwise.  The solve is p2i_krig_solve with the samples standing in for frames (F = B, R = T = 1, z = stz, counts = stcounts): a sample
 * without gauges gets (0, 0), a degenerate or failed one its gauge mean over all its frames.
 * p2i_stkrig_gather: stpix [B][cap] ((y << 16) | x), stt [B][cap] (frame index), stz [B][cap] (all zero past the count), stcounts [B]
 *   = the sum of the sample's frame counts (it may exceed cap: only the first cap points are stored, the caller refuses).
 * p2i_stkrig_bins: fp64 partial bins part [B][n_tlags + 1][chunks][n_lags][3] = (pairs, sum (z_i - z_j)^2 / 2, sum h), h the SPATIAL
 *   distance: temporal lag u = 0 holds the pairs i < j of one frame, u >= 1 all pairs (i in frame t, j in frame t + u); a pair with h
 *   < n_lags lag_width goes to bin (u, min(floor(h / lag_width), n_lags - 1)).  n_lags <= 32, n_tlags <= 7 and < T.
 * p2i_stkrig_fit: bins [B][n_tlags + 1][n_lags][3] (the chunks added in order), then for the 17 x 25 candidates kappa_q = 2^((q - 6) /
 *   2), a_c = lag_width 2^((c - 6) / 3) the count-weighted least squares (nugget, psill) of gamma = nugget + psill g(sqrt(hbar^2 +
 *   (kappa_q u)^2) / a_c) over the non-empty bins, with p2i_krig_fit's fallbacks; fit [B][5] fp64 = (nugget, psill, range, kappa,
 *   weighted SSE) of the smallest SSE, cand [B] = its q 25 + c (the lowest on a tie) or -1 (degenerate sample), params [B][4].
 * p2i_stkrig_factor: L [nsys][np][np] fp32 = the Cholesky factor of K = [C(d(i, j))] + nugget I of samples s0 .. s0 + nsys - 1, by
 *   p2i_krig_factor's panel / update kernels; status[s] is set to 1 where a pivot is not > 0 (the caller zeroes it beforehand).
 * p2i_stkrig_predict: out [B][T][H W] = mean[b] + sum_i alpha[b][i] (C(d((t, p), i)) + nugget [p = x_i and t = t_i]). */
int p2i_stkrig_gather(const int* pix, const float* z, const int* counts, int B, int T, int fcap, int cap, int* stpix, int* stt,
                      float* stz, int* stcounts, void* stream);
int p2i_stkrig_bins(const int* pix, const float* z, const int* counts, const double* vel, int B, int T, int cap, int chunks, int n_lags,
                    int n_tlags, double lag_width, double* part, void* stream);
int p2i_stkrig_fit(const double* part, int B, int chunks, int n_lags, int n_tlags, double lag_width, int model, double* bins,
                   double* fit, int* cand, float* params, void* stream);
int p2i_stkrig_factor(const p2i_krig_systems* sys, const int* stt, const float* velf, float* L, void* stream);
int p2i_stkrig_predict(const int* stpix, const int* stt, const float* alpha, const float* mean, const int* stcounts,
                       const float* params, const float* velf, int model, int B, int T, int H, int W, int cap, float* out, void* stream);

/* ---- leave-one-site-out (LOSO) cross-validation of space-time kriging (no counterpart in the reference).  A
 * site is the set of a sample's points that share a pixel (at most one per frame).  With W = L^-1, u = K^-1 1, s = 1^T u and alpha the
 * dual coefficients, for a site S: B_SS = (W^T W)_SS - u_S u_S^T / s, e_S = B_SS^-1 alpha_S, zhat_-S = z_S - e_S, sigma^2_-S =
 * diag(B_SS^-1).  The system is built by p2i_stkrig_factor / p2i_krig_solve / p2i_krig_invert on the site-major point set.  W is fp32,
 * everything after it fp64; all sums run in a fixed order.
 * p2i_stkrig_gather_sites: the sample's points sorted by (pixel, frame) in p2i_stkrig_gather's layout (stpix, stt, stz [B][cap],
 *   stcounts [B]), with site_start [B][cap + 1] (the first point of site g; entries nsites[b] .. cap hold the point count), nsites [B],
 *   psite [B][cap] (site of a sorted point, -1 past the count), back [B][cap] (t fcap + rank within frame t, -1 past the count) and
 *   fsite [B T][fcap] (site of a frame's gauge in p2i_krig_compact's layout, -1 past the frame's count).  fcap, cap <= 4096.
 * p2i_stkrig_site_gram: gram [nsys][np / 32][2][32][32] fp64: for column tile J the tiles G[J][J] and G[J + 1][J] of G = Winv^T Winv
 *   (the second is zero for the last J).  A run of at most 32 consecutive columns lies inside these.
 * p2i_stkrig_loso: for every site of samples s0 .. s0 + nsys - 1 writes zhat_-S to pred and sigma^2_-S to var, both [B T][fcap] in
 *   p2i_krig_compact's layout, at the site's points only (the caller zeroes them).  NaN for a site whose B_SS has a pivot not > 0 and
 *   for every point of a sample with one site only, a degenerate fit (cand[b] < 0; cand may be NULL) or status[s] != 0.  T <= 32. */
int p2i_stkrig_gather_sites(const int* pix, const float* z, const int* counts, int B, int T, int fcap, int cap, int* stpix, int* stt,
                            float* stz, int* stcounts, int* site_start, int* nsites, int* psite, int* back, int* fsite, void* stream);
int p2i_stkrig_site_gram(const float* Winv, int nsys, int np, double* gram, void* stream);
int p2i_stkrig_loso(const p2i_krig_systems* sys, const double* gram, const double* sol, const float* alpha, const int* site_start,
                    const int* nsites, const int* back, int T, int fcap, float* pred, float* var, void* stream);

/* ---- Lagrangian space-time ordinary kriging (no counterpart in the reference): the space-time block above with
 * its distance measured in the frame that moves with the rain, d = sqrt((dy - v_y dt)^2 + (dx - v_x dt)^2 + kappa^2 dt^2), dy, dx, dt
 * the integer pixel and frame differences of two points and v = (v_y, v_x) the sample's advection velocity in pixels per frame.  The
 * nugget applies at dt = 0 and dy = dx = 0 only.  vel [B][2] fp64 and velf [B][2] fp32 hold (v_y, v_x) per sample; the velocity
 * estimate and the bins are fp64, K, its factor and c0 fp32, the predictor's sum fp64.  All sums run in a fixed order.  Gather, fit,
 * solve, inverse and the leave-one-site-out entry points are the space-time block's (p2i_stkrig_gather, p2i_stkrig_fit,
 * p2i_krig_solve, p2i_krig_invert, p2i_stkrig_gather_sites, p2i_stkrig_site_gram, p2i_stkrig_loso), unchanged.
 * p2i_lagkrig_velocity: candidates v = (i, j) vstep, |i|, |j| <= nhalf <= 16, index c = (i + nhalf) n + (j + nhalf), n = 2 nhalf + 1.
 *   Over the pairs (gauge a in frame t, gauge b in frame t + u), 1 <= u <= n_tlags (<= 7, < T), of p2i_krig_compact's per-frame
 *   arrays, with w = exp(-|x_b - x_a - v u|^2 / (2 bandwidth^2)) (bandwidth in pixels): part [B][chunks][n n][3] = the partial sums
 *   of (w, w (z_a - z_b)^2 / 2, w over the pairs with x_b != x_a) of workgroup `chunks` index (it takes the rows a = chunk mod chunks).
 * p2i_lagkrig_pick: adds the chunks in order into weight [B][n n] = W(v) = sum w, support [B][n n] = N(v) = sum w over the pairs of
 *   distinct pixels and score [B][n n] = (sum w (z_a - z_b)^2 / 2) / W(v) (+inf where W(v) = 0), and takes the candidate of the
 *   smallest score among those with N(v) >= N(0) / 2; ties go to the smaller i^2 + j^2, then to the lower c (no pair, or zero
 *   variance: v = 0).  vel, velf [B][2] = (i, j) vstep, vcand [B] = c.
 * The three stages that see the distance are the space-time block's entry points with a velocity in place of NULL; a NULL velocity
 * IS the plain space-time model, so the library cannot tell a forgotten one: the caller checks that it has one (the Python binding's
 * lagkrig_* wrappers do, and that is the only such guard).
 * p2i_stkrig_bins with vel: h = |x_j - x_i - v u| for a pair (i in frame t, j in frame t + u); the same part layout, to be fitted by
 *   p2i_stkrig_fit.  With vel = 0 the bins are the NULL call's bit for bit.
 * p2i_stkrig_factor, p2i_stkrig_predict with velf: the distance above (one device function serves both and is symmetric in its two
 *   points bit for bit, so a gauge is reproduced in its own frame at nugget 0). */
int p2i_lagkrig_velocity(const int* pix, const float* z, const int* counts, int B, int T, int cap, int chunks, int n_tlags, int nhalf,
                         double vstep, double bandwidth, double* part, void* stream);
int p2i_lagkrig_pick(const double* part, int B, int chunks, int nhalf, double vstep, double* score, double* weight, double* support,
                     double* vel, float* velf, int* vcand, void* stream);

/* ---- moving-neighbourhood space-time ordinary kriging (no counterpart in the reference): every target is
 * predicted from its k nearest points in the space-time metric, from a k x k system of its own.  pix / z / counts are
 * p2i_krig_compact's per-frame arrays (fcap slots per frame, B T frames); there is no limit on the points of a sample.  params [B][4]
 * fp32 = (nugget, psill, range, kappa); cand [B] (nullable: p2i_stkrig_fit's, < 0 marks a degenerate sample).
 * Candidates of a target in frame t: the points of its sample in frames t' with |t' - t| <= frames (0 <= frames < T).  Key, fp64:
 * (dy^2 + dx^2) + (kappa kappa) dt^2, one rounded product and one rounded sum.  Neighbours: the first m = min(k, candidates) in
 * ascending (key, frame, raster index), 1 <= k <= 64.  With K_ij = C(d(i, j)) + nugget [i = j], c0_i = C(d(target, i)) + nugget [same
 * pixel and frame], d the fp32 distance of the space-time block above: K a = c0, K u = 1, mu = (1^T a - 1) / 1^T u, lambda = a - mu u,
 * prediction lambda^T z, variance psill + nugget - lambda^T c0 - mu clamped at 0 (exactly 0 on a gauge pixel in its own frame).  K, its
 * factor and c0 are fp32, every sum fp64 in a fixed order.  stat [B][2] fp64 (written): the sample's gauge mean and point count.
 * Rules: a sample without gauges gives 0 and NaN variance; a degenerate sample its gauge mean and NaN; a target without a candidate
 * the sample's gauge mean and NaN; a non-positive pivot the mean of the selected values and NaN, and adds 1 to status [B] (int32,
 * zeroed by the caller).
 * p2i_lkrig_predict: out, var (nullable) [B][T][H W]; nbr (nullable) [B][T][H W][k] int32 = the selection of the kernel itself, point
 *   index t' fcap + slot in selection order, -1 past m.
 * p2i_lkrig_loso: the points as targets, each without the candidates at its own pixel (leave-one-site-out); pred, var [B T][fcap], 0
 *   past the frame's count, NaN where no candidate is left or the sample is degenerate.
 * velf: NULL for all of the above.  Otherwise the same two in the Lagrangian frame: velf [B][2] fp32 = (v_y, v_x)
 * in pixels per frame, one velocity per sample.  Key, fp64, every operation rounded once and none fused: with fdt = t - t' (target minus
 * point), e_y = (t_y - g_y) - v_y fdt and e_x likewise (one product, one sum each), key = ((e_y e_y + e_x e_x) + (kappa kappa) dt^2); the
 * order is (key, point index).  d in K and c0 is the fp32 Lagrangian distance of the block above (sqrt((dy - v_y dt)^2 + (dx - v_x dt)^2
 * + kappa^2 dt^2)); the nugget stays on the same pixel and frame, leave-one-site-out leaves out the target's pixel in every frame, and
 * everything else is as above.  With v = 0 the key and the selection are those of the NULL call bit for bit. */
int p2i_lkrig_predict(const int* pix, const float* z, const int* counts, const float* params, const int* cand, int model, int k,
                      int frames, int B, int T, int H, int W, int fcap, double* stat, float* out, float* var, int* status, int* nbr,
                      const float* velf, void* stream);
int p2i_lkrig_loso(const int* pix, const float* z, const int* counts, const float* params, const int* cand, int model, int k, int frames,
                   int B, int T, int fcap, double* stat, float* pred, float* var, int* status, const float* velf, void* stream);

/* ---- scale-aware verification: fractions skill score and radially averaged power spectra (no counterpart in
 * the reference).  Inputs are DEVICE arrays as for exp1 (p2i_eval_input descriptors, the same transform and uint8 table); every pixel of the crop [top, top + S) x [left, left + S) counts, S <= P2I_SCALE_MAX_CROP.
 * p2i_scale_fss: one aligned piece of T frames.  For threshold q (HOST array, <= P2I_EXP1_MAX_THR) and window size n >= 1 (HOST
 *   array, <= P2I_SCALE_MAX_SCALES), with I_p = (pred >= q), I_g = (truth >= q) (NaN compares false) and c(y, x) = the number of set
 *   pixels in rows y - n/2 .. y - n/2 + n - 1 and the same range of columns (outside the crop: 0): part[T][nthr][3 nscales + 1]
 *   (int64) = per scale sum c_p^2, sum c_g^2, sum c_p c_g over the frame, then sum I_g.  workspace NULL: 16-bit tables in LDS, S <=
 *   P2I_SCALE_LDS_CROP; otherwise uint32 [T][nthr][2][S][S] of table workspace, any S.  The integers are the same on both paths.
 * p2i_scale_fss_merge: acc[i] += sum_t part[t][i], i < n (int64).
 * p2i_scale_dft_rows: G[t][field][y][kx][2] (fp64 re, im) = sum_x f[y][x] exp(-2 pi i x kx / S), kx <= S/2, of the transformed crop
 *   f of T frames of ONE input (field 0: prediction, 1: truth; G holds both); twiddle [2][S] = cos, sin(2 pi m / S) (DEVICE, computed
 *   on the host); nanflag[t][2] (int32, zeroed by the caller) is set to 1 where the crop holds a NaN.
 * p2i_scale_dft_cols: psd[t][field][ky][kx] = |sum_y G[..][y][kx] exp(-2 pi i y ky / S)|^2 / S^2 for both fields.
 * p2i_scale_rings: P[t][field][r] = (sum_{i in [offsets[r], offsets[r+1])} weight[i] psd[..][order[i]]) / count[r], r < R = S/2 + 1,
 *   summed in list order (order: int32 indices ky (S/2 + 1) + kx; weight, count: fp64; all DEVICE).
 * p2i_scale_spectrum_merge: out[field][r] = the mean of P[t][field][r] in frame order over the frames t < T with nanflag[t][0] ==
 *   nanflag[t][1] == 0 (NaN when there is none); out[2 R] = the number of frames left out. */
#define P2I_SCALE_MAX_SCALES 16
#define P2I_SCALE_LDS_CROP 128
#define P2I_SCALE_MAX_CROP 1024
int p2i_scale_fss(const p2i_eval_input* pred, const p2i_eval_input* truth, int T, int S, const double* lut,
                  const double* thresholds_host, int nthr, const int* scales_host, int nscales, int divide_by_3, void* workspace,
                  int64_t* part, void* stream);
int p2i_scale_fss_merge(const int64_t* part, int64_t T, int n, int64_t* acc, void* stream);
int p2i_scale_dft_rows(const p2i_eval_input* in, int T, int S, int field, const double* lut, int divide_by_3, const double* twiddle,
                       double* G, int* nanflag, void* stream);
int p2i_scale_dft_cols(const double* G, int T, int S, const double* twiddle, double* psd, void* stream);
int p2i_scale_rings(const double* psd, int T, int S, const int* order, const double* weight, const int* offsets, const double* count,
                    int R, double* P, void* stream);
int p2i_scale_spectrum_merge(const double* P, const int* nanflag, int64_t T, int R, double* out, void* stream);

/* ---- probabilistic verification of a prediction and its variance against the truth (no counterpart in the
 * reference).  Inputs are DEVICE arrays as for exp1 (p2i_eval_input descriptors); the crop is rows x cols.  Scored on the inputs'
 * own 0-255 scale in fp64: per pixel mu = pred, s2 = var (a NULL var descriptor, or one with NULL data: var_scalar for every pixel), y = truth, sigma = sqrt(s2), Phi / phi the standard normal cdf / pdf, predictive
 * distribution N(mu, s2), left-censored at 0 when `censor`; mu' = max(mu, 0) under censoring, mu otherwise; e = y - mu';
 * z = (y - mu) / sigma, l = -mu / sigma.  rank[rows * cols] (int32; NULL: every pixel) selects the pixels with rank >= 0.  A
 * selected pixel is SKIPPED when mu, s2 or y is NaN, s2 < 0, or (censor and y < 0); every other selected pixel is scored.
 * p2i_prob_record: the record's word counts nf (fp64) and ni (int64) for these sizes (K thresholds, L levels, E edges -> NS = E + 1
 *   sigma-bins, NB PIT bins, RB reliability bins).  A record is nf doubles followed by ni int64:
 *     fp64  [0] sum CRPS   sigma > 0, plain:    sigma [z (2 Phi(z) - 1) + 2 phi(z) - 1/sqrt(pi)]
 *                          sigma > 0, censored: sigma [-l Phi(l)^2 + z (2 Phi(z) - 1) + 2 phi(z) - 2 phi(l) Phi(l)
 *                                                      - (1 - Phi(l sqrt 2)) / sqrt(pi)];  sigma == 0: |e|
 *           [1] sum e  [2] sum |e|  [3] sum e^2  [4] sum s2  [5] sum z  [6] sum z^2 (the last two over sigma > 0 only)
 *           [7 ..+L)   sum of interval widths hi - lo per level: lo, hi = mu -+ h sigma, both clamped at 0 under censoring
 *           [..+K)     sum p per threshold: p = Phi((mu - xq) / sigma); sigma == 0: p = 1[transform_mmhr(mu') >= q]
 *           [..+K)     sum (p - o)^2 per threshold: o = 1[transform_mmhr(y) >= q] through exp1's uint8 table / device pow
 *           [..+NS)    sum s2 per sigma-bin: bin = the number of edges <= sigma (0: underflow, E: overflow)
 *           [..+NS)    sum e^2 per sigma-bin
 *     int64 [0] scored pixels  [1] skipped pixels  [2] scored pixels with sigma == 0
 *           [3 ..+L)   pixels with lo <= y <= hi per level
 *           [..+K)     sum o per threshold
 *           [..+NB)    PIT histogram in units of 2^-32: weight 1 in bin min(floor(u NB), NB - 1), u = Phi(z); sigma == 0: u = 0,
 *                      0.5, 1 for y <, ==, > mu'.  Censored, sigma > 0 and y == 0: with P0 = Phi(l) and m = min(floor(P0 NB),
 *                      NB - 1), rint(2^32 (P0 - m / NB) / P0) in bin m (P0 == 0: weight 1 in bin 0) ...
 *           [..+NB)    ... and the PIT prefix table: rint(2^32 / (NB P0)) at m - 1 when m > 0, standing for that weight in every
 *                      bin 0 .. m - 1: histogram[j] = pit[j] + sum_{i >= j} prefix[i]
 *           [..+NS)    pixels per sigma-bin
 *           [..+K RB)  pixels per (threshold, reliability bin min(floor(p RB), RB - 1))
 *           [..+K RB)  sum o per (threshold, reliability bin)
 *           [..+K RB)  sum rint(2^32 p) per (threshold, reliability bin)
 * p2i_prob_accumulate: one aligned piece of T frames; writes one record per P2I_PROB_WG_PIXELS consecutive pixels of the piece
 *   (frame-major, row-major) to part (part_words = its capacity in 64-bit words).  thresholds (mm/h), xq (the same on the pixel
 *   scale), halfwidths (Phi^-1((1 + level) / 2)) and edges (ascending) are HOST arrays.  No floating-point atomics: the same bits on
 *   every run.
 * p2i_prob_merge: acc[w] += the sum of part[0 .. nparts)[w] in a fixed order (64 strided partial sums in ascending record order, then
 *   a tree), w < nf as fp64, the rest as int64. */
#define P2I_PROB_MAX_LEVELS 8
#define P2I_PROB_MAX_EDGES 16
#define P2I_PROB_MAX_PIT_BINS 64
#define P2I_PROB_MAX_REL_BINS 32
#define P2I_PROB_WG_PIXELS 1024
int p2i_prob_record(int nthr, int nlevels, int nedges, int pit_bins, int rel_bins, int* nf, int* ni);
int p2i_prob_accumulate(const p2i_eval_input* pred, const p2i_eval_input* var, double var_scalar, const p2i_eval_input* truth, int64_t T,
                        int rows, int cols, const int* rank, const double* lut, const double* thresholds_host, const double* xq_host,
                        int nthr, const double* halfwidths_host, int nlevels, const double* edges_host, int nedges, int pit_bins,
                        int rel_bins, int censor, int divide_by_3, double* part, int64_t part_words, void* stream);
int p2i_prob_merge(const double* part, int64_t nparts, int nf, int ni, double* acc, void* stream);

/* ---- object-based verification: connected rain objects and their integer moments, for SAL and the object population (DESIGN.md
 * section 23; no counterpart in the reference).  Inputs are DEVICE arrays as for exp1 (p2i_eval_input descriptors, the transform and
 * uint8 table); every pixel of the crop [top, top + S) x [left, left + S) counts, S <=
 * P2I_OBJECTS_MAX_CROP.  R = the transformed pixel (mm/h) and Q = rint(R 2^24) (half-even; 0 for a NaN), Q < 2^32.  Levels: nthr
 * absolute thresholds (HOST array, <= P2I_EXP1_MAX_THR) give the mask R >= q, and one relative level, the last, R >= max(sal_factor
 * Rmax, sal_floor) with Rmax the maximum of the field's own crop in that frame; NaN compares false.  nlev = nthr + 1.  An object is
 * a connected component (connectivity 4 or 8, no wrap, cut at the crop edge) of a level's mask; its label is the smallest raster
 * index y S + x of its pixels.  All results are integers below 200 2^24 2^10 2^20 < 2^62 and do not depend on the path or the run.
 * p2i_objects_quantize: field 0 (prediction) or 1 (truth) of one aligned piece of T frames: q[T][2][S S] (uint32) = Q,
 *   bits[T][2][S S] (uint16) = bit j set where the pixel is in level j's mask, rec[T][2][5] (int64) = sum Q, sum Q y, sum Q x over
 *   the crop, max Q, 1 if the crop holds a NaN.
 * p2i_objects_label: labels[T][2][nlev][S S] = a set pixel's object label, all ones elsewhere; wide == 0: uint16 labels, one
 *   workgroup per record with the labels in LDS, S <= P2I_OBJECTS_LDS_CROP; wide != 0: uint32 labels in the caller's workspace, tiles
 *   of P2I_OBJECTS_TILE^2 labelled in LDS, united across their borders and flattened, any S.
 * p2i_objects_count: lev[T][2][nlev][5] (int64) = objects, their total area, sum Q, sum Q y, sum Q x over object pixels;
 *   counts[T 2 nlev] (int64) = the objects again, contiguous for the scan.
 * p2i_objects_scan: offsets[n + 1] (int64) = the exclusive prefix of counts[n], offsets[n] = the total.
 * p2i_objects_fill: table[rows][6] (int64, ZEROED by the caller, rows = offsets[T 2 nlev]) = per record, from offsets[record], its
 *   objects in ascending label order: label, area, sum Q, max Q, sum Q y, sum Q x.  Overwrites labels. */
#define P2I_OBJECTS_LDS_CROP 128
#define P2I_OBJECTS_TILE 64
#define P2I_OBJECTS_MAX_CROP 1024
int p2i_objects_quantize(const p2i_eval_input* in, int T, int S, int field, const double* lut, const double* thresholds_host, int nthr,
                         double sal_factor, double sal_floor, int divide_by_3, uint32_t* q, uint16_t* bits, int64_t* rec, void* stream);
int p2i_objects_label(const uint16_t* bits, int T, int S, int nlev, int connectivity, int wide, void* labels, void* stream);
int p2i_objects_count(const void* labels, int wide, const uint32_t* q, int T, int S, int nlev, int64_t* lev, int64_t* counts,
                      void* stream);
int p2i_objects_scan(const int64_t* counts, int64_t n, int64_t* offsets, void* stream);
int p2i_objects_fill(void* labels, int wide, const uint32_t* q, int T, int S, int nlev, const int64_t* offsets, int64_t rows,
                     int64_t* table, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* P2I_HIP_H */
