/*
 * cer_mvs.h - C ABI of libcermvs.so: the MI355X (gfx950) kernels behind the CER-MVS
 * depth-inference hot path.  Plain pointers and sizes only; no torch types.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (a torch tensor's data_ptr());
 *     tensors are dense, row-major, float32 unless stated; nothing is allocated inside
 *     (workspace is passed in) and nothing is retained after return;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); the call only
 *     enqueues work on it and returns (asynchronous), so it is hipGraph-capturable;
 *   - return 0 on success, a negative CER_E* for an argument error (nothing was launched),
 *     or a positive hipError_t from the launch; never throws.  Compute entry points keep no state between calls and are
 *     re-entrant; the library holds exactly two pieces of process-wide state, both set through their own entry points and read by later
 *     launches: the per-device overflow flag (cer_overflow_flag) and the cost-volume algorithm selector (cer_cost_build_algo).
 *     (The opt-in kernel forms of round 4 and their switches live in variants/libcermvs_optin.so only: include/cer_mvs_variants.h.)
 *
 * Each function cites the reference interface (file:line under the reference tree) it
 * replaces.  INTEGRATION.md shows the binding a reference maintainer would add.
 */
#ifndef CER_MVS_H
#define CER_MVS_H

#ifdef __cplusplus
extern "C" {
#endif

#define CER_OK 0
#define CER_EINVAL (-1)   /* null pointer / non-positive size                       */
#define CER_ESHAPE (-2)   /* shape not supported by this build (e.g. C % 64 != 0)   */
#define CER_EALIGN (-3)   /* pointer not 16-byte aligned                            */

/* ABI version: major*1000 + minor.  Bumped on any signature change. */
int cer_abi_version(void);
/* Static description of the last-resort error codes above / hipError_t names. */
const char* cer_error_string(int code);
/* Number of visible HIP devices (>=1) or a negative CER_E*; used by loaders to fail loudly. */
int cer_device_count(void);

/* Saturation is never silent.  The split-f16 kernels clamp an operand whose scaled value leaves the f16 range (update block,
 * "s16" path: ReLU-class activations beyond 4094 = 65504 / 2^4; cost-volume feature rows beyond 1023).  cer_overflow_flag
 * registers a caller-owned DEVICE int for the CURRENT device (hipGetDevice; one per device, NULL = off, the default; launches use
 * the flag of the device they run on) that such kernels or into when they clamp.  The kernels of the s16 update loop check
 * what they clamp themselves, in every launch, before the ReLU (so that a NaN is reported, not turned into 0): bit 2 the hidden
 * map of the fused delta head (it never reaches memory), bit 4 the frag16 output of the lookup (c1) and of the RELU epilogue of
 * cer_conv3x3_s16 (c2).  The disparity features that the s16 convs generate (100 * (d[q] - d[p]) at scale 2^6) are clamped
 * beyond |d[q] - d[p]| = 10.235 without a check in the generator: the writers of the disparity (cer_delta_sum_f32, the delta
 * form of cer_lookup_encode_f32) raise bit 8 when !(|d| <= 5.1175) instead.  Tensors written by other kernels are checked after
 * the fact: cer_f16_scan_overflow ors `bit` into *flag if any half of a split-f16 buffer (frag16 tensors, split feature rows;
 * `bytes` % 16 == 0) sits at the f16 maximum or is not finite - a value in (4093, 4094] at scale 2^4 rounds to that half
 * without being clamped, so a scan may report it.  The host reads the flag when convenient.
 * NOT reported (tests/saturation_cases.py lists every clamp): the split of the wide-range "f16x3" kernels and of the encoders'
 * trunk (cer_split1/2/8, the stem, the point-wise convs' PC_YMAX) clamps at +-65504 in the operand's own units, silently - the
 * remedy the saturation error names (activations at scale 1 instead of 2^4) is 16 x wider than the s16 path, not unlimited. */
int cer_overflow_flag(int* flag);
int cer_f16_scan_overflow(const void* data, long bytes, int* flag, int bit, void* stream);

/* ------------------------------------------------------------------------------------
 * alt_cuda_corr.forward  (reference: alt_cuda_corr/correlation.cpp:23-33,
 * correlation_kernel.cu:18-119,260-286).  Literal semantics, any radius:
 *   corr[b,n,ky+rd*kx,h,w] = sum_c fmap1[b,h,w,c] * bilerp(fmap2[b], x-r+kx, y-r+ky),
 *   (x,y) = coords[b,n,h,w,:], rd = 2r+1, texels outside fmap2 read as 0.
 * fmap1 [B,H1,W1,C]  fmap2 [B,H2,W2,C]  coords [B,N,H1,W1,2]  corr [B,N,rd*rd,H1,W1].
 * corr is fully overwritten (the reference zero-fills then accumulates, :273).  C % 64 == 0, C <= 256.
 */
int cer_alt_corr_forward_f32(const float* fmap1, const float* fmap2, const float* coords, float* corr,
                             int B, int N, int H1, int W1, int H2, int W2, int C, int radius, void* stream);

/* alt_cuda_corr.backward (correlation.cpp:36-48, correlation_kernel.cu:122-256,288-324), radius 0:
 * fmap1_grad [B,H1,W1,C] and fmap2_grad [B,H2,W2,C] are overwritten (fmap2_grad is zero-filled
 * inside, then accumulated with atomics); coords_grad is zero-filled, as in the reference (:307).
 */
int cer_alt_corr_backward_f32(const float* fmap1, const float* fmap2, const float* coords, const float* corr_grad,
                              float* fmap1_grad, float* fmap2_grad, float* coords_grad,
                              int B, int N, int H1, int W1, int H2, int W2, int C, int radius, void* stream);
/* Deterministic fmap2 gradient (no float atomics).  cer_alt_corr_backward_f32 with fmap2_grad = NULL
 * gives fmap1_grad only; then
 *   cer_alt_corr_bwd_tuples_f32: per (sample, footprint texel) a key (b*H2*W2 + texel, or the sentinel B*H2*W2 for texels
 *     outside the map), a coefficient and the source pixel (b*H1*W1 + p): arrays of B*N*H1*W1*(2r+2)^2 entries;
 *   the caller sorts the keys stably (`order` = the permutation) and computes seg[t] = first sorted position with key >= t,
 *     t = 0 .. B*H2*W2 (T + 1 entries);
 *   cer_alt_corr_bwd_reduce_f32: fmap2_grad[t, :] = sum of coef * fmap1[src, :] over segment t, in sorted order. */
int cer_alt_corr_bwd_tuples_f32(const float* coords, const float* corr_grad, long* keys, float* coef, int* src,
                                int B, int N, int H1, int W1, int H2, int W2, int radius, void* stream);
int cer_alt_corr_bwd_reduce_f32(const float* fmap1, const long* order, const float* coef, const int* src, const long* seg,
                                float* fmap2_grad, long T, int C, void* stream);

/* ------------------------------------------------------------------------------------
 * Epipolar cost-volume build, one cascade stage (reference: CorrBlock.__init__
 * core/corr.py:56-91, projective_transform utils/projective_ops.py:16-28, direct_corr
 * core/corr.py:28-43 and the kernel above), fused: no coordinate tensors are materialised.
 *
 *   origin[p]   = shift ? (disp_in[p] < (D/2)*incre ? (D/2)*incre : disp_in[p]) : disp_in[p]
 *   hyp[p,k]    = (float)(k - D/2) * incre + origin[p],                       k = 0..D-1
 *   (X,Y,Z,_)   = Pij[v] * (x, y, 1, hyp[p,k]);  (u,w) = clamp((X/Z, Y/Z), +-1e4)
 *   c[v,p,k]    = sum_c fmap1[p,c] * bilerp(fmap2[v], u, w)      (texels outside -> 0;
 *                                                                 non-finite (u,w) -> 0)
 * fmap1 [h1*w1, C] and fmap2 [V, h2+4, w2+4, C] are NHWC and already carry the reference's 1/8
 * scaling (core/corr.py:30-31); fmap2 has a 2-texel ZERO BORDER on every side (texel (y,x) of view v at
 * ((v*(h2+4) + y+2)*(w2+4) + x+2)*C) - the kernel clamps cells into the border instead of testing bounds.
 * Pij [V,4,4] row-major = K_j P_j P_i^-1 K_i^-1.
 *
 * Output rows have `row_stride` floats (>= D, multiple of 4); only columns [0,D) are written
 * here (cer_pyramid_f32 fills the pooled levels behind them).
 *   mode 0: vol [V, P, row_stride], vol[v,p,k] = c[v,p,k]               (per-view, literal)
 *   mode 1: vol [P, row_stride],    vol[p,k]   = sum_v c[v,p,k]         (view-sum fold)
 *   mode 2: as mode 1 but adds into the existing vol (accumulate across calls)
 * (h1, w1) is the reference-pixel grid this call covers and y0 the image row of its first row: a multi-GPU rank that owns
 * a row slab passes its slab height and first row (fmap1 / disp_in / vol then hold only those rows); y0 = 0 otherwise.
 * fuse_levels >= 1 (mode 1, D <= 64 only; else CER_EINVAL): the epilogue also scales level 0 by fuse_scale (1/V: the view mean)
 * and writes the avg-pooled levels 1..fuse_levels-1 behind it - what cer_pyramid_f32(vol, ..., fuse_levels, fuse_scale) would do in
 * a second pass (core/corr.py:94-97).  fuse_levels = 1: level 0 only, SCALED (the level-0-only rows the lookup pools on the fly);
 * fuse_levels = 0: level 0 only, unscaled, fuse_scale ignored, mode 2 allowed.  The same meaning in all three builders
 * (cer_cost_build_f32, cer_cost_lines_f32, cer_cost_lines_reduce_f32) since ABI 1060: before, this entry point treated 1 like 0.
 * origin_out [P] may be NULL.  C % 64 == 0.  `incre` is the reference's Python float (core/raft.py:81): the kernel
 * uses (float)incre for the hypothesis spacing and (float)((D/2)*incre) for the shift limit, as torch does.
 */
int cer_cost_build_f32(const float* fmap1, const float* fmap2, const float* Pij, const float* disp_in,
                       float* vol, float* origin_out,
                       int V, int h1, int w1, int h2, int w2, int C, int D, int row_stride,
                       double incre, int shift, int mode, int y0, int fuse_levels, float fuse_scale, void* stream);
/* Implementation choice of the fold modes (1, 2) of cer_cost_build_f32 when called through the host layer: 0 = automatic
 * (cer_cost_lines_f32 below wherever it applies, else the walk), 1 = always the wave-per-pixel walk.  Returns the previous
 * setting.  (Process-wide switch for tests and A/B timing; the library's entry points themselves are stateless.) */
int cer_cost_build_algo(int algo);

/* ------------------------------------------------------------------------------------
 * The same cost volume (fold modes 1 / 2 of cer_cost_build_f32; C == 64, D <= 64) on epipolar-line tiles
 * (csrc/cost_lines.hip): per source view the reference grid is cut into 32-pixel digital lines along the view's
 * epipolar direction; per (view, tile) the dot products of the tile's reference rows with every texel of the tile's
 * epipolar band are MFMA products (split-f16, fp32-class) and every sample gathers its 4 dots from LDS.  Cells, weights
 * and the treatment of out-of-map / non-finite samples are those of cer_cost_build_f32 (same fp32 expressions); results
 * agree to fp32 rounding of the 64-channel dot.
 *
 * cer_feat_split_f16: fp32 rows [blocks, block_texels, 64] -> split-f16 operand planes, same bytes: per block 8 planes
 *   p = hl * 4 + ks (hl 0 / 1: hi = f16(xs) / lo = f16(xs - hi) of xs = x * 2^6; ks: 16-channel group), each [block_texels][16];
 *   a block = one view (block_texels = (h2+4)*(w2+4), zero border included and kept zero) or the reference map (h1*w1).
 *   |x| > 1023 saturates: *overflow_flag (device int, may be NULL) is or-ed with 1.
 * cer_cost_lines_workspace: bytes of `workspace` (per-view partial volumes [V,P,D] + tile parameters + the hand-over list below).
 * cer_cost_lines_f32: arguments as cer_cost_build_f32 with the split rows in place of fmap1 / fmap2; mode 1 or 2 only.
 *   view_slot (device int [V], may be NULL = identity): view v's rows are block view_slot[v] of fmap2_split - the multi-GPU
 *   forward all-gathers every rank's split rows into one [G, ceil(V/G), ...] buffer and builds from it without a reordering copy.
 */
int cer_feat_split_f16(const float* src, void* dst, long blocks, long block_texels, int C, int* overflow_flag, void* stream);
long cer_cost_lines_workspace(int V, int h1, int w1, int D);
int cer_cost_lines_f32(const void* fmap1_split, const void* fmap2_split, const int* view_slot, const float* Pij, const float* disp_in,
                       float* vol, float* origin_out, void* workspace,
                       int V, int h1, int w1, int h2, int w2, int C, int D, int row_stride,
                       double incre, int shift, int mode, int y0, int fuse_levels, float fuse_scale, int two_term, void* stream);
/* two_term (round 6, ABI 1070; 0 or 1, else CER_EINVAL): 0 = three-term split-f16 dots, fp32-class (4e-8 relative L1 from the walk); 1 = the lo planes
 * of fmap2_split are NOT READ - the source features enter the dots as f16 (the reference rows keep both halves): half the bytes of the band-fragment
 * stream that bounds the tile kernel (stage 0 at the bench workload 1.58 -> 1.02 ms), 1.2e-5 relative L1 on the volume, ~5e-6 on the final disparity.
 * RAFT's "auto" calibration decides per set of weights ("+c2" forms); the planes keep their layout either way.
 * The two halves of cer_cost_lines_f32, for callers that build views as their features become available (RAFT.forward encodes the
 * source views in batches and builds each batch's partial volumes on a second stream while the next batch is being encoded):
 * _views_ writes the partial volumes of views v0 .. v0 + nv - 1 into the V-view workspace (Pij, view_slot, fmap2_split indexed by
 * the absolute view number); _reduce_ sums all V partials in view order into vol (origin, scale, pooled levels as above). */
int cer_cost_lines_views_f32(const void* fmap1_split, const void* fmap2_split, const int* view_slot, const float* Pij, const float* disp_in,
                             void* workspace, int V, int v0, int nv, int h1, int w1, int h2, int w2, int C, int D,
                             double incre, int shift, int y0, int two_term, void* stream);
int cer_cost_lines_reduce_f32(const void* workspace, const float* disp_in, float* vol, float* origin_out, int V, int h1, int w1, int D,
                              int row_stride, double incre, int shift, int mode, int fuse_levels, float fuse_scale, void* stream);

/* Correlation pyramid (reference: core/corr.py:94-97, F.avg_pool2d([1,2]) x (L-1)), in place on
 * rows laid out [level0 (D) | level1 (D/2) | level2 (D/4) | ... | pad]: first level0 *= scale
 * (1/V for the view-mean fold, 1 otherwise), then each level = pairwise mean of the previous.
 * vol [rows, row_stride].
 */
int cer_pyramid_f32(float* vol, long rows, int D, int row_stride, int num_levels, float scale, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-level correlation lookup (reference: CorrBlock.__call__ core/corr.py:102-143 with
 * bilinear_sampler1 utils/bilinear_sampler.py:6-25):
 *   c        = max((disp[p] - origin[p]) / incre + D/2, 0)
 *   out[v, i*(2r+1) + (dx+r), p] = lerp(level_i[v,p,:], c/2^i + dx)   (zero outside the row)
 * vol [nv, P, row_stride] (nv = V per-view, or 1 for the folded volume); out [nv, L*(2r+1), P].
 */
int cer_corr_lookup_f32(const float* vol, const float* origin, const float* disp, long disp_view_stride,
                        float* out, int nv, long P, int D, int row_stride, double incre, int num_levels, int radius,
                        int level0_only /* see cer_lookup_encode_f32 */, void* stream);
/* disp is [P] shared by all views (disp_view_stride = 0; RAFT.forward passes V identical copies,
 * core/raft.py:99) or [nv, P] (disp_view_stride = P). */

/* View aggregation "mean" + first corr_encoder layer on already looked-up features (reference:
 * core/update.py:103,61-62): out[p, co] = relu(b[co] + sum_k w[k, co] * mean_v feats[v, k, p]).
 * feats [nv, K, P] planar (the CorrBlock.__call__ layout), w [K, Cout], out [P, Cout]; Cout == 64. */
int cer_corr_encode_f32(const float* feats, const float* w, const float* b, float* out,
                        int nv, int K, long P, int Cout, void* stream);

/* Same lookup on the folded (view-mean) volume fused with the first corr_encoder layer
 * (reference: core/update.py:103 mean, :61-62 Conv2d(33,64,1)+ReLU): out [P, Cout] NHWC.
 * w [Cin=L*(2r+1), Cout] (transposed 1x1 weight), b [Cout].  Cout == 64.
 * Rows (both lookup entry points): level0_only = 0 - the row holds the whole pyramid [level0 | level1 | ...] (row_stride >= its length,
 *   else CER_ESHAPE) and the levels are read from it; level0_only = 1 (round 5; an explicit argument since ABI 1060 - it used to be
 *   inferred from row_stride, which is ambiguous for D <= 5) - the row holds LEVEL 0 ONLY (row_stride >= D) and level l is formed on the
 *   fly as the pairwise means ((a + b) * 0.5 level by level, core/corr.py:94-97) in the association cer_pyramid_f32 uses: bit-identical
 *   values, 43 % fewer bytes read (RAFT.forward builds its folded volume that way: cer_cost_lines_reduce_f32 with fuse_levels = 1);
 *   at most 4 levels in that form (CER_ESHAPE beyond).
 * delta_taps (may be NULL): the PREVIOUS GRU iteration's disparity update rides on this launch - core/update.py:114, core/raft.py:101:
 *   disp[p] += 0.01 * (delta_bias + sum over delta_nhalf (1 or 2) x 9 tap planes T[half][tap][p + (ky-1, kx-1)], zero outside the
 *   image), i.e. cer_delta_sum_f32 (same summation order: bit-identical), before the lookup of pixel p reads it; `disp` is then
 *   updated IN PLACE (img_w must be given: rows of P / img_w pixels).  With NULL `disp` is only read.
 */
int cer_lookup_encode_f32(const float* vol, const float* origin, float* disp,
                          const float* w, const float* b, float* out,
                          long P, int D, int row_stride, double incre, int num_levels, int radius, int Cout,
                          int out_split /* 0: fp32 [P, Cout]; 1: split32 layout (f16x3 convs); 2: frag16 layout of an image
                                           img_w pixels wide with scale 2^log2s_out (s16 convs) - both below */,
                          int log2s_out, int img_w, const float* delta_taps, int delta_nhalf, float delta_bias, int level0_only,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * 3x3, stride 1, zero-padded convolution as an implicit GEMM on exact-fp32 MFMA
 * (v_mfma_f32_16x16x4_f32), channels-last.  This one kernel family carries every 3x3 of the
 * update block (reference: core/update.py:13-15,63-64,69-71).
 *
 * The K dimension is the concatenation of up to CER_CONV_MAX_SRC sources; source s is
 *   kind 0: a tensor [h*w, ch[s]]                              (ch multiple of 16)
 *   kind 1: the disparity encoder of disp [h*w] (update.py:80-85,97): 49 channels
 *           100*(disp0[y+uy-3, x+ux-3] - disp[y,x]) (disp0 = zero-padded disp), padded to 64
 *   kind 3: (cer_conv3x3_f16x3 only) a tensor [h*w, ch[s]] in the split32 layout described below (ch multiple of 32);
 *           the tensor sources of one call are all kind 0 or all kind 3; weights are packed as for kind 0
 * Weights are pre-packed by cer_conv3x3_pack_f32.  acc is initialised from `init` [h*w, Cout]
 * when non-NULL, else from bias [Cout] (or 0).  Epilogues (epi):
 *   0 LINEAR  out[p,co]  = acc
 *   1 RELU    out[p,co]  = max(acc, 0)
 *   2 GATES   co <  Cout/2: out [p,co] = sigmoid(acc)                (z)
 *             co >= Cout/2: out2[p,co-Cout/2] = sigmoid(acc) * aux[p,co-Cout/2]   (r * net)
 *   3 GRU     q = tanh(acc); out[p,co] = (1 - aux2[p,co]) * aux[p,co] + aux2[p,co] * q
 *             (aux = net, aux2 = z; update.py:23-24)
 */
#define CER_CONV_MAX_SRC 4
#define CER_EPI_LINEAR 0
#define CER_EPI_RELU 1
#define CER_EPI_GATES 2
#define CER_EPI_GRU 3
/* "split32" activation layout (f16x3 kernels only): a [P, C] tensor (C % 32 == 0) whose fp32 slots hold, per pixel and
 * 32-channel chunk, 32 hi halves followed by 32 lo halves (x = hi + 2^-11 lo; same bytes as fp32).  A producer epilogue
 * writes it with CER_EPI_OUT_SPLIT or'ed into `epi` (RELU / LINEAR: out; GATES: out2 = r*h; GRU: out), a consumer reads it
 * as source kind 3 (staging = plain 16-byte copies, no conversion arithmetic) or, with CER_EPI_AUX_SPLIT, as the previous
 * hidden state `aux` of the GATES / GRU epilogues (reconstructed as hi + 2^-11 lo).  cer_split32_f32 converts. */
#define CER_EPI_OUT_SPLIT 0x100
#define CER_EPI_AUX_SPLIT 0x200
/* cer_conv3x3_s16 only: the weights were packed with `collapsed | 2` and the two correction terms of the split-f16 product of the
 * TENSOR sources (xh*wl + xl*wh, 2^-11 of the main term) run on the block-scaled fp8 matrix instruction (twice the f16 rate). */
#define CER_EPI_CORR_FP8 0x400
/* cer_conv3x3_s16 only (round 6): the weights were packed with `collapsed | 4` and the same two correction terms run on the FP6 (e2m3) form of
 * that instruction - half its matrix-pipe passes again - with one E8M0 scale per K block of 16 channels x [hi | lo] on either operand
 * (activations: per pixel, chosen while the halo tile is staged; weights: per output channel and tap, chosen by the packer). */
#define CER_EPI_CORR_FP6 0x800
#define CER_EPI_DELTA 4   /* cer_conv3x3_f16x3 only - see cer_delta_proj_pack */

typedef struct {
    const float* src[CER_CONV_MAX_SRC];
    int ch[CER_CONV_MAX_SRC];     /* logical channels of each source (49 for kind 1) */
    int kind[CER_CONV_MAX_SRC];
    int nsrc;
} cer_conv_inputs;

/* Number of floats cer_conv3x3_pack_f32 writes for (Cout, padded K channels). */
long cer_conv3x3_packed_size(int Cout, int Kpad);
/* Pack OIHW weights [Cout, Cin, 3, 3] whose Cin is the concatenation described by (ch, kind)
 * into the MFMA B-fragment order.  HOST pointers (done once at model load). */
int cer_conv3x3_pack_f32(const float* w_oihw, float* packed, int Cout, int Cin,
                         const int* ch, const int* kind, int nsrc);

int cer_conv3x3_f32(const cer_conv_inputs* in, const float* packed_w, const float* bias, const float* init,
                    float* out, float* out2, const float* aux, const float* aux2,
                    int h, int w, int Cout, int epi, void* stream);

/* Same convolution on the f16 matrix cores with fp32-equivalent accuracy ("f16x3": every fp32 operand is
 * split x = f16(x) + 2^-11 * f16((x - f16(x)) * 2^11); three v_mfma_f32_32x32x16_f16 per tile into two fp32
 * accumulators; the dropped lo*lo term is 2^-22 relative).  Same arguments and epilogues as cer_conv3x3_f32;
 * weights packed by cer_conv3x3_f16x3_pack (size in 2-byte halves from cer_conv3x3_f16x3_packed_size;
 * Kpad = sum over sources of channels rounded up to 32, 64 for kind 1).  Cout % 64 == 0. */
long cer_conv3x3_f16x3_packed_size(int Cout, int Kpad);
int cer_conv3x3_f16x3_pack(const float* w_oihw, void* packed, int Cout, int Cin,
                           const int* ch, const int* kind, int nsrc);
/* `packed_collapsed` (may be NULL): a second packing of the same weights in which a kind-1 source is ONE 81-tap
 * filter on the raw disparity (the 3x3 conv over the 49 unfold features of core/update.py:80-85,97 is linear in
 * the disparity: W9[s] = sum_{t+u=s} w[u][t] minus the centre terms).  Tiles whose pixels all have their 3x3
 * neighbourhood inside the image use it (3 MFMA steps instead of 18 for that source); border tiles keep the
 * literal form.  Built by cer_conv3x3_f16x3_pack_collapsed, size (halves) from cer_conv3x3_f16x3_collapsed_size. */
long cer_conv3x3_f16x3_collapsed_size(int Cout, const int* ch, const int* kind, int nsrc);
int cer_conv3x3_f16x3_pack_collapsed(const float* w_oihw, void* packed, int Cout, int Cin,
                                     const int* ch, const int* kind, int nsrc);
int cer_conv3x3_f16x3(const cer_conv_inputs* in, const void* packed_w, const void* packed_collapsed,
                      const float* bias, const float* init,
                      float* out, float* out2, const float* aux, const float* aux2,
                      int h, int w, int Cout, int epi, void* stream);

/* ---- round 2: the same convolutions, "s16" form (csrc/conv_s16.hip) - the update block's fast path.
 * Arithmetic: every fp32 operand x is carried as the two f16 halves of xs = x * 2^k (k a per-tensor power of two):
 * hi = f16(xs), lo = f16(xs - hi) (unscaled residual), and x*w ~= (xh*wh + xh*wl + xl*wh) / (2^kx 2^kw): three
 * v_mfma_f32_32x32x16_f16 into ONE fp32 accumulator per tile (fp32-class: measured rms error 1.6e-8 of sum|x||w| at
 * K = 1248, an fp32 fmaf chain has 2.7e-8).  All sources of a conv share the product scale 2^log2S = 2^kx(src) 2^kw(src).
 *
 * Tensor layouts (m-tile-major, so that every wave-level access of the kernels is one contiguous KiB).  An m-tile is 2 rows x
 * 16 columns of pixels, lane order li = (y & 1) * 16 + (x & 15); a tensor of an h x w image holds ceil(h/2) * ceil(w/16)
 * m-tiles = cer_s16_padded_pixels(h, w) pixels (allocate [padded pixels, C] floats; padding pixels are never read as data).
 *   "frag16" (split activations, C % 16 == 0): per (m-tile, 16-channel group) 1 KiB of hi halves | 1 KiB of lo halves of
 *       x * 2^log2s; inside a plane the 16-byte piece (kg = (c >> 3) & 1, li) holds channels 8kg .. 8kg+7 (MFMA fragment order);
 *   "acc32"  (fp32, C % 32 == 0): per (m-tile, 32-channel tile, j < 4) 1 KiB, lane (kg, li) holds channels 8j + 4kg + 0..3 -
 *       the accumulator order: `init` of cer_conv3x3_s16 and the output of its LINEAR epilogue;
 *   "f32x8"  (fp32, C % 16 == 0): per (m-tile, 16-channel group, q < 2) 1 KiB, lane (kg, li) holds channels 8kg + 4q + 0..3 -
 *       the z gate between the GATES and GRU epilogues.
 * cer_s16_layout_f32 converts plain fp32 [h*w, C] to layout 0 | 1 | 2 (inverse = 0; log2s used by layout 0) or back.
 *
 * Sources: kind 2 = frag16 tensor (C % 32 == 0) with scale 2^log2sx[s]; kind 1 = disparity [P] fp32, plain (49 encoder
 * channels, generated in the kernel with scale 2^log2sx[s]; at most one).  `ch`/`kind` list the sources in the weights'
 * input-channel order; the packing reorders steps itself (tensors first, disparity last).
 * cer_conv3x3_s16_scale returns log2S for a weight tensor (< -1000 on error); cer_conv3x3_s16_pack builds the literal
 * (collapsed = 0) or collapsed (= 1, needs a kind-1 source; used by interior tiles) packing, size in 2-byte halves from
 * cer_conv3x3_s16_packed_size.  HOST pointers.  `collapsed | 2`: the tensor sources' steps in the fp8-correction form (for launches
 * with CER_EPI_CORR_FP8: per 32-channel tap and 32 output channels 4 KiB = f16 hi halves of the two 16-channel halves | the e4m3
 * A operand of v_mfma_scale_f32_32x32x64_f8f6f4: [lo * 2^5 | hi * 2^-6] of each half); same size.  `collapsed | 4` (round 6): the FP6 form for
 * launches with CER_EPI_CORR_FP6 (the instruction's e2m3 A operand: 32 six-bit fields [lo * 2^11 | hi] of each half over one power of two per
 * lane, whose E8M0 byte follows the 24 bytes of fields; csrc/pack.cpp pack_chunk6); same size.  A launch with CER_EPI_CORR_FP8 / _FP6
 * and a kind-1 source needs packed_collapsed AND edge_w (the fp8 kernels evaluate the disparity source in the collapsed form with
 * the rim correction only; CER_ESHAPE otherwise); tile_mt = 4 is not available for Cout = 64 in that form (3 is used).
 * cer_conv3x3_s16: bias (fp32 [Cout], plain) or init (acc32 [., Cout]) - at most one - seed the accumulators; epilogues:
 *   LINEAR: out acc32 [., Cout];  with CER_EPI_OUT_SPLIT or'ed in, and RELU always: out frag16 with scale 2^log2s_out;
 *   GATES (Cout = 128): out = z f32x8 [., 64], out2 = r * h frag16 (2^log2s_out), aux = h frag16 (2^log2s_aux);
 *   GRU: out = new h frag16 (2^log2s_out), aux = h frag16 (2^log2s_aux; may alias out), aux2 = z f32x8;
 *   DELTA (Cout % 128 == 0): out = tap planes T [Cout/128, 9, h*w] (plain) as for cer_conv3x3_f16x3, aux = projection weights
 *   packed by cer_delta_proj_s16_pack, log2s_aux = their scale.
 * tile_mt: 0 = choose the tile height from (h, w) and the CU count; else force it (tests: 2 | 4 for Cout % 128 == 0,
 * 2 | 3 | 4 for Cout = 64; other values choose automatically). */
long cer_conv3x3_s16_packed_size(int Cout, const int* ch, const int* kind, int nsrc, int collapsed);
int cer_conv3x3_s16_scale(const float* w_oihw, int Cout, int Cin, const int* ch, const int* kind, const int* log2sx, int nsrc);
int cer_conv3x3_s16_pack(const float* w_oihw, void* packed, int Cout, int Cin, const int* ch, const int* kind, const int* log2sx,
                         int nsrc, int collapsed, int log2S);
/* edge_w (may be NULL): rim-correction filters packed by cer_conv3x3_s16_edge_pack (size in 2-byte halves from
 * cer_conv3x3_s16_edge_size; same log2sx / log2S as the weights).  With them EVERY tile evaluates the disparity source in the
 * collapsed form and pixels on the image's 1-pixel rim subtract, as a few extra MFMA steps after the main loop, what the taps
 * whose feature position lies outside the image contributed (the 3x3 conv zero-pads the feature map, core/update.py:80-85);
 * without them border tiles run the literal form (36 steps instead of 6 for that source). */
long cer_conv3x3_s16_edge_size(int Cout);
int cer_conv3x3_s16_edge_pack(const float* w_oihw, void* out, int Cout, int Cin, const int* ch, const int* kind, const int* log2sx,
                              int nsrc, int log2S);
int cer_conv3x3_s16(const cer_conv_inputs* in, const int* log2sx, const void* packed_w, const void* packed_collapsed,
                    const void* edge_w, int log2S, const float* bias, const float* init, float* out, float* out2, const float* aux, const float* aux2,
                    int h, int w, int Cout, int epi, int log2s_out, int log2s_aux, int tile_mt, void* stream);
long cer_delta_proj_s16_packed_size(int C);
int cer_delta_proj_s16_pack(const float* w2_oihw, void* packed, int C, int* log2s_out);
long cer_s16_padded_pixels(int h, int w);
int cer_s16_layout_f32(const float* src, float* dst, int h, int w, int C, int layout, int log2s, int inverse, void* stream);
/* Image rows [y0, y0 + nrows) of a frag16 tensor (h x w image, C channels) -> rows [nrows * w, C] (to_tensor = 0) or back
 * (to_tensor = 1), as bit-exact copies of the 16-byte hi | lo pieces (the row-slab halo exchange). */
int cer_s16_rows_f32(float* tensor, float* rows, int h, int w, int C, int y0, int nrows, int to_tensor, void* stream);

/* fp32 [P, C] -> split32 (inverse = 0) or back (inverse = 1); C % 32 == 0. */
int cer_split32_f32(const float* src, float* dst, long P, int C, int inverse, void* stream);

/* Fused delta head (reference: core/update.py:68-71,114; core/raft.py:101).  cer_conv3x3_f16x3 with epi =
 * CER_EPI_DELTA computes hid = relu(conv3x3(net)) (Cout = 256) but never writes it: each 128-channel block
 * projects its hidden tile onto the nine taps of the following 256->1 conv,
 *   T[half][tap][p] = sum_{c in half} w2[0, c, tap] * hid[p, c],           out = T [Cout/128, 9, h*w],
 * with `aux` = the projection weights packed by cer_delta_proj_pack (2-byte halves, size from
 * cer_delta_proj_packed_size).  cer_delta_sum_f32 finishes:
 *   delta[p] = 0.01 * (bias + sum_half sum_tap T[half][tap][p + tap offset]) (zero padding),
 *   disp_out[p] = disp_in[p] + delta[p]   (delta may be NULL; disp_out may alias disp_in). */
long cer_delta_proj_packed_size(int C);
int cer_delta_proj_pack(const float* w2_oihw, void* packed, int C);
int cer_delta_sum_f32(const float* T, int nhalf, float bias, const float* disp_in, float* disp_out, float* delta,
                      int h, int w, void* stream);

/* delta head tail (reference: core/update.py:70-71,114 and core/raft.py:101):
 *   delta[p] = 0.01 * (b + sum_{tap,c} w[tap,c] * hid[p+tap, c]);  disp_out[p] = disp_in[p] + delta[p]
 * hid [h*w, C] (already ReLU'd), w [9, C] (tap-major), C % 256 == 0.  delta may be NULL.
 */
int cer_delta_tail_f32(const float* hid, const float* w, float bias, const float* disp_in,
                       float* disp_out, float* delta, int h, int w_, int C, void* stream);

/* Fused encoder passes (reference: core/extractor.py:49-57,143-150; InstanceNorm2d defaults :28-31).
 * cer_plane_stats_f32: x [planes, plane_size] (one plane per (image, channel), NCHW) -> stats [planes, 2] =
 *   (mean, 1/sqrt(biased_var + eps)), accumulated in fp64.
 * cer_norm_act_f32: out = relu_out( relu_a(norm(x)) + relu_b(norm_r(res)) ) elementwise; x_stats / res / res_stats
 *   may be NULL (no normalisation / no residual); flags: 1 relu_a, 2 relu_b, 4 relu_out; out may alias x.
 * Planes whose size is not a multiple of 4 take a scalar path. */
int cer_plane_stats_f32(const float* x, float* stats, long planes, long plane_size, float eps, void* stream);
int cer_norm_act_f32(const float* x, const float* x_stats, const float* res, const float* res_stats, float* out,
                     long planes, long plane_size, int flags, void* stream);

/* ------------------------------------------------------------------------------------
 * Encoder engine (reference: core/extractor.py:60-155, BasicEncoder "HR"), channels-last,
 * batched, on the split-f16 MFMA path (fp32-equivalent accuracy):
 *
 * cer_enc_stem_f32      7x7 stride-2 pad-3 conv 3->32 of NCHW images [N,3,H,W] (normalize != 0: x*(2/255)-1 first,
 *                       core/raft.py:40-41) -> raw channels-last [N, ho*wo, 32]; weights [147][32] (ci,ky,kx major).
 * cer_enc_conv_f16x3    k x k (taps = 9 or 1), stride 1 or 2, zero pad k/2, Cin,Cout multiples of 32 (stride 2: Cout
 *                       multiple of 64).  The producer's instance norm + ReLU is applied while staging:
 *                         x' = tf_relu ? relu(n(x)) : n(x),  n(x) = tf_stats ? (x - mean[n,c]) * rstd[n,c] : x.
 *                       epi 0 RAW : out [N, ho*wo, Cout] = conv + bias
 *                       epi 1 FMAP: out [N, (ho+2b)*(wo+2b), Cout] = (conv + bias) * out_scale inside a b-texel border
 *                                   (border texels are NOT written: zero the buffer once)
 *                       epi 2 CTX : channels < Cout/2 -> tanh -> out [N, ho*wo, Cout/2]; the rest -> relu -> out2
 * stats_partial (RAW / stem, may be NULL): per-block (sum, sum of squares) per output channel,
 *                       [N][tiles][Cout][2] with tiles = cer_enc_conv_tiles(...) / cer_enc_stem_tiles(...);
 * cer_enc_stats_reduce_f32  partials -> stats [N*C][2] = (mean, 1/sqrt(biased var + eps)) in fp64 (deterministic).
 * cer_enc_merge_f32     out = relu?( fa(a) + fb(b) ) channels-last, f = optional norm with stats, flags 1 relu a,
 *                       2 relu b, 4 relu sum  (core/extractor.py:49-57).
 * Weights: cer_enc_conv_pack (OIHW -> fragment order; size in 2-byte halves from cer_enc_conv_packed_size). */
int cer_enc_stem_tiles(int ho, int wo);
/* The stem on the matrix cores (csrc/enc_stem.hip): same operands and outputs as cer_enc_stem_f32, single-accumulator split-f16
 * MFMA arithmetic (fp32-class).  Weights are packed once on the host from OIHW [32][3][7][7] (cer_enc_stem_s16_pack returns the
 * power-of-two weight scale it applied in *log2s_w; packed buffer: cer_enc_stem_s16_packed_size() halves = two fragment layouts,
 * the second for the round-4 producer / consumer kernel that serves W % 4 == 0 images with 16-byte loads); stats_partial is
 * [N][cer_enc_stem_s16_tiles(ho, wo)][32][2] (8 x 32-pixel output tiles). */
long cer_enc_stem_s16_packed_size(void);
int cer_enc_stem_s16_tiles(int ho, int wo);
int cer_enc_stem_s16_pack(const float* w_oihw, void* packed, int* log2s_w);
int cer_enc_stem_s16(const float* images, const void* packed_w, const float* bias, float* out, float* stats_partial, int N, int H, int W,
                     int normalize, int log2s_w, void* stream);
int cer_enc_stem_f32(const float* images, const float* wgt_k_co, const float* bias, float* out, float* stats_partial,
                     int N, int H, int W, int normalize, void* stream);
long cer_enc_conv_packed_size(int Cout, int Cin, int taps);
int cer_enc_conv_pack(const float* w_oihw, void* packed, int Cout, int Cin, int taps);
int cer_enc_conv_tiles(int ho, int wo, int stride, int taps, int Cout);
int cer_enc_conv_f16x3(const float* src, const float* tf_stats, int tf_relu, const void* packed_w, const float* bias,
                       float* out, float* out2, float* stats_partial, int N, int h, int w, int Cin, int Cout,
                       int taps, int stride, int epi, int out_border, float out_scale, void* stream);
int cer_enc_stats_reduce_f32(const float* partial, float* stats, int N, int nblk, int C, long pixels, float eps, void* stream);
int cer_enc_merge_f32(const float* a, const float* a_stats, const float* b, const float* b_stats, float* out,
                      int N, long pixels, int C, int flags, void* stream);
/* Round 4: the same convolutions with producer / consumer wave roles (csrc/enc_pc.hip; reference: core/extractor.py:49-57,
 * 143-155).  Operand preparation (the producer layer's instance norm + ReLU, split to hi|lo f16) runs in four producer waves
 * UNDER the matrix work of four consumer waves of the same 512-thread persistent block, and the block's input may be the residual
 * merge of TWO tensors formed on the fly,
 *     x = relu4( relu1(n_A(A)) + relu2(n_B(B)) ),   n(t) = stats ? (t - mean[n,c]) * rstd[n,c] : t,   flags = 1 | 2 | 4 as in
 * cer_enc_merge_f32 (srcB NULL: x = relu1(n_A(A))), so that no merged activation has to be produced by a pass of its own;
 * merged_out (optional, stride 1, needs srcB) receives x once per pixel [N, h*w, Cin] for a later residual branch.
 * Same packed weights (cer_enc_conv_pack), same arithmetic (three f16 MFMA terms, two fp32 accumulators) and the same epilogues
 * (epi 0 RAW / 1 FMAP / 2 CTX) as cer_enc_conv_f16x3; stats_partial (RAW) is [N][cer_enc_pc_tiles(...)][Cout][2].
 * epi 3 FSPLIT (64 -> 64 1x1 only): as FMAP, but the scaled map is written straight into the split-f16 operand planes of
 * cer_cost_lines_f32 - `out` = [N][8 planes][(ho+2b)*(wo+2b)][16] halves, exactly what cer_feat_split_f16 makes of the FMAP output
 * (border texels are not written: zero the buffer once); `out2`, if not NULL, is the device overflow flag (int*; bit 1 on saturation).
 * Shapes: cer_enc_pc_supported(Cin, Cout, taps, stride, epi) != 0 - the "HR" encoder's: 32->32 3x3; 32->64 3x3 / 1x1 stride 2;
 * 64->64 3x3; 64->64 1x1 FMAP; 64->128 1x1 CTX.  Everything else returns CER_ESHAPE (use cer_enc_conv_f16x3).
 * Round 6 (ABI 1070), the FP6-correction form: with `flags & 8` and weights packed by cer_enc_conv_pack_f6 (same size and plane order as
 * cer_enc_conv_pack; the lo planes hold e2m3 K blocks instead) the two correction terms of a 32-channel tap run as ONE
 * v_mfma_scale_f32_32x32x64_f8f6f4 with both operands in e2m3 and one power-of-two scale per (pixel | output channel, 16-channel block):
 * half the matrix-pipe cycles of the three-term f16 form, ~15 instead of ~22 product bits in the correction terms (features 4e-5 relative L1
 * from the f16 form, 7e-6 on the final disparity: RAFT's "auto" calibration decides per set of weights).  Same shapes, epilogues and outputs. */
int cer_enc_pc_supported(int Cin, int Cout, int taps, int stride, int epi);
int cer_enc_pc_tiles(int ho, int wo, int Cout, int taps, int stride);
int cer_enc_conv_pack_f6(const float* w_oihw, void* packed, int Cout, int Cin, int taps);
int cer_enc_pc_conv(const float* srcA, const float* statsA, const float* srcB, const float* statsB, int flags, float* merged_out,
                    const void* packed_w, const float* bias, float* out, float* out2, float* stats_partial, int N, int h, int w,
                    int Cin, int Cout, int taps, int stride, int epi, int out_border, float out_scale, void* stream);

/* NCHW [C,h,w] -> NHWC [h*w,C] with a scale (feature maps: scale = 1/8, core/corr.py:30-31)
 * and NHWC -> NCHW, dst = src * scale in one fp32 rounding.  Any C >= 1 and P >= 1 (64 x 64 tiles through LDS, ragged edges masked;
 * no alignment requirement): the update block passes C = 64 and, for the concatenated GRU input of ConvGRU.forward, C = 177. */
int cer_nchw_to_nhwc_f32(const float* src, float* dst, int C, long P, float scale, void* stream);
int cer_nhwc_to_nchw_f32(const float* src, float* dst, int C, long P, float scale, void* stream);
/* Batched NCHW [N,C,h,w] -> channels-last [N,(h+2b)*(w+2b),C] * scale with a b-texel zero border (the source-map
 * layout of cer_cost_build_f32 with b = 2; reference: core/corr.py:29-35 permute, /8.0, contiguous). */
int cer_nchw_to_nhwc_border_f32(const float* src, float* dst, int N, int C, int h, int w, int border, float scale, void* stream);

/* ---- after the path: geometric-consistency filtering of the depth maps ------------------------
 * One reference depth map against S <= 10 source views, fused (reference: fusion.py:39-83 reproject_with_depth,
 * :86-106 check_geometric_consistency, :226-236 vote and averaged depth; utils/bilinear_sampler.py:32-41).
 *   depth_ref [h*w], depth_src [S, h*w] (device);  cams [S][CER_GEO_CAM_FLOATS] (device), per source view, row-major fp32:
 *     K_ref^-1 [9] | (E_src E_ref^-1) rows 0..2 [12] | K_src [9] | K_src^-1 [9] | (E_ref E_src^-1) rows 0..2 [12] | K_ref [9]
 *   thre1, thre2: the reference's Python floats (mask i, i = 2..10: dist < i/thre1 and |d_reproj - d|/d < i/thre2).
 * Outputs (any may be NULL): geo_mask [h*w] 0/1 (mask10 of all views, or mask_i of >= i views for some i < 1+S),
 * depth_est [h*w] = (sum of mask10-consistent reprojected depths + depth_ref) / (count + 1);
 * mask_count [CER_GEO_COUNTERS] (unsigned): the area of geo_mask is ADDED, spread over the counters (their sum is the area -
 * one hot address would serialise the blocks' atomics).
 * Per-view tensors of the reference's API, written only when the pointer is given: masks9 [9, S, h*w] (0/1),
 * depth_reprojected [S, h*w] (zero outside mask10), x_src, y_src, rel_diff [S, h*w]. */
#define CER_GEO_CAM_FLOATS 60
#define CER_GEO_COUNTERS 64
int cer_geo_consistency_f32(const float* depth_ref, const float* depth_src, const float* cams, int S, int h, int w,
                            double thre1, double thre2, unsigned char* geo_mask, float* depth_est, unsigned int* mask_count,
                            unsigned char* masks9, float* depth_reprojected, float* x_src, float* y_src, float* rel_diff,
                            void* stream);

/* Multi-resolution merge of two depth maps (reference: multires.py:16-40): out [h2, w2] = where(|r - im2| < th * r, im2, r) with
 * r = im1 [h1, w1] resized to [h2, w2] like cv2.resize(INTER_LINEAR) on float32; cer_resize_linear_f32 is that resize alone (the
 * reference's optional down_sample step; equal sizes: a copy, as cv2.resize returns one).  Device pointers, fp32, row-major. */
int cer_multires_merge_f32(const float* im1, int h1, int w1, const float* im2, int h2, int w2, double th, float* out, void* stream);
int cer_resize_linear_f32(const float* src, int h, int w, float* dst, int ho, int wo, void* stream);

/* Training step (ABI 1080; csrc/train_ops.hip, cer-mvs_amd/train.py).  fp32; every output is written whole (no memset needed); no atomics:
 * the same bits on every run.
 *
 * Train-mode lookup (reference: CorrBlock.__call__ core/corr.py:102-143 with test_mode=False, the pyramid core/corr.py:94-97,
 * utils/bilinear_sampler.py:6-25).  corr [V, D, P] is DirectCorr's output as it lies in memory (D-major); origin, disp [P] (the
 * disparity is shared by all views); out [V, L*(2r+1), P].  c = max((disp - origin) / incre + D//2, 0); level l (length D >> l) is the
 * avg-pool by pairs, level by level, formed in LDS; tap t in [-r, r] of level l samples x = t + c / 2^l, bilinear between floor(x)
 * and floor(x)+1, zero outside [0, len_l - 1].  The backward writes grad_corr [V, D, P], the gradient with respect to level 0 (a
 * level-l texel hands g * 2^-l to each of its 2^l level-0 texels); disp and origin get none (the reference detaches both).
 * CER_ESHAPE: D > 128, L > 4, a level shorter than 2 texels, L*(2r+1) > 64, V > 65535.  CER_EINVAL: null pointer, size <= 0,
 * incre <= 0. */
int cer_train_lookup_fwd_f32(const float* corr, const float* origin, const float* disp, float* out, int V, long P, int D,
                             float incre, int num_levels, int radius, void* stream);
int cer_train_lookup_bwd_f32(const float* grad_out, const float* origin, const float* disp, float* grad_corr, int V, long P, int D,
                             float incre, int num_levels, int radius, void* stream);
/* Bilinear upsample with align_corners=True (the loss's F.interpolate, loss.py:18-19), n planes in one launch: in [n, h, w] ->
 * out [n, H, W] in torch's upsample_bilinear2d arithmetic (scale = (float)(h-1)/(H-1), 0 for H == 1; src = scale * dst; i0 = (int)src,
 * the +1 neighbour clamped at the last row / column; lambda = src - i0).  The adjoint is a gather: grad_in [n, h, w] from
 * grad_out [n, H, W] in two passes (x into work [n, H, w], then y); each input texel sums, in ascending order, over the output
 * columns / rows whose footprint holds it - the ranges [range[2j], range[2j+1]) that cer_upsample_ac_ranges writes (range_x: w
 * pairs for (w, W), range_y: h pairs for (h, H), copied to the device by the caller). */
int cer_upsample_bilinear_ac_f32(const float* in, float* out, int n, int h, int w, int H, int W, void* stream);
int cer_upsample_bilinear_ac_bwd_f32(const float* grad_out, float* grad_in, float* work, const int* range_y, const int* range_x,
                                     int n, int h, int w, int H, int W, void* stream);
/* HOST function (range is host memory, 2 * in_size ints): for every input texel j of a resize in_size -> out_size, the half-open range of
 * outputs whose two source texels include j ([0, 0) if none).  Same float arithmetic as the kernels. */
int cer_upsample_ac_ranges(int in_size, int out_size, int* range);

/* Scan session (ABI 1090; csrc/scan_ops.hip, cer-mvs_amd/scan.py): what is done once per image of a scan.  No atomics; the same bits on every run.
 *
 * Image preparation: the reference driver's scale_operation followed by crop_operation (utils/data_utils.py:58-78) in one pass that
 * computes only the crop window.  src: one image on the device - cer_image_prep_u8: [H0, W0, 3] bytes as an image reader returns
 * them (swap_rb != 0: output channel c reads byte 2 - c, BGR -> RGB); cer_image_prep_f32: [3, H0, W0] floats, values 0..255.
 * dst [3, H, W] floats, raw 0..255 (the encoders' stem normalises).  (H2, W2): the size after the resize (the caller's int(s * H0),
 * int(s * W0)); (y0, x0): first row / column of the window inside the resized image; (H, W): the window.  Bilinear with
 * align_corners=True in torch's upsample_bilinear2d arithmetic, as cer_upsample_bilinear_ac_f32 above (the scale is computed once on the host;
 * src = scale * dst, i0 = (int)src clamped to the image, lambda = src - i0); l0y * (l0x a + l1x b) + l1y * (l0x c + l1x d).  H2 == H0 and W2 == W0: a copy
 * (no arithmetic: bit-identical to the source).  CER_EINVAL: null pointer, size <= 0, window outside the resized image;
 * CER_EALIGN: W % 4 == 0 and dst not 16-byte aligned. */
int cer_image_prep_u8(const unsigned char* src, float* dst, int H0, int W0, int H2, int W2, int y0, int x0, int H, int W, int swap_rb,
                      void* stream);
int cer_image_prep_f32(const float* src, float* dst, int H0, int W0, int H2, int W2, int y0, int x0, int H, int W, void* stream);
/* Reference rows: the interior h x w of ONE bordered block of split-f16 operand planes (cer_feat_split_f16's layout: 8 planes of
 * [(h + 2 border) * (w + 2 border)][16 halves], what the encoders' feature head writes for a source view) -> the plain block (8 planes of
 * [h * w][16]) that cer_cost_lines_f32 takes as fmap1_split.  16-byte loads and stores. */
int cer_feat_ref_rows_f16(const void* slot, void* out, int h, int w, int border, void* stream);

/* Point cloud of a fused scan (ABI 1100; csrc/cloud.hip, cer-mvs_amd/fusion.py point_cloud / color_grid): the host tail of the reference's
 * fusion() (fusion.py:262-279) on the device.  masks [N, h, w] bytes (non-zero = set), depth_est [N, h, w], colors [N, 3, h, w] floats 0..1,
 * cams [N, CER_CLOUD_CAM_DOUBLES] DOUBLES per view: K^-1 row-major [9] | rows 0-2 of E^-1 [12] | padding (the float32 inverses, promoted).
 * `order` is HOST memory: the n_order views to emit, each in 0 .. N-1 (checked before anything is launched).  Output: the set pixels of
 * view order[0] first, then order[1], ..., row-major inside a view (numpy's boolean-indexing order) - xyz [n, 3] floats =
 * float(E^-1 (K^-1 (x d, y d, d), 1)), the products and sums in fp64, one rounding; rgb [n, 3] bytes = (uint8)(c * 255.0f), truncated.
 * The order is a function of the masks alone: per-block counts from wave ballots, one 64-bit exclusive scan, ranks from ballot + mbcnt -
 * no atomics, the same bytes on every run.
 *   cer_cloud_partials: HOST function: the number of partial counts, n_order * ceil(h w / CER_CLOUD_TILE), that the workspaces hold:
 *     partials [that many] unsigned, offsets [that many + 1] and view_base [n_order + 1] 64-bit.
 *   cer_cloud_count_u8: count pass + scan.  view_base[k] = points in front of view order[k]; view_base[n_order] = n.  The caller reads
 *     view_base once, allocates exactly n points and passes n as `total` and the allocation as `capacity`.
 *   cer_cloud_emit_f32: the emit pass over the same masks, order and offsets.  Never writes at or beyond `capacity`.  CER_ESHAPE: total !=
 *     capacity; capacity == 0: returns 0 and launches nothing (xyz and rgb may then be NULL).
 * CER_EINVAL: null pointer, size <= 0, an `order` entry outside 0 .. N-1, negative total / capacity.  CER_ESHAPE: h w beyond 2^31 - 1. */
#define CER_CLOUD_TILE 2048
#define CER_CLOUD_CAM_DOUBLES 24
long cer_cloud_partials(int n_order, int h, int w);
int cer_cloud_count_u8(const unsigned char* masks, int N, int h, int w, const int* order, int n_order, unsigned int* partials,
                       long long* offsets, long long* view_base, void* stream);
int cer_cloud_emit_f32(const unsigned char* masks, const float* depth_est, const double* cams, const float* colors, int N, int h, int w,
                       const int* order, int n_order, const long long* offsets, long long total, long long capacity, float* xyz,
                       unsigned char* rgb, void* stream);
/* Colour planes at the depth grid: prepared images [n, 3, H, W], values 0..255 -> colors [n, 3, h, w], values 0..1, for H = k h and W = k w
 * with one integer k >= 1 (CER_ESHAPE otherwise; also for h or 3 n beyond 65535, which are grid dimensions).  Every tap is divided by 255 (IEEE float32 division), then resized as
 * F.interpolate(bilinear, align_corners=False) does on the host (fusion._resize): ly0 * (lx0 a + lx1 b) + ly1 * (lx0 c + lx1 d), every
 * product and sum rounded to float32, no fma.  At an integer ratio the weights are 0, 1/2 or 1 and the result is the host's bit for bit. */
int cer_color_grid_f32(const float* prepared, float* colors, int n, int H, int W, int h, int w, void* stream);
/* inference.disp_to_depth (reference: inference.py:57-58) on n floats: depth = disp == 0 ? 0 : 1 / disp, correctly rounded. */
int cer_disp_to_depth_f32(const float* disp, float* depth, long n, void* stream);

/* Cloud-to-cloud evaluation (ABI 1110; csrc/cloud_eval.hip, cer-mvs_amd/cloud_eval.py): the exact nearest neighbour of every query point in a
 * target cloud within a cut-off - what DTU's accuracy / completeness and Tanks-and-Temples' precision / recall / F are means and shares of.
 * The target is indexed by a sparse uniform grid that exists only as sorted keys (memory follows the points, not the scene's extent).  No
 * atomics; the same bytes on every run.  Points and queries are [n, 3] floats; `origin` is HOST memory, 3 doubles; cell > 0.
 *
 * Sizes (n, m, ncells), in every entry point: negative -> CER_EINVAL; 2^31 or more -> CER_ESHAPE; zero -> CER_OK with nothing launched
 * (decided before the pointers are looked at).  Then: a null pointer, a non-finite origin, a cell that is not a positive finite number, a
 * max_dist that is negative or NaN -> CER_EINVAL.
 *
 *   cer_grid_keys_f32: keys[i] = (cz + B) << 42 | (cy + B) << 21 | (cx + B), B = CER_GRID_COORD_LIMIT - 1, with the cell coordinate
 *     c = floor((double(p) - origin) / cell) per axis (an IEEE fp64 division).  A point with a non-finite coordinate gets the sentinel
 *     2^63 - 1, which sorts last and which no cell's key reaches (every field is at most 2^21 - 2).  clamp == 0 (the target side): a
 *     coordinate with |c| >= CER_GRID_COORD_LIMIT returns CER_ESHAPE - `flag`, one device int of the caller's, carries the finding, and the
 *     call synchronises the stream to read it.  clamp != 0 (the query side, whose keys only order the queries): coordinates are clamped
 *     into the range instead, flag may be NULL and nothing is synchronised.
 *   cer_grid_pack_f32: records[i] = (x, y, z, (int)order[i]) of point order[i], 16 bytes each (CER_EALIGN unless 16-byte aligned): the
 *     target in the order of its stably sorted keys, `order` being the sort's permutation (the original indices).
 *   cer_grid_partials: HOST function: ceil(n / CER_GRID_TILE), the partial counts the cell passes need: partials [that many] unsigned,
 *     offsets [that many + 1] 64-bit.
 *   cer_grid_cells_count_i64: over the SORTED keys: per-block counts of cell heads (a key that is not the sentinel and differs from its
 *     predecessor) and their scan; totals[0] = the number of occupied cells, totals[1] = the number of keys below the sentinel.  The caller
 *     reads totals once and allocates cell_keys [ncells] and cell_start [ncells + 1].
 *   cer_grid_cells_i64: cell_keys[r] = the r-th distinct key, ascending; cell_start[r] = its first sorted position; cell_start[ncells] =
 *     totals[1].  Never writes beyond those sizes.  CER_ESHAPE: ncells > n.  ncells == 0 launches nothing.
 *   cer_grid_nearest_f32: per query, at the query's own position in idx / dist (qorder: the order in which the queries are WALKED, a
 *     permutation of 0 .. m-1 that puts neighbours in space next to each other, or NULL for the input order - it changes the speed only):
 *       dx, dy, dz = fp64 differences of the float32 coordinates; d2 = (dx*dx + dy*dy) + dz*dz in fp64, no contraction;
 *       a target point is a candidate iff d2 <= double(max_dist) * double(max_dist); the winner is the smallest (d2, original index);
 *       idx = its original index, dist = float(sqrt(d2)) with a correctly rounded fp64 square root; no candidate, or a query with a
 *       non-finite coordinate: idx = -1, dist = +inf.  Sentinel-keyed (non-finite) target points are beyond cell_start[ncells]: never seen.
 *     `n` is cell_start[ncells]'s bound (the record count).  The search enumerates ceil(max_dist / cell) + 1 rings of cells around the
 *     query's cell and skips a row or a cell only when the true bounds of the points it can hold, widened by 1e-6 cells against the two
 *     roundings of the key arithmetic, exceed the best distance so far - exactness does not rest on the keys.  CER_ESHAPE: more than 4096
 *     rings (max_dist / cell), ncells > n.  n == 0, ncells == 0 or m == 0: nothing is launched; with m > 0 the caller fills idx = -1 and
 *     dist = +inf itself. */
#define CER_GRID_TILE 2048
#define CER_GRID_COORD_LIMIT (1 << 20)
long cer_grid_partials(long n);
int cer_grid_keys_f32(const float* points, long n, const double* origin, double cell, int clamp, long long* keys, int* flag, void* stream);
int cer_grid_pack_f32(const float* points, const long long* order, long n, void* records, void* stream);
int cer_grid_cells_count_i64(const long long* keys, long n, unsigned int* partials, long long* offsets, long long* totals, void* stream);
int cer_grid_cells_i64(const long long* keys, long n, const long long* offsets, long long ncells, long long* cell_keys, long long* cell_start,
                       void* stream);
int cer_grid_nearest_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells,
                         const double* origin, double cell, const float* queries, const long long* qorder, long m, float max_dist,
                         long long* idx, float* dist, void* stream);

/* Greedy radius thinning on the same grid (ABI 1120; cer-mvs_amd/cloud_eval.py radius_thin): the reduction of the DTU evaluation
 * script - visit the points in a given order; a point that is still in the set stays and removes every point within the radius - as the
 * fixed point of parallel rounds.  The cloud is indexed IN VISITING ORDER (cer_grid_keys_f32 .. cer_grid_pack_f32 on the permuted points), so
 * the fourth word of a record is the point's rank.  `state`: one byte per point of that cloud, non-finite ones included (every record's
 * fourth word indexes it), indexed by rank, zeroed by the caller: 0 undecided, 1 kept, 2 removed.  Point i ends kept iff no kept point j with
 * rank j < rank i has d2(i, j) <= double(radius)^2, d2 as in cer_grid_nearest_f32 (inclusive; exact duplicates are neighbours): the set the
 * sequential loop yields, and the only one.  Sizes and errors as above (n: the record count, n_active <= n; radius must be a positive finite
 * number: CER_EINVAL; more than 4096 rings (radius / cell), ncells > n or n_active > n: CER_ESHAPE).
 *
 *   cer_grid_thin_round_f32: one round.  `active`: n_active sorted positions (indices into records), ascending, or NULL for 0 .. n_active-1.
 *     Every listed point that is still undecided looks at its neighbours of lower rank: one of them kept -> removed; else one of them
 *     undecided -> unchanged; else -> kept.  state is updated in place with plain byte loads and stores (states only move from undecided to
 *     their final value, so a stale read costs a round at most and never a wrong answer): the result of the loop does not depend on the
 *     schedule, the number of rounds may.  The undecided point of lowest rank decides in every round.  The cells are enumerated and cut as in
 *     cer_grid_nearest_f32, against the fixed limit radius^2.
 *   cer_grid_thin_compact_i32: out[0 .. *total) = the entries of `active` (NULL as above) whose point is still undecided, in the list's order;
 *     *total (one device 64-bit integer) = their number.  compact.hpp's count / scan / emit: partials [cer_grid_partials(n_active)] unsigned,
 *     offsets [that many + 1] 64-bit, out [n_active] at most, out != active (CER_EINVAL).  n_active == 0 launches nothing. */
int cer_grid_thin_round_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells,
                            const double* origin, double cell, const int* active, long n_active, float radius, unsigned char* state,
                            void* stream);
int cer_grid_thin_compact_i32(const void* records, long n, const unsigned char* state, const int* active, long n_active,
                              unsigned int* partials, long long* offsets, int* out, long long* total, void* stream);

/* k nearest neighbours and the count within a radius on the same grid (ABI 1140; cer-mvs_amd/cloud_eval.py CloudIndex.knn / knn_mean_distance
 * / count_within, remove_statistical_outliers / remove_radius_outliers).  The first seven arguments are the index as
 * cer_grid_nearest_f32 takes it, queries / qorder / m as there; sizes, errors and their order as there (max_dist and radius: negative or
 * NaN -> CER_EINVAL; more than 4096 rings, ncells > n -> CER_ESHAPE; n == 0, ncells == 0 or m == 0 -> CER_OK with nothing launched, the
 * caller fills the outputs; then null pointers -> CER_EINVAL).  No atomics, no LDS; every output element is written exactly once; the same
 * bytes on every run.  Every check runs before any launch.
 *
 *   cer_grid_knn_f32: d2 = (dx*dx + dy*dy) + dz*dz in fp64 on the float32 coordinates, no contraction; a target point is a candidate iff
 *     d2 <= double(max_dist) * double(max_dist).  Row q of idx / dist ([m, k], at the query's own position) holds the min(k, candidates)
 *     smallest (d2, original index) pairs in ascending lexicographic order: idx = the original index, dist = float(sqrt(d2)) with a
 *     correctly rounded fp64 square root; unused slots are idx = -1, dist = +inf; count[q] = the number of used slots.  A query with a
 *     non-finite coordinate has count 0; a non-finite target point is never a neighbour; a query that is itself an indexed point finds
 *     itself at d2 = 0 (no self-exclusion).  mean[q] (fp64) = ((s_0 + s_1) + ... + s_{c-1}) / c with s_j = sqrt(d2_j) in fp64, added in
 *     ascending order, c = count[q]; +inf for c = 0.  idx, dist and mean may each be NULL (nothing is written there); count may not
 *     (CER_EINVAL).  k < 1 -> CER_EINVAL (with max_dist's check); k > CER_KNN_MAX -> CER_ESHAPE (with ncells > n's).
 *   cer_grid_count_within_f32: count[q] = the number of indexed points with d2 <= double(radius) * double(radius), inclusive (the point
 *     itself when the query is an indexed point); 0 for a query with a non-finite coordinate. */
#define CER_KNN_MAX 32
int cer_grid_knn_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells, const double* origin,
                     double cell, const float* queries, const long long* qorder, long m, int k, float max_dist, long long* idx, float* dist,
                     int* count, double* mean, void* stream);
int cer_grid_count_within_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells,
                              const double* origin, double cell, const float* queries, const long long* qorder, long m, float radius,
                              int* count, void* stream);

/* Surface normals on the same grid (ABI 1150; cer-mvs_amd/cloud_eval.py CloudIndex.normals / estimate_normals): the plane through
 * the k nearest neighbours of every query, by the eigenvectors of their covariance.  The argument head, the sizes, the errors and their order
 * are cer_grid_knn_f32's; points (the array the index was packed from: a record's fourth word indexes it) joins count among the pointers
 * that may not be NULL (CER_EINVAL); viewpoints, normal, curvature and mom may each be NULL.  No atomics, no LDS; every output element is
 * written exactly once; the same bytes on every run.  Every check runs before any launch.
 *
 *   Neighbours: exactly the c = count[q] entries cer_grid_knn_f32 lists for (queries, k, max_dist), in its ascending (d2, index) order; a query
 *     that is an indexed point is among its own neighbours.  Their coordinates are read from points by original index.
 *   Moments, fp64, no contraction, about the query: d_j = double(p_j) - double(q) per axis; S1 = ((d_0 + d_1) + ...) (3 sums), S2_ab the same
 *     over d_a * d_b for ab = xx, xy, xz, yy, yz, zz (6 sums).  mom[q] ([m, 9] doubles) = S1 then S2 in that order; zeros for c = 0.
 *   mean = S1 / c, C_ab = S2_ab / c - mean_a * mean_b; the eigenvalues l0 <= l1 <= l2 and eigenvectors of C by cyclic Jacobi in fp64.
 *   A query is VALID iff it is finite, c >= 3, l2 > 0 and l1 > 1e-12 * l2 (the last excludes a collinear neighbourhood).  Valid: normal[q]
 *     ([m, 3] floats) = the unit eigenvector of l0, rounded once from fp64; curvature[q] = float(max(l0, 0) / ((l0 + l1) + l2)), the surface
 *     variation.  Invalid: normal (0, 0, 0), curvature NaN.
 *   Sign: canonically the component of largest magnitude is positive (the lowest axis on a tie).  With viewpoints ([m, 3] floats, one per
 *     query): v = double(viewpoint) - double(q), s = (n_x * v_x + n_y * v_y) + n_z * v_z with n the fp64 eigenvector in canonical sign; the
 *     normal is negated iff s < 0.  A viewpoint with a non-finite coordinate leaves the canonical sign. */
int cer_grid_normals_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells, const double* origin,
                         double cell, const float* queries, const long long* qorder, long m, int k, float max_dist, const float* points,
                         const float* viewpoints, float* normal, float* curvature, int* count, double* mom, void* stream);

/* Rigid registration of two clouds (ABI 1130; csrc/cloud_align.hip, cer-mvs_amd/cloud_eval.py rigid_transform / pair_moments / icp, DESIGN.md
 * 3w): what point-to-point ICP needs beside cer_grid_nearest_f32.  fp64 arithmetic on float32 coordinates with every association fixed, no
 * atomics, grids and summation trees that depend on the sizes alone: the same bits on every run and every machine.  Sizes and errors as
 * above: negative -> CER_EINVAL, 2^31 and beyond -> CER_ESHAPE; then T / pivot null or with a non-finite entry -> CER_EINVAL; zero -> CER_OK
 * with nothing launched; then null pointers -> CER_EINVAL.  Every check runs before any launch.
 *
 *   cer_cloud_transform_f32: out[i][r] = float(((T[4r] * x + T[4r+1] * y) + T[4r+2] * z) + T[4r+3]), (x, y, z) = points[i] promoted to fp64;
 *     T: 12 HOST doubles, the upper 3 x 4 of the motion, row-major.  No fused multiply-add.  Non-finite coordinates propagate by IEEE rules.
 *     out [n, 3] is written whole and may not overlap points (CER_EINVAL).
 *   cer_cloud_moment_partials: HOST function: ceil(m / CER_MOMENT_TILE), the blocks of the first pass; `partials` below holds
 *     CER_MOMENT_COUNT * that many doubles.
 *   cer_cloud_pair_moments_f64: a pair is (a[i], b[idx[i]]) for every i < m with idx[i] >= 0 (cer_grid_nearest_f32's -1: no pair) and a
 *     finite a[i]; idx[i] must be a valid row of b.  pivot: 3 HOST doubles.  With A = double(a) - pivot, B = double(b) - pivot and D =
 *     double(a) - double(b), out (CER_MOMENT_COUNT DEVICE doubles, written whole) = [k, the number of pairs | sum A (3) | sum B (3) | sum
 *     A[r] * B[c] at 7 + 3 r + c | sum (Dx*Dx + Dy*Dy) + Dz*Dz, the d2 of cer_grid_nearest_f32].  Two passes: every 256-thread block sums
 *     CER_MOMENT_TILE consecutive pairs (a thread its pairs t, t + 256, ... in ascending order, the wave a butterfly, the four waves (w0 + w1)
 *     + (w2 + w3)), then one block of 1024 threads sums the partials (a thread p, p + 1024, ...; butterfly; a pairwise tree over 16 waves). */
#define CER_MOMENT_TILE 2048
#define CER_MOMENT_COUNT 17
int cer_cloud_transform_f32(const float* points, long n, const double* T, float* out, void* stream);
long cer_cloud_moment_partials(long m);
int cer_cloud_pair_moments_f64(const float* a, const float* b, const long long* idx, long m, const double* pivot, double* partials,
                               double* out, void* stream);

/* Point-to-plane registration (ABI 1160; csrc/cloud_align.hip, cer-mvs_amd/cloud_eval.py plane_moments / rigid_from_plane_moments /
 * icp(method="plane")): the normal equations of the linearised point-to-plane step.  Sizes, errors, their order and the
 * summation shape are cer_cloud_pair_moments_f64's; fp64, every association fixed, no fused multiply-add, no atomics.
 *
 *   cer_cloud_plane_moment_partials: HOST function: ceil(m / CER_MOMENT_TILE); `partials` holds CER_PLANE_MOMENT_COUNT * that many doubles.
 *   cer_cloud_plane_moments_f64: a pair is (a[i], b[q], n = nrm[q]) for every i < m with q = idx[i] >= 0 (a valid row of b and of nrm), a
 *     finite a[i], and n finite and not (0, 0, 0) (cer_grid_normals_f32's "no plane").  nrm: [rows of b, 3] floats, used as given (not
 *     normalised).  pivot: 3 HOST doubles.  With A = double(a) - pivot, D = double(a) - double(b), r = (Dx*nx + Dy*ny) + Dz*nz,
 *     c = (A1*n2 - A2*n1, A2*n0 - A0*n2, A0*n1 - A1*n0) and J = (c0, c1, c2, n0, n1, n2), out (CER_PLANE_MOMENT_COUNT DEVICE doubles, written
 *     whole) = [k, the number of pairs | sum J_i * J_j for i <= j, row-major (21) | sum J_i * r (6) | sum r * r | sum (Dx*Dx + Dy*Dy) +
 *     Dz*Dz, the d2 of cer_grid_nearest_f32]. */
#define CER_PLANE_MOMENT_COUNT 30
long cer_cloud_plane_moment_partials(long m);
int cer_cloud_plane_moments_f64(const float* a, const float* b, const float* nrm, const long long* idx, long m, const double* pivot,
                                double* partials, double* out, void* stream);

/* Surface mesh of a fused scan (ABI 1170; csrc/mesh.hip, cer-mvs_amd/mesh.py): the fused depth maps integrated into a dense
 * volume of truncated signed distances, and marching tetrahedra on it.  A grid is origin (3 HOST doubles), voxel and (nx, ny, nz): node
 * (i, j, k) sits at origin + (i, j, k) * voxel (one product and one sum per axis); volumes are [nz, ny, nx], x fastest.  fp64 arithmetic with
 * every association as written, no fused multiply-add, IEEE divisions; no atomics; the same bytes on every run.
 *
 * Checks, in this order, all before any launch: (1) a negative size -> CER_EINVAL; (2) too large -> CER_ESHAPE (nx ny nz >= 2^31 -
 * CER_MESH_TILE; h w >= 2^31; nv or nf >= 2^31); (3) origin null or non-finite, voxel (and trunc) not a positive finite number ->
 * CER_EINVAL; (4) nothing to do -> CER_OK with nothing launched (no nodes; no views for the integration; an axis of 1 - no cell - for the
 * three extraction calls; no vertex and no face, or no capacity, for the emit); (5) a null pointer -> CER_EINVAL (with views listed: also
 * N, h or w of 0).
 *
 *   cer_tsdf_integrate_f32: depths float32 [N, h, w]; masks uint8 [N, h, w] or NULL (every pixel); cams [N, CER_CLOUD_CAM_DOUBLES] doubles
 *     per view: K row-major [9] | rows 0-2 of E [12] | padding (the float32 FORWARD matrices, promoted); views: n_views DEVICE ints, each in
 *     0 .. N-1 (the caller checks them; a kernel skips one that is not).  For every node p and each listed view in list order:
 *       cx = ((E00 px + E01 py) + E02 pz) + E03, cy, cz likewise; ux = (K00 cx + K01 cy) + K02 cz, uy, uz likewise;
 *       a = ux / uz + 0.5, b = uy / uz + 0.5.  The view contributes iff uz > 0, 0 <= a < w, 0 <= b < h (in fp64; NaN fails), the mask at
 *       (xi, yi) = (floor(a), floor(b)) is set, d = double(depth[yi, xi]) is finite and > 0, and sdf = d - uz >= -trunc.  It adds
 *       (sdf >= trunc ? 1.0 : sdf / trunc) to an fp64 sum that starts at 0, and 1 to the count.
 *     weight (int32) = the count; tsdf (float32) = float(sum / count), 1.0f where the count is 0.  One thread owns a node.
 *   cer_mesh_partials: HOST function: the partial counts of the extraction, ceil(8 nodes / CER_MESH_TILE) + ceil(12 cells /
 *     CER_MESH_TILE) (0 without a cell): partials [that many] unsigned, offsets [that many + 2] 64-bit.
 *   cer_mesh_cells_u16: cells [nz-1, ny-1, nx-1] unsigned shorts: bit c (c = 0..7) set iff corner c - node (i + (c & 1), j + ((c >> 1) & 1),
 *     k + ((c >> 2) & 1)) - has tsdf < 0 (so 0.0 and -0.0 are outside); bit 8 set iff the cell is valid: every corner has weight >=
 *     min_weight and a finite tsdf.
 *   cer_mesh_count: the per-block counts of set vertex slots and set face slots and their scans; totals[0] = nv, totals[1] = nf (2 DEVICE
 *     64-bit integers).  Tets in corner-listing order: (0,1,3,7) (0,3,2,7) (0,2,6,7) (0,6,4,7) (0,4,5,7) (0,5,1,7).  With ins / out the
 *     inside / outside corners of a tet in listing order, XY the vertex on the lattice edge between corners X and Y, and det the integer
 *     determinant of [B-A, C-A, D-A] on corner offsets: one inside, A = ins[0], (B, C, D) = out: (AB, AC, AD), the last two swapped if det <
 *     0; three inside, A = out[0], (B, C, D) = ins: (AB, AC, AD), swapped if det > 0; two inside, (A, B) = ins, (C, D) = out, q = (AC, AD,
 *     BD, BC): (q0, q1, q2) and (q0, q2, q3), both swapped if det < 0.  Face slot (cell * 6 + tet) * 2 + s; a lattice edge is (node a, d =
 *     1..7 as a bit vector), vertex slot node * 8 + d, set iff the endpoints' signs differ and a valid cell contains the edge.
 *   cer_mesh_emit_f32: vertices float32 [vcap, 3] and faces int32 [fcap, 3] in slot order: the first min(nv, vcap) vertices and min(nf,
 *     fcap) faces, never a byte beyond.  nv, nf: what cer_mesh_count found.  A vertex: t = f0 / (f0 - f1) on the endpoint values promoted
 *     to fp64, per axis origin + (double(idx) + (d_a ? t : 0.0)) * voxel, rounded once to float32.  vmap: [nodes * 8] ints of workspace -
 *     the output index of every set vertex slot, which the faces read (32 bytes per node). */
#define CER_MESH_TILE 2048
long cer_mesh_partials(int nx, int ny, int nz);
int cer_tsdf_integrate_f32(const float* depths, const unsigned char* masks, const double* cams, int N, int h, int w, const int* views,
                           int n_views, const double* origin, double voxel, int nx, int ny, int nz, double trunc, float* tsdf, int* weight,
                           void* stream);
int cer_mesh_cells_u16(const float* tsdf, const int* weight, int nx, int ny, int nz, int min_weight, unsigned short* cells, void* stream);
int cer_mesh_count(const unsigned short* cells, int nx, int ny, int nz, unsigned int* partials, long long* offsets, long long* totals,
                   void* stream);
int cer_mesh_emit_f32(const float* tsdf, const unsigned short* cells, const double* origin, double voxel, int nx, int ny, int nz,
                      const long long* offsets, long long nv, long long nf, long long vcap, long long fcap, int* vmap, float* vertices,
                      int* faces, void* stream);

/* Per-vertex attributes of a triangle mesh (ABI 1180; csrc/mesh.hip, cer-mvs_amd/mesh.py), under the rules of the section
 * above: fp64 with every association as written, no fused multiply-add, IEEE division and square root, no atomics, the same bytes on every
 * run.  Checks in the section's order, all before any launch: (1) a negative size -> CER_EINVAL; (2) nv, 3 nf or h w >= 2^31 -> CER_ESHAPE;
 * (3) tol not a positive finite number -> CER_EINVAL; (4) nothing to do -> CER_OK with nothing launched (nv == 0; for the colours also
 * n_views == 0: rgb and seen are the caller's to zero; the normals with nf == 0 and nv > 0 DO launch and write zeros); (5) a null pointer
 * -> CER_EINVAL (the colours: also N, h or w of 0; the normals: faces and order may be null iff nf == 0).
 *
 *   cer_mesh_vertex_colors_u8: vertices float32 [nv, 3], promoted to double; depths, masks (or NULL: every pixel), cams and views as
 *     cer_tsdf_integrate_f32 takes them; colors float32 [N, 3, h, w], planar.  One thread owns a vertex p; for each listed view in list order:
 *       cx = ((E00 px + E01 py) + E02 pz) + E03, cy, cz likewise; ux = (K00 cx + K01 cy) + K02 cz, uy, uz likewise (the integration's);
 *       x = ux / uz, y = uy / uz, a = x + 0.5, b = y + 0.5.  The view SEES the vertex iff uz > 0, 0 <= a < w, 0 <= b < h (in fp64, before
 *       any conversion; NaN fails), the mask at (floor(a), floor(b)) is set (or masks is NULL), d = double(depth) at that pixel is finite
 *       and > 0, and fabs(d - uz) <= tol (inclusive; world units) - the occlusion test: a vertex more than tol behind or in front of the
 *       surface the view recorded at that pixel takes no colour from that view.
 *       The sample is bilinear over pixel centres at integer coordinates: x0 = floor(x), fx = x - x0, y0 = floor(y), fy = y - y0; taps x0,
 *       x0 + 1 clamped to [0, w-1] and y0, y0 + 1 clamped to [0, h-1], all four used whatever their masks; per channel, with cYX the tap
 *       at row Y, column X promoted to double: top = (1 - fx) * c00 + fx * c01, bot = (1 - fx) * c10 + fx * c11, val = (1 - fy) * top +
 *       fy * bot.  val is added to an fp64 sum per channel (starting at 0) and 1 to the count.
 *     seen int32 [nv] = the count.  rgb uint8 [nv, 3]: with m = sum / double(count) and q = m * 255.0 the byte is q >= 255 ? 255 : (q > 0 ?
 *     (uint8) q : 0) - truncation, as the cloud's (uint8)(c * 255); NaN gives 0; (0, 0, 0) where the count is 0.
 *   cer_mesh_vertex_normals_f32: any indexed triangle mesh: vertices float32 [nv, 3], faces int32 [nf, 3].  The incidence is a CSR list
 *     over the 3 nf corner entries faces.reshape(-1), corner id = 3 * face + corner: order int32 [3 nf] = the corner ids stably sorted by
 *     their vertex (within one vertex the ids ascend), starts int32 [nv + 1] = the first position of every vertex in that order.  One
 *     thread per vertex v walks e = starts[v] .. starts[v + 1] - 1: for face order[e] / 3 with indices (ia, ib, ic) and A, B, C their
 *     positions promoted to double, U = B - A, W = C - A, n = (Uy Wz - Uz Wy, Uz Wx - Ux Wz, Ux Wy - Uy Wx) - twice the area long, so the
 *     sum is area-weighted - added per component to an fp64 sum that starts at 0.  A face that lists v twice is visited twice.  A corner id
 *     or a face index outside its range is skipped (the Python layer refuses such faces).  len = sqrt((sx sx + sy sy) + sz sz); normals
 *     float32 [nv, 3] = float(s / len) per component where len > 0 and finite, else (0, 0, 0) (an unreferenced vertex, cancelling faces,
 *     NaN). */
int cer_mesh_vertex_colors_u8(const float* vertices, long long nv, const float* depths, const unsigned char* masks, const float* colors,
                              const double* cams, int N, int h, int w, const int* views, int n_views, double tol, unsigned char* rgb,
                              int* seen, void* stream);
int cer_mesh_vertex_normals_f32(const float* vertices, long long nv, const int* faces, long long nf, const int* starts, const int* order,
                                float* normals, void* stream);

/* Connected components and sub-meshes of any indexed triangle mesh (ABI 1190; csrc/mesh.hip, cer-mvs_amd/mesh.py mesh_components /
 * select_faces / remove_small_components): integers only, no atomics, the same bytes on every run.  faces int32 [nf, 3];
 * starts int32 [nv + 1] and order int32 [3 nf]: the CSR corner list of cer_mesh_vertex_normals_f32.  Checks in this order, all before any
 * launch: (1) a negative size (nv, nf, n_sweeps, nv_out, nf_out) -> CER_EINVAL; (2) nv or 3 nf >= 2^31 -> CER_ESHAPE; (3) nothing to do ->
 * CER_OK with nothing launched (the sweeps: nv == 0 or n_sweeps == 0; the selection: nv == 0 or nf == 0 - no face is kept and no vertex
 * survives, totals are the caller's to zero - and for the emit also nv_out == 0 and nf_out == 0); (4) a null pointer -> CER_EINVAL (the
 * sweeps: faces and order may be null iff nf == 0; the emit: out_vertices and index may be null iff nv_out == 0, out_faces iff nf_out == 0).
 * A face index outside 0 .. nv-1, a corner id outside 0 .. 3 nf - 1 and a label outside 0 .. nv-1 are skipped, never read through (the
 * Python layer refuses such faces).
 *
 * Components.  Two vertices are connected iff a chain of faces links them through shared vertex INDICES: a face links its three indices (one
 *   with repeated indices is still a face).  This is vertex connectivity, not shared-edge adjacency: two pieces that touch in one vertex
 *   are one component.  The root of a component is its smallest vertex index; components are numbered 0 .. nc-1 by ascending root; an
 *   unreferenced vertex is a component of its own with no face; a face's component is that of its first index.
 *   cer_mesh_label_sweeps_i32: labels int32 [nv], which the caller initialises to 0, 1, .., nv-1; flags: n_sweeps ints, which the caller
 *     zeroes.  Launches n_sweeps sweeps in stream order; sweep i owns flags[i].  In a sweep one thread owns vertex v and is the only writer
 *     of labels[v]: m = labels[labels[v]]; for every corner e in starts[v] .. starts[v + 1] - 1 and every index u of face order[e] / 3,
 *     m = min(m, labels[labels[u]]); if m < labels[v], it stores m and stores 1 into the sweep's flag.  In place: a label read from another
 *     vertex is this sweep's or the previous one's, either way the index of a vertex of the same component; labels only fall; the only
 *     fixed point is labels[v] = the root, so the final bytes are unique although the intermediate ones are not.  The flag store is the
 *     only store several threads make to one address, all of them the same value.  No loop's trip count depends on another thread's
 *     stores: no find-root walk, no spin, no grid-wide barrier - a sweep is two dependent loads per neighbour and ends.  The component's
 *     minimum advances at least one hop per sweep, so a sweep that changes nothing comes within nv + 1 sweeps; sweeps past it change
 *     nothing and leave their flags 0.
 * Selection.  Face q is kept iff keep[q] != 0 (keep: nf bytes) and its three indices are in range; vertex p survives iff a kept face is
 *   among the faces around it, gathered through the CSR list (no scatter).  Kept faces and surviving vertices keep their order; the indices
 *   are renumbered.  Both leave through the ordered compaction of cer_mesh_count, CER_MESH_TILE positions per block, the vertex tiles
 *   followed by the face tiles.
 *   cer_mesh_select_partials: HOST function: ceil(nv / CER_MESH_TILE) + ceil(nf / CER_MESH_TILE) (0 if nv or nf is 0): partials [that
 *     many] unsigned, offsets [that many + 2] 64-bit.
 *   cer_mesh_select_count: ONE count launch over both kinds of tile, which also stores used [nv] bytes (1 iff the vertex survives), then the
 *     two-block scan; totals[0] = nv_out, totals[1] = nf_out (2 DEVICE 64-bit integers).
 *   cer_mesh_select_emit_f32: nv_out, nf_out: what the count found, and the rows of the outputs - never a byte beyond them.  A vertex emit
 *     writes out_vertices float32 [nv_out, 3] (the position's bits), index int32 [nv_out] (the old index of every surviving vertex) and
 *     vmap int32 [nv] (workspace: the new index of every surviving vertex); a face emit writes out_faces int32 [nf_out, 3] = vmap of the
 *     old indices.  Workspace: 5 bytes per vertex (used, vmap) and 12 bytes per CER_MESH_TILE positions. */
int cer_mesh_label_sweeps_i32(const int* faces, long long nf, const int* starts, const int* order, long long nv, int* labels, int* flags,
                              int n_sweeps, void* stream);
long cer_mesh_select_partials(long long nv, long long nf);
int cer_mesh_select_count(const int* faces, long long nf, const int* starts, const int* order, long long nv, const unsigned char* keep,
                          unsigned char* used, unsigned int* partials, long long* offsets, long long* totals, void* stream);
int cer_mesh_select_emit_f32(const float* vertices, long long nv, const int* faces, long long nf, const unsigned char* keep,
                             const unsigned char* used, const long long* offsets, long long nv_out, long long nf_out, int* vmap,
                             float* out_vertices, int* index, int* out_faces, void* stream);

/* Mesh simplification (ABI 1200; csrc/mesh.hip, cer-mvs_amd/mesh.py simplify_vertex_clustering): vertex clustering
 * (Rossignac-Borrel) with the mean or Lindstrom's quadric minimiser as the representative, for any indexed triangle mesh, under the rules
 * of the section "Surface mesh": fp64 with every association as written, no fused multiply-add, IEEE division, no fast-math, no atomics,
 * the same bytes on every run.  vertices float32 [nv, 3]; faces int32 [nf, 3]; starts int32 [nv + 1] and corner_order int32 [3 nf]: the CSR
 * corner list of cer_mesh_vertex_normals_f32.
 *
 * Checks, in that section's order, all before any launch: (1) a negative size (nv, nf, ncells) -> CER_EINVAL; (2) nv, 3 nf or ncells >=
 * 2^31, or ncells > nv -> CER_ESHAPE; (3) origin null or non-finite, cell or regularisation not a positive finite number -> CER_EINVAL (the
 * representatives only; regularisation is checked in both forms); (4) nothing to do -> CER_OK with nothing launched (the map: nv == 0 - with
 * ncells == 0 and nv > 0 it DOES launch and writes -1; the representatives: ncells == 0; the faces and the heads: nf == 0); (5) a null
 * pointer -> CER_EINVAL (the representatives: colors and rep_colors may be null together; in the quadric form faces and corner_order may be
 * null iff nf == 0; the mean form reads none of faces, starts and corner_order; the faces: cluster may be null iff nv == 0).  An index, a
 * corner id or a sorted position outside its range is skipped, never read or written through (the Python layer refuses such faces).
 *
 * 1. Clusters: the occupied cells of the sparse grid of cer_grid_keys_f32 over the vertices, origin = the per-axis minimum of the finite
 *    vertices (HOST doubles), c = floor((double(p) - origin) / cell) per axis.  order int64 [nv]: the vertex indices stably sorted by key;
 *    cell_keys int64 [ncells]: the distinct keys, ascending; cell_start int64 [ncells + 1]: the first sorted position of every cell, and
 *    cell_start[ncells] = the number of finite vertices.  Cluster r has the members order[cell_start[r] .. cell_start[r + 1] - 1], ascending
 *    vertex index ("member order").  A vertex with a non-finite coordinate belongs to no cluster.
 *    cer_mesh_cluster_map_i32: cluster int32 [nv]: cluster[order[p]] = r for cell_start[r] <= p < cell_start[r + 1], -1 for p >=
 *    cell_start[ncells].  One thread per sorted position; order is a permutation, so every address has one writer.
 * 2. Representative, mean (quadric == 0): per axis s = the fp64 sum, starting at 0, of the promoted member coordinates in member order;
 *    mean = s / double(count); reps float32 [ncells, 3] = float(mean).
 * 3. Representative, quadric (quadric != 0): with (cx, cy, cz) the cell coordinates that cell_keys[r] holds, base = origin + (double(c) +
 *    0.5) * cell per axis.  For every member v in member order and every corner e = starts[v] .. starts[v + 1] - 1, the face corner_order[e] /
 *    3 with positions A, B, C promoted to double: U = B - A, W = C - A, n = (Uy Wz - Uz Wy, Uz Wx - Ux Wz, Ux Wy - Uy Wx) (the normals
 *    kernel's), d = (nx (Ax - basex) + ny (Ay - basey)) + nz (Az - basez); then Mxx += nx nx, Mxy += nx ny, Mxz += nx nz, Myy += ny ny, Myz
 *    += ny nz, Mzz += nz nz, qx += nx d, qy += ny d, qz += nz d, all fp64 sums that start at 0.  A face that names two members is visited once
 *    per member (the sum of vertex quadrics).  Then
 *      lam = (regularisation * ((Mxx + Myy) + Mzz)) / 3.0;  a = Mxx + lam, dd = Myy + lam, ff = Mzz + lam;
 *      tx = qx + lam * (meanx - basex), ty, tz likewise (mean: item 2's fp64 quotient, not rounded);
 *      c00 = dd ff - Myz Myz, c01 = Mxz Myz - Mxy ff, c02 = Mxy Myz - Mxz dd, c11 = a ff - Mxz Mxz, c12 = Mxy Mxz - a Myz, c22 = a dd - Mxy Mxy;
 *      det = (a c00 + Mxy c01) + Mxz c02;
 *      x = ((c00 tx + c01 ty) + c02 tz) / det, y = ((c01 tx + c11 ty) + c12 tz) / det, z = ((c02 tx + c12 ty) + c22 tz) / det
 *    - the solution of (M + lam I) x = q + lam (mean - base) by cofactors.  The representative is float(base + x) per axis and took[r] = 1 iff
 *    lam > 0, det > 0, det, x, y and z are finite and fabs of each of x, y, z <= cell / 2.0 (fp64 compares); otherwise it is item 2's mean and
 *    took[r] = 0 (took: ncells bytes; all 0 in the mean form).  The regulariser pulls the minimiser to the mean along directions the planes
 *    leave free and bounds the condition number by 3 / regularisation + 1.
 * 4. Colours (colors uint8 [nv, 3] or NULL): per channel the integer sum of the member bytes divided by the count, integer division;
 *    rep_colors uint8 [ncells, 3].
 *    cer_mesh_cluster_reps_f32: items 2 to 4, ONE thread per cluster for its whole member walk (a wave-wide reduction would change the
 *    order of the sums).
 * 5. Faces.  cer_mesh_cluster_faces_i32: a face is VALID iff its three indices are in 0 .. nv-1, all three have a cluster (>= 0) and the
 *    three clusters are distinct.  triples int32 [nf, 3]: the clusters of a valid face rotated cyclically so that the smallest comes first
 *    (orientation kept), (-1, -1, -1) for an invalid face; valid: nf bytes.
 *    cer_mesh_face_heads_u8: perm int64 [nf]: the faces sorted lexicographically by triple, stably (the caller: a stable sort by
 *    (t1 << 31) | t2 as 64-bit integers, then a stable sort by t0), so equal triples keep ascending face index.  keep[perm[p]] = valid[perm[p]]
 *    && (p == 0 || triples[perm[p]] != triples[perm[p - 1]]): of the valid faces that are equal after rotation the lowest face index survives;
 *    opposite orientations are different triples and both stay.  keep: nf bytes, one writer each.
 * 6. Output: cer_mesh_select_count / cer_mesh_select_emit_f32 on (reps, triples, keep) - surviving faces keep their input order, a cluster
 *    without a surviving face is dropped, surviving clusters keep ascending order. */
int cer_mesh_cluster_map_i32(const long long* order, const long long* cell_start, long long nv, long long ncells, int* cluster, void* stream);
int cer_mesh_cluster_reps_f32(const float* vertices, long long nv, const int* faces, long long nf, const int* starts, const int* corner_order,
                              const long long* order, const long long* cell_start, const long long* cell_keys, long long ncells,
                              const double* origin, double cell, int quadric, double regularisation, const unsigned char* colors, float* reps,
                              unsigned char* rep_colors, unsigned char* took, void* stream);
int cer_mesh_cluster_faces_i32(const int* faces, long long nf, const int* cluster, long long nv, int* triples, unsigned char* valid,
                               void* stream);
int cer_mesh_face_heads_u8(const int* triples, const unsigned char* valid, const long long* perm, long long nf, unsigned char* keep,
                           void* stream);

/* Mesh edges and smoothing (ABI 1210; csrc/mesh.hip, cer-mvs_amd/mesh.py mesh_edges / mesh_topology / smooth_mesh): the
 * unique-neighbour list of every vertex of any indexed triangle mesh - its duplicate-free edge table with a count per direction - and
 * Taubin's lambda|mu (or plain Laplacian) smoothing as one gather kernel over that list, under the rules of the section "Surface mesh":
 * fp64 with every association as written, no fused multiply-add, IEEE division, no atomics, one writer per address, the same bytes on
 * every run.  faces int32 [nf, 3]; vertices float32 [nv, 3].
 *
 * Checks, in that section's order, all before any launch: (1) a negative size (nv, nf, nn, n_steps) -> CER_EINVAL; (2) nv, 6 nf (hence
 * 3 nf) or nn >= 2^31 -> CER_ESHAPE; (3) a non-finite weight (the steps) -> CER_EINVAL; (4) nothing to do -> CER_OK with nothing launched
 * (the keys and the count: nf == 0 - totals are the caller's to zero; the emit: nf == 0 or nn == 0; prepare and finish: nv == 0; the steps:
 * nv == 0 or n_steps == 0); (5) a null pointer -> CER_EINVAL (prepare: nbrs, along, against and walk may be null iff nn == 0; the steps:
 * walk may be null iff nn == 0, and state_a == state_b is refused).  An index, a list position or an output row outside its range is
 * skipped, never read or written through (the Python layer refuses such faces).
 *
 * 1. Directed edges.  Face (i0, i1, i2) has the directed edges i0->i1, i1->i2, i2->i0; one with equal ends is skipped, so a face with a
 *    repeated index contributes only its edges between distinct indices.
 *    cer_mesh_edge_keys_i64: keys int64 [6 nf]: face q writes keys[6 q ..], two per directed edge a->b: (a << 32) | (b << 1) - the entry
 *    (owner a, other b), "along" - and (b << 32) | (a << 1) | 1 - the entry (owner b, other a), "against"; -1 for a skipped edge or an index
 *    outside 0 .. nv-1.  The CALLER sorts the keys ascending (equal keys are indistinguishable: any sort): the -1 come first, and the keys of
 *    one (owner, other) pair form one run, ordered by owner, then other.
 * 2. Neighbour list.  One entry per run: nbrs[e] = other, along[e] = the run's keys with bit 0 clear = the directed edges owner->other,
 *    against[e] = those with bit 0 set = the directed edges other->owner; entries ordered by (owner, other).  The entry (u, v) mirrors (v, u)
 *    with the two counts swapped; nn, the number of entries, is even; the undirected edge table is the entries with owner < other.  Runs
 *    leave through the ordered compaction of cer_mesh_count over the 6 nf sorted positions, CER_MESH_TILE per block: a position is a head
 *    iff its key is >= 0 and (it is position 0 or key >> 1 differs from the key before it >> 1).
 *    cer_mesh_edge_partials: HOST function: ceil(6 nf / CER_MESH_TILE): partials [that many] unsigned, offsets [that many + 2] 64-bit.
 *    cer_mesh_edge_count: one count launch and the scan; totals[0] = nn (totals: 2 DEVICE 64-bit integers, the second is written 0).
 *    cer_mesh_edge_emit_i32: nn: what the count found, and the rows of the outputs - never a byte beyond them.  The head of a run walks its
 *    run forward and writes owner, nbrs, along, against int32 [nn].  nbr_starts int32 [nv + 1] is the caller's: the first entry of every
 *    owner (a binary search of 0 .. nv in owner).
 * 3. Smoothing.  cer_mesh_smooth_prepare_f32, one thread per vertex v over its run e = nbr_starts[v] .. nbr_starts[v + 1] - 1: a vertex is
 *    FINITE iff its three input floats are; walk int32 [nn]: walk[e] = nbrs[e] if that vertex is finite, else -1; BOUNDARY iff an entry of
 *    its run has along + against == 1; FROZEN iff it is not finite, or no entry of its run is finite, or fixed_boundary != 0 and it is
 *    boundary.  flags [nv] bytes = 1 (finite) | 2 (frozen) | 4 (boundary); state double [nv, 3] = the promoted input.  All of this is
 *    computed once, from the input.
 *    cer_mesh_smooth_steps_f64: n_steps steps in stream order, one launch each and no host wait between them; step i = 0, 1, .. reads
 *    state_a and writes state_b if i is even and the reverse if i is odd, with weight w = w_even or w_odd, so the result is in state_b
 *    iff n_steps is odd.  (Laplacian: w_even = w_odd = lambda; Taubin: w_even = lambda, w_odd = mu, two steps per iteration.)  One thread
 *    per vertex: a frozen vertex copies its three doubles; any other, per axis, with p its value in the source buffer:
 *      s = 0.0;  s = s + source[walk[e]] for e ascending, skipping walk[e] outside 0 .. nv-1, count = the entries taken;
 *      m = s / double(count);  q = p + w * (m - p).
 *    Sums in registers, no shared memory.
 *    cer_mesh_smooth_finish_f32: out float32 [nv, 3] = float(state), rounded once; a frozen vertex gets the bits of its input. */
long cer_mesh_edge_partials(long long nf);
int cer_mesh_edge_keys_i64(const int* faces, long long nf, long long nv, long long* keys, void* stream);
int cer_mesh_edge_count(const long long* sorted_keys, long long nf, unsigned int* partials, long long* offsets, long long* totals,
                        void* stream);
int cer_mesh_edge_emit_i32(const long long* sorted_keys, long long nf, const long long* offsets, long long nn, int* owner, int* nbrs,
                           int* along, int* against, void* stream);
int cer_mesh_smooth_prepare_f32(const float* vertices, long long nv, const int* nbr_starts, const int* nbrs, const int* along,
                                const int* against, long long nn, int fixed_boundary, int* walk, unsigned char* flags, double* state,
                                void* stream);
int cer_mesh_smooth_steps_f64(double* state_a, double* state_b, long long nv, const int* nbr_starts, const int* walk, long long nn,
                              const unsigned char* flags, double w_even, double w_odd, int n_steps, void* stream);
int cer_mesh_smooth_finish_f32(const double* state, const float* vertices, const unsigned char* flags, long long nv, float* out,
                               void* stream);

/* Mesh hole filling (ABI 1220; csrc/mesh_fill.hip, cer-mvs_amd/mesh.py mesh_holes / fill_holes): the small boundary loops
 * of any indexed triangle mesh closed by one face or by a fan around the loop's mean, starting from the neighbour list of the section "Mesh
 * edges and smoothing" and under the rules of the section "Surface mesh": integers, fp64 with every association as written, no fused
 * multiply-add, IEEE division, no atomics, one writer per address, the same bytes on every run.  faces int32 [nf, 3]; vertices float32
 * [nv, 3]; nbr_starts int32 [nv + 1], nbrs, along, against int32 [nn]: what cer_mesh_edge_emit_i32 and its caller produce.
 *
 * Checks, in that section's order, all before any launch: (1) a negative size (nv, nn, nh, nf, added_vertices, added_faces) ->
 * CER_EINVAL; (2) nv, nn, nh, nv + added_vertices or 3 (nf + added_faces) >= 2^31, nh > nv, added_vertices > nh, or max_edges < 3 ->
 * CER_ESHAPE; (3) nothing to do -> CER_OK with nothing launched (the successors and the heads: nv == 0; the fill: nh == 0); (4) a null
 * pointer -> CER_EINVAL.  The optional pointers are null iff absent: the successors: nbrs, along and against iff nn == 0; the heads:
 * vertices iff the finiteness test is not wanted; the fill: vertices and out_vertices iff added_vertices == 0 (holes of three edges only),
 * colors and out_colors together iff there are no colours - one of the two alone is refused.  An index, a list position or an output row
 * outside its range is skipped, never read or written through (the Python layer refuses such faces).
 *
 * 1. Boundary half-edges and simple vertices.  With the counts of the neighbour list, the directed edge a->b is a BOUNDARY HALF-EDGE iff
 *    along(a, b) == 1 and against(a, b) == 0: one face runs along it and none against it.  Vertex v is SIMPLE iff exactly one boundary
 *    half-edge leaves it and exactly one enters it (in v's run: exactly one entry with along == 1 and against == 0, and exactly one with
 *    along == 0 and against == 1).  next int32 [nv]: next[v] = the head of the leaving half-edge of a simple vertex; -1 where no boundary
 *    half-edge touches v; -2 ("pinched") where some do but v is not simple - a bow-tie vertex, the ends of an inconsistent edge, a vertex
 *    beside a non-manifold edge.
 *    cer_mesh_hole_next_i32: one thread per vertex walks its run of the list once and writes next[v].
 * 2. Holes.  A HOLE is a cycle h = a0 -> a1 -> .. -> a(n-1) -> a0 of next through simple vertices only, a(k+1) = next[a_k]; h is its
 *    smallest index and 3 <= n <= max_edges.  (A cycle of two edges is impossible: a->b and b->a would both be boundary half-edges, but
 *    each is counted against the other.)  With vertices given, a cycle that holds a vertex with a non-finite coordinate is not a hole.  A
 *    cycle through a pinched vertex, or longer than max_edges - the outer rim of an open scan - is left alone.  next is injective on the
 *    simple vertices, so a walk along it either returns to its start or ends at a pinched vertex.
 *    cer_mesh_hole_heads_i32: length int32 [nv]: length[v] = n if v is the head of a hole of n edges, else 0.  One thread per vertex
 *    with next[v] >= 0 follows next for at most max_edges steps and stops at a negative entry (no hole), at an index below v (v is not
 *    the head), at a non-finite member (with vertices) or back at v.
 *    The holes, in the order of their heads (ascending), are numbered 0 .. nh-1 ("position"): heads int32 [nh] and lengths int32 [nh] are
 *    the caller's compaction of length's non-zero entries.
 * 3. Fill.  The nv vertices and nf faces of the input come first in the output, bit-identical and in order (the caller's copies); then
 *    the fill follows, hole by hole in head order.  For n == 3 the fill is the ONE face (a0, a2, a1) and no vertex.  For n >= 4 it is one
 *    new vertex c, per axis in fp64
 *      s = 0.0;  s = s + double(p[a_k]) for k = 0 .. n-1;  m = s / double(n);  c = float(m), rounded once,
 *    and the n faces (a(k+1), a_k, c) for k = 0 .. n-1, indices mod n.  The new vertices sit behind the old ones in head order: c = nv +
 *    vertex_offsets[i]; the faces of hole i start at nf + face_offsets[i]: face_offsets and vertex_offsets int64 [nh] are the caller's
 *    exclusive sums of (n == 3 ? 1 : n) and (n >= 4 ? 1 : 0), and added_faces and added_vertices their totals - the rows of the outputs
 *    behind nf and nv, never a byte beyond them.  hole int32 [nf + added_faces]: -1 for an input face (the caller's), otherwise the position
 *    of the face's hole.  colors uint8 [nv, 3]: the colour of c is the members' integer sum per channel divided by n, integer division (the
 *    rule of "Mesh simplification", item 4).
 *    Every fill face runs against the half-edge it closes - (a(k+1), a_k, .) holds a(k+1)->a_k, and (a0, a2, a1) holds a1->a0, a2->a1 and
 *    a0->a2 - so a hole in an oriented mesh leaves the mesh oriented, every filled boundary edge becomes interior, and the spokes c-a_k
 *    are interior and consistent.
 *    cer_mesh_hole_fill_f32: one thread per hole walks its cycle once more, sums in registers in the order above, and writes the centre,
 *    its colour, the faces and hole[] of its hole; no shared memory.  out_vertices float32 [nv + added_vertices, 3], out_faces int32
 *    [nf + added_faces, 3], out_colors uint8 [nv + added_vertices, 3]: only the rows behind nv and nf are written. */
int cer_mesh_hole_next_i32(const int* nbr_starts, const int* nbrs, const int* along, const int* against, long long nv, long long nn,
                           int* next, void* stream);
int cer_mesh_hole_heads_i32(const int* next, const float* vertices, long long nv, int max_edges, int* length, void* stream);
int cer_mesh_hole_fill_f32(const int* next, const int* heads, const int* lengths, const long long* face_offsets,
                           const long long* vertex_offsets, long long nh, const float* vertices, const unsigned char* colors, long long nv,
                           long long nf, long long added_vertices, long long added_faces, float* out_vertices, int* out_faces, int* hole,
                           unsigned char* out_colors, void* stream);

/* Mesh surface sampling (ABI 1230; csrc/mesh_sample.hip, cer-mvs_amd/mesh.py face_areas / sample_mesh / sample_mesh_even / evaluate_mesh,
 * DESIGN.md 3zg): points on the surface of any indexed triangle mesh with a density proportional to area, under the rules of the section
 * "Surface mesh": integers, fp64 with every association as written, no fused multiply-add, IEEE division and square root, no atomics, one
 * writer per address, the same bytes on every run.  vertices float32 [nv, 3]; faces int32 [nf, 3]; colors uint8 [nv, 3].
 *
 * Checks, in that section's order, all before any launch: (1) a negative size (nv, nf, n) -> CER_EINVAL; (2) nv >= 2^31, 3 nf >= 2^31,
 * n >= 2^31, a shift outside CER_SAMPLE_SHIFT_MIN .. CER_SAMPLE_SHIFT_MAX, or samples wanted from no face (n > 0 and nf == 0) ->
 * CER_ESHAPE; (3) nothing to do -> CER_OK with nothing launched (the areas and the weights: nf == 0; the samples: n == 0); (4) a null
 * pointer -> CER_EINVAL.  vertices may be null iff nv == 0.  The optional pointers of the samples are null iff absent: words, uv, normals
 * each on its own, colors and out_colors together - one of the two alone is refused.  An index outside [0, nv) is skipped, never read
 * through, and the search of item 3 ends inside its table whatever the table holds.
 *
 * 1. Areas.  areas float64 [nf]: 0 when an index of the face is outside [0, nv), two of its indices are equal, or one of its nine
 *    coordinates is not finite.  Otherwise, in fp64 on the float32 coordinates of its corners a, b, c,
 *      e1 = b - a;  e2 = c - a;  nx = e1y*e2z - e1z*e2y;  ny = e1z*e2x - e1x*e2z;  nz = e1x*e2y - e1y*e2x;
 *      area = 0.5 * sqrt((nx*nx + ny*ny) + nz*nz),
 *    the square root correctly rounded.
 *    cer_mesh_face_areas_f64: one thread per face.
 * 2. Weights.  weights int64 [nf]: weights[f] = (long long)floor(ldexp(areas[f], shift)); the scaling by a power of two is exact.  The
 *    caller takes amax = the largest area (a maximum is exact under any association), (m, e) = frexp(amax) and shift = 32 - e: the largest
 *    weight is then in [2^31, 2^32), and with 3 nf < 2^31 the sum of all weights is below 2^63.  The weights are integers, so the caller's
 *    inclusive prefix sum cum int64 [nf] and the total W = cum[nf - 1] are exact whatever the shape of its scan.  A face smaller than
 *    2^-32 of the largest gets weight 0 and is never drawn; the sampling density is uniform to 2^-31 of the largest face per face; the
 *    area that the weights stand for is ldexp(double(W), -shift).  An area that is not a number, is negative or scales to 2^63 and beyond
 *    (none of the table the shift was taken from does) gets 0.  shift = 32 - e of any double lies in CER_SAMPLE_SHIFT_MIN ..
 *    CER_SAMPLE_SHIFT_MAX.
 *    cer_mesh_face_weights_i64: one thread per face.
 * 3. Samples.  Sample i of a call has the global index k = offset + i, 64-bit unsigned (it wraps).  Its four random words x0 .. x3 are
 *    row i of words uint32 [n, 4] when given; otherwise Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53 and 0xCD9E8D57, key
 *    increments 0x9E3779B9 and 0xBB67AE85) of the counter (k & 0xffffffff, k >> 32, 0, 0) under the key (seed & 0xffffffff, seed >> 32).
 *    Face: r = x0 * 2^32 + x1; t = floor(r * W / 2^64), the high half of the 128-bit product; f = the smallest index with cum[f] > t - a
 *    bisection on [0, nf - 1]; a W below 1 (not a caller's table) counts as 0.
 *    Position: a = x2, b = x3; if a + b >= 2^32 (in 64 bits) then a = 2^32 - 1 - a and b = 2^32 - 1 - b - the fold of the unit square onto
 *    the triangle, uniform and without a square root;  u = (double(a) + 0.5) * 2^-32, v = (double(b) + 0.5) * 2^-32, w = (1.0 - u) - v: all
 *    three exact, and w >= 0.  Per axis p = float((w*A + u*B) + v*C) with the face's corners A, B, C, rounded once.  A face whose indices
 *    are out of range or equal gives NaN in points and normals, and colour 0.
 *    points float32 [n, 3]; face int32 [n]; uv float64 [n, 2] = (u, v); normals float32 [n, 3]: the face's (nx, ny, nz) of item 1, each
 *    divided in fp64 by sqrt((nx*nx + ny*ny) + nz*nz) and rounded once (NaN for a face without area); out_colors uint8 [n, 3]: per
 *    channel min(255, floor(((w*cA + u*cB) + v*cC) + 0.5)) in fp64 on the corners' bytes.
 *    Sample k is a pure function of (seed, k, mesh): it does not depend on n, on the launch grid or on the run.
 *    cer_mesh_sample_f32: one thread per sample; about log2(nf) dependent reads of cum, then the face's corners. */
#define CER_SAMPLE_SHIFT_MIN (-992)
#define CER_SAMPLE_SHIFT_MAX 1105
int cer_mesh_face_areas_f64(const float* vertices, long long nv, const int* faces, long long nf, double* areas, void* stream);
int cer_mesh_face_weights_i64(const double* areas, long long nf, int shift, long long* weights, void* stream);
int cer_mesh_sample_f32(const float* vertices, long long nv, const int* faces, long long nf, const long long* cum, unsigned long long seed,
                        unsigned long long offset, const unsigned* words, long long n, const unsigned char* colors, float* points, int* face,
                        double* uv, float* normals, unsigned char* out_colors, void* stream);

/* Mesh distance (ABI 1240; csrc/mesh_dist.hip, csrc/grid_walk.hpp, cer-mvs_amd/mesh.py MeshIndex / mesh_distances /
 * evaluate_mesh(method="exact")): for every query point the nearest face of any indexed triangle mesh within a cut-off - what
 * cer_grid_nearest_f32 is for clouds - under the rules of the section "Surface mesh": integers, fp64 on the float32 inputs with every
 * association as written, no fused multiply-add, IEEE division and square root, no atomics, one writer per address, the same bytes on every
 * run.  vertices float32 [nv, 3]; faces int32 [nf, 3]; areas float64 [nf]: cer_mesh_face_areas_f64's.
 *
 * The distance of a point p to a triangle (a, b, c): Ericson's closest point by regions.  dot(x, y) = (x0*y0 + x1*y1) + x2*y2;
 *   ab = b-a, ac = c-a, ap = p-a, bp = p-b, cp = p-c;
 *   d1 = dot(ab,ap), d2 = dot(ac,ap), d3 = dot(ab,bp), d4 = dot(ac,bp), d5 = dot(ab,cp), d6 = dot(ac,cp);
 *   vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4.
 * The first region that holds decides:
 *   1. d1 <= 0 && d2 <= 0: the closest point q is the corner a itself;
 *   2. d3 >= 0 && d4 <= d3: the corner b itself;
 *   3. vc <= 0 && d1 >= 0 && d3 <= 0: v = d1 / (d1 - d3), w = 0;
 *   4. d6 >= 0 && d5 <= d6: the corner c itself;
 *   5. vb <= 0 && d2 >= 0 && d6 <= 0: v = 0, w = d2 / (d2 - d6);
 *   6. va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0: w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w;
 *   7. otherwise: den = (va + vb) + vc, v = vb / den, w = vc / den.
 * In the regions 3 and 5 to 7, per axis, q = (a + v*ab) + w*ac.  Then r = q - p and dist2 = (rx*rx + ry*ry) + rz*rz.
 * A face is a candidate iff dist2 <= double(max_dist)^2: inclusive, and false for a NaN (the 0 / 0 of a near-degenerate face loses).  The
 * winner is the smallest (dist2, face index).  Faces with areas[f] not above 0 - an index outside [0, nv), a repeated index, a coordinate
 * that is not finite, a computed area of 0 - are not indexed and are never anybody's nearest face.  A query that is not finite gets no face.
 * Per query: dist float32 = float(sqrt(dist2)), +inf without a face; face int32, -1 without; closest float32 [m, 3] (optional): q rounded
 * once, NaN without a face.
 *
 * The index is the grid of "Cloud evaluation" with triangles in place of points: the frame (origin, cell) and the 63-bit key are
 * cer_grid_keys_f32's, cell coordinate c = floor((double(x) - origin) / cell).  A face is entered in every cell of the box [cell of its
 * smallest corner coordinate, cell of its largest] per axis.
 *   cer_mesh_tri_cells_i64: cells int64 [nf] = the product of the box's three extents, 0 for a face that is left out.  A cell coordinate
 *     outside the key range (flag[0]) or a face of more than CER_TRI_MAX_CELLS cells (flag[1]) returns CER_ESHAPE after the launch - flag,
 *     two device ints of the caller's, carries the finding; the call synchronises the stream to read it.  One thread per face.
 *   The caller forms cum int64 [nf], the inclusive prefix sums of cells (integers: exact under any scan), and npairs = cum[nf - 1] < 2^31.
 *   cer_mesh_tri_pairs_i64: face f writes keys[p] = the cell's key and ids[p] = f for p in [cum[f - 1], cum[f]), z-major, then y, then x;
 *     a face whose box does not have exactly that many cells or whose positions leave [0, npairs) writes nothing (the caller's keys start
 *     as the sentinel 2^63 - 1).  One thread per face.
 *   The caller sorts the pairs by key with a stable sort (faces stay ascending inside a cell) and runs cer_grid_cells_count_i64 /
 *   cer_grid_cells_i64 on the sorted keys: cell_keys [ncells], cell_start [ncells + 1].
 *   cer_mesh_tri_pack_f32: records [nf] of 48 bytes, (x, y, z, 0) of the corners a, b, c - three 16-byte loads per candidate; zeros for an
 *     index outside [0, nv).  One thread per face.
 *   cer_mesh_tri_nearest_f32: one thread per query, in the order qorder int64 [m] (a permutation; null: 0 .. m-1), walking the rows of cells
 *     around the query, nearest first, against the best dist2 so far; pair_face int32 [npairs]: ids in sorted order.  A face id outside
 *     [0, nf), a pair position outside [0, npairs) and a vertex index outside [0, nv) are skipped, never read through.
 *
 * Checks, in the order of the section "Surface mesh", all before any launch: (1) a negative size, an origin or cell that is not finite, a
 * cell not above 0, a max_dist that is negative or no number -> CER_EINVAL; (2) nv >= 2^31, 3 nf >= 2^31, npairs >= 2^31, m >= 2^31, more
 * cells than pairs, ceil(max_dist / cell) beyond 4096 rings -> CER_ESHAPE; (3) nothing to do (nf == 0; the pairs also npairs == 0; the
 * search also m == 0 or ncells == 0) -> CER_OK with nothing launched; (4) a null pointer -> CER_EINVAL (vertices may be null iff nv == 0;
 * qorder and closest are null iff absent), then records that are not 16-byte aligned -> CER_EALIGN. */
#define CER_TRI_MAX_CELLS 4096
int cer_mesh_tri_cells_i64(const float* vertices, long long nv, const int* faces, long long nf, const double* areas, const double* origin,
                           double cell, long long* cells, int* flag, void* stream);
int cer_mesh_tri_pairs_i64(const float* vertices, long long nv, const int* faces, long long nf, const double* areas, const double* origin,
                           double cell, const long long* cum, long long npairs, long long* keys, int* ids, void* stream);
int cer_mesh_tri_pack_f32(const float* vertices, long long nv, const int* faces, long long nf, void* records, void* stream);
int cer_mesh_tri_nearest_f32(const void* records, long long nf, const int* pair_face, long long npairs, const long long* cell_keys,
                             const long long* cell_start, long long ncells, const double* origin, double cell, const float* queries,
                             const long long* qorder, long long m, float max_dist, int* face, float* dist, float* closest, void* stream);

/* Multi-GPU row-slab exchange (cer-mvs_amd/slab.py): up to CER_COPY_MAX_SEG contiguous fp32 ranges copied by ONE launch -
 * the pack of a rank's (net, disp) border strips into its send buffer, and the refresh of its halo rows from the gathered
 * strips.  n[i] floats from src[i] to dst[i]; n[i] == 0 skips a segment.  Device pointers; ranges must not overlap. */
#define CER_COPY_MAX_SEG 4
typedef struct cer_copy_segments {
    const float* src[CER_COPY_MAX_SEG];
    float* dst[CER_COPY_MAX_SEG];
    long n[CER_COPY_MAX_SEG];
} cer_copy_segments;
int cer_copy_segments_f32(const cer_copy_segments* seg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CER_MVS_H */
