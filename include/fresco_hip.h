/*
 * fresco_hip.h -- C ABI of libfresco_hip.so: the MI355X (gfx950 / CDNA4) kernels behind FRESCO's
 * flow-guided attention, feature warp and feature-optimisation hot path.
 *
 * Conventions (every entry point):
 *   - plain device pointers + explicit sizes; no torch / C++ types cross this boundary;
 *   - returns FRESCO_OK (0) or a negative FRESCO_E* code; nothing is thrown, nothing printed;
 *   - never allocates: scratch memory is passed in by the caller, sized by the matching
 *     *_workspace_bytes() query (host-only, no GPU needed);
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = the null stream);
 *   - no global state (except the opt-in fresco_prof_* timing log and per-device caches of launch settings):
 *     concurrent calls on different streams / devices with disjoint buffers are safe.
 *
 * Environment switches, for tests and measurement only:
 *   read per call:          FRESCO_GRAM_Z, FRESCO_GRAM_COOP, FRESCO_GRAM_SPLIT_WG, FRESCO_OPT_SPLIT, FRESCO_OPT_SVTAIL;
 *   read once per process:  FRESCO_FN_CONV_PATCH, FRESCO_FN_XCD_MAP;
 *   read by fresco_amd:     FRESCO_GMFLOW_LIBRARY_OPS, FRESCO_HIP_LIB (the library file to load).
 *
 * Reference interface each entry point replaces (paths relative to the FRESCO tree):
 *   src/diffusion_hacked.py  = DH,  src/flow_utils.py = FU,  src/utils.py = UT,
 *   src/ebsynth/deps/gmflow/gmflow/geometry.py = GEO.
 *
 * "half" below is IEEE binary16 (the dtype the SD-1.5 pipeline runs in, run_fresco.py:63-80).
 */
#ifndef FRESCO_HIP_H
#define FRESCO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRESCO_OK 0
#define FRESCO_EINVAL (-1)      /* null pointer / non-positive size / inconsistent arguments   */
#define FRESCO_EUNSUPPORTED (-2) /* shape outside what the kernels are instantiated for        */
#define FRESCO_EWORKSPACE (-3)  /* workspace too small                                          */
#define FRESCO_ELAUNCH (-4)     /* hipGetLastError() != hipSuccess after a launch              */

/* dtype codes for entry points that accept more than one element type */
#define FRESCO_F16 0
#define FRESCO_F32 1
#define FRESCO_BF16 2 /* bfloat16: the entry points below that take a `dtype`, fresco_adain, fresco_chan_mean_std, fresco_ddpm_*, fresco_freeu_*, fresco_hed_fuse, fresco_canny_hysteresis */

/* library / build identification: "fresco_hip <version> gfx950" */
const char* fresco_version(void);
/* last HIP error string seen by a FRESCO_ELAUNCH on this thread ("" if none) */
const char* fresco_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Opt-in kernel timing for bench.py's roofline figures (the ONLY process-global state of the
 * library; off by default).  While enabled, the launches tagged below are bracketed by HIP events
 * recorded on the launch stream.  fresco_prof_read synchronises on the recorded events, returns the
 * number of records copied (launch order) and clears the log.
 *   tags[i], dims[4*i..4*i+3], ms[i]:
 *     FRESCO_PROF_ATTN_FLASH : dims = {B*H, Lq, M, D}     FRESCO_PROF_KV_PACK : {groups, H, M, D}
 *     FRESCO_PROF_TEMPORAL   : dims = {chunk*N, HW, H, D}
 * ------------------------------------------------------------------------------------------ */
#define FRESCO_PROF_ATTN_FLASH 1
#define FRESCO_PROF_KV_PACK 2
#define FRESCO_PROF_TEMPORAL 3
/* feature optimisation, dims = {B, C, hw, 0}: */
#define FRESCO_PROF_OPT_TSIGN 4
#define FRESCO_PROF_OPT_TGRAD 5
#define FRESCO_PROF_OPT_COLNORM 6
#define FRESCO_PROF_OPT_GRAM 7
#define FRESCO_PROF_OPT_SV 8
#define FRESCO_PROF_OPT_ADAM 9
#define FRESCO_PROF_LINEAR 10 /* dims = {M, N, K, nw} */
#define FRESCO_PROF_ATTN_F32 11 /* dims = {B, Lq, Lk, D} */
#define FRESCO_PROF_FN_GEMM 12  /* dims = {M, N, K, kernel height (0: linear layer)} */
#define FRESCO_PROF_EBSYNTH_LEVEL 13 /* one pyramid level of fresco_ebsynth_run: dims = {level, tw, th, patch} */
int fresco_prof_enable(int capacity);
int fresco_prof_disable(void);
int fresco_prof_read(int max_records, int* tags, int* dims, float* ms);

/* ------------------------------------------------------------------------------------------
 * (a2 + a3)  Dense attention with shared / per-batch keys  -- replaces the two
 * F.scaled_dot_product_attention calls at DH:281-285 (spatial-guided) and DH:303-305
 * (efficient cross-frame), the K/V row selection + repeat at DH:225-247, and the head
 * split / merge views at DH:250-254, 371.
 *
 *   out[b, l, h*D + d] = sum_m softmax_m( scale * <q[b,l,h,:], K[g,m,h,:]> + diag_bias*[l==m] ) * V[g,m,h,d]
 *
 *   q   : (B, Lq, H*D) half, row-major (what attn.to_q returns)
 *   k,v : row-major matrices of H*D-wide half rows.  Key group g (0 <= g < n_groups) uses the M
 *         rows   g*group_rows + (kv_rows ? kv_rows[m] : m),  m = 0..M-1.
 *         Query batch b attends to group  g = b / (B / n_groups).
 *           cross-frame : n_groups = unet_chunk_size, group_rows = N*HW, kv_rows = flat indices of
 *                         the True entries of controller.attn_mask (N,HW), or NULL with M = HW for
 *                         "every frame uses frame 0" (former_frame_index, DH:227).
 *           spatial     : n_groups = B, group_rows = HW, kv_rows = NULL, M = HW,
 *                         q = to_q(ref), k = to_k(ref), v = current query, scale = 0.2/sqrt(D).
 *   out : (B, Lq, H*D) half, always dense.
 *   Row strides (in elements, multiples of 8, >= H*D): q row r starts at q + r*q_ld, k / v row r at k + r*kv_ld -- dense
 *   callers pass H*D; q, k, v may be column slices of one fused projection output (B, HW, 3*H*D).
 *   dtype = FRESCO_F16 or FRESCO_BF16 for q, k, v and out (any other code: FRESCO_EINVAL before any HIP call; "half" above
 *   reads as the element type).  Elements are 2 bytes either way: same workspace, same packed key image geometry.
 *   D in {8, 16, 32, 40, 64, 80, 96, 128}, both element types.  Softmax in fp32, P and V in the element type, accumulation
 *   fp32.
 *   Numerics, fp16: the exponent scale  scale*log2(e)  is folded into the fp16 query (one rounding) only for
 *   queries whose logits are provably small (scale*log2e*|q|*max|k| <= 16, a per-wavefront decision from
 *   the key norms the pack pass records); otherwise scores are scaled in fp32.  Logits are assumed to stay
 *   below 6e4 in log2 units.
 *   Numerics, bf16: scores and softmax in fp32, P and O^T products on the bf16 MFMA; the softmax scale is never folded into
 *   the bf16 Q (one bf16 rounding of scale*q costs more than P's own rounding) but applied to the fp32 scores; the running
 *   max is kept on the bf16 grid.
 *   Workspace: packed K / V^T images of every key group and head plus one float per 64-key tile.
 * ------------------------------------------------------------------------------------------ */
size_t fresco_attn_workspace_bytes(int n_groups, int H, int M, int D);
int fresco_attn_fwd(const void* q, const void* k, const void* v, const int32_t* kv_rows,
                    void* out, void* workspace, size_t workspace_bytes,
                    int B, int H, int Lq, int D,
                    int n_groups, int M, int64_t group_rows,
                    float scale, float diag_bias, int64_t q_ld, int64_t kv_ld, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a1)  Fused linear projections  attn.to_q / to_k / to_v (DH:201, 214-215, 260-261) and to_out[0] (DH:375):
 *           out_j = x W_j^T (+ b_j),   j = 0 .. nw-1,  nw <= 3
 *   x    : (M, K) half, row stride x_ld (elements);  read once for all nw outputs
 *   x_rows : NULL, or int32 (M): problem row m reads x row x_rows[m] (each inside the x buffer -- the caller's contract).
 *          Used for the K / V projection of the tokens the efficient cross-frame pass selects (DH:225-247) when nothing
 *          else reads K and V: project only what is gathered.
 *   W_j  : (N, K) half row-major = the weight of nn.Linear j, read where it lives (nothing is stacked or cached:
 *          in-place updates of a module's weight are seen by the next call);  W1 / W2 unused beyond nw
 *   b_j  : (N) half or NULL
 *   out_j: (M, N) half, row stride ld_j (elements); unused outputs NULL
 *   dtype = FRESCO_F16 or FRESCO_BF16 for ALL operands (x, W_j, b_j, out_j; strides stay in elements of 2 bytes; "half"
 *   above reads as the element type).  Any other dtype code: FRESCO_EINVAL, before any HIP call.
 *   fp32 accumulation, one rounding to nearest even at the store (what the library GEMM behind nn.Linear does); bf16 runs
 *   the same kernel on v_mfma_f32_32x32x16_bf16.
 *   Supported: K in {320, 640} (SD-1.5 up_blocks.3 / up_blocks.2), N % 64 == 0, nw * N <= 2048 (fresco_linear_plan
 *   answers without a launch); anything else returns FRESCO_EUNSUPPORTED and the caller keeps its own GEMM.
 * ------------------------------------------------------------------------------------------ */
int fresco_linear(const void* x, int64_t x_ld, const int32_t* x_rows, const void* W0, const void* W1, const void* W2,
                  const void* b0, const void* b1, const void* b2, void* out0, void* out1, void* out2, int64_t ld0,
                  int64_t ld1, int64_t ld2, int nw, int M, int N, int K, int dtype, void* stream);

/* The launch fresco_linear would make for (nw, M, N, K), decided on the host alone (no launch, no HIP call, no GPU needed):
 * returns what that entry point returns for the same four arguments -- FRESCO_EINVAL for nw outside 1..3 or a size <= 0,
 * FRESCO_EUNSUPPORTED for N % 64 != 0, K outside {320, 640} or an LDS plan beyond 160 KiB (ring + x staging + an nw * N
 * bias image, charged with or without biases: nw * N <= 2048) -- and, on FRESCO_OK, writes the grid (row_blocks =
 * ceil(M / 256), splits) and the number of 64-feature tiles of the nw * N / 64 a workgroup walks (the last split may get
 * fewer).  Each output pointer may be NULL.  Callers use it to ask "is this width supported"; tests, which loop regime of
 * the kernel a shape lands in (one tile per split; several, where the weight ring wraps and a split may begin inside an
 * output or run across two or three). */
int fresco_linear_plan(int nw, int M, int N, int K, int* row_blocks, int* splits, int* tiles_per_split);


/* Cross-frame pass with the K | V projection of the selected rows FUSED into the key pack -- for layer calls
 * whose only reader of K and V is the cross-frame pass (DH:201-247 on the cross-frame-only steps): replaces
 * attn.to_k / attn.to_v on the gathered rows (DH:214-215 restricted to the tokens DH:239-247 keep) + the pack.
 *   x      : hidden states, rows of K_in features, row r at x + r*x_ld
 *   x_rows : int32 (n_groups * M): key m of group g is row x_rows[g*M + m] of x (rows may repeat; must be in range --
 *            the table is not checked on the device)
 *   Wk, Wv : (H*D, K_in) row-major weights of the bias-free projections (read where they live, every call)
 *   q, out, workspace (fresco_attn_workspace_bytes(n_groups, H, M, D)), B, H, Lq, D, n_groups, M, scale, q_ld: as
 *   fresco_attn_fwd; batch element b uses key group b / (B / n_groups).
 *   dtype = FRESCO_F16 or FRESCO_BF16 for q, x, Wk, Wv and out (any other code: FRESCO_EINVAL; every argument check
 *   answers before any HIP call).
 * K = x[rows] Wk^T and V = x[rows] Wv^T are rounded to the element type exactly once (as the two-launch path rounds them)
 * and go straight into the packed key image: they never exist in HBM.  bf16: the projection on the bf16 MFMA with the
 * same contraction order and one fp32 chain per output, the ones column / row of the image in bf16, max |k|^2 over the
 * rounded K; then the bf16 flash kernels of fresco_attn_fwd (scale never folded).
 * Supported: (D, K_in) = (40, 320), (80, 640) with H*D == K_in (SD-1.5's decoder self-attentions);
 * fresco_attn_kvproj_supported says so, anything else returns FRESCO_EUNSUPPORTED and the caller uses fresco_linear with
 * x_rows + fresco_attn_fwd. */
int fresco_attn_kvproj_supported(int H, int D, int K_in);
int fresco_attn_fwd_kvproj(const void* q, const void* x, int64_t x_ld, const int32_t* x_rows, const void* Wk,
                           const void* Wv, void* out, void* workspace, size_t workspace_bytes, int B, int H, int Lq,
                           int D, int n_groups, int M, int K_in, float scale, int64_t q_ld, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a4)  Temporal-guided (FLATTEN) attention -- replaces DH:309-367: 3 rearrange+gather round
 * trips, the per-pixel N x N masked SDPA and the inverse gather.
 *
 *   for every aligned pixel p, CFG half c, head h, frames f,g in [0,N):
 *     row(f) = fwd_map[f*HW + p]
 *     out[c*N+f, row(f), h, :] = sum_g softmax_g( scale*<q[c*N+f,row(f),h,:], k[c*N+g,row(g),h,:]>
 *                                                 | mask[p,f,g] ) * v[c*N+g,row(g),h,:]
 *   q,k,v,out : (chunk*N, HW, H*D) half;  q, k, v rows start every q_ld / k_ld / v_ld elements (multiples of 8, >= H*D;
 *   dense callers pass H*D), out is dense;  fwd_map : (N, HW) int64 (a permutation per frame);
 *   mask : (HW, N, N) uint8/bool, non-zero = may attend (diagonal always set, FU:120-131).
 *   D in {8, 16, 32, 40, 64, 80}; chunk*N*HW < 2^31.  N <= 32: MFMA kernel (needs N * (6*(H*D + 8) + 4 + N) bytes
 *   <= 160 KiB of LDS for 16 < N <= 32: every SD-1.5 shape fits); N > 32: vector-ALU kernel while 6*N*H*D + 4*N + N*N
 *   bytes <= 160 KiB; otherwise FRESCO_EUNSUPPORTED.  Row-table entries outside [0, HW) are skipped (no row is read or
 *   written for them; a table that is not a permutation is the caller's bug).  A query whose mask row is all zero
 *   yields NaN, like the reference's softmax over an all -inf row.
 *   dtype = FRESCO_F16 or FRESCO_BF16 for q, k, v and out (any other code: FRESCO_EINVAL before any HIP call).  The scale
 *   (the reference's 0.2 key factor included) stays an fp32 factor of the scores.
 * ------------------------------------------------------------------------------------------ */
int fresco_temporal_attn(const void* q, const void* k, const void* v, const int64_t* fwd_map,
                         const uint8_t* mask, void* out,
                         int chunk, int N, int HW, int H, int D, float scale,
                         int64_t q_ld, int64_t k_ld, int64_t v_ld, int dtype, void* stream);

/* Multi-GPU: frames are sharded over ranks, the temporal pass is sharded by TRAJECTORY, so that
 * every byte crosses the fabric once and the kernel's HBM traffic shrinks with the world size.  Rank r owns the
 * n_loc frames [f0, f0+n_loc) of both CFG halves and the trajectory range [r*P, (r+1)*P), P = HW / world.
 *   fresco_temporal_pack  : buf[(d*n_loc + fl)*chunk + c][pl][0:3C] = (q | k | v)[c*n_loc + fl][fwd_map[f0+fl][d*P + pl]]
 *                           (q, k, v: local (chunk*n_loc, HW, C) with row strides q_ld / k_ld / v_ld); an all-to-all over
 *                           the leading `world` dimension then leaves on rank r the rows of ALL N frames of its range as
 *                           (N, chunk, P, 3C);
 *   fresco_temporal_attn_packed : the attention on such rows, no row table: qkv (N, chunk, P, 3C), mask (P, N, N) = the
 *                           mask rows of the range, out (N, chunk, P, C); dtype = FRESCO_F16 or FRESCO_BF16 for qkv and
 *                           out (any other code: FRESCO_EINVAL before any HIP call);
 *   fresco_temporal_unpack: after the all-to-all back, buf (world, n_loc, chunk, P, C) holds this rank's frames' result rows
 *                           per range:  out[c*n_loc + fl][fwd_map[f0+fl][d*P + pl]] = buf[(d*n_loc + fl)*chunk + c][pl]. */
int fresco_temporal_pack(const void* q, const void* k, const void* v, const int64_t* fwd_map, void* buf, int chunk,
                         int n_loc, int f0, int HW, int C, int world, int64_t q_ld, int64_t k_ld, int64_t v_ld,
                         void* stream);
int fresco_temporal_attn_packed(const void* qkv, const uint8_t* mask, void* out, int chunk, int N, int P, int H, int D,
                                float scale, int dtype, void* stream);
int fresco_temporal_unpack(const void* buf, const int64_t* fwd_map, void* out, int chunk, int n_loc, int f0, int HW,
                           int C, int world, void* stream);
/* fresco_temporal_pack / fresco_temporal_unpack move 16-byte pieces of 16-bit words and do no arithmetic: they are
 * element-type agnostic for 2-byte types (fp16 and bf16 alike) and need no dtype. */

/* ------------------------------------------------------------------------------------------
 * (a8)  flow_warp / bilinear_sample  (GEO:41-72): bilinear, zeros padding, align_corners=True.
 *   x, out : (B, C, h, w) fp32;  flow : (Bf, 2, h, w) fp32, channel 0 = x, 1 = y.
 *   Batch b samples with flow[b % Bf]  (Bf = B, or the un-repeated N when x holds `chunk` copies).
 * ------------------------------------------------------------------------------------------ */
int fresco_flow_warp(const float* x, const float* flow, float* out,
                     int B, int C, int h, int w, int Bf, void* stream);

/* F.interpolate(x * mul, scale_factor=s, mode='bilinear') (align_corners=False, no antialias);
 * (B,C,H,W) -> (B,C,ho,wo) fp32 with the source-coordinate scale rscale = 1/s as torch computes
 * it when scale_factor is given (FU:26,30,35; DH:439,441,937). */
int fresco_resize_bilinear(const float* x, float* out, int BC, int H, int W, int ho, int wo,
                           float rscale_h, float rscale_w, float mul, void* stream);

/* F.max_pool2d(x, kernel_size=k) (stride k, floor) on (BC,H,W) fp32 -> (BC,H/k,W/k)  (FU:27,31; DH:440,442) */
int fresco_max_pool(const float* x, float* out, int BC, int H, int W, int k, void* stream);

/* fp32 attention for the flow network (f3): out = softmax(scale * q k^T) v, one head.
 *   GMFlow's full / window attention (gmflow/transformer.py:8-17, 92-95; windows = batch entries), global
 *   correlation softmax (gmflow/matching.py:7-36: v = pixel grid, Dv = 2) and flow propagation
 *   (gmflow/transformer.py:356-372: v = flow, Dv = 2).
 *   q (B,Lq,D), k (B,Lk,D), v (B,Lk,Dv), out (B,Lq,Dv): fp32 row-major, dense.  D in {32, 64, 128}, Dv <= 128.
 *   fp32-class accuracy on the fp16 matrix pipe: operands split into fp16 pieces (33-bit logits, 22-bit P V products),
 *   fp32 softmax (the flows feed integer decisions downstream).
 *   workspace: NULL -- every 128-query workgroup stages and splits its own K / V tiles -- or
 *     fresco_attn_f32_workspace_bytes(B, Lk, D, Dv) bytes, 16-byte aligned: K and V are converted to the kernel's split-fp16
 *     LDS images ONCE per launch instead of once per workgroup (what pays as soon as two workgroups share a key set:
 *     Lq >= 256).  Same results either way, bit for bit.
 *   flag: NULL -- the operands must stay in the range the fp16 pieces can hold, |q scale log2 e|, |k|, |v| < 1000 (the
 *     caller's duty; nothing is checked on the device) -- or one int32 of device memory the caller lends for the call, which
 *     lifts the limit: *flag is raised when any operand is beyond that range or not finite, and an exact-fp32 MFMA kernel
 *     behind the split-fp16 one then recomputes the launch (it returns at once when the flag is clear: in range the results
 *     are those without a flag, bit for bit).  How the flag gets raised:
 *       flag_is_zero == 0: the call clears *flag and runs a range pass over q, k, v in front of the attention;
 *       flag_is_zero != 0: no memset, no range pass -- the k / v test runs inside the split pass, the q test in the
 *         attention kernel's prologue.  The CALLER guarantees *flag to be ZERO in stream order when the call is issued, and
 *         untouched by anyone else until the call's kernels are done (fresco_amd.ops hands out the words of a zero-filled
 *         pool, each once).  Only the workspace kernels carry the in-kernel test: workspace == NULL is FRESCO_EINVAL, and
 *         so is flag == NULL.  Results: those of flag_is_zero == 0 with a workspace, bit for bit, in range and out of range.
 *   fresco_amd.ops.attention_f32 -- and with it the flow network -- always passes a flag: workspace + flag_is_zero for
 *   Lq >= 256 (every attention call of the flow network), neither below.
 *   Every argument check answers before any HIP call: FRESCO_EINVAL (null q / k / v / out, non-positive size or scale, the
 *   flag_is_zero rule), FRESCO_EUNSUPPORTED (B > 65535, a (D, Dv) outside the list), FRESCO_EWORKSPACE. */
size_t fresco_attn_f32_workspace_bytes(int B, int Lk, int D, int Dv); /* 0 for an unsupported (D, Dv) */
int fresco_attn_f32(const float* q, const float* k, const float* v, float* out, void* workspace, size_t workspace_bytes,
                    int* flag, int flag_is_zero, int B, int Lq, int Lk, int D, int Dv, float scale, void* stream);

/* ---- the flow network's dense layers (f3): GMFlow's CNN encoder, transformer projections / FFN / LayerNorms, upsampler head
 * (gmflow/backbone.py:7-117, transformer.py:111-237, gmflow.py:44-90).  fp32 in, fp32 out, fp32-class accuracy on the fp16
 * matrix pipe: a tensor that feeds a product exists as a pair of fp16 planes (hi, lo), x = hi + lo to 2^-22, written by its
 * producer (fresco_fn_prep / fresco_fn_layernorm / fresco_fn_gemm's epilogue); products are hi hi + hi lo + lo hi.
 * The planes hold x * split_scale (a power of two: the matrix pipe flushes fp16 subnormals, so lo pieces must stay normal
 * numbers; fresco_amd uses 2^6 for activations, |x| < 1000, and 2^10 for weights, |w| < 60; beyond that the scaled value
 * saturates -- finite, wrong -- and the producer ORs 1 into the caller's `range_flag` word (int32 in device memory, cleared
 * by the caller, may be NULL): fresco_amd's flow network checks it once per forward and recomputes with library ops);
 * fresco_fn_gemm multiplies its fp32 accumulators by acc_scale = 1 / (scale_A * scale_W) before the bias.
 * Activations are NHWC: rows m = (image, y, x), channels contiguous -- the transformer's (B, L, C) token layout. */

/* out[m][n] = act( sum_k A(m, k) W[n][k] + bias[n] ),  m < M, n < N, K % 32 == 0.
 *   kh == 0: A = a_hi + a_lo, (M, K) row-major with row stride lda (halfs)               -- nn.Linear / 1 x 1 conv
 *   kh  > 0: implicit im2col of an NHWC tensor (n_img, H, W, cin = K / (kh kw)), pixel stride lda >= cin, cin % 32 == 0,
 *            k = (ky, kx, ci), zero padding `pad`, stride `stride`, dilation `dilation` >= 1: tap (ky, kx) of output pixel
 *            (oy, ox) reads pixel (oy stride - pad + ky dilation, ox stride - pad + kx dilation); M must be
 *            n_img * OH * OW, OH = (H + 2 pad - dilation (kh - 1) - 1) / stride + 1                 -- nn.Conv2d
 *   w_hi / w_lo: (N, K) row-major fp16 planes; bias (N) fp32 or NULL; act 0 none, 1 ReLU, 2 GELU (erf form).
 *   out (M, ldc) fp32 and / or out_hi / out_lo (M, ldo) fp16 planes of the result (either may be NULL, not both; planes need
 *   N % 8 == 0).  zeros: 16 bytes of zeros in device memory (the source of every row outside the problem and of a
 *   convolution's zero padding: the operands arrive by LDS-DMA).  stats (convolutions whose OH * OW is a multiple of 256;
 *   a_rows / out_rows (linear layers only, int32 (M) device tables or NULL): problem row m reads input row a_rows[m], its
 *   results go to output row out_rows[m] (a token gather / scatter folded into the product).  stats: (M / 64) * N * 2 doubles that
 *   receive per-column partial sums / sums of squares of the results for fresco_fn_colstats_finish (InstanceNorm2d without a
 *   second pass over the convolution's output). */
int fresco_fn_gemm(const void* a_hi, const void* a_lo, int64_t lda, const void* w_hi, const void* w_lo, const float* bias,
                   float* out, void* out_hi, void* out_lo, int64_t ldc, int64_t ldo, int M, int N, int K, int act,
                   float acc_scale, float split_scale, int n_img, int H, int W, int kh, int kw, int stride, int pad,
                   int dilation, void* stats, const void* zeros, const int32_t* a_rows, const int32_t* out_rows,
                   int32_t* range_flag, int out_col_block, int64_t out_block_stride, void* stream);
/* out_col_block > 0 (fp32 output only, N % out_col_block == 0): column n of the product goes to matrix n / out_col_block of
 * out_col_block columns (row stride ldc >= out_col_block), the matrices out_block_stride floats apart -- several projections of
 * one input as ONE product (W = their weight rows stacked), every projection's rows contiguous (round 6: q | k | v and k | v of the
 * flow network's attention layers).  0: one (M, ldc) matrix. */

/* nn.InstanceNorm2d statistics (affine=False, biased variance): x (n_img * rows, C) fp32 NHWC -> mean, rstd = 1 / sqrt(var +
 * eps), (n_img, C) each.  fp64 partial sums in a fixed order.  C <= 256. */
size_t fresco_fn_colstats_workspace_bytes(int n_img, int rows, int C);
int fresco_fn_colstats(const float* x, float* mean, float* rstd, void* workspace, size_t workspace_bytes, int n_img, int rows,
                       int C, float eps, void* stream);
int fresco_fn_colstats_finish(const void* stats, float* mean, float* rstd, int n_img, int rows, int C, float eps, void* stream);

/* y = relu_b?( relu_a?( (x - mean[img]) * rstd[img] ) + residual ) on (M, C) fp32 rows (mean / rstd / residual may be NULL;
 * img = m / rows_per_img).  Writes y (M, C) fp32 and / or the fp16 planes out_hi / out_lo with row stride ldo >= C, channels
 * C .. ldo-1 zeroed (K padding of the product that reads them).  C % 4 == 0, ldo % 4 == 0. */
int fresco_fn_prep(const float* x, const float* mean, const float* rstd, const float* residual, float* y, void* out_hi,
                   void* out_lo, int64_t M, int C, int ldo, int rows_per_img, int relu_a, int relu_b, float split_scale,
                   int32_t* range_flag, void* stream);

/* nn.LayerNorm(128) (+ residual): y = residual + ((x - mean) / sqrt(var + eps)) gamma + beta on (M, 128) fp32 rows; fp32 y
 * (row stride ldy) and / or fp16 planes (row stride ldo). */
int fresco_fn_layernorm(const float* x, const float* gamma, const float* beta, const float* residual, float* y, void* out_hi,
                        void* out_lo, int64_t ldy, int64_t ldo, int64_t M, int C, float eps, float split_scale,
                        int32_t* range_flag, void* stream);

/* The encoder's stem: Conv2d(3, 64, 7, stride 2, padding 3, bias=False) (gmflow/backbone.py:69) on the matrix pipe (split-fp16
 * products, fp32-class accuracy; round 6 -- rounds 5: direct fp32 FMAs).  x (n_img, H, W, 3) NHWC fp32; w_hi / w_lo: fp16
 * planes (scale 2^10, as fresco_fn_prep writes them) of the (64, 224) matrix W'[cout][32 ky + 3 kx + ci] = weight[cout][ci][ky][kx],
 * the 11 surplus positions of every kernel row ZERO; out (n_img, OH, OW, 64) NHWC fp32, OH = (H - 1) / 2 + 1.
 * stats (may be NULL): fp64 InstanceNorm partial sums of `out`, (n_img OH OW / 64) slabs x 64 channels x 2, combined by
 * fresco_fn_colstats_finish; needs OW % 64 == 0 and OH OW % 256 == 0 (FRESCO_EUNSUPPORTED otherwise).
 * range_flag (may be NULL): OR 1 when an input value leaves the operand planes' range (|x| >= 1015). */
int fresco_fn_conv7_rgb(const float* x, const void* w_hi, const void* w_lo, float* out, void* stats, int n_img, int H, int W,
                        int32_t* range_flag, void* stream);

/* Convex upsampling by 8 (gmflow.py:75-90): out (B, 2, 8h, 8w) = softmax-over-9-weighted mix of the 3 x 3 coarse neighbourhood
 * of 8 * flow.  logits (B, h, w, 576) = the mask head's NHWC rows (channel = n * 64 + ky * 8 + kx), flow (B, h * w, 2). */
int fresco_fn_convex_upsample(const float* logits, const float* flow, float* out, int B, int h, int w, void* stream);

/* forward_backward_consistency_check (gmflow/geometry.py:75-96) fused with the colour-difference
 * occlusion refinement of get_flow_and_interframe_paras (DH:919-926).  Pair n couples frame n with frame
 * (n+1) mod N: fwd_flow[n] maps frame n onto n+1, bwd_flow[n] the reverse; all fp32.
 *   fwd_occ[n] = |fwd + warp(bwd, fwd)| > alpha*(|fwd|+|bwd|) + beta  OR  mean_c |img[n]   - warp(img[n+1], fwd)| > color_thr
 *   bwd_occ[n] = |bwd + warp(fwd, bwd)| > alpha*(|fwd|+|bwd|) + beta  OR  mean_c |img[n+1] - warp(img[n],   bwd)| > color_thr
 *   images (N,C,H,W) in 0..255 or NULL (consistency check only); flows (N,2,H,W); occs (N,H,W) in {0,1}.
 *   Reference constants: alpha 0.01, beta 0.5, color_thr 255*0.25. */
int fresco_flow_occlusion(const float* images, const float* fwd_flow, const float* bwd_flow, float* fwd_occ,
                          float* bwd_occ, int N, int C, int H, int W, float alpha, float beta, float color_thr,
                          void* stream);

/* Dilate (UT:81-93): replicate pad (k-1)/2, k x k box sum, clamp [0,1]; (BC,H,W) fp32, k odd */
int fresco_dilate(const float* x, float* out, int BC, int H, int W, int k, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a7)  warp_tensor frame chain (FU:41-51).  `lat` (chunk*N, C, h, w) fp32 is updated IN PLACE:
 *   for c in chunk: for i in 0..N-2:  lat[c*N+i+1] = lat[c*N+i+1]*(1-m) + warp(lat[c*N+i], bwd_flow[i])*m,
 *                                      m = (1-bwd_occ[i]) * sal[i+1] * warp_sal[i]
 *                   last:             lat[c*N+N-1] blended with warp(lat[c*N], fwd_flow[N-1]),
 *                                      m = (1-fwd_occ[N-1]) * sal[N-1] * warp_sal_last
 *   bwd_flow, fwd_flow : (N,2,h,w); bwd_occ, fwd_occ, sal, warp_sal : (N,h,w); warp_sal_last : (h,w).
 *   The chain is sequential in the frame index (N launches), parallel over chunk, C, h, w.
 * ------------------------------------------------------------------------------------------ */
int fresco_warp_fuse_chain(float* lat, const float* bwd_flow, const float* fwd_flow,
                           const float* bwd_occ, const float* fwd_occ, const float* sal,
                           const float* warp_sal, const float* warp_sal_last,
                           int chunk, int N, int C, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a9)  adaptive_instance_normalization (UT:58-78) over rows of L = h*w elements:
 *   out = (content - mean_c) / sqrt(var_c + eps_content) * sqrt(var_s + eps_style) + mean_s,
 *   unbiased variance.  The reference's style eps is 1.0 (UT:73 passes chunk into eps).
 *   content, style, out : (rows, L), dtype FRESCO_F16, FRESCO_BF16 or FRESCO_F32 (all three the same; fp32 arithmetic,
 *   one rounding to nearest even at the store).
 * ------------------------------------------------------------------------------------------ */
int fresco_adain(const void* content, const void* style, void* out, int rows, int L,
                 float eps_content, float eps_style, int dtype, void* stream);

/* calc_mean_std (src/utils.py:58-67): per row (= one (sample, channel) plane of L values, dtype F16 / BF16 / F32):
 *   mean[row] = mean(x), stdv[row] = sqrt(unbiased variance + eps), both fp32.  L > 1. */
int fresco_chan_mean_std(const void* x, float* mean, float* stdv, int rows, int L, float eps, int dtype,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * (a6)  optimize_feature (DH:416-488): Adam on an fp32 copy of the features against
 *   L = 2*mean(|(c2 - W_b c1)(1-occ_b)| + |(c1 - W_f c2)(1-occ_f)|) + intra_weight*mean|V V^T - T|.
 *
 *   cs        : (chunk*N, C, h, w) fp32, updated in place (the optimised parameter)
 *   fwd_flow, bwd_flow : (N, 2, h, w) fp32 at feature resolution (already scaled), or NULL
 *   fwd_occ, bwd_occ   : (N, h, w) fp32, or NULL           (temporal term off when NULL)
 *   target    : (chunk*N, hw, hw) fp32 Gram target, or NULL (spatial term off when NULL)
 *   iters Adam steps (lr, beta1, beta2, eps as torch.optim.Adam); no autograd: analytic
 *   gradients.  The adjoint of the bilinear warp is evaluated as a deterministic gather over a
 *   per-call CSR of the tap matrix (no atomics), so results are run-to-run reproducible.
 *   ctx == NULL: fresco_opt_run keeps everything on `stream` and touches no state outside its arguments.
 *   ctx = a context (fresco_ctx_create / _destroy: a side stream + events, created on first use on the device current
 *   then, owned by the CALLER; the library keeps no process-wide stream table): with chunk == 2 and N * h * w >= 2048, the
 *   two CFG halves (independent problems) run as two pipelines: one on `stream`, one on the context's side stream, forked
 *   from and joined back into `stream` by events inside the call -- the caller sees ordinary stream order
 *   (FRESCO_OPT_SPLIT=0 keeps everything on `stream`; the results are bit-identical either way).  One call at a time per
 *   context (a second concurrent call on the same context, or a call on another device than the context's, runs on one
 *   stream); use one context per host thread / stream.
 *
 *   fresco_opt_loss_grad evaluates the closure once: grad (same shape as cs) and, if loss != NULL,
 *   loss[0] = temporal term, loss[1] = spatial term (device floats).  Test / debugging entry.
 * ------------------------------------------------------------------------------------------ */
size_t fresco_opt_workspace_bytes(int chunk, int N, int C, int h, int w, int has_temporal,
                                  int has_target);

int fresco_ctx_create(void** ctx);
int fresco_ctx_destroy(void* ctx); /* waits for the context's stream; FRESCO_EINVAL while a call is using it */
int fresco_opt_run(void* ctx, float* cs, const float* fwd_flow, const float* bwd_flow,
                   const float* fwd_occ, const float* bwd_occ, const float* target,
                   void* workspace, size_t workspace_bytes,
                   int chunk, int N, int C, int h, int w,
                   float intra_weight, int iters, float lr, float beta1, float beta2, float eps,
                   void* stream);

int fresco_opt_loss_grad(const float* cs, const float* fwd_flow, const float* bwd_flow,
                         const float* fwd_occ, const float* bwd_occ, const float* target,
                         float* grad, float* loss, void* workspace, size_t workspace_bytes,
                         int chunk, int N, int C, int h, int w, float intra_weight, void* stream);

/* Frame-sharded optimize_feature (multi-GPU): this rank owns n_loc consecutive frames of
 * both CFG halves out of N_total.  cs, target : local (chunk*n_loc, ...).  The temporal term couples
 * neighbouring frames, so before EVERY step the host hands over the current values of the frame before
 * (halo_l) and after (halo_r) the owned range, each (chunk, C, h, w) fp32 (ring order, wrap-around).
 * fwd_flow, bwd_flow : (n_loc+1, 2, h, w), fwd_occ, bwd_occ : (n_loc+1, h, w) -- entry j belongs to the
 * frame pair (f0-1+j, f0+j) mod N_total; both loss terms are normalised by the GLOBAL batch 2*N_total.
 * begin: zero the Adam state, build the warp-adjoint CSRs; step `it` = 1..iters: one Adam iteration.
 * With n_loc = N_total and halos = own last / first frame this reproduces fresco_opt_run.
 * part: the step as one host call (3) or as two, so that the neighbour exchange of the halo frames can run UNDER the
 * launches that do not read them.  part = 1: normalisation, the residual signs of the interior pairs, Gram and S V
 * products (halo_l / halo_r are not read and may be NULL); part = 2: the residual signs of the two pairs that touch a halo
 * frame, then Adam (halos required); part = 3: both, the undivided step.  Part 1 followed by part 2 performs, per element,
 * exactly the operations of the undivided step: results are identical bit for bit.  Typical loop of a rank:
 * start the (asynchronous) exchange of the frames Adam(it-1) produced -> part 1 of step it -> wait for the halos ->
 * part 2 of step it. */
size_t fresco_opt_sharded_workspace_bytes(int chunk, int n_loc, int C, int h, int w, int has_temporal,
                                          int has_target);
int fresco_opt_sharded_begin(const float* fwd_flow, const float* bwd_flow, const float* fwd_occ,
                             const float* bwd_occ, void* workspace, size_t workspace_bytes,
                             int chunk, int n_loc, int N_total, int C, int h, int w, int has_target,
                             void* stream);
int fresco_opt_sharded_step(float* cs, const float* halo_l, const float* halo_r,
                            const float* fwd_flow, const float* bwd_flow, const float* fwd_occ,
                            const float* bwd_occ, const float* target, void* workspace,
                            size_t workspace_bytes, int chunk, int n_loc, int N_total, int C, int h, int w,
                            float intra_weight, int it, float lr, float beta1, float beta2, float eps,
                            int part, void* stream);

/* Gram target of get_intraframe_paras (DH:889-895): T[b] = V V^T, V = rows of x (B,C,h,w)
 * viewed as (B, hw, C) and L2-normalised; fp32 (B,hw,hw).  workspace: fresco_gram_target_workspace_bytes(B, C, hw) bytes
 * (B*C*hw + 33*B*hw floats, each block rounded up to 256 bytes; 0 for a non-positive size). */
size_t fresco_gram_target_workspace_bytes(int B, int C, int hw);
int fresco_gram_target(const float* x, float* target, void* workspace, size_t workspace_bytes,
                       int B, int C, int hw, void* stream);

/* ------------------------------------------------------------------------------------------
 * (f1)  FLATTEN pixel correspondences -- get_mapping_ind / get_single_mapping_ind (FU:56-138) without
 * the per-pixel Python loop.  Inputs are the reference's intermediates at the reduced resolution
 * (produced with fresco_resize_bilinear, scale_factor = 1/scale):
 *   flow   : (N-1, 2, H, W) resized bwd flow, channel 0 = x, 1 = y, NOT yet divided by scale
 *   occ    : (N-1, H, W)    resized bwd occlusion (> 0.5 = occluded)
 *   frames : (N, 3, H*W)    resized images
 * Outputs: fwd_map, bwd_map (N, H*W) int64, mask (H*W, N, N) uint8 {0,1}.  Integers are bit-exact with
 * the reference's CPU run (ties: the earliest source wins, unlinked targets get the unused sources in
 * ascending order).
 * ------------------------------------------------------------------------------------------ */
size_t fresco_mapping_workspace_bytes(int N, int H, int W);
int fresco_mapping_ind(const float* flow, const float* occ, const float* frames, int64_t* fwd_map,
                       int64_t* bwd_map, uint8_t* mask, void* workspace, size_t workspace_bytes,
                       int N, int H, int W, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * (f2)  DDPM step of src/pipe_FRESCO.py:14-77 (+ classifier-free guidance, 212-214), elementwise over n
 * values, dtype FRESCO_F16 / FRESCO_BF16 / FRESCO_F32 (fp32 arithmetic inside, one rounding at the store):
 *   fresco_ddpm_x0  : eps = eps_text ? eps_uncond + guidance*(eps_text - eps_uncond) : eps_uncond
 *                     (written to eps_out if non-NULL);  x0 = (xt - sqrt_beta_prod*eps) / sqrt_alpha_prod
 *   fresco_ddpm_prev: out = c_x0*x0 + c_xt*xt + sigma*noise[i % noise_period]
 *                     (noise_period = n, or one frame's element count for repeat_noise)
 * The background-smoothing hack between the two (VAE decode -> warp_tensor -> VAE encode of x0) stays
 * with the caller.
 * ------------------------------------------------------------------------------------------ */
int fresco_ddpm_x0(const void* xt, const void* eps_uncond, const void* eps_text, void* x0, void* eps_out,
                   int64_t n, float guidance, float sqrt_beta_prod, float sqrt_alpha_prod, int dtype,
                   void* stream);
int fresco_ddpm_prev(const void* x0, const void* xt, const void* noise, void* out, int64_t n,
                     int64_t noise_period, float c_x0, float c_xt, float sigma, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * (g)  Ebsynth -- guided patch-based synthesis that propagates a stylised keyframe to another frame (video_blend.py's
 * second stage; the reference's ebsynthRun, src/ebsynth/deps/ebsynth/include/ebsynth.h).  Coarse to fine over an image
 * pyramid: per level, PatchMatch (propagation at jumps 4, 2, 1 + random search) of the nearest-neighbour field (NNF,
 * target pixel -> centre of its source patch) under the weighted SSD of style + guide channels plus a uniformity term,
 * then a patch vote; a stop mask freezes pixels whose style stopped changing.  DESIGN.md section 9.
 *   images  : uint8, channel-interleaved, row-major: src_style (src_h, src_w, n_style), src_guide (src_h, src_w,
 *             n_guide), tgt_guide / tgt_modulation (tgt_h, tgt_w, n_guide); tgt_modulation may be NULL;
 *             guide error per channel = guide_weights[c] * (mod/255) * diff^2
 *   weights : HOST arrays of n_style / n_guide floats
 *   levels  : -1 = fresco_ebsynth_max_levels(); per-level HOST arrays (coarse first) of `levels` ints
 *   outputs : out_style (tgt_h, tgt_w, n_style) uint8, out_error (tgt_h, tgt_w) fp32 patch error of the final NNF,
 *             out_nnf (tgt_h, tgt_w, 2) int32 (x, y) or NULL
 * n_style <= 8, n_guide <= 24, odd patch >= 3, every side >= 2 * patch + 1, levels <= fresco_ebsynth_max_levels():
 * FRESCO_EUNSUPPORTED otherwise, before any launch.  Same inputs and seed give bit-identical outputs.
 * The whole pyramid runs on `stream` with no host synchronisation.
 * ------------------------------------------------------------------------------------------ */
#define FRESCO_EBSYNTH_VOTE_PLAIN 1    /* weight 1            */
#define FRESCO_EBSYNTH_VOTE_WEIGHTED 2 /* weight 1 / (1 + E)  */
/* largest level count whose coarsest level keeps min(side of source, side of target) >= 2 * patch + 1 (0: none) */
int fresco_ebsynth_max_levels(int src_w, int src_h, int tgt_w, int tgt_h, int patch);
size_t fresco_ebsynth_workspace_bytes(int n_style, int n_guide, int src_w, int src_h, int tgt_w, int tgt_h,
                                      int patch, int levels, int with_modulation);
int fresco_ebsynth_run(const uint8_t* src_style, const uint8_t* src_guide, const uint8_t* tgt_guide,
                       const uint8_t* tgt_modulation, const float* style_weights, const float* guide_weights,
                       int n_style, int n_guide, int src_w, int src_h, int tgt_w, int tgt_h, float uniformity,
                       int patch, int vote_mode, int levels, const int* search_vote_iters,
                       const int* patchmatch_iters, const int* stop_threshold, int extra_pass_3x3, uint64_t seed,
                       int32_t* out_nnf, uint8_t* out_style, float* out_error, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Batched form: n problems that share the channel counts, the source and target sizes, the weights and every
 * per-level argument run through one launch sequence (the launches and copies of one fresco_ebsynth_run).  Every
 * image and output is n images of the single call's layout, back to back (problem b of src_style starts at
 * b * src_h * src_w * n_style bytes); seeds is a HOST array of n.  Problem b gives the same image, E and NNF, bit for
 * bit, as fresco_ebsynth_run with its inputs and seeds[b]: the random stream does not depend on the batch position.
 * 1 <= n <= FRESCO_EBSYNTH_MAX_BATCH (the seeds travel in kernel arguments): FRESCO_EINVAL below,
 * FRESCO_EUNSUPPORTED above, FRESCO_EWORKSPACE under fresco_ebsynth_batch_workspace_bytes(n, ...) (0 outside the
 * range), all before any launch.  fresco_ebsynth_run is n = 1 of this code; its workspace is the n = 1 size. */
#define FRESCO_EBSYNTH_MAX_BATCH 64
size_t fresco_ebsynth_batch_workspace_bytes(int n, int n_style, int n_guide, int src_w, int src_h, int tgt_w,
                                            int tgt_h, int patch, int levels, int with_modulation);
int fresco_ebsynth_run_batch(int n, const uint8_t* src_style, const uint8_t* src_guide, const uint8_t* tgt_guide,
                             const uint8_t* tgt_modulation, const float* style_weights, const float* guide_weights,
                             int n_style, int n_guide, int src_w, int src_h, int tgt_w, int tgt_h, float uniformity,
                             int patch, int vote_mode, int levels, const int* search_vote_iters,
                             const int* patchmatch_iters, const int* stop_threshold, int extra_pass_3x3,
                             const uint64_t* seeds, int32_t* out_nnf, uint8_t* out_style, float* out_error,
                             void* workspace, size_t workspace_bytes, void* stream);
/* Single stages of the run, with the run's kernels, on channel-interleaved uint8 images (for tests):
 *   resample : bilinear downsample of an (ih, iw, nc <= 16) image to (oh, ow): sample point (x, y) * iw / ow, taps
 *              clamped, truncated to a byte;
 *   stop_mask: 255 where some of the ns <= 8 style channels changed by >= stop_threshold, dilated by the patch.
 * workspace: fresco_ebsynth_stage_workspace_bytes(w, h, ow, oh) (w, h, w, h for the mask). */
size_t fresco_ebsynth_stage_workspace_bytes(int w, int h, int ow, int oh);
int fresco_ebsynth_resample(const uint8_t* in, int iw, int ih, int nc, uint8_t* out, int ow, int oh, void* workspace,
                            size_t workspace_bytes, void* stream);
int fresco_ebsynth_stop_mask(const uint8_t* style_new, const uint8_t* style_old, int w, int h, int ns,
                             int stop_threshold, int patch, uint8_t* mask, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * (h)  Video blending -- the per-frame step of video_blend.py process_seq that merges the forward and backward Ebsynth
 * propagations of an in-between frame (src/ebsynth/blender: histogram_blend.blend, poisson_fusion).  DESIGN.md
 * section 10.  Images are uint8 BGR (h, w, 3), masks uint8 (h, w) of 0 / 1, error maps fp32 (h, w), flow fp32
 * (2, h, w) with the x plane first.  Sides 2..4096 (FRESCO_EUNSUPPORTED otherwise, before any launch); every call runs
 * on `stream` with no host synchronisation, and same inputs give bit-identical outputs.
 *   fresco_blend_frame: mask = 0 where weight1 d1 < (1 - weight1) d2, else 1 (all 0 at weight1 == 0, all 1 at
 *     weight1 == 1), OR the previous mask warped by grid_sample(nearest, zeros, align_corners) at pixel + flow
 *     (prev_mask and flow both NULL or both set; out_mask must not be prev_mask); the min-error image, its histogram
 *     blend with weights (1 - weight1, weight1) and, with FRESCO_BLEND_GRADIENT, the Poisson fusion with the HOST
 *     array grad_weight[3] (L, a, b), solved exactly.  9 launches with gradient blending, 3 without.
 *   stage entry points (tests): Lab conversions of n_pixels; the histogram blend of a and b onto min_error's Lab
 *     statistics; the Poisson fusion of blend_bgr with the gradients of i1 / i2 (i2 where mask > 0).  out_lab (nullable)
 *     receives the Lab bytes that the final conversion to out_bgr reads.
 * workspace: fresco_blend_workspace_bytes(w, h) for every call but the Lab conversions (0 for unsupported sides).
 * ------------------------------------------------------------------------------------------ */
#define FRESCO_BLEND_GRADIENT 1
size_t fresco_blend_workspace_bytes(int w, int h);
int fresco_blend_frame(const uint8_t* oa, const uint8_t* ob, const float* d1, const float* d2, int w, int h,
                       double weight1, const uint8_t* prev_mask, const float* flow, int flags,
                       const float* grad_weight, uint8_t* out_mask, uint8_t* out_bgr, void* workspace,
                       size_t workspace_bytes, void* stream);
int fresco_bgr_to_lab_u8(const uint8_t* bgr, uint8_t* lab, int n_pixels, void* stream);
int fresco_lab_to_bgr_u8(const uint8_t* lab, uint8_t* bgr, int n_pixels, void* stream);
int fresco_histogram_blend(const uint8_t* a, const uint8_t* b, const uint8_t* min_error, int w, int h,
                           double weight1, double weight2, uint8_t* out_bgr, uint8_t* out_lab, void* workspace,
                           size_t workspace_bytes, void* stream);
int fresco_poisson_fusion(const uint8_t* blend_bgr, const uint8_t* i1, const uint8_t* i2, const uint8_t* mask, int w,
                          int h, const float* grad_weight, uint8_t* out_bgr, uint8_t* out_lab, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (i)  Ebsynth guides -- the guide images video_blend.py builds (src/ebsynth/blender/guide.py), batched over n uint8
 * images of (h, w, c), channel-interleaved, back to back.  DESIGN.md section 9.
 *   fresco_edge_guide  : cv2.filter2D(img, -1, [[0,-1,0],[-1,4,-1],[0,-1,0]]), BORDER_REFLECT_101, saturated.
 *   fresco_warp_nearest: flow_calc.warp(img, flow, 'nearest') -- grid_sample(nearest, zeros, align_corners=True) at
 *                        pixel + flow through flow_utils' fp32 normalise / unnormalise, ties to even; flow is n fp32
 *                        (2, h, w) planes, x first (what read_flow gives).
 * 2 <= w, h; 1 <= c <= 16; 1 <= n <= 65535 (FRESCO_EUNSUPPORTED / FRESCO_EINVAL otherwise, before the launch); out must
 * not be img.  One launch on `stream` each, no host synchronisation, exact (integer) results.
 * ------------------------------------------------------------------------------------------ */
int fresco_edge_guide(const uint8_t* img, uint8_t* out, int n, int w, int h, int c, void* stream);
int fresco_warp_nearest(const uint8_t* img, const float* flow, uint8_t* out, int n, int w, int h, int c, void* stream);

/* ------------------------------------------------------------------------------------------
 * (j)  FlowCalc glue -- what FRESCO's FlowCalc.get_flow (src/ebsynth/flow/flow_utils.py) runs around GMFlow, batched
 * over P frame pairs of n distinct frames.  DESIGN.md section 9.2.  Padding: InputPadder(mode='sintel',
 * padding_factor=8): H' = H + ph, ph = ((H / 8 + 1) * 8 - H) % 8, ph / 2 rows on top and ph - ph / 2 below; W' alike.
 *   fresco_flowcalc_input : frames (n, H, W, 3) uint8 (cv2.imread's BGR order, fed as is); first / second (P) int32
 *                           frame indices in [0, n) on the device.  out (2P, 3, H', W') fp32: first images, then second
 *                           images, replicate-padded and normalised as GMFlow.forward does it on the device,
 *                           (x * fp32(1 / 255) - mean) / std, not contracted -- bit-identical to torch.
 *   fresco_flowcalc_output: flows (2P, 2, H', W') fp32, GMFlow's bidirectional output (pair p's forward field at p, its
 *                           backward field at P + p).  Per pair: InputPadder.unpad, then forward_backward_consistency_check
 *                           on the unpadded fields (the arithmetic of fresco_flow_occlusion, same bits).  Writes bwd_flow
 *                           (P, 2, H, W) fp32 and bwd_occ (P, H, W) uint8 0 / 255; fwd_flow / fwd_occ (both or neither)
 *                           receive the forward field and fwd_occ -- what the swapped pair would write.
 * 2 <= H, W; 2P <= 65535 (input) / P <= 65535 (output).  One launch on `stream` each, no host synchronisation.
 * ------------------------------------------------------------------------------------------ */
int fresco_flowcalc_input(const uint8_t* frames, const int* first, const int* second, float* out, int n, int P, int H,
                          int W, void* stream);
int fresco_flowcalc_output(const float* flows, float* bwd_flow, uint8_t* bwd_occ, float* fwd_flow, uint8_t* fwd_occ,
                           int P, int H, int W, float alpha, float beta, void* stream);

/* ------------------------------------------------------------------------------------------
 * (k)  FreeU (src/free_lunch_utils.py:25-52, 127-147, 291-311) at the decoder's up-block sites.  DESIGN.md section 11.
 * dtype FRESCO_F16 / FRESCO_BF16 / FRESCO_F32 for every tensor of a call (fp32 arithmetic, one rounding to nearest even
 * at the store); tensors are dense NCHW; same inputs give bit-identical outputs (fixed reduction trees, no float atomics).
 *   fresco_freeu_fourier : Fourier_filter(x, threshold = 1, scale) in closed form -- the four scaled FFT bins are the
 *     frequencies {-1, 0}^2, so the filter is x plus (scale - 1) / (H W) times a seven-term combination of plane sums; no
 *     FFT, one read and one write of x for planes up to 64 x 64.  x (B, C, H, W); out[b] starts at out +
 *     b * out_batch_stride elements (>= C H W: the result can land in the tail of a concat buffer).  scale == 1.0f is a
 *     plain strided copy (the reference returns x up to its FFT noise).  2 <= H, W and H + W <= 8192.
 *   fresco_freeu_backbone: m = mean over C of hidden (B, C, H, W); per sample lo = min m, hi = max m;
 *     hidden[:, :n_scaled] *= (b - 1) * ((m - lo) / (hi - lo)) + 1 IN PLACE (the reference mutates its input, and callers
 *     that kept a handle on it see that); with cat != NULL, hidden after the update is also written to cat[:, :C],
 *     cat[b] at cat + b * cat_batch_stride elements.  b == 1 runs like any other value.  A constant mean map gives
 *     0 / 0 like the reference: the scaled channels become non-finite.  Three launches; workspace from
 *     fresco_freeu_workspace_bytes (0 for sizes the call would refuse), 16-byte aligned.
 * FRESCO_EUNSUPPORTED for H or W < 2 (or sizes beyond the limits above, B > 65535); FRESCO_EINVAL for null pointers,
 * non-positive sizes, an unknown dtype, n_scaled outside [0, C], a batch stride under C H W, cat == hidden, or pointers
 * not aligned to the element size; FRESCO_EWORKSPACE for a short workspace; all before any launch.  16-byte accesses are
 * used when the pointers, H W and the batch stride allow; anything else takes the element-wise form of the same kernels.
 * ------------------------------------------------------------------------------------------ */
size_t fresco_freeu_workspace_bytes(int B, int C, int H, int W);
int fresco_freeu_fourier(const void* x, void* out, int64_t out_batch_stride, int B, int C, int H, int W, float scale,
                         int dtype, void* stream);
int fresco_freeu_backbone(void* hidden, void* cat /* may be NULL */, int64_t cat_batch_stride, int B, int C, int n_scaled,
                          int H, int W, float b, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * (l)  The HED annotator of the ControlNet condition (src/ControlNet/annotator/hed/__init__.py).  DESIGN.md section 12.
 * The network's 3 x 3 convolutions are fresco_fn_gemm calls (bias + ReLU in the epilogue); these are the pieces around
 * them.  "Planes" are the (hi, lo) fp16 operands of fresco_fn_gemm: x * split_scale = hi + lo, saturating beyond +-65000;
 * a producer that had to saturate (or saw a NaN) ORs 1 into *range_flag (may be NULL).  Same inputs give bit-identical
 * outputs (no float atomics).
 *   fresco_hed_input    : frames (n, H, W, 3) uint8 RGB, norm[3] fp32 ON THE DEVICE -> the planes of (x - norm) as NHWC rows
 *     of 32 channels, channels 3..31 zero: (n H W, 32) each.  The first convolution reads them as a 3 x 3 convolution with
 *     cin = 32 (K = 288, weights zero-padded); its zero padding is applied to x - norm, as in the reference.
 *   fresco_hed_side_pool: h (n, H, W, C) fp32 NHWC, the last (post-ReLU) activation of a block, C in {64, 128, 256, 512},
 *     read once.  proj (n, H, W) fp32 = sum_c h[..][c] w[c] + bias[0]  (w: C floats, bias: 1 float or NULL; fused
 *     multiply-adds in a fixed order).  pool_hi / pool_lo: the planes of max_pool2d(h, 2, 2) as (n, H / 2, W / 2, C) rows,
 *     floor semantics (an odd last row / column is dropped).  Either proj or the plane pair may be NULL, not both.
 *   fresco_hed_fuse     : side maps s1 .. s5, level k of shape (n, H >> (k - 1), W >> (k - 1)) fp32 -> for every level
 *     cv2.resize(INTER_LINEAR) to (H, W) [source position ((d + 0.5) (src / dst) - 0.5), the scale in double, positions
 *     clamped to the first / last sample, horizontal pass then vertical, fp32, identity at level 1], the mean in fp32
 *     (adds in level order, / 5), 1 / (1 + exp(-mean)) in double, * 255, clip, truncation: out (n, H, W) uint8.
 *     logit (n, H, W) fp32 (optional): the mean.  cond (n, 3, H, W) of cond_dtype (optional): ((u / 255) 2 - 1) 0.5 + 0.5
 *     in fp32, rounded once, the same in the three channels -- the ControlNet condition run_fresco.py:199-200 builds.
 * FRESCO_EUNSUPPORTED: C outside the list, H or W < 16 (fuse; < 2 for a pooled output), n H W >= 2^31.  FRESCO_EINVAL: null
 * pointers, non-positive sizes or scale, an unknown cond_dtype, h / w / the planes not 16-byte aligned (they are read and
 * written in 16-byte pieces).  All before any launch.
 * ------------------------------------------------------------------------------------------ */
int fresco_hed_input(const uint8_t* frames, const float* norm, void* out_hi, void* out_lo, int n, int H, int W,
                     float split_scale, int32_t* range_flag, void* stream);
int fresco_hed_side_pool(const float* h, const float* w, const float* bias /* may be NULL */, float* proj /* may be NULL */,
                         void* pool_hi /* may be NULL */, void* pool_lo, int n, int H, int W, int C, float split_scale,
                         int32_t* range_flag, void* stream);
int fresco_hed_fuse(const float* s1, const float* s2, const float* s3, const float* s4, const float* s5, uint8_t* out,
                    float* logit /* may be NULL */, void* cond /* may be NULL */, int cond_dtype, int n, int H, int W,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * (m)  The EGNet saliency detector behind the background smoothing (src/EGNet/model.py, resnet.py; called by
 * src/utils.py::get_saliency).  DESIGN.md section 13.  The network's convolutions are fresco_fn_gemm / fresco_fn_conv7_rgb
 * calls (BatchNorm folded into weights and bias); these are the pieces around them.  Planes and range_flag as in section (l).
 * Same inputs give bit-identical outputs (no float atomics).
 *   fresco_egnet_input     : frames (n, H, W, 3) uint8 -> cv2sod's tensor as NHWC fp32 rows (n, H / 2, W / 2, 3): channel c
 *     minus (104.00699, 116.66877, 122.67892)[c], then the mean of each 2 x 2 block = F.interpolate(scale_factor=0.5,
 *     bilinear); the block sum is exact and (sum / 4 - mean) is rounded to fp32 once; an odd last row / column is dropped.
 *   fresco_egnet_pool      : MaxPool2d(3, stride 2, padding 1, ceil_mode=True) on x (n, H, W, 64) fp32 NHWC -> the planes
 *     of the pooled map, (n, OH, OW, 64), and its fp32 values where `out` is given; OH follows PyTorch's rule (ceil, minus
 *     one where the last window would start beyond the input and its left padding).
 *   fresco_egnet_resize_add: F.interpolate(x, (H, W), bilinear, align_corners=True) on x (n, h, w, C) fp32 NHWC [+ addend
 *     (n, H, W, C)] [ReLU] -> out fp32 and / or the planes, C % 32 == 0, C <= 512.  The source position d (h - 1) / (H - 1)
 *     is a quotient and a remainder of integers (exact taps, the weight rounded once); h == H and w == W copies x exactly.
 *   fresco_egnet_saliency  : logit (n, h, w) fp32 -> align_corners=True resize to (Hs, Ws), 1 / (1 + expf(-x)), k x k box
 *     sum with replicate padding (added in row order), clamp to [0, 1], 1 - x: out (n, 1, Hs, Ws) fp32; logit_out
 *     (n, Hs, Ws) (optional): the resized logit.  k odd, <= 15.
 * FRESCO_EUNSUPPORTED: C outside the above, H or W < 2 (input), k even or > 15, n H W >= 2^31, a resized side > 32768.  FRESCO_EINVAL: null pointers,
 * non-positive sizes or scale, fp32 rows read in 16-byte pieces not 16-byte aligned, planes not 8-byte aligned.  All before
 * any launch.
 * ------------------------------------------------------------------------------------------ */
int fresco_egnet_input(const uint8_t* frames, float* out, int n, int H, int W, void* stream);
int fresco_egnet_pool(const float* x, float* out /* may be NULL */, void* out_hi, void* out_lo, int n, int H, int W, int C,
                      float split_scale, int32_t* range_flag, void* stream);
int fresco_egnet_resize_add(const float* x, const float* addend /* may be NULL */, float* out /* may be NULL */,
                            void* out_hi /* may be NULL */, void* out_lo, int n, int h, int w, int H, int W, int C, int relu,
                            float split_scale, int32_t* range_flag, void* stream);
int fresco_egnet_saliency(const float* logit, float* out, float* logit_out /* may be NULL */, int n, int h, int w, int Hs,
                          int Ws, int k, void* stream);

/* ------------------------------------------------------------------------------------------
 * (n)  The Canny annotator of the ControlNet condition (`controlnet_type: canny`): OpenCV's generic
 * Canny(src, low, high, apertureSize = 3, L2gradient = false) on 8-bit 3-channel frames, batched
 * (reference: src/ControlNet/annotator/canny/__init__.py; DESIGN.md section 14 has the rules).  All integer: same inputs give
 * the same bits.
 *   fresco_canny_workspace_bytes: what fresco_canny_hysteresis needs for (n, H, W); 0 for sizes the calls refuse.
 *   fresco_canny_classify  : frames (n, H, W, 3) uint8 -> cls (n, H, W) uint8: 0 (no edge), 1 (weak: a local maximum of
 *     the gradient magnitude above `low`), 2 (strong: above `high` as well).  3 x 3 Sobel per channel with replicated
 *     borders, |dx| + |dy|, the channel of the largest magnitude (the first on ties), zero magnitude outside the frame,
 *     non-maximum suppression along the quantised gradient direction.  low > high: the two are swapped.  One launch.
 *   fresco_canny_hysteresis: cls -> out (n, H, W) uint8: 255 on every class 1 / 2 pixel whose 8-connected component of
 *     class 1 / 2 pixels holds a class 2 pixel, else 0 (a class byte >= 3 counts as 0; frames are independent).  cond,
 *     when given: the ControlNet condition (n, 3, H, W) of cond_dtype (FRESCO_F16 / FRESCO_BF16 / FRESCO_F32),
 *     ((out / 255) * 2 - 1) * 0.5 + 0.5 in fp32 in that order, rounded once -- what fresco_hed_fuse writes.  Union-find
 *     labelling in four launches whatever the picture; no host loop, no read-back, no synchronisation.
 * FRESCO_EINVAL: null frames / cls / out / workspace, non-positive n / H / W, a workspace not 4-byte aligned or a cond not
 * aligned to its element, an unknown cond_dtype with a non-null cond.  FRESCO_EUNSUPPORTED: n H W >= 2^31.
 * FRESCO_EWORKSPACE: a short workspace.  All before any launch.
 * ------------------------------------------------------------------------------------------ */
size_t fresco_canny_workspace_bytes(int n, int H, int W);
int fresco_canny_classify(const uint8_t* frames, uint8_t* cls, int n, int H, int W, int low, int high, void* stream);
int fresco_canny_hysteresis(const uint8_t* cls, uint8_t* out, void* cond /* may be NULL */, int cond_dtype, void* workspace,
                            size_t workspace_bytes, int n, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRESCO_HIP_H */
