/*
 * gencomm_hip.h -- C ABI of libgencomm_hip.so: the MI355X (gfx950) implementation of GenComm's
 * generative-communication hot path.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every tensor pointer is DEVICE memory, float32, contiguous, NCHW unless stated;
 *   - the caller owns every buffer, including the scratch workspace (query *_workspace_bytes);
 *     the library allocates nothing and is re-entrant per stream; its only process-global state is
 *     the mode table (gencomm_set_mode) and the two diagnostics (kernel timer, kernel log), see below;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); all work is
 *     enqueued on it and nothing synchronises the host, so calls may be captured in a hipGraph;
 *   - every entry point returns 0 on success, non-zero on error (1 bad argument / unsupported
 *     configuration, 2 workspace too small, 3 HIP runtime error) and never exits the process
 *     (contrast the reference's CHECK_* macros, opencood/pcdet_utils/iou3d_nms/src/iou3d_nms.cpp:14-25);
 *     gencomm_last_error() returns a thread-local description of the last failure.
 *
 * What each entry point replaces in the reference (paths relative to the reference checkout):
 *   gencomm_unet_prepare      DiffusionUNet parameter reads + get_timestep_embedding + temb MLP
 *                             (opencood/models/gencomm_modules/unet.py:10-28, :222-228, :309-312)
 *                             and every ResnetBlock.temb_proj (unet.py:124), for all T steps at once
 *   gencomm_unet_fwd          DiffusionUNet.forward (unet.py:307-344) = GenComm.gen_pred
 *                             (opencood/models/gencomm_modules/cond_diff.py:317-319)
 *   gencomm_q_sample_fwd      GenComm.q_sample (cond_diff.py:262-264)
 *   gencomm_denoise_fwd       GenComm.forward eval+train maths: ego repeat (cond_diff.py:332-337),
 *                             q_sample (:262-264, :372), p_sample_loop / p_sample / p_mean_variance /
 *                             q_posterior (:321-329, :302-315, :281-299, :272-279)
 *   gencomm_enhancer_fwd      Enhancer.forward -> Enhancer_block -> FRFN -> SplitAttn
 *                             (opencood/models/gencomm_modules/enhancer.py:367-383, :346-357, :222-250, :315-333)
 *   gencomm_msgext_fwd        MessageExtractorv2.forward (message_extractor_v2.py:103-118; DeformConv2d = torchvision DCNv1)
 *   gencomm_pillar_encode_fwd PointPillar encoder front half: PillarVFE + PointPillarScatter (heter_encoders.py:22-50)
 *   gencomm_warp_attfuse_fwd  AttFusion.forward + warp_affine_simple + ScaledDotProductAttention
 *                             (opencood/models/fuse_modules/fusion_in_one.py:131-151, :41-45;
 *                              opencood/models/sub_modules/torch_transformation_utils.py:323-332)
 *
 * Supported UNet family: ch = 8, ch_mult = all ones (levels <= 4), 1 <= num_res_blocks <= 4,
 * resamp_with_conv = true, dropout = 0, C % 8 == 0 -- a superset of every shipped GenComm yaml
 * (60/60 use ch 8, ch_mult [1,1], 2 res-blocks, attn_resolutions [16] = no AttnBlock).
 * `attn_mask`: bit l set = the AttnBlocks of level l exist (nominal resolution 128 >> l is in
 * attn_resolutions, unet.py:237,:252-253,:286-287); they run as flash-style streaming attention.
 */
#ifndef GENCOMM_HIP_H
#define GENCOMM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define GENCOMM_ABI_VERSION 12

int gencomm_abi_version(void);
const char* gencomm_last_error(void);
/* The code-generation flags the library was compiled with (set by the build: -DGENCOMM_BUILD_FLAGS). The kernels must be
 * built WITHOUT packed fp32 instructions (-Xclang -target-feature -Xclang -packed-fp32-ops): a v_pk_fma_f32 in
 * conv8h_kernel's epilogue returned wrong values under multi-workgroup occupancy; the Python binding
 * refuses a library whose build info lacks that switch and tests/test_abi.py disassembles the code object to check. */
const char* gencomm_build_info(void);

/* Library modes.  Explicit, atomic process-wide settings that every entry point reads ONCE when it is called (they
 * travel with the call from there on); the library reads no environment variable.  gencomm_set_mode returns 0 or 1
 * (unknown key / value out of range); gencomm_get_mode returns the value, -1 for an unknown key.
 *   GENCOMM_MODE_ARITH        0 (default): the hot path's 3x3 / 5x5 / Linear products on the f16 matrix pipe from exact THREE-term
 *                             splits of both fp32 operands (fp16 + fp16 + a bf8 third term: products to 2^-26, fp32 accumulation --
 *                             not narrower than an fp32 FMA); the general convolutions around the path (gencomm_conv2d_fwd, the
 *                             sparse convolutions) on exact-fp32 MFMA kernels; 1: exact-fp32 instruction kernels everywhere;
 *                             3: as 0, plus the general convolutions on the two-term fp16 split of round 2 (22-bit products: faster,
 *                             narrower than fp32 -- opt-in);
 *                             2: bf16 denoise mode (the reference's --half / autocast analogue, train_ddp.py:139-141): the
 *                             UNet's 8-channel intermediates are stored as bf16 and multiplied by single bf16 MFMAs
 *                             (fp32 accumulation, GroupNorm statistics in f64, the sampler's carried state in fp32);
 *                             inference only, no AttnBlock, W divisible by 4 at every level
 *   GENCOMM_MODE_SAMPLER      2: the loop is carried on conv_in's 8-channel output (one fused kernel per step replaces
 *                             conv_out + update + conv_in); 1: literal per-step structure of cond_diff.py:321-329 (tests
 *                             compare the two); 0 (default): automatic -- 2 on maps large enough for the 64x16-tile
 *                             kernels (x_t stays out of HBM), 1 on small, cache-resident maps (shorter dependent chain)
 *   GENCOMM_MODE_TILE_WANT    0 (default): automatic tile choice; > 0: minimum number of 64x16 workgroups before the
 *                             64x16-tile kernels are used (1 forces them onto small maps: tests)
 *   GENCOMM_MODE_ENH_FUSE     Enhancer at C = 64 -- 2 (default): Linear1 + depthwise stage + Linear2 in one kernel;
 *                             1: Linear1 + depthwise stage fused; 0: separate launches
 *   GENCOMM_MODE_CONV8H_MASK  diagnostic bit mask of 8-channel layer variants allowed on the f16 pipe (-1: all)
 *   GENCOMM_MODE_XCD_REMAP    1 (default): workgroup -> tile mapping keeps neighbouring tiles on one XCD; 0: grid order
 *   GENCOMM_MODE_DATAFLOW     1: the body of a UNet call (every layer between conv_in and conv_out) runs as ONE persistent launch
 *                             whose workgroups take (layer, agent, tile) items from per-XCD queues and wait on per-(layer, agent)
 *                             completion counters (no grid barrier); 0 (default): one launch per layer.  Same device functions, same results
 *                             -- EXCEPT when a dependency wait exhausts its bounded spin (a busy or shared GPU): the remaining tiles are
 *                             then skipped so that the grid drains, the entry point still returns GC_OK, and the activations are
 *                             invalid.  A caller that turns this mode on MUST poll gencomm_dataflow_error() after the call.  The mode
 *                             is opt-in, measured 2x slower than the per-layer launches, and kept for that measurement only
 *   GENCOMM_MODE_TILE8        0: 64x16-pixel tiles in every 8-channel layer of the f16 pipe; n > 0: launches with fewer than n
 *                             such workgroups run 64x8 tiles (half the dependent chain per workgroup, 28.8 KB of LDS: the half-resolution
 *                             level of large maps).  Same arithmetic; results identical up to the summation order of the statistics.
 *                             -1 (default): automatic = 256 (a third of a resident round: the half-resolution launches of ONE four-agent
 *                             scene; single-scene latency 10.07 -> 9.78 ms, batched throughput unchanged), off while GENCOMM_MODE_TILE_WANT
 *                             forces a tile size
 *   GENCOMM_MODE_BWD_STREAMS  1 (default): on calls of at least 2^17 pixels (n H W) gencomm_unet_bwd forks its weight-gradient launches onto a
 *                             library-owned side stream of the device (hipEventRecord on the caller's stream / hipStreamWaitEvent) and joins
 *                             them back before its last launches, so they overlap the input-gradient chain (15.2 -> 13.7 ms per training step
 *                             at 4 x 64 x 200 x 704); every buffer is still ordered on the caller's stream when the call returns.  2: on every
 *                             call (costs host time on small maps).  0: every launch on the caller's stream
 *   GENCOMM_MODE_PERSIST      bit mask of the 8-channel f16-pipe layer variants (1 conv1 8 -> 8, 2 conv1 16 -> 8, 4 conv2 + identity residual,
 *                             8 conv2 + 1x1 shortcut, 16 Upsample) that run as a PERSISTENT kernel when a launch has more 64x16 tiles than the device
 *                             has resident slots (3 per CU): every workgroup walks several tiles and requests the next tile's loads one tile
 *                             ahead, so that a slot does not sit through the first-load wait and the store drain of every tile.  Same tile
 *                             function, same arithmetic; results identical up to the summation order of the statistics.  Default 16: measured per
 *                             variant on MI355X only the Upsample convolution gains (38.7 -> 35.0 us per launch); the GroupNorm'd variants
 *                             lose 0 .. 13 % (registers carried across the tile: up to 96 B of scratch)
 *   GENCOMM_MODE_RESFUSE_EMU  0 (default).  1: TIMING EXPERIMENT ONLY -- the 8 -> 8 ResnetBlocks run the launch pattern a fused
 *                             conv1 + conv2 block would have (statistics-only conv1 pass; conv2 pass reading the block input with twice
 *                             the matrix work), an upper bound of that fusion's gain; the outputs are NOT the UNet's */
enum {
  GENCOMM_MODE_ARITH = 0, GENCOMM_MODE_SAMPLER = 1, GENCOMM_MODE_TILE_WANT = 2, GENCOMM_MODE_ENH_FUSE = 3,
  GENCOMM_MODE_CONV8H_MASK = 4, GENCOMM_MODE_XCD_REMAP = 5, GENCOMM_MODE_DATAFLOW = 6, GENCOMM_MODE_RESFUSE_EMU = 7,
  GENCOMM_MODE_TILE8 = 8, GENCOMM_MODE_BWD_STREAMS = 9, GENCOMM_MODE_PERSIST = 10
};
int gencomm_set_mode(int key, long long value);
long long gencomm_get_mode(int key);

/* Diagnostic kernel timer: gencomm_timer_start(family, capacity) arms it for ONE kernel family, gencomm_timer_start_mask
 * for a set (bit f = family f; 0 <= f < gencomm_timer_num_kernels(), name via gencomm_timer_kernel_name); until it is
 * stopped every launch of an armed family (up to `capacity` launches) is bracketed by a pair of HIP events on the stream
 * it is launched on, and its ALGORITHMIC byte count (the tensor bytes the layer has to read and write, computed by the
 * host from the launch shape) is recorded with it. gencomm_timer_stop synchronises those events and returns the summed
 * device time and the number of launches; gencomm_timer_stop_families returns them per family (arrays of n_families
 * entries, any may be NULL) together with the summed algorithmic bytes. Process-global diagnostic state (with the modes
 * above the only one); do not arm it while capturing a graph. */
int gencomm_timer_num_kernels(void);
const char* gencomm_timer_kernel_name(int family);
int gencomm_timer_start(int family, int capacity);
int gencomm_timer_start_mask(unsigned long long family_mask, int capacity);
int gencomm_timer_stop(double* total_ms, int* launches);
int gencomm_timer_stop_families(double* ms, int* launches, double* algorithmic_bytes, int n_families);

/* Diagnostic kernel log: between gencomm_klog_start and gencomm_klog_stop every launch site of the hot path notes the exact
 * kernel instantiation it chose; gencomm_klog_stop writes "name<TAB>count<NEWLINE>" lines into buf (status 1 when cap is
 * too small).  bench.py prints it so that the timed instantiations (in-kernel Philox noise: latent_step_h_kernel<2>,
 * conv_out_h_kernel<2>) are named next to the number.  Process-global diagnostic state like the timer. */
int gencomm_klog_start(void);
int gencomm_klog_stop(char* buf, int cap);

/* Diagnostic: the shader clock the device actually runs at while other work is in flight.  One wave spins for about `spin_us`
 * microseconds of the constant 100 MHz counter (s_memrealtime) and writes {shader-clock ticks (s_memtime), 100 MHz ticks} to
 * out_dev[2] (unsigned long long, device memory): MHz = 100 * ticks[0] / ticks[1].  Launch it on a stream of its own beside the
 * workload (tools/diag/clock_under_load.py). */
int gencomm_clock_probe(unsigned long long* out_dev, int spin_us, void* stream);

/* Diagnostic: out[i][j] (double, [n_a][n_b], j fastest) = the convex-quadrilateral IoU that gencomm_nms_rotated_fwd compares with
 * its threshold (before its rounding to float), of the BEV quadrilaterals (x, y of the first four corners) of corners_a[i] and
 * corners_b[j]; corners_* are [n][8][3] float32 as the NMS takes them, either orientation. The same device function as the NMS
 * (csrc/detect_kernels.h quad_iou_d), one thread per pair. n_a == 0 or n_b == 0 is a no-op. */
int gencomm_quad_iou_fwd(const float* corners_a, int n_a, const float* corners_b, int n_b, double* out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * UNet parameters.  The "raw" blob is the concatenation of the module's parameters in EXECUTION
 * order; enumerate it with gencomm_unet_param_info (name = the reference's state_dict key under
 * `denoiser.`, e.g. "down.0.block.1.conv2.weight"; tensors keep the reference layout: conv OIHW,
 * linear [out,in]).  gencomm_unet_prepare turns it into the kernels' layout ([ic][tap][oc] conv
 * weights) and evaluates the timestep path for t = 0..T-1 into a bias table; call it once per
 * weight update.
 * -------------------------------------------------------------------------------------------- */
int gencomm_unet_num_params(int C, int levels, int res_blocks, int attn_mask);
int gencomm_unet_param_info(int C, int levels, int res_blocks, int attn_mask, int index,
                            char* name, int name_cap, long long* numel, long long* offset);
long long gencomm_unet_raw_floats(int C, int levels, int res_blocks, int attn_mask);
long long gencomm_unet_prepared_floats(int C, int levels, int res_blocks, int attn_mask, int T);
int gencomm_unet_prepare(const float* raw, float* prepared, int C, int levels, int res_blocks, int attn_mask, int T,
                         void* stream);

/* One DiffusionUNet call BACKWARDS (the training branch back-propagates through every call: cond_diff.py:342-360; what
 * torch autograd does for unet.py:307-344 in the reference). Re-runs the forward with every intermediate kept, then:
 * grad_xt [n][C][H][W] and grad_cond [n][2][H][W] are OVERWRITTEN with the gradients w.r.t. the two inputs; grad_raw
 * (gencomm_unet_raw_floats floats, the raw blob's layout) must be ZERO on entry and holds the gradient of EVERY parameter
 * on return: conv / norm / nin parameters, and the timestep path (temb.dense.{0,1}, every <block>.temb_proj), which enters
 * the forward only through each ResnetBlock's conv1 bias and is chained from this call's d conv1.bias by one small kernel.
 * `raw` = the parameter blob in the reference's layouts (what gencomm_unet_prepare consumed). attn_mask must be 0. */
long long gencomm_unet_bwd_workspace_bytes(int n, int C, int H, int W, int levels, int res_blocks, int attn_mask);
/* Forward of a call that will be differentiated: as gencomm_unet_fwd, but every intermediate (and its GroupNorm statistics)
 * stays in `workspace` (gencomm_unet_bwd_workspace_bytes; one workspace per call in flight -- MI355X has the HBM for it),
 * to be handed to gencomm_unet_bwd with forward_done = 1. With forward_done = 0 gencomm_unet_bwd re-runs that forward itself. */
int gencomm_unet_fwd_train(const float* prepared, const float* x_t, const float* cond, float* x0_out, int t,
                           int n, int C, int H, int W, int levels, int res_blocks, int attn_mask, int T,
                           void* workspace, long long workspace_bytes, void* stream);
/* ABI v8: gencomm_unet_fwd_train with the sampler's update of step t >= 1 fused into conv_out's epilogue, as the inference loop runs it
 * (cond_diff.py:272-279, :302-315): x_prev = coef1_t x0_hat + coef2_t x_t + sigma_t eps; sched_row = the five schedule constants of
 * timestep t on the device (row t of the table gencomm_denoise_fwd takes); eps = step_noise [n][C][H][W] when given, else the sampler's
 * in-kernel Philox field of (seed, t) -- the field gencomm_denoise_fwd adds. x0_hat is not stored, x_t is only read (x_prev != x_t). */
int gencomm_unet_fwd_train_step(const float* prepared, const float* x_t, const float* cond, float* x_prev, int t, const float* sched_row,
                                const float* step_noise, unsigned long long seed, int n, int C, int H, int W, int levels, int res_blocks,
                                int attn_mask, int T, void* workspace, long long workspace_bytes, void* stream);
int gencomm_unet_bwd(const float* prepared, const float* raw, const float* x_t, const float* cond, int t, const float* grad_x0,
                     float* grad_xt, float* grad_cond, float* grad_raw, int n, int C, int H, int W, int levels, int res_blocks,
                     int attn_mask, int T, int forward_done, void* workspace, long long workspace_bytes, void* stream);

/* ABI v8: gencomm_unet_bwd for a call inside the sampler chain (cond_diff.py:272-315 differentiated): grad_x0 = d_prev = d x_{t-1} as it
 * stands (NOT multiplied by coef1_t), and grad_xt = alpha * (the call's gradient with respect to x_t) + beta * d_prev is formed in the epilogue
 * of conv_in's input-gradient layer (alpha = coef1_t, beta = coef2_t) -- the two elementwise passes around the call disappear. grad_cond and
 * grad_raw are the gradients for grad_x0 as given: multiply them by alpha when accumulating (the call is linear in grad_x0). d_prev may be
 * NULL (then alpha / beta are ignored: gencomm_unet_bwd); grad_xt must not alias d_prev. */
int gencomm_unet_bwd_chain(const float* prepared, const float* raw, const float* x_t, const float* cond, int t, const float* grad_x0,
                           float alpha, float beta, const float* d_prev, float* grad_xt, float* grad_cond, float* grad_raw, int n, int C,
                           int H, int W, int levels, int res_blocks, int attn_mask, int T, int forward_done, void* workspace,
                           long long workspace_bytes, void* stream);

/* One 8 -> 8 channel 3x3 convolution (pad 1, bias) as the UNet's ResnetBlock / Upsample layers run it
 * (unet.py:52, :99-118), without norm or residual: dst[n,8,H,W] = conv(src[n,8,H,W], w[8,8,3,3]) + bias; dstat (nullable)
 * receives per-(sample, channel) {sum, sum of squares} of dst as [n][8][2] doubles. split = 1: the f16-pipe kernel with
 * exact three-term operand splits on 64x16 tiles (conv8h_kernels.h); 0: the exact-fp32 kernel; 0x100 | mask: diagnostic
 * instantiation that issues only the selected terms of the six-instruction product (bit 0 hi w1, 1 lo w1, 2 hi w2, 3 lo w2,
 * 4 hi w3, 5 t wb), so that each operand plane / table is tested alone. scratch >= 4096 floats. Unit-test entry. */
int gencomm_conv8_fwd(const float* src, const float* w_oihw, const float* bias, float* dst, double* dstat,
                      float* scratch, int n, int H, int W, int split, void* stream);

/* ABI v8: 3x3 stride-1 pad-1 convolution 16 -> 16 channels without bias -- FRFN.partial_conv3 at C = 64 (enhancer.py:218, :229-232: the
 * first C / 4 channels of the LayerNorm output) and, transposed = 1, its input gradient (w is the forward weight [16][16][3][3] in both
 * cases) -- on the UNet's exact-fp32 8-channel kernel: x / y are the first 16 channels of [n][x_ct][H][W] / [n][y_ct][H][W] tensors (so
 * the layer reads its slice of the LayerNorm output and writes its slice of Linear1's input without copies); x != y; scratch of
 * gencomm_conv3x3_c16_scratch_floats() floats. The general convolution took 160-250 us for this layer at 4 x 200 x 704 (72 MB of traffic). */
long long gencomm_conv3x3_c16_scratch_floats(void);
int gencomm_conv3x3_c16_fwd(const float* x, int x_ct, const float* w, int transposed, float* y, int y_ct, float* scratch, int n, int H, int W,
                            void* stream);

/* Scratch for one UNet call / the denoise loop on n agents of [C, H, W]. */
long long gencomm_denoise_workspace_bytes(int n, int C, int H, int W, int levels, int res_blocks, int attn_mask);

/* Diagnostic for GENCOMM_MODE_DATAFLOW: the persistent kernel's error word of the last UNet call on this workspace -- 0: every
 * dependency wait was satisfied; k + 1: a workgroup gave up (bounded spin) waiting for the predecessor of body op k, the call's
 * result is then invalid; -1: bad arguments.  Synchronises `stream`. */
int gencomm_dataflow_error(const void* workspace, int n, int C, int H, int W, int levels, int res_blocks, int attn_mask, void* stream);
/* Diagnostic: the kernel's counter block of the last call ([8] tickets taken per XCD queue, [64][n] finished tiles per body op and
 * agent, the error word) copied to host_out[count]. Synchronises `stream`. */
int gencomm_dataflow_words(const void* workspace, int n, int C, int H, int W, int levels, int res_blocks, int attn_mask,
                           unsigned int* host_out, int count, void* stream);

/* x0_hat[n,C,H,W] = UNet(cat[cond[n,2,H,W], x_t[n,C,H,W]], t) for one integer timestep t. */
int gencomm_unet_fwd(const float* prepared, const float* x_t, const float* cond, float* x0_out, int t,
                     int n, int C, int H, int W, int levels, int res_blocks, int attn_mask, int T,
                     void* workspace, long long workspace_bytes, void* stream);

/* The whole sampler.  sched = device float[T][5] rows {sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod,
 * posterior_mean_coef1, posterior_mean_coef2, exp(0.5*posterior_log_variance_clipped)}.
 * x_start of agent i = feat[src_row[i]] (src_row: device int32[n]; the ego row of i's scene).
 * noise0 [n,C,H,W] and step_noise [T,n,C,H,W] (loop order t = T-1..0; entry T-1 unused) are either
 * both given (explicit noise: parity tests) or both NULL (in-kernel Philox4x32-7 + Box-Muller keyed by `seed`; the step noise is sigma_t z rounded to fp16).
 * out [n,C,H,W] receives pred_feature; it is also the in-place x_t buffer of the loop. */
int gencomm_denoise_fwd(const float* prepared, const float* sched,
                        const float* feat, int n_feat_rows, const int* src_row, const float* cond,
                        float* out, const float* noise0, const float* step_noise, unsigned long long seed,
                        int n, int C, int H, int W, int levels, int res_blocks, int attn_mask, int T,
                        void* workspace, long long workspace_bytes, void* stream);

/* gencomm_denoise_fwd with the Philox key optionally read from DEVICE memory at kernel run time (seed_dev != NULL
 * overrides `seed`): a captured hipGraph of the call can be replayed with fresh noise by rewriting one 8-byte word. */
int gencomm_denoise_fwd_dseed(const float* prepared, const float* sched,
                              const float* feat, int n_feat_rows, const int* src_row, const float* cond,
                              float* out, const float* noise0, const float* step_noise, unsigned long long seed,
                              const unsigned long long* seed_dev,
                              int n, int C, int H, int W, int levels, int res_blocks, int attn_mask, int T,
                              void* workspace, long long workspace_bytes, void* stream);

/* q_sample alone (cond_diff.py:262-264 with the ego repeat of :332-337 folded in):
 *   out[i] = sched_row[0] * feat[src_row[i]] + sched_row[1] * eps[i]
 * sched_row: device float[5] (one row of the table above).  noise NULL = Philox stream `stream_id`
 * of `seed` (gencomm_denoise_fwd uses stream_id = T for this draw and t for the step draws). */
int gencomm_q_sample_fwd(const float* sched_row, const float* feat, int n_feat_rows, const int* src_row,
                         const float* noise, unsigned long long seed, unsigned int stream_id,
                         float* out, int n, int C, int H, int W, void* stream);

/* The sampler's in-kernel step noise of (seed, timestep stream_id = t), written out: out[n,C,H,W] = nu_t = fp16(sigma_t z)
 * as float32 -- the exact values gencomm_denoise_fwd adds at step t when noise0 / step_noise are NULL (same device
 * functions, same counter layout, in both sampler structures and every tile size); sched_row = device float[5] row of t
 * ([4] = sigma_t).  unrounded != 0 writes sigma_t z before the fp16 rounding instead (statistics tests).  The reference
 * draws torch.randn per step (cond_diff.py:307, MDD_utils.py:232-235); this entry exists so that a run with in-kernel
 * noise can be replayed through the oracle with explicit noise (step_noise[T-1-t] = nu_t / sigma_t).  q_sample's
 * initial noise is read back with gencomm_q_sample_fwd (zero feat, sched_row {0, 1, ..}, stream_id = T). */
int gencomm_step_noise_fwd(const float* sched_row, unsigned long long seed, unsigned int stream_id, float* out,
                           int n, int C, int H, int W, int unrounded, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Enhancer (live parameters only: block_1.{norm1,norm2,mlp.*}, split_attn.*), raw blob enumerated
 * like the UNet's; names are the reference's state_dict keys under `enhancer.`.
 * -------------------------------------------------------------------------------------------- */
int gencomm_enhancer_num_params(int C);
int gencomm_enhancer_param_info(int C, int index, char* name, int name_cap, long long* numel, long long* offset);
long long gencomm_enhancer_raw_floats(int C);
long long gencomm_enhancer_workspace_bytes(int n, int C, int H, int W);
/* out[n,C,H,W] = split_attn(block_1(x[n,C,H,W])) per agent (agents are independent). */
int gencomm_enhancer_fwd(const float* raw, const float* x, float* out, int n, int C, int H, int W,
                         void* workspace, long long workspace_bytes, void* stream);
/* Diagnostic entries for the kernel tests (additive to ABI v12).
 * gencomm_enhancer_workspace_layout: byte offsets of the token-major intermediates inside the workspace, in the order
 *   {Y = x + LN1(x) [n][HW][C], Z = LN2(Y), partial convolution applied in place [n][HW][C], Zc = Z[..., :C/4] before it [n][HW][C/4],
 *    Hd = GELU(Linear1) [n][HW][4C], G = GELU(dw(x1)) x2 [n][HW][2C], O = Linear2 + Y [n][HW][C], colsum [n][C], gate [n][C]}.
 *   O shares its storage with the front of Hd.
 * gencomm_enhancer_fwd_stages: the launches of stages first_stage .. last_stage (inclusive) of gencomm_enhancer_fwd alone, on whatever
 *   the workspace holds: 1 LayerNorms, 2 partial convolution, 3 Linear1 + GELU, 4 depthwise + gate, 5 Linear2 + residual + pool sums
 *   (clears colsum first), 6 channel gate, 7 scale + transpose. x may be NULL when stage 1 is not run, out when stage 7 is not. A range
 *   that cuts through a fused launch (3-4 under GENCOMM_MODE_ENH_FUSE 1, 3-5 under 2, both at C = 64 only) is GC_ERR_ARG. */
int gencomm_enhancer_workspace_layout(int n, int C, int H, int W, long long* byte_offsets);
int gencomm_enhancer_fwd_stages(const float* raw, const float* x, float* out, int n, int C, int H, int W,
                                void* workspace, long long workspace_bytes, int first_stage, int last_stage, void* stream);

/* ----------------------------------------------------------------------------------------------
 * MessageExtractorv2 (opencood/models/gencomm_modules/message_extractor_v2.py:70-120): the producer
 * of `conditions`. out[n,2,H,W] = fuse(dcn(x, offset_conv(x)) * se_gate). x [n,C,H,W], C % 8 == 0.
 * Raw blob enumerated like the UNet's; names = state_dict keys under `message_extractor_m<k>.`
 * (`bev_extractor.{offset1,dcn1,fuse.0,fuse.2,attn.1,attn.3}.{weight,bias}`).
 * -------------------------------------------------------------------------------------------- */
int gencomm_msgext_num_params(int C);
int gencomm_msgext_param_info(int C, int index, char* name, int name_cap, long long* numel, long long* offset);
long long gencomm_msgext_raw_floats(int C);
long long gencomm_msgext_workspace_bytes(int n, int C, int H, int W);
int gencomm_msgext_fwd(const float* raw, const float* x, float* out, int n, int C, int H, int W,
                       void* workspace, long long workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * PointPillars front half, eval mode (opencood/models/heter_encoders.py:22-50 = PillarVFE
 * opencood/models/sub_modules/pillar_vfe.py:105-155 + PointPillarScatter point_pillar_scatter.py:42-76):
 * voxel_features [M,P,4] (P <= 32), voxel_num_points int32 [M], voxel_coords int32 [M,4] = (b,z,y,x)
 * -> out [B,64,ny,nx] (zero where no pillar). linear_w [64,10]; BatchNorm1d running statistics are
 * folded on the device into scratch128 (device float[128]). voxel_size3 / pc_range6 are HOST arrays.
 * The cell index is the reference's `z + y*nx + x`.
 * -------------------------------------------------------------------------------------------- */
int gencomm_pillar_encode_fwd(const float* voxel_features, const int* voxel_num_points, const int* voxel_coords,
                              const float* linear_w, const float* bn_weight, const float* bn_bias,
                              const float* bn_running_mean, const float* bn_running_var,
                              float* out, float* scratch128, int M, int P, int B, int nx, int ny,
                              const float* voxel_size3, const float* pc_range6, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Warp every agent into its scene's ego frame and fuse with per-pixel attention over agents,
 * keeping the ego row.  theta: device double[n][2][3], theta[i] = normalised affine that maps ego
 * grid coordinates to agent i's (= affine_matrix[b, 0, j] of normalize_pairwise_tfm,
 * opencood/utils/transformation_utils.py:68-92).  scene_off: device int32[B+1], agents of scene b
 * are rows scene_off[b] .. scene_off[b+1]-1 of x.  out [B,C,H,W].  At most 8 agents per scene.
 * -------------------------------------------------------------------------------------------- */
int gencomm_warp_attfuse_fwd(const float* x, const double* theta, const int* scene_off, float* out,
                             int B, int n, int C, int H, int W, void* stream);

/* ---- General 2-D convolution for the layers around the hot path -------------------------------------
 * Replaces the nn.Conv2d / nn.ConvTranspose2d (+ BatchNorm2d eval + ReLU) stacks of
 *   BaseBEVBackbone            opencood/models/sub_modules/base_bev_backbone.py:40-92, :94-123
 *   DownsampleConv/DoubleConv  opencood/models/sub_modules/downsample_conv.py:17-24
 *   cls/reg/dir heads          opencood/models/heter_model_baseline_w_gencomm_stage1.py:137-142
 * prepare: OIHW (transposed = 0), ConvTranspose2d IOHW with kernel == stride (transposed = 1), or (transposed = 2) the INPUT-GRADIENT
 *          convolution of a stride-1 layer straight from its forward OIHW weights (Cin = the forward's output channels, Cout = its input
 *          channels; taps flipped, channels transposed: what flip + transpose + contiguous + prepare did in four launches) -> k-major matrix
 *          [Cin*KH*KW][Cout] (resp. [Cin][Cout*KH*KW]) of the same number of floats, followed -- for GEMM shapes the f16-pipe kernel takes
 *          (3x3 / 2x2, Cin >= 16, Cin % 8 == 0, >= 32 GEMM rows; 1x1 and transposed convolutions stay on the exact-fp32 kernel: measured faster) -- by the three-term operand form of the weights and their per-row
 *          power-of-two scales (csrc/conv_h3_kernels.h), written by the same launch.  `prepared` must hold
 *          gencomm_conv2d_prepared_floats(Cin, Cout, KH, KW, transposed) floats (= Cin*Cout*KH*KW for the other shapes; -1: bad dims).
 * fold:    BatchNorm2d (eval) and/or conv bias -> per-channel scale/shift; pass NULL for the four BN tensors
 *          (and/or conv_bias) when absent.
 * fwd:     y[:, out_coff:out_coff+Cout] = act(conv(x) * scale + shift); supported: 3x3 stride 1|2 any pad, 1x1 stride 1, 7x7 stride 2
 *          any pad (the ResNet stem, ABI v12: exact fp32 MFMA);
 *          ups = s > 1 runs ConvTranspose2d(kernel = stride = s) (KH = KW = 1 on the prepared matrix, output H*s x W*s).
 *          KH = KW = 2 with ups = 2 (stride 1, pad 0; output 2H x 2W): the sub-pixel form of a TRANSPOSED 3x3 stride-2 pad-1 convolution,
 *          i.e. the input gradient of base_bev_backbone.py:57-63's stride-2 layers: GEMM row c*4 + a*2 + b = output channel c at
 *          pixel (2u + a, 2v + b), window = input rows u, u + 1 x columns v, v + 1 (zero beyond the map).
 *          y has out_ctotal channels (write into a slice of a concat buffer without a copy).
 *          Arithmetic follows GENCOMM_MODE_ARITH: 0 (default) = shapes whose prepared buffer carries the three-term form run on the f16
 *          matrix pipe with six matrix instructions per product block (operands split exactly into fp16 hi + fp16 lo + a third term:
 *          products accurate to 2^-26, fp32 accumulation; activations under a running power-of-two scale, weights under a per-row one:
 *          any finite fp32 input is safe), every other shape on the exact fp32 MFMA; 1 = exact fp32 MFMA for every shape; 3 (opt-in) =
 *          3x3 with Cin % 8 == 0 and 1x1 / ConvTranspose2d with >= 128 GEMM rows from two-term splits (22-bit products). */
int gencomm_conv2d_prepare(const float* weight, float* prepared, int Cin, int Cout, int KH, int KW, int transposed, void* stream);
long long gencomm_conv2d_prepared_floats(int Cin, int Cout, int KH, int KW, int transposed);
int gencomm_conv2d_fold(const float* bn_weight, const float* bn_bias, const float* bn_running_mean, const float* bn_running_var,
                        const float* conv_bias, float eps, int C, float* scale, float* shift, void* stream);
int gencomm_conv2d_fwd(const float* x, const float* prepared, const float* scale, const float* shift, float* y,
                       int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad, int relu,
                       int ups, int out_ctotal, int out_coff, void* stream);
/* the same (no transposed-conv mode, whole-tensor output) with act in {0 none, 1 ReLU, 2 erf-GELU (nn.GELU), 3 ReLU applied after
 * the residual add (ResNet BasicBlock), 4 LeakyReLU with negative_slope 0.01 (nn.LeakyReLU(), before the residual add)} and an optional residual [N][Cout][Ho][Wo]: Linear + GELU, Linear + skip connection,
 * conv + BatchNorm + identity + ReLU in one launch */
int gencomm_conv2d_act_res_fwd(const float* x, const float* prepared, const float* scale, const float* shift, const float* residual,
                               float* y, int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad, int act,
                               void* stream);

/* ---- Detection tail ---------------------------------------------------------------
 * Replaces, for one agent's head outputs (batch 1), the torch/numpy/shapely chain of
 *   VoxelPostprocessor.post_process   opencood/data_utils/post_processor/voxel_postprocessor.py:1130-1244
 * det_decode: sigmoid(cls) > score_threshold, delta_to_boxes3d (:1351-1396), direction classifier fix (:1159-1175),
 *   boxes_to_corners_3d + project_box3d (box_utils.py:152-204, :278-316), remove_large_pred_bbx / remove_bbx_abnormal_z
 *   (box_utils.py:1062-1112; a box with a NaN or infinite corner fails them, as torch's max / min propagate it there); survivors
 *   are APPENDED in anchor order at position *count (device int, in/out -- zero it
 *   before the first agent, call once per agent for late fusion). Layouts: cls [A][H][W], reg [7A][H][W],
 *   dir [A*num_bins][H][W] or NULL, anchors [H][W][A][7] float32, transformation_matrix [16] float32 (device).
 *   corners [capacity][8][3], scores / anchor_index [capacity]; entries beyond capacity are dropped but still counted:
 *   the caller must compare *count with capacity.
 * nms_rotated: box_utils.nms_rotated (:915-960; scores sorted descending, exact ties by descending index; any finite
 *   float is a valid score -- negative ones and zero order as numbers do, -0.0 below +0.0; NaN is not; the `top`
 *   best kept, top <= 1024; IoU of the BEV quadrilaterals = first four corners, in float64, suppressed when
 *   (float)iou > iou_threshold), then -- when keep_range6 != NULL -- mask_boxes_outside_range_numpy (:384-421, all 8
 *   corners inside, bounds inclusive). *n_candidates is a DEVICE int (at most gencomm_nms_max_candidates() are
 *   considered). Outputs in pick order; *out_count device int.
 * bbox_overlaps: opencood/utils/box_overlaps.pyx:17-57, (N,4) x (K,4) -> (N,K), bit-identical to the compiled source.
 * det_mc_decode (multi-class heads, VoxelPostprocessor.post_process_v2xreal :787-943): all n_agents agents of a call in one
 *   set of three launches per 8 agents. Per agent k (host arrays of device pointers / ints): cls [A*num_class][H][W] (class c
 *   of anchor j in channel j*num_class + c), reg [7A][H][W], anchors [H][W][A][7] float32, transformation_matrix [16].
 *   score, label = max over the class sigmoids (the first maximum wins), score > score_threshold, delta_to_boxes3d_v2xreal
 *   (no direction fix), boxes_to_corners_3d + project_box3d. Candidates in agent, then anchor order from slot 0: corners
 *   [capacity][8][3], unprojected [capacity][8][3] (may be NULL), scores, labels (1-based) [capacity]; *count (device) = all
 *   candidates (entries beyond capacity are dropped but counted), *violations (device) = candidates that
 *   remove_large_pred_bbx_v2xreal / remove_bbx_abnormal_z_v2xreal (box_utils.py:1115-1166) reject, a non-finite corner included -- kept, not dropped:
 *   the reference asserts there are none. Workspace: gencomm_det_mc_workspace_bytes (H, W: host arrays of n_agents).
 * det_mc_gather: after gencomm_nms_rotated_fwd on (corners, scores, count), score_labels[t] = {out_scores[t],
 *   labels[out_index[t]]} and out_unprojected[t] = unprojected[out_index[t]] (both NULL or neither) for t < *out_count. */
long long gencomm_det_workspace_bytes(int H, int W, int A);
long long gencomm_nms_workspace_bytes(void);
int gencomm_nms_max_candidates(void);
int gencomm_det_decode_fwd(const float* cls_preds, const float* reg_preds, const float* dir_preds, const float* anchors,
                           const float* transformation_matrix, int H, int W, int A, int num_bins, float score_threshold,
                           float dir_offset, int order_hwl, float* corners, float* scores, int* anchor_index, int* count,
                           int capacity, void* workspace, long long workspace_bytes, void* stream);
int gencomm_nms_rotated_fwd(const float* corners, const float* scores, const int* n_candidates, float iou_threshold, int top,
                            const float* keep_range6, float* out_boxes, float* out_scores, int* out_index, int* out_count,
                            void* workspace, long long workspace_bytes, void* stream);
int gencomm_bbox_overlaps_fwd(const float* boxes, const float* query_boxes, float* overlaps, int N, int K, void* stream);
long long gencomm_det_mc_workspace_bytes(const int* H, const int* W, int n_agents, int A);
int gencomm_det_mc_decode_fwd(const float* const* cls_preds, const float* const* reg_preds, const float* const* anchors,
                              const float* const* transformation_matrices, const int* H, const int* W, int n_agents, int A,
                              int num_class, float score_threshold, int order_hwl, float* corners, float* unprojected,
                              float* scores, int* labels, int* count, int* violations, int capacity, void* workspace,
                              long long workspace_bytes, void* stream);
int gencomm_det_mc_gather_fwd(const int* out_index, const int* out_count, const float* out_scores, const int* labels,
                              const float* unprojected, int capacity, int top, float* score_labels, float* out_unprojected,
                              void* stream);

/* MaxFusion.forward (opencood/models/fuse_modules/fusion_in_one.py:87-124): same warp, element-wise max over the
 * agents of a scene instead of the attention; arguments as gencomm_warp_attfuse_fwd. */
/* Backward of gencomm_warp_attfuse_fwd (what autograd does for fusion_in_one.py:131-151 + F.grid_sample in the reference's
 * training runs): grad_x [n][C][H][W] is OVERWRITTEN with the gradient w.r.t. x given grad_out [B][C][H][W]; the bilinear
 * gather's adjoint uses float atomics (summation order varies in the last bits). */
/* scratch: gencomm_warp_attfuse_bwd_scratch_floats(n, H, W) floats.  The ego's gradient (identity warp) is written once per pixel; the
 * other agents' gradients are GATHERED per source pixel from the few output pixels that sampled it (deterministic, no float atomics)
 * whenever their transform is rigid-like (decided on the device from theta); anything else takes the scatter with float atomics. */
long long gencomm_warp_attfuse_bwd_scratch_floats(int n, int H, int W);
int gencomm_warp_attfuse_bwd(const float* x, const double* theta, const int* scene_off, const float* grad_out, float* grad_x, float* scratch,
                             int B, int n, int C, int H, int W, void* stream);
int gencomm_warp_maxfuse_fwd(const float* x, const double* theta, const int* scene_off, float* out,
                             int B, int n, int C, int H, int W, void* stream);

/* Backward of gencomm_warp_maxfuse_fwd (torch.max(dim=0) over the warped agents + F.grid_sample): grad_x [n][C][H][W] is OVERWRITTEN.
 * The winner of every (scene, channel, output pixel) is recomputed with the forward's arithmetic; among equal maxima the LOWEST agent
 * index wins (torch's CPU rule; exact ties are common: agents that miss a pixel contribute 0), a NaN wins, the first NaN first.
 * scratch: gencomm_warp_maxfuse_bwd_scratch_floats(B, n, C, H, W) floats (a one-byte winner map [B][C][H W] and the per-agent plan).
 * Path per agent as in gencomm_warp_attfuse_bwd: identity ego written once per pixel, rigid-like agents gathered per source pixel
 * (no float atomics: two runs are bit-identical), anything else scattered with float atomics; scratch == NULL: every agent scatters. */
long long gencomm_warp_maxfuse_bwd_scratch_floats(int B, int n, int C, int H, int W);
int gencomm_warp_maxfuse_bwd(const float* x, const double* theta, const int* scene_off, const float* grad_out, float* grad_x, float* scratch,
                             int B, int n, int C, int H, int W, void* stream);

/* Fast lane for callers that chain Enhancer -> fusion themselves (ScenePipeline): call
 * gencomm_enhancer_fwd with out == NULL (the token-major result and the channel gate stay in the
 * workspace, the NHWC->NCHW transpose launch is skipped), then this entry point with the SAME
 * workspace pointer and (n, C, H, W). Same maths as gencomm_warp_attfuse_fwd(enhancer output). C in {64,128,256}. */
int gencomm_warp_attfuse_tok_fwd(const void* enhancer_workspace, const double* theta, const int* scene_off, float* out,
                                 int B, int n, int C, int H, int W, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Training building blocks (NCHW fp32, correctness-first; the inference path never calls them): what torch autograd's
 * conv / layer_norm / gelu backward functions do in the reference's training runs for the Enhancer
 * (opencood/models/gencomm_modules/enhancer.py:346-357, :222-250) and the dense conv stacks.
 *   gencomm_conv2d_wgrad     dw[Cout][Cin][K][K] += sum dy (x) x, db[Cout] += sum dy (db may be NULL); K = 1 or 3, stride 1 or 2
 *                            (input gradients: gencomm_conv2d_fwd with the transposed, tap-flipped weight)
 *   gencomm_ln_nchw_fwd      LayerNorm over the channel axis of every pixel; residual != 0: out = x + LN(x)
 *   gencomm_ln_nchw_bwd      dx (= or +=), dgamma +=, dbeta +=; scratch: n * HW * 2 floats
 *   gencomm_dwconv3x3_fwd    depthwise 3x3 pad 1 (+ bias); flip != 0: correlation with the flipped taps = input gradient
 *   gencomm_dwconv3x3_wgrad  dw[C][3][3] +=, db[C] += (db may be NULL)
 *   gencomm_gelu_bwd         out = g * GELU'(v), erf form
 *   gencomm_lincomb_fwd      out = a x + b y + c z (y, z may be NULL; out may alias an input; 16-byte aligned pointers): the
 *                            sampler chain's x_{t-1} = c1 x0_hat + c2 x_t + sigma eps (cond_diff.py:272-315) and its adjoint
 * -------------------------------------------------------------------------------------------- */
int gencomm_conv2d_wgrad(const float* dy, const float* x, float* dw, float* db, int N, int Cin, int Hi, int Wi, int Cout,
                         int K, int stride, int pad, void* stream);
/* The same with caller-owned scratch of gencomm_conv2d_wgrad_scratch_floats(...) floats (0 = the shape needs none). Wide 3x3 layers
 * (Cin, Cout >= 32: the BEV backbone, opencood/models/sub_modules/base_bev_backbone.py:40-92) then store per-workgroup partial sums and
 * add them in a fixed order -- deterministic, and 10x faster than the f32 atomics of the scratch-less form on 256-channel layers. */
long long gencomm_conv2d_wgrad_scratch_floats(int N, int Cin, int Hi, int Wi, int Cout, int K, int stride, int pad);
/* The same gradient (dw, db +=; stride 1, pad = K / 2, K = 1 or 3) with a FIXED order of additions: every workgroup writes its partial
 * sums into scratch (gencomm_conv2d_wgrad_fixed_scratch_floats(...) floats, required) and one pass adds them in workgroup order, so two
 * runs give the same bits. gencomm_conv2d_wgrad / _ws meet in dw with float atomics for every shape but the wide 3x3 one with scratch.
 * The V2VNet training path uses this form. */
long long gencomm_conv2d_wgrad_fixed_scratch_floats(int N, int Cin, int Hi, int Wi, int Cout, int K);
int gencomm_conv2d_wgrad_fixed(const float* dy, const float* x, float* dw, float* db, int N, int Cin, int Hi, int Wi, int Cout, int K,
                               float* scratch, long long scratch_floats, void* stream);
int gencomm_conv2d_wgrad_ws(const float* dy, const float* x, float* dw, float* db, int N, int Cin, int Hi, int Wi, int Cout,
                            int K, int stride, int pad, float* scratch, long long scratch_floats, void* stream);
/* GroupNorm (+ SiLU when silu != 0) over NCHW for any channel count and group size (unet.py:36-37, :31-33): the general-width
 * DiffusionUNet's normalisation; stat = n * groups * 2 floats of caller scratch (mean, rstd per sample and group). */
int gencomm_gn_nchw_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stat, float eps, int silu,
                        int n, int C, int groups, int HW, void* stream);
int gencomm_ln_nchw_fwd(const float* x, const float* gamma, const float* beta, float* out, float eps, int residual, int n, int C, int HW, void* stream);
int gencomm_ln_nchw_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, float* scratch,
                        float eps, int accumulate, int n, int C, int HW, void* stream);
int gencomm_dwconv3x3_fwd(const float* x, const float* w, const float* b, float* y, int n, int C, int H, int W, int flip, void* stream);
int gencomm_dwconv3x3_wgrad(const float* x, const float* dy, float* dw, float* db, int n, int C, int H, int W, void* stream);
/* ABI v8: the same two with the depthwise layer's input taken as the first C channels of an [n][x_ct][H][W] tensor and, act = 1, as
 * GELU(x) evaluated on the values read (enhancer.py:236-243: x1 = GELU(Linear1(.))[:, :hidden] feeds the depthwise convolution) -- the
 * training forward no longer writes the GELU outputs of Linear1, the weight gradient reads Linear1's output instead. act = 0 and
 * x_ct = C are the plain calls above. */
int gencomm_dwconv3x3_act_fwd(const float* x, int x_ct, int act, const float* w, const float* b, float* y, int n, int C, int H, int W, int flip,
                              void* stream);
int gencomm_dwconv3x3_act_wgrad(const float* x, int x_ct, int act, const float* dy, float* dw, float* db, int n, int C, int H, int W, void* stream);
int gencomm_gelu_bwd(const float* v, const float* g, float* out, long long count, void* stream);
int gencomm_lincomb_fwd(float* out, const float* x, const float* y, const float* z, float a, float b, float c, long long count, void* stream);
/* Elementwise pieces of the Enhancer's backward on channel slices (slice = channels [c0, c0 + nch) of an [n][ct][HW] tensor), op:
 *   0 copy: o0 slice = a slice                                    (replaces cat / contiguous)
 *   1 o0 = GELU(a[:, :nch]), o1 = GELU(a[:, nch:])                (a has 2 nch channels; o0, o1 have nch)
 *   2 o0 = GELU(a) * b                                            (gated product, enhancer.py:241-246)
 *   3 o0 = GELU'(a) c b, o1 slice = GELU'(d slice) c GELU(a)      (a = u, b = x2, c = d gated, d = Linear1 output; o1 / d share ct, c0)
 *   4 o0 slice = GELU'(a slice) b                                 (a, o0 share ct, c0; b has nch channels)
 *   5 o0 = GELU(a) * GELU(d slice)                                (ABI v8; d has o1_ct channels, its slice starts at o1_c0: op 2 reading
 *                                                                  x2 = GELU(Linear1 output) from Linear1's output itself)
 *   6 o0 = GELU'(a) c GELU(d slice), o1 slice = GELU'(d slice) c GELU(a)   (ABI v8; op 3 without b: x2 recomputed from d)
 * GELU' = Phi(x) + x phi(x) with the library's erf form (|Phi error| <= 0.85e-7) and one v_exp_f32 for the density.
 * When HW % 4 == 0 and every pointer is 16-byte aligned a lane handles four pixels with 128-bit accesses.
 * nc_scale: out = x * a[n][c] + b[n][c] (b may be NULL);  nc_dot: out[n][c] = sum_p x (* y) with f64 accumulation (out is zeroed). */
int gencomm_ew_slice_fwd(int op, const float* a, const float* b, const float* c, const float* d, float* o0, float* o1, int n, int nch, int HW,
                         int a_ct, int a_c0, int o0_ct, int o0_c0, int o1_ct, int o1_c0, void* stream);
int gencomm_nc_scale_fwd(const float* x, const float* a, const float* b, float* out, int n, int C, int HW, void* stream);
int gencomm_nc_dot_fwd(const float* x, const float* y, float* out, int n, int C, int HW, void* stream);

/* ----------------------------------------------------------------------------------------------
 * iou3d_nms with the reference extension's own semantics (opencood/pcdet_utils/iou3d_nms: src/iou3d_nms_kernel.cu:104-372,
 * src/iou3d_nms.cpp:30-135; Python wrappers iou3d_nms_utils.py:32-46, :147-181, :255-289). Boxes are [n][7] float32
 * (x, y, z, dx, dy, dz, heading). gencomm_iou3d_pairwise_fwd: out[num_a][num_b] = BEV overlap area (mode 0,
 * boxes_overlap_bev_gpu) or BEV IoU (mode 1, boxes_iou_bev_gpu). gencomm_iou3d_nms_fwd: boxes already in descending
 * score order (as nms_gpu / nms_normal_gpu pass them); keep[0..*count) = indices kept, ascending -- the reference returns
 * the count on the host after a blocking copy of the masks, here masks, greedy reduction, keep list and count all stay on
 * the device and the call is asynchronous. normal != 0 ignores the heading (nms_normal_gpu). At most
 * gencomm_iou3d_max_boxes() boxes. (The live GenComm post-processor uses the shapely-semantics NMS below,
 * gencomm_nms_rotated_fwd; this API serves the FPV-RCNN / iou-loss callers of the extension.)
 * -------------------------------------------------------------------------------------------- */
int gencomm_iou3d_pairwise_fwd(const float* boxes_a, int num_a, const float* boxes_b, int num_b, int mode, float* out, void* stream);
int gencomm_iou3d_max_boxes(void);
long long gencomm_iou3d_nms_workspace_bytes(int n);
int gencomm_iou3d_nms_fwd(const float* boxes, int n, float thresh, int normal, long long* keep, int* count,
                          void* workspace, long long workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Point cloud -> voxels with the semantics of spconv's CPU point-to-voxel as the reference's dataloader uses it
 * (opencood/data_utils/pre_processor/sp_voxel_preprocessor.py:25-29, :54-68): points [n][nfeat] (x, y, z first), voxels
 * in order of first appearance, points in input order, at most max_points per voxel / max_voxels voxels,
 * coords (z, y, x), grid = round((range[3:6] - range[0:3]) / voxel_size). Outputs are sized for max_voxels
 * (voxels [max_voxels][max_points][nfeat] zero-padded, coords_zyx [max_voxels][3], num_points [max_voxels]); *count = the
 * number of voxels produced (device int). Deterministic (stable radix sort + scans, no order-dependent atomics).
 * -------------------------------------------------------------------------------------------- */
long long gencomm_voxelize_workspace_bytes(int n);
int gencomm_voxelize_fwd(const float* points, int n, int nfeat, const float* voxel_size3, const float* range6, int max_points,
                         int max_voxels, float* voxels, int* coords_zyx, int* num_points, int* count,
                         void* workspace, long long workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Batched lidar front end: the raw clouds of all A agents of a call -> collated voxels in one launch sequence, with no host
 * read and no per-call memset (csrc/voxel_batch_kernels.h). Per agent: shuffle (perm, an INPUT), mask_ego_points
 * (pcd_utils.py:84-86: the closed box -1.95 <= x <= 2.95, -1.1 <= y <= 1.1 is removed, before the projection),
 * project_points_by_matrix_torch (box_utils.py:1169: float32 fused multiply-add chain over (x, y, z, 1); x, y, z only are
 * replaced), then exactly the gencomm_voxelize_fwd result of that agent's points (max_points and max_voxels per agent), then
 * SpVoxelPreprocessor.collate_batch: agents back to back, the agent index in front of (z, y, x).
 *   points [n][nfeat] float32; offsets [A + 1] device int32, logical point i belongs to agent a when offsets[a] <= i <
 *   offsets[a + 1]; transforms [A][16] float32 row-major 4x4 or null; perm [n] device int32 or null: logical point i is input
 *   row perm[i] (a row index outside [0, n) drops the point); mask_ego 0 / 1.
 *   cap_rows = min(A * max_voxels, n) rows are the capacity of voxels [cap_rows][max_points][nfeat], coords_azyx [cap_rows][4]
 *   (16-byte aligned) and num_points [cap_rows]; counts [A] and *total (device ints) = voxels per agent and their sum. Rows
 *   [0, total) are written completely (zero padding included), the rows behind them are not touched.
 * Keys are agent * cells + cell: 32 bits where A * cells < 2^32, 64 bits otherwise; an argument error (status 1) when A * cells reaches 2^63.
 * Deterministic: one stable radix sort, scans, one writer per output element, no atomics.
 * -------------------------------------------------------------------------------------------- */
long long gencomm_voxelize_batch_workspace_bytes(int n, int A, int max_voxels);
int gencomm_voxelize_batch_fwd(const float* points, int n, int nfeat, const int* offsets, int A, const float* transforms, const int* perm,
                               int mask_ego, const float* voxel_size3, const float* range6, int max_points, int max_voxels, int cap_rows,
                               float* voxels, int* coords_azyx, int* num_points, int* counts, int* total,
                               void* workspace, long long workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * V2X-ViT fusion building blocks (opencood/models/fuse_modules/fusion_in_one.py:355-407, sub_modules/hmsa.py:117-150,
 * sub_modules/mswin.py:47-83); NCHW fp32 per agent. The Linear layers around them run through gencomm_conv2d_fwd (1x1),
 * the LayerNorms through gencomm_ln_nchw_fwd; gencomm_amd/v2xvit.py is the module with the reference's state_dict keys.
 *   gencomm_warp_affine_fwd  warp_affine_simple: out[i] = bilinear sample of x[i] on the float64 affine grid theta[i] [2][3]
 *   gencomm_hgt_attn_fwd     qkv [n][3 heads dim_head][HW] (q | k | v blocks) -> out [n][heads dim_head][HW]: per pixel and head,
 *                            softmax attention across the agents of each scene (scene_off [B+1]); relation matrices folded into
 *                            the k / v projections by the caller (all agents have type 0 in GenComm's use).
 *                            dim_head 8, 16, 32 or 64. A scene holds 1..8 agents: scene_off lives on the device, so the host
 *                            entry cannot check it, and gencomm_hgt_attn_fwd / _bwd leave the rows of `out` / `dqkv` that
 *                            belong to a scene of more than 8 (or fewer than 1) agents UNTOUCHED, without an error. The
 *                            caller checks the scene sizes (the Python modules do: MAX_AGENTS_PER_SCENE)
 *   gencomm_win_attn_fwd     per agent, head and window x window tile: softmax(q k^T / sqrt(dim_head) + pos[dy][dx]) v,
 *                            pos_embedding [2 window - 1][2 window - 1]
 * -------------------------------------------------------------------------------------------- */
int gencomm_warp_affine_fwd(const float* x, const double* theta, float* out, int n, int C, int H, int W, void* stream);
int gencomm_hgt_attn_fwd(const float* qkv, const int* scene_off, float* out, int B, int heads, int dim_head, int HW, void* stream);
int gencomm_win_attn_fwd(const float* qkv, const float* pos_embedding, float* out, int n, int heads, int dim_head, int window, int H, int W,
                         void* stream);
/* Backward of the three blocks above (training with fusion_method v2xvit): gencomm_warp_affine_bwd zeroes dx and scatters dout
 * through the bilinear weights; gencomm_hgt_attn_bwd overwrites dqkv; gencomm_win_attn_bwd overwrites dqkv, ACCUMULATES dpos
 * [(2 window - 1)^2] and needs the forward's output `out` and gencomm_win_attn_bwd_scratch_floats floats of scratch. */
int gencomm_warp_affine_bwd(const double* theta, const float* dout, float* dx, int n, int C, int H, int W, void* stream);
int gencomm_hgt_attn_bwd(const float* qkv, const int* scene_off, const float* dout, float* dqkv, int B, int heads, int dim_head, int HW,
                         void* stream);
long long gencomm_win_attn_bwd_scratch_floats(int n, int heads, int window, int H, int W);
int gencomm_win_attn_bwd(const float* qkv, const float* pos_embedding, const float* out, const float* dout, float* dqkv, float* dpos,
                         float* scratch, int n, int heads, int dim_head, int window, int H, int W, void* stream);
/* CoBEVT fusion building blocks (opencood/models/fuse_modules/fusion_in_one.py:409-464, fuse_modules/swap_fusion_modules.py:87-128);
 * gencomm_amd/cobevt.py is the module with the reference's state_dict keys.
 *   gencomm_swap_attn_fwd    qkv [B L][3 heads dim_head][H][W] (q | k | v blocks, head-major) -> out [B L][heads dim_head][H][W]: per
 *                            scene, head and group, attention over the group's L window^2 tokens (agent, w1, w2) jointly:
 *                            softmax(q k^T / sqrt(dim_head) + bias_table[rel(i, j)][head]) v with rel = the module's
 *                            relative_position_index, (li - lj + L - 1)(2 window - 1)^2 + (hi - hj + window - 1)(2 window - 1) +
 *                            (wi - wj + window - 1); bias_table [(2 L - 1)(2 window - 1)^2][heads].  grid_mode 0: a group is the
 *                            window x window tile (x, y) of the map; 1: the grid cell (x, y), pixels (w1 H / window + x,
 *                            w2 W / window + y).  num_agents [B] (device): the keys of agents l >= num_agents[b] are masked, the
 *                            queries of all L agents are computed; values outside 1 .. L are clamped.  window 4 or 8, dim_head 16, 32
 *                            or 64, L <= 8, H and W multiples of window: anything else is an argument error
 *   gencomm_agent_mean_fwd   out [B][count] = mean over the L rows of x [B][L][count]
 * Training (gencomm_amd/cobevt_bwd.py):
 *   gencomm_swap_attn_train_fwd  gencomm_swap_attn_fwd plus lse [B L][heads][H][W]: per query the running max plus the log of the
 *                            running softmax denominator.  Same kernel template with one more store: `out` is bit-identical to
 *                            gencomm_swap_attn_fwd's on the same inputs
 *   gencomm_swap_attn_bwd    the adjoint, from the forward's inputs, `out` and `lse` and the output gradient dout [B L][heads dim_head]
 *                            [H][W].  With P_ij = exp(s_ij - lse_i): D_i = sum_d dO_id O_id, dS_ij = P_ij (dO_i . v_j - D_i),
 *                            dQ_i = scale sum_j dS_ij k_j, dK_j = scale sum_i dS_ij q_i, dV_j = sum_i P_ij dO_i.
 *                            dqkv [B L][3 heads dim_head][H][W] is OVERWRITTEN: every element is stored exactly once, nothing is read
 *                            from it and no atomics touch it; the k and v rows of masked agents (l >= num_agents[b]) get exact zeros,
 *                            the queries of all L agents take part.  dtable [(2 L - 1)(2 window - 1)^2][heads] is ACCUMULATED
 *                            (dtable[rel(i, j)][head] += dS_ij over every group and scene): the caller zeroes it.  The sum goes
 *                            through a per-workgroup table in LDS and then global float atomics, so its order is NOT fixed: dtable
 *                            may differ in the last bits between two runs, dqkv may not.  Two launches (a query pass and a key pass,
 *                            both recomputing the scores on the fp32 matrix cores), no scratch.  Same domain as the forward
 * -------------------------------------------------------------------------------------------- */
int gencomm_swap_attn_fwd(const float* qkv, const float* bias_table, const int* num_agents, float* out, int B, int L, int heads, int dim_head,
                          int window, int H, int W, int grid_mode, void* stream);
int gencomm_agent_mean_fwd(const float* x, float* out, int B, int L, long long count, void* stream);
int gencomm_swap_attn_train_fwd(const float* qkv, const float* bias_table, const int* num_agents, float* out, float* lse, int B, int L, int heads,
                                int dim_head, int window, int H, int W, int grid_mode, void* stream);
int gencomm_swap_attn_bwd(const float* qkv, const float* bias_table, const int* num_agents, const float* out, const float* lse, const float* dout,
                          float* dqkv, float* dtable, int B, int L, int heads, int dim_head, int window, int H, int W, int grid_mode,
                          void* stream);
/* V2VNet fusion building blocks (opencood/models/fuse_modules/fusion_in_one.py:238-353, sub_modules/convgru.py); gencomm_amd/v2vnet.py is
 * the module with the reference's state_dict keys. The convolutions between them run through gencomm_conv2d_fwd.
 *   gencomm_v2v_warp_pairs_fwd  out[p] = warp_affine_simple(x[src_row[p]], theta[p]) for P (target, source) pairs; x [rows][C][H][W] is
 *                               read in place, theta [P][2][3] float64, src_row [P] (device; rows outside x are NOT detected). A pair
 *                               whose theta is exactly the identity is copied
 *   gencomm_v2v_aggregate_fwd   node k of n_nodes owns the pairs pair_off[k] .. pair_off[k + 1] - 1 (1..8 of them; a node with another
 *                               count is left UNTOUCHED, pair_off lives on the device) and the state h[node_row[k]]:
 *                               m_p = (y[p] + e[k]) * mask_p with mask_p = the warp of a map of ones under theta[p], computed in the
 *                               kernel; agg = mean_p m_p (op 0, divisor = the number of pairs) or max_p m_p (op 1, fmaxf);
 *                               out_mode 0: out [n_nodes][2 C][H][W] = [h | agg], out_mode 1: out [n_nodes][C][H][W] = h + agg
 *   gencomm_gru_gate_fwd        h [n][C][HW] = sigmoid(g[n][c]) * tanh(g[n][C + c]) over g [n][2 C][HW]: a ConvGRU cell whose hidden
 *                               state is zero (g = the convolution with the stacked [update-gate; candidate] weights)
 * -------------------------------------------------------------------------------------------- */
int gencomm_v2v_warp_pairs_fwd(const float* x, const double* theta, const int* src_row, float* out, int P, int C, int H, int W, void* stream);
int gencomm_v2v_aggregate_fwd(const float* y, const float* e, const float* h, const double* theta, const int* node_row, const int* pair_off,
                              float* out, int n_nodes, int C, int H, int W, int op, int out_mode, void* stream);
int gencomm_gru_gate_fwd(const float* g, float* h, int n, int C, int HW, void* stream);
/* Training of the V2VNet fusion (gencomm_amd/v2vnet.py, trainable=True): the adjoints of the three entries above. No float atomics
 * except where noted; every output element is written exactly once, zeros included.
 *   gencomm_gru_gate_bwd             dg [n][2 C][HW] from g and dh [n][C][HW]: dg[:C] = dh tanh(c) s (1 - s), dg[C:] = dh s (1 - tanh(c)^2),
 *                                    s = sigmoid(g[:C]) and c = g[C:] recomputed
 *   gencomm_v2v_aggregate_train_fwd  gencomm_v2v_aggregate_fwd (the same bits in `out`) which for op 1 also writes winner [n_nodes][C][H][W]:
 *                                    the index, within the node's pairs, of the winning message under torch.max's rule (a strictly greater
 *                                    value replaces the current one: the lowest index among equal maxima; a NaN replaces anything but an
 *                                    earlier NaN). winner may be null for op 0
 *   gencomm_v2v_aggregate_bwd        dagg = the second channel half of dout [n_nodes][2 C][H][W] (out_mode 0) or dout [n_nodes][C][H][W]
 *                                    itself (out_mode 1); d m_p = dagg / N_k (op 0) or dagg [winner == p] (op 1);
 *                                    dy [P][C][H][W] = d m_p mask_p, de [n_nodes][C][H][W] = sum_p d m_p mask_p, the masks recomputed as in
 *                                    the forward. A node with a pair count outside 1..8 is left UNTOUCHED. The gradient of h is a slice of
 *                                    dout (out_mode 0) or dout (out_mode 1): node_row is not read
 *   gencomm_v2v_warp_pairs_bwd       dx[r] (+)= sum over the pairs p with src_row[p] == r of the adjoint of the bilinear warp of
 *                                    dwarped[p] under theta[p]; dx [rows][C][H][W]; row_pair_off [rows + 1] / row_pairs [P] (device) list the
 *                                    pairs by source row. accumulate 1 adds into dx, 0 overwrites every element (a row that no pair reads
 *                                    becomes zero). Per pair, decided on the device: an exactly-identity theta is an addition, a tame theta
 *                                    (L1 row norms of the inverse pixel-space matrix <= 1.5, |det| > 0.6: every rigid transform) is gathered
 *                                    per source pixel -- with such pairs only, two runs are bit-identical -- and anything else is scattered
 *                                    WITH FLOAT ATOMICS afterwards. scratch: gencomm_v2v_warp_pairs_bwd_scratch_floats(P) floats
 * -------------------------------------------------------------------------------------------- */
int gencomm_gru_gate_bwd(const float* g, const float* dh, float* dg, int n, int C, int HW, void* stream);
int gencomm_v2v_aggregate_train_fwd(const float* y, const float* e, const float* h, const double* theta, const int* node_row, const int* pair_off,
                                    float* out, unsigned char* winner, int n_nodes, int C, int H, int W, int op, int out_mode, void* stream);
int gencomm_v2v_aggregate_bwd(const float* dout, const double* theta, const int* node_row, const int* pair_off, const unsigned char* winner,
                              float* dy, float* de, int n_nodes, int C, int H, int W, int op, int out_mode, void* stream);
long long gencomm_v2v_warp_pairs_bwd_scratch_floats(int P);
int gencomm_v2v_warp_pairs_bwd(const float* dwarped, const double* theta, const int* src_row, const int* row_pair_off, const int* row_pairs,
                               float* dx, float* scratch, int P, int rows, int C, int H, int W, int accumulate, void* stream);
/* CodeFilling codebook codec (opencood/models/sub_modules/codebook.py, UMGMQuantizer: a 1..3-level residual multi-codebook quantizer over
 * rows of C channels); gencomm_amd/codebook.py is the module with the reference's state_dict keys; csrc/codebook_kernels.h has the kernel.
 * Envelope: C 64 | 128 | 256, m 1 | 2 | 4, levels 1..3, k[l] a power of two in 16..256 (k: HOST array of `levels` ints); anything else is an
 * argument error that names the argument.
 *   params   gencomm_umgm_param_floats floats, per level: {latentStageEncoder, quantizationHead, latentHead, dequantizationHead, sideHead,
 *            restoreHead} x (weight [C][C], bias [C]) -- the latentHead / sideHead slots of the last level are present and unread --, the
 *            codebook [m][k][C / m], the temperature [m] padded to 4 floats
 *   layout   HW == 0: x / restored are rows [n][C]; HW > 0: NCHW [n][C][HW] (n agents, n HW rows), read and written in place; keep (NCHW
 *            only, may be null) [n] bytes: a non-zero entry makes that agent's restored map its input, bit for bit (code_loss is taken before)
 *   gencomm_umgm_fwd         ONE launch for the whole codec plus a one-workgroup sum: restored, codes [levels][rows][m] int64 (argmax of the
 *                            logits), sampled (may be null) the sampled indices in the same shape, logits [levels][rows, m, k_l] concatenated (null: never
 *                            formed in memory), code_loss [1] =
 *                            mean((restored - x)^2) through per-workgroup partial sums added in a fixed order (no float atomics: two runs
 *                            give the same bits).  noise 0: the sampled index is the code; 1: uniforms [levels][rows, m, k_l] float32, the
 *                            kernel applies clamp(eps, 1 - eps) and -log(-log u); 2: the uniforms are drawn in the kernel, Philox4x32-7
 *                            keyed by `seed`, one counter per (level, row, group, codeword quad): independent of the tiling.
 *                            workspace: gencomm_umgm_workspace_bytes(rows, C)
 *   gencomm_umgm_noise_fwd   the uniforms noise 2 draws for `seed`, written as noise 1 reads them ([levels][n, m, k_l], n rows)
 *   gencomm_umgm_encode_fwd  the reference's encode(): codes = argmin of the distance per level, residuals carried (same kernel, decoder off)
 *   gencomm_umgm_decode_fwd  codes -> restored (same kernel, encoder off); a code outside 0 .. k - 1 is clamped
 * -------------------------------------------------------------------------------------------- */
long long gencomm_umgm_param_floats(int C, int m, const int* k, int levels);
long long gencomm_umgm_workspace_bytes(long long rows, int C);
int gencomm_umgm_fwd(const float* params, const float* x, const unsigned char* keep, const float* uniforms, unsigned long long seed, int noise,
                     float* restored, long long* codes, long long* sampled, float* logits, float* code_loss, long long n, int HW, int C, int m,
                     const int* k, int levels, void* workspace, long long workspace_bytes, void* stream);
int gencomm_umgm_encode_fwd(const float* params, const float* x, long long* codes, long long n, int HW, int C, int m, const int* k, int levels,
                            void* stream);
int gencomm_umgm_decode_fwd(const float* params, const long long* codes, float* restored, long long n, int HW, int C, int m, const int* k, int levels,
                            void* stream);
int gencomm_umgm_noise_fwd(float* out, unsigned long long seed, long long n, int m, const int* k, int levels, void* stream);
/* Straight-through backward of the codec: the gradient of (restored, code_loss) of a gencomm_umgm_fwd call with respect to x and to
 * every parameter. The forward of the trainable path IS gencomm_umgm_fwd with `sampled` requested; the backward recomputes the forward's
 * intermediates per 64-row tile and takes the one-hot from `sampled` (an argmax is never re-decided). No float atomics: two calls give
 * the same bits.
 *   params, x, keep, uniforms, seed, noise, n, HW, C, m, k, levels   as the forward call got them (noise 0: p = softmax(logit))
 *   sampled      [levels][rows][m] int64, what the forward returned
 *   d_restored   layout of x, may be null; a kept agent's part goes straight to dx
 *   d_loss       DEVICE pointer to one float, may be null (no host read)
 *   dx           layout of x, every element written once
 *   dparams      gencomm_umgm_param_floats floats in the order of params, every slot written (the unread latentHead / sideHead slots of
 *                the last level and the temperature padding: zeros); the temperature's gradient has gone through LowerBound's rule
 *                (passes where temperature >= 1e-6 or the gradient is negative). May be null with dx_only.
 *   dx_only      1: skip all parameter-gradient work (a frozen codec that passes gradients through)
 *   workspace    gencomm_umgm_bwd_workspace_bytes(rows, C, m, k, levels), 16-byte aligned
 * gencomm_rows_wgrad_fixed: dw [Co][Ci] = g^T a over rows, g [rows][Co], a [rows][Ci] row-major, on the fp32 matrix pipe; row ranges
 * are summed in a fixed order. Co, Ci multiples of 64 in 64 .. 4096; scratch: gencomm_rows_wgrad_fixed_scratch_floats floats. */
long long gencomm_umgm_bwd_workspace_bytes(long long rows, int C, int m, const int* k, int levels);
int gencomm_umgm_bwd(const float* params, const float* x, const unsigned char* keep, const float* uniforms, unsigned long long seed, int noise,
                     const long long* sampled, const float* d_restored, const float* d_loss, float* dx, float* dparams, int dx_only, long long n,
                     int HW, int C, int m, const int* k, int levels, void* workspace, long long workspace_bytes, void* stream);
long long gencomm_rows_wgrad_fixed_scratch_floats(long long rows, int Co, int Ci);
int gencomm_rows_wgrad_fixed(const float* g, const float* a, float* dw, long long rows, int Co, int Ci, float* scratch, long long scratch_floats,
                             void* stream);
/* STAMP's ConvNeXtBlock (opencood/models/stamp_modules/feature_alignnet_modules.py:303-348; the blocks of AdapterConvNext,
 * stamp_modules/adapter.py:120-144) for all n maps of a call in ONE launch (csrc/convnext_kernels.h; additive, ABI v12):
 *   y = x + gamma * pwconv2(GELU(pwconv1(LayerNorm_C(dwconv7x7(x)))))
 * x, y NCHW fp32 [n][C][H][W]; dwconv depthwise 7x7, zero padding 3, with bias (:323); LayerNorm over the channel axis of each pixel, biased
 * variance, eps 1e-6, weight and bias (:324, channels_last); erf-GELU (:326); pwconv1 C -> 4 C, pwconv2 4 C -> C (:325, :327) on the exact
 * fp32 MFMA, the [pixels, 4 C] hidden tensor never in memory; gamma [C] (:328), NULL where the reference has `gamma is None`.
 * Weights as the reference stores them: dw_weight [C][1][7][7], w1 [4 C][C], w2 [C][4 C] (16-byte aligned): there is no prepared form.
 * C must be 64 or 128, the two instantiations (any other: returns -1, gencomm_last_error() names C); y must not overlap x (neighbouring
 * tiles read the halo: status 1, nothing launched).  No float atomics: two runs give the same bits. */
int gencomm_convnext_block_fwd(const float* x, const float* dw_weight, const float* dw_bias, const float* ln_weight, const float* ln_bias,
                               const float* w1, const float* b1, const float* w2, const float* b2, const float* gamma, float* y,
                               int n, int C, int H, int W, void* stream);
/* HEAL's PyramidFusion (opencood/models/fuse_modules/pyramid_fuse.py; csrc/pyramid_kernels.h; additive, ABI v12).  fp32 NCHW throughout, no
 * float atomics: two runs give the same bits.
 *   gencomm_gconv3x3_prepare   weight [C][cpg][3][3] of a Conv2d(C, C, 3, padding 1, groups 32) -> packed [32][cpg][9][cpg] (32 cpg cpg 9
 *                              floats): packed[((g cpg + ci) 9 + tap) cpg + co] = weight[g cpg + co][ci][tap]
 *   gencomm_gconv3x3_fwd       y = act(scale * conv3x3_grouped(x) + shift), conv2 of the ResNeXt Bottleneck (sub_modules/resblock.py:67-122 with
 *                              groups 32, width_per_group 4).  x [n][C][H][W], y [n][C][Ho][Wo], Ho = (H - 1) / stride + 1; cpg in {4, 8, 16},
 *                              C = 32 cpg in and out, stride 1 | 2, padding 1, dilation 1: anything else returns -1 and
 *                              gencomm_last_error() names it.  scale / shift [C]: gencomm_conv2d_fold's output; relu != 0: ReLU.
 *   gencomm_pyramid_score_fwd  the single-supervision head of one level (pyramid_fuse.py:143-162): occ = Conv2d(C, 1, 1)(x) (weight [C],
 *                              bias [1]), score = (sigmoid(occ) + 1e-4) * mask; both [n][1][H][W].  rect [n][4] int32 = (h0, h1, w0, w1):
 *                              mask = 1 inside rows [h0, h1) x columns [w0, w1) and 0 outside (an empty range: 0 everywhere); h0 < 0 = no
 *                              mask for this agent; rect NULL = no mask at all.
 *   gencomm_warp_weightfuse_fwd  weighted_fuse (pyramid_fuse.py:17-63), arguments as gencomm_warp_attfuse_fwd plus score [n][1][H][W]: per
 *                              output pixel the warped score of every agent of the scene (warp_affine_simple, align_corners False), exact 0
 *                              -> -inf, softmax over the agents, out[c] = sum_j p_j warp(x_j)[c]; a pixel where every agent is -inf is
 *                              exactly 0 (the reference's NaN -> 0).  At most 8 agents per scene. */
int gencomm_gconv3x3_prepare(const float* weight, float* packed, int cpg, void* stream);
int gencomm_gconv3x3_fwd(const float* x, const float* packed, const float* scale, const float* shift, float* y, int n, int C, int cpg, int H, int W,
                         int stride, int relu, void* stream);
int gencomm_pyramid_score_fwd(const float* x, const float* weight, const float* bias, const int* rect, float* occ, float* score, int n, int C, int H,
                              int W, void* stream);
int gencomm_warp_weightfuse_fwd(const float* x, const float* score, const double* theta, const int* scene_off, float* out, int B, int n, int C, int H,
                                int W, void* stream);
/* Training HEAL's PyramidFusion (csrc/pyramid_bwd_kernels.h; additive, ABI v12): the adjoints of the four entries above.  No float atomics,
 * every output element is written once, every parameter gradient is a sum of per-workgroup partials (scratch) added in index order: two
 * runs give the same bits.  Status 2 for a scratch smaller than the matching _scratch_floats query (-1 outside the domain).
 *   gencomm_gconv3x3_prepare_t   weight -> packed_t[((g cpg + co) 9 + tap) cpg + ci] = weight[g cpg + co][ci][8 - tap]: the pack of the
 *                              input gradient (channels swapped inside each group, taps flipped).
 *   gencomm_gconv3x3_dgrad     dx [n][C][H][W] from dy [n][C][Ho][Wo] (H, W: the FORWARD INPUT's size, odd sizes included): the forward
 *                              tiles on dy with packed_t; unit_scale / zero_shift: [C] ones / zeros.  Stride 2 spreads dy onto the
 *                              stride-1 grid first, into `spread` (n C H W floats; may be NULL at stride 1).
 *   gencomm_gconv3x3_wgrad_fixed  dw [C][cpg][3][3] = sum over maps and output pixels of dy (x) x; no bias.
 *   gencomm_pyramid_score_bwd  with sg = sigmoid(occ): d_pre = d_occ + d_score mask sg (1 - sg); dx = d_pre weight[c], dw[c] = sum d_pre
 *                              x[c], db = sum d_pre.  occ: the forward's output.  rect as in the forward (the module passes none in
 *                              train() mode, as the reference skips the crop there).  d_occ or d_score may be NULL (not both); dx may be
 *                              NULL; dw and db may be NULL together (a frozen head: no scratch is needed then).
 *   gencomm_warp_weightfuse_bwd  from x, score, theta, scene_off (as given to the forward) and dout [B][C][H][W]: dx [n][C][H][W] and
 *                              dscore [n][1][H][W].  The shares are recomputed with the forward's cells; dscore is exactly 0 where the
 *                              warped score was 0 and where nobody scores; an agent outside the map gets zeros; an agent under the exact
 *                              identity gets dx = p dout without interpolation.  Gathered per source pixel for every transform (a
 *                              singular one scans the map). */
int gencomm_gconv3x3_prepare_t(const float* weight, float* packed_t, int cpg, void* stream);
int gencomm_gconv3x3_dgrad(const float* dy, const float* packed_t, const float* unit_scale, const float* zero_shift, float* dx, float* spread, int n,
                           int C, int cpg, int H, int W, int stride, void* stream);
long long gencomm_gconv3x3_wgrad_fixed_scratch_floats(int n, int cpg, int H, int W, int stride);
int gencomm_gconv3x3_wgrad_fixed(const float* x, const float* dy, float* dw, int n, int C, int cpg, int H, int W, int stride, float* scratch,
                                 long long scratch_floats, void* stream);
long long gencomm_pyramid_score_bwd_scratch_floats(int n, int C, int H, int W);
int gencomm_pyramid_score_bwd(const float* x, const float* weight, const float* occ, const int* rect, const float* d_occ, const float* d_score,
                              float* dx, float* dw, float* db, int n, int C, int H, int W, float* scratch, long long scratch_floats, void* stream);
long long gencomm_warp_weightfuse_bwd_scratch_floats(int n, int H, int W);
int gencomm_warp_weightfuse_bwd(const float* x, const float* score, const double* theta, const int* scene_off, const float* dout, float* dx,
                                float* dscore, float* scratch, long long scratch_floats, int B, int n, int C, int H, int W, void* stream);
/* MPDA's feature aligner (opencood/models/mpda_modules/wg_fusion_modules.py, resizer.py; csrc/mpda_kernels.h; additive, ABI v12).  fp32 NCHW
 * in, out and accumulation; every output element is stored exactly once, no atomics: two runs give the same bits.
 *   gencomm_quad_attn_fwd      attention inside 2 x 2 groups, by index arithmetic on the maps (nothing is rearranged in memory).  With
 *                              X = H / 2, Y = W / 2 and token t = 2 w1 + w2, group (x, y) holds the pixels (2 x + w1, 2 y + w2) for
 *                              grid_mode 0 ('(x w1) (y w2)', window) and (w1 X + x, w2 Y + y) for grid_mode 1 ('(w1 x) (w2 y)', grid).
 *                              Per query map n, head m and group: out = softmax(dim_head^-0.5 q k^T + bias) v over the 4 tokens, channel
 *                              m dim_head + d of each tensor.  ARGUMENT FORM: three separate pointers, each AT ITS FIRST CHANNEL, plus the
 *                              channel totals of the tensors they point into: q [N][q_ct][H][W], k and v [Nkv][kv_ct][H][W] (map n of q
 *                              is q + n q_ct H W).  Cross attention (CrossAttention, :12-97): three tensors, q_ct = kv_ct = heads
 *                              dim_head.  Self attention from one to_qkv output t [N][3 inner][H][W] (Attention, :101-174):
 *                              q = t, k = t + inner H W, v = t + 2 inner H W, q_ct = kv_ct = 3 inner.  Nkv = N, or Nkv = 1: the one
 *                              key / value map serves every query map (the reference's ego.repeat(n, 1, 1, 1)).  bias_table NULL (no
 *                              bias) or [9][heads] = rel_pos_bias.weight at window_size 2, read at rel = (hi - hj + 1) 3 + (wi - wj + 1)
 *                              for query token (hi, wi), key token (hj, wj): the module's rel_pos_indices buffer.  out
 *                              [N][heads dim_head][H][W].  Domain: dim_head in {16, 32, 64}, heads 1..65535, N 1..65535, H and W even and
 *                              >= 2, q_ct / kv_ct >= heads dim_head, all four pointers 8-byte aligned; anything else, and any null
 *                              pointer but bias_table, returns a non-zero status without a launch and gencomm_last_error() names it.
 *   gencomm_resize_bilinear_fwd  x [N][C][Hi][Wi] -> y [N][C][Ho][Wo] as F.interpolate(size=(Ho, Wo), mode='bilinear', align_corners=False)
 *                              on torch's CPU arithmetic: source coordinate max((o + 0.5) (float)in / out - 0.5, 0), lower index
 *                              truncated, upper neighbour clamped to the last row / column, columns interpolated inside each row
 *                              first, then the two rows.  A weight of exactly 0 drops its term: Hi == Ho and Wi == Wo returns the
 *                              input's bits. */
int gencomm_quad_attn_fwd(const float* q, const float* k, const float* v, const float* bias_table, float* out, int N, int Nkv, int heads,
                          int dim_head, int H, int W, int q_ct, int kv_ct, int grid_mode, void* stream);
int gencomm_resize_bilinear_fwd(const float* x, float* y, int N, int C, int Hi, int Wi, int Ho, int Wo, void* stream);
/* MPDA training (csrc/mpda_bwd_kernels.h; additive, ABI v12).  No float atomics: two runs give the same bits in every output.
 *   gencomm_quad_attn_train_fwd  gencomm_quad_attn_fwd plus dropout on the 4 x 4 probabilities.  keep [N][heads][X Y] uint16, one word per
 *                              group (group index x Y + y): bit 4 i + j set = probability (query token i, key token j) survives and is
 *                              multiplied by keep_scale = 1 / (1 - p), clear = 0.  keep NULL (keep_scale ignored), or all 16 bits set with
 *                              keep_scale 1, gives gencomm_quad_attn_fwd's bits.  Nothing else is saved for the backward.
 *   gencomm_quad_attn_bwd      the adjoint, from q, k, v, bias_table, keep / keep_scale (as given to the forward) and dout
 *                              [N][heads dim_head][H][W]; the scores are recomputed.  dq is written in q's form ([N][q_ct][H][W] at the
 *                              first query channel), dk and dv in k's and v's ([Nkv][kv_ct][H][W]): in the self form dq | dk | dv are the
 *                              channel blocks of one dqkv [N][3 inner][H][W].  Only the heads dim_head channels from each pointer on are
 *                              written, each element once.  Nkv = 1 with N > 1: dk / dv are the sums over the N query maps, added in map
 *                              order from per-map slabs in the workspace.  dbias [9][heads] = sum over maps and groups of dS at rel(i, j),
 *                              per-workgroup partials (workspace) added in a fixed order; bias_table NULL: dbias may be NULL and is not
 *                              written.  Domain as gencomm_quad_attn_fwd, all seven float pointers and the workspace 8-byte aligned;
 *                              status 2 for a workspace smaller than gencomm_quad_attn_bwd_workspace_bytes (-1 outside the domain; 0
 *                              bytes needs no workspace pointer).
 *   gencomm_resize_bilinear_bwd  the adjoint of gencomm_resize_bilinear_fwd as a gather per source pixel: dy [N][C][Ho][Wo] -> dx
 *                              [N][C][Hi][Wi], every element written once, with the forward's own weights.  Hi == Ho and Wi == Wo
 *                              returns dy's bits.
 *   gencomm_leaky_relu_fwd / _bwd  y = x > 0 ? x : slope x over n floats; dx = y > 0 ? dy : slope dy, from the OUTPUT y. */
int gencomm_quad_attn_train_fwd(const float* q, const float* k, const float* v, const float* bias_table, const unsigned short* keep, float keep_scale,
                                float* out, int N, int Nkv, int heads, int dim_head, int H, int W, int q_ct, int kv_ct, int grid_mode, void* stream);
long long gencomm_quad_attn_bwd_workspace_bytes(int N, int Nkv, int heads, int dim_head, int H, int W, int has_bias);
int gencomm_quad_attn_bwd(const float* q, const float* k, const float* v, const float* bias_table, const unsigned short* keep, float keep_scale,
                          const float* dout, float* dq, float* dk, float* dv, float* dbias, int N, int Nkv, int heads, int dim_head, int H, int W,
                          int q_ct, int kv_ct, int grid_mode, void* workspace, long long workspace_bytes, void* stream);
int gencomm_resize_bilinear_bwd(const float* dy, float* dx, int N, int C, int Hi, int Wi, int Ho, int Wo, void* stream);
int gencomm_leaky_relu_fwd(const float* x, float* y, long long n, float slope, void* stream);
int gencomm_leaky_relu_bwd(const float* y, const float* dy, float* dx, long long n, float slope, void* stream);
/* The adjoint of that block (csrc/convnext_bwd_kernels.h; additive, ABI v12).  Given the block's input x, dy and the parameters it writes
 * dx and, unless dx_only, the gradient of every parameter (d_gamma ignored where gamma is NULL); every output element is WRITTEN once, no
 * float atomics, parameter gradients are fixed-order sums of per-slab partials: two runs give the same bits.  u and h are recomputed per
 * 64-pixel tile and 64-column hidden chunk; nothing of size [pixels, 4 C] is stored: the workspace holds two [n][C][H][W] maps, per-tile
 * and per-slab partial sums and two re-laid weight matrices (gencomm_convnext_block_bwd_workspace_bytes; 16-byte aligned).  One call is at
 * most 6 launches (3 with dx_only = 1, which serves a frozen block with a trainable input).  slabs: how many pixel slabs the parameter
 * gradients are summed over, 0 = automatic (at most 192).  Status 1 and nothing launched for: C other than 64 / 128, a null pointer, a
 * workspace that is too small (status 2), dx overlapping x, dx overlapping dy without being dy itself (dx == dy is allowed). */
long long gencomm_convnext_block_bwd_workspace_bytes(int n, int C, int H, int W, int dx_only, int slabs);
int gencomm_convnext_block_bwd(const float* x, const float* dy, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                               const float* ln_bias, const float* w1, const float* b1, const float* w2, const float* b2, const float* gamma,
                               float* dx, float* d_dw_weight, float* d_dw_bias, float* d_ln_weight, float* d_ln_bias, float* d_w1, float* d_b1,
                               float* d_w2, float* d_b2, float* d_gamma, int dx_only, int slabs, int n, int C, int H, int W, void* workspace,
                               long long workspace_bytes, void* stream);
/* radix-3 split attention over the three window branches (sub_modules/split_attn.py:31-62): out = sum_r softmax_r(fc2(ReLU(LN(fc1(
 * mean_HW(a + b + c))))))[r] * branch_r (+ residual); fc1 [C][C], fc2 [3 C][C] without biases; scratch >= 4 n C floats; C <= 256 */
int gencomm_split3_attn_fwd(const float* a, const float* b, const float* c, const float* fc1_w, const float* ln_w, const float* ln_b,
                            const float* fc2_w, const float* residual, float* out, float* scratch, int n, int C, int HW, void* stream);

/* BatchNorm2d with BATCH statistics (training mode; base_bev_backbone.py:47-52: eps 1e-3, momentum 0.01) around the HIP convolutions of
 * the backbone / shrink stacks: y = act(gamma (x - mean_batch) / sqrt(var_batch + eps) + beta) over NCHW, running statistics updated as
 * nn.BatchNorm2d does (unbiased variance; pass null to leave them alone); save [C][2] = (mean, rstd) for the backward; scratch >= 2 C
 * doubles. Backward: dx overwritten, dgamma / dbeta accumulated, y = the forward's output (supplies the ReLU mask).
 * ABI v8: `relu` bit 1 of gencomm_bn2d_train_bwd set = dgamma / dbeta are WRITTEN (the caller need not zero them); clear = accumulated.
 * ABI v9: `relu` bit 2 (value 4) of either call set = `scratch` arrives ZEROED (the caller carved it from a zero-filled pool: no memset
 * launch here); gencomm_bn2d_train_fwd takes `num_batches_tracked` (device int64, may be null) and adds 1 to it inside its own kernel --
 * nn.BatchNorm2d's counter without a launch of its own (batchnorm.py: `self.num_batches_tracked.add_(1)`). */
int gencomm_bn2d_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y, float* save,
                           double* scratch, float momentum, float eps, int relu, int n, int C, int HW, long long* num_batches_tracked,
                           void* stream);
int gencomm_bn2d_train_bwd(const float* x, const float* y, const float* dy, const float* save, const float* gamma, float* dx, float* dgamma,
                           float* dbeta, double* scratch, int relu, int n, int C, int HW, void* stream);
/* ABI v10: one conv -> BatchNorm2d(batch statistics) -> ReLU layer (base_bev_backbone.py:40-83) per call and direction -- compositions of
 * gencomm_conv2d_prepare / _fwd / _wgrad_ws and gencomm_bn2d_train_*, so that a layer costs the host ONE foreign call instead of three or four.
 * fwd: weight OIHW [Cout][Cin][K][K] (K 1 | 3, stride 1 | 2), bias may be null; unit_scale / zero_shift: [Cout] ones / zeros; prepared:
 * scratch of gencomm_conv2d_prepared_floats(Cin, Cout, K, K, 0) floats; pre = the convolution's output (kept for the backward), y, save
 * [Cout][2]; stat_scratch: 2 Cout doubles, ZEROED by the caller.  bwd (stride 1): dpre scratch [N][Cout][Ho][Wo]; dw / dbias (may be null)
 * arrive ZEROED and are accumulated into, dgamma / dbeta written, dx may be null; unit_scale / zero_shift: [Cin]; prepared:
 * gencomm_conv2d_prepared_floats(Cout, Cin, K, K, 2) floats; wgrad_scratch as gencomm_conv2d_wgrad_ws. */
int gencomm_convbn_train_fwd(const float* x, const float* weight, const float* bias, const float* unit_scale, const float* zero_shift,
                             const float* gamma, const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                             float momentum, float eps, int relu, float* prepared, float* pre, float* y, float* save, double* stat_scratch,
                             int N, int Cin, int H, int W, int Cout, int K, int stride, int pad, void* stream);
int gencomm_convbn_train_bwd(const float* x, const float* weight, const float* pre, const float* y, const float* gy, const float* save, const float* gamma,
                             const float* unit_scale, const float* zero_shift, int relu, float* dpre, float* dx, float* dw, float* dbias, float* dgamma,
                             float* dbeta, double* stat_scratch, float* prepared, float* wgrad_scratch, long long wgrad_scratch_floats,
                             int N, int Cin, int H, int W, int Cout, int K, int pad, void* stream);

/* Training path of the PointPillars per-pillar network (pillar_vfe.py:31-54): the Linear layer runs as a 1x1 convolution over the
 * [1, C, 1, M P] point-slot layout (gencomm_conv2d_fwd / _wgrad), BatchNorm1d with batch statistics as gencomm_bn2d_train_*, and the
 * max over the P slots of a pillar here: x [C][M][P] -> out [M][C] with the arg-max slot (first maximum), backward = routing. */
int gencomm_slot_max_fwd(const float* x, float* out, unsigned char* arg, int C, int M, int P, void* stream);
/* The same layer in ONE piece for training mode (BatchNorm1d with batch statistics), without the [M P, C] intermediates (csrc/pfn_kernels.h):
 * the statistics of the Linear output follow exactly from the inputs' first and second moments over all M P slots, ReLU(BN(.)) is
 * monotone in the Linear output, and the dense part of BatchNorm's backward folds into the same moments -- two launches forward, two
 * backward, instead of a 1x1 convolution, BatchNorm and slot-max over five 393-MB tensors at the stage-1 recipe's 48 000 pillars.
 * feats [M][P][F] (slots beyond a pillar's point count zeroed, pillar_vfe.py:96-100), weight [C][F]; F in {9, 10, 11}, C in {32, 64, 128, 256},
 * P <= 255.  fwd: out [M][C], arg [M][C] (the extreme slot), save [C][2] (mean, rstd), moments [gencomm_pfn_moment_doubles(F)] (kept for
 * the backward); running statistics / num_batches_tracked updated as nn.BatchNorm1d does (may be null).  bwd: dweight [C][F], dgamma,
 * dbeta WRITTEN (each may be null); scratch: gencomm_pfn_bwd_scratch_doubles(F, C) doubles (per-block partial sums, added up in a fixed order). */
int gencomm_pfn_train_fwd(const float* feats, const float* weight, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          long long* num_batches_tracked, float momentum, float eps, float* out, unsigned char* arg, float* save, double* moments,
                          int M, int P, int F, int C, void* stream);
int gencomm_pfn_train_bwd(const float* feats, const float* weight, const float* gamma, const float* beta, const float* save, const double* moments,
                          const float* gout, const unsigned char* arg, float* dweight, float* dgamma, float* dbeta, double* scratch,
                          int M, int P, int F, int C, void* stream);
long long gencomm_pfn_moment_doubles(int F);
long long gencomm_pfn_bwd_scratch_doubles(int F, int C);
int gencomm_slot_max_bwd(const float* dout, const unsigned char* arg, float* dx, int C, int M, int P, void* stream);

/* Detection-head terms of the training criterion in one launch, forward and gradients (opencood/loss/point_pillar_loss.py:36-126 with
 * :129-170 and :216-245; called through point_pillar_gencomm_loss.py:16-58): sigmoid focal classification loss, smooth-L1 regression loss
 * on the sin-difference encoding, softmax cross entropy of the heading bin, each weighted and divided by batch_size.
 * cls [B][A][H][W], reg [B][7A][H][W], dir [B][A*A][H][W] (the reference's view(-1, anchor_num): logits of anchor a = channels a*A..a*A+A-1;
 * null: no direction term), pos / neg [B][H][W][A], tgt [B][H][W][7A]; A <= 8.  sums [4] (double, ZEROED BY THE CALLER) += cls, reg, dir loss, their sum;
 * gcls / greg / gdir = d (cls + reg + dir loss) / d map, overwritten.  anchor_yaw: HOST array of A radians (float64 like the reference). */
int gencomm_head_loss(const float* cls, const float* reg, const float* dir, const float* pos, const float* neg, const float* tgt, float* gcls,
                      float* greg, float* gdir, double* sums, int B, int A, int H, int W, int num_bins, const double* anchor_yaw, double dir_offset,
                      float pos_cls_weight, float gamma, float alpha, float cls_weight, float sigma, float reg_weight, float dir_weight,
                      int batch_size, void* stream);

/* Multi-class detection-head terms of the V2X-Real training criteria, forward and gradients, in two launches (a per-sample count of the
 * positive slots, then the loss): opencood/loss/point_pillar_v2xreal_gencomm_loss.py:88-160 (and its stage-2 twin point_pillar_v2xreal_loss.py)
 * with WeightedSmoothL1Loss :12-70, cls_loss_func :168-199, add_sin_difference :221-233; labels / targets as generate_label_v2xreal and
 * collate_batch_v2xreal produce them (opencood/data_utils/post_processor/voxel_postprocessor.py:312-461, :622-656).
 * cls [B][S*K][H][W], reg [B][7S][H][W] (float32, contiguous); labels [B][H][W][S] (values -1 ignore, 0 background, 1..K class),
 * targets [B][H][W][S][7], both float32 (dtype 0) or float64 (dtype 1). S = slots per location, 1 <= K <= 8 classes; the logits of slot j are
 * channels j*K .. j*K+K-1, its regression channels 7j .. 7j+6. Per sample, with P = #{label > 0}: sigmoid focal loss (alpha 0.25, gamma 2,
 * float32) over the one-hot of the label value, weighted [label >= 0] / max(P, 1); smooth-L1 (beta 1/9, strict <, NaN targets ignored) on the
 * sin-difference encoding, weighted [label > 0] / max(P, 1), in the targets' dtype. Both are divided by B and weighted by cls_weight / reg_weight.
 * count [B] (unsigned, ZEROED BY THE CALLER) receives P; sums [3] (double, ZEROED BY THE CALLER) += conf_loss, reg_loss, their sum;
 * gcls / greg = d (conf_loss + reg_loss) / d map, overwritten. */
int gencomm_head_loss_mc(const float* cls, const float* reg, const void* labels, const void* targets, int dtype, unsigned* count, float* gcls,
                         float* greg, double* sums, int B, int S, int K, int H, int W, double cls_weight, double reg_weight, void* stream);

/* Training-time anchor target assignment on the device (csrc/target_kernels.h), replacing the per-sample CPU assigner
 * VoxelPostprocessor.generate_label (opencood/data_utils/post_processor/voxel_postprocessor.py:188-310) and generate_label_v2xreal
 * (:312-463) with their helpers boxes_to_corners_3d / corner2d_to_standup_box (opencood/utils/box_utils.py:152-204, :225-248) and
 * bbox_overlaps (opencood/utils/box_overlaps.pyx:17-57), and the stacking of collate_batch / collate_batch_v2xreal (:577-655): every sample
 * of the batch and every class in TWO launches, the anchors x boxes IoU matrix is never stored.
 *   standup: anchors [n_anchors][7] float64 (one class's [H][W][R][7] array) -> out [n_anchors][4] float32 stand-up boxes (x1, y1, x2, y2),
 *            float32 corners as the reference forms them; hwl = 1 for order 'hwl'. Done once per anchor array, kept by the caller.
 *   assign:  boxes [B][max_num][box_width] (box_dtype 0: float32, 1: float64; box_width 7, or 8 with the class id 1..nc in column 7),
 *            mask [B][max_num] (mask_dtype 0: float32, 1: float64, 2: int32, 3: int64, 4: uint8 / bool; a box is valid where mask == 1);
 *            anchors / standup: HOST arrays of nc DEVICE pointers (per class [n_anchors][7] float64 and its stand-up boxes),
 *            pos_threshold / neg_threshold: HOST arrays of nc doubles (compared in float32, as numpy does); n_anchors = H W R per class,
 *            R anchors per location and class; max_num <= 256, nc <= 8.
 *            multiclass 0 (nc = 1, generate_label): pos / neg [B][H][W][R] = pos_equal_one / neg_equal_one, targets [B][H][W][7R]; the
 *            deltas of a positive anchor read row j of the UNFILTERED boxes for the j-th valid box, as :279 does.
 *            multiclass 1 (generate_label_v2xreal, box_width 8): the boxes of class k are those with mask == 1 and column 7 - 1 == k, in input
 *            order; pos [B][H][W][nc R] = the label map (-1 ignore, 0 background, class id), slot k R + r; targets [B][H][W][nc R][7];
 *            neg [B][H][W][R] = neg_equal_one of the LAST class (:460).
 *            Outputs are float32 (out_dtype 0) or float64 (1), written completely (zeros included); the deltas are computed in float64
 *            from the float64 anchors and rounded once.
 *            workspace: gencomm_target_assign_workspace_bytes(B, nc, max_num) bytes, ZEROED ONCE by the caller when it is allocated;
 *            every call leaves it zeroed for the next one (no memset per call). One call at a time per workspace. */
long long gencomm_target_assign_workspace_bytes(int B, int nc, int max_num);
int gencomm_target_standup_fwd(const double* anchors, int n_anchors, int hwl, float* out, void* stream);
int gencomm_target_assign_fwd(const void* boxes, int box_dtype, int box_width, const void* mask, int mask_dtype, const double* const* anchors,
                              const float* const* standup, const double* pos_threshold, const double* neg_threshold, int B, int nc, int max_num,
                              int n_anchors, int R, int multiclass, void* pos, void* neg, void* targets, int out_dtype, void* workspace,
                              long long workspace_bytes, void* stream);

/* Training path of MessageExtractorv2's deformable 3x3 convolution (message_extractor_v2.py:78,:108; DCNv1, padding 1, one offset
 * group), split into its sampling half and its GEMM half so that the backward is GEMMs on the general kernels + one scatter:
 *   gencomm_dcn_sample_fwd   col[n][c * 9 + k][p] = bilinear sample of x[n][c] at tap k's displaced position (zero outside)
 *                            -- the deformable convolution is then gencomm_conv2d_fwd(col, W [64][9 C], 1x1)
 *   gencomm_dcn_scatter_bwd  given dcol: dx += scatter of the bilinear weights (atomics; dx zeroed or pre-filled by the caller),
 *                            doffset [n][18][H][W] = d loss / d offset (overwritten) */
int gencomm_dcn_sample_fwd(const float* x, const float* offset, float* col, int n, int C, int H, int W, void* stream);
int gencomm_dcn_scatter_bwd(const float* x, const float* offset, const float* dcol, float* dx, float* doffset, int n, int C, int H, int W,
                            void* stream);
/* The same with caller-owned scratch of gencomm_dcn_scatter_scratch_floats(n, C, H, W) floats: the input gradient is then formed without
 * global atomics for every bilinear corner within 4 pixels of its sampling pixel's 16 x 16 tile (per-tile regions stored, then summed per
 * output pixel); dx must be zero on entry in both forms. */
long long gencomm_dcn_scatter_scratch_floats(int n, int C, int H, int W);
int gencomm_dcn_scatter_bwd_ws(const float* x, const float* offset, const float* dcol, float* dx, float* doffset, int n, int C, int H, int W,
                               float* scratch, long long scratch_floats, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Sparse 3-D convolutions of the SECOND encoder without spconv (opencood/models/heter_encoders.py:52-81,
 * sub_modules/sparse_backbone_3d.py:33-152, mean_vfe.py:14-33, height_compression.py:10-30). A sparse tensor is
 * (keys int64 [n] ascending, features fp32 [n][C]); key = ((b D + z) H + y) W + x. dims3 = (D, H, W); kernel3 / stride3 /
 * pad3 = (z, y, x). spconv's arithmetic is not part of the reference checkout: parity unpinned, semantics as published
 * (SubMConv3d: output sites = input sites; SparseConv3d: every site whose receptive field holds an active input).
 *   gencomm_sp_index_fwd    coords [n][4] int32 (b, z, y, x) -> keys (sorted) and perm (sorted row -> input row)
 *   gencomm_sp_sites_fwd    output sites of a strided SparseConv3d: out_keys (capacity gencomm_sp_sites_capacity, ascending),
 *                           *n_out (device int)
 *   gencomm_sp_rules_fwd    rulebook nbr [K][n_out] int32: input row of out_coord * stride - pad + offset, -1 if inactive
 *                           (SubMConv3d: out_keys = in_keys, stride 1, pad = k / 2)
 *   gencomm_sp_prepare      weights -> kernel layout; layout 0 = spconv 2.x [Cout][kD][kH][kW][Cin], 1 = spconv 1.x
 *                           [kD][kH][kW][Cin][Cout]; 2 / 3 = the input-gradient convolution of a layout-0 weight (see below)
 *   gencomm_sp_conv_fwd     y[j][co] = act(scale[co] * sum_o sum_ci w[o][ci][co] x[nbr[o][j]][ci] + shift[co]): gather-GEMM on
 *                           v_mfma_f32_32x32x2_f32; scale / shift = folded BatchNorm1d (gencomm_conv2d_fold)
 *   gencomm_sp_dense_fwd    SparseConvTensor.dense(): out [B][C][D][H][W] (zeroed here)
 *   gencomm_mean_vfe_fwd    MeanVFE: out[j] = sum over all point slots of voxel perm[j] / max(num_points, 1)
 * -------------------------------------------------------------------------------------------- */
int gencomm_sp_out_dims(const int* in_dims3, const int* kernel3, const int* stride3, const int* pad3, int* out_dims3);
long long gencomm_sp_index_workspace_bytes(int n);
int gencomm_sp_index_fwd(const int* coords_bzyx, int n, int B, const int* dims3, long long* keys, int* perm,
                         void* workspace, long long workspace_bytes, void* stream);
long long gencomm_sp_sites_capacity(int n_in, const int* kernel3, const int* stride3);   /* entries out_keys must hold */
long long gencomm_sp_sites_workspace_bytes(int n_in, const int* kernel3, const int* stride3);
int gencomm_sp_sites_fwd(const long long* in_keys, int n_in, int B, const int* in_dims3, const int* kernel3, const int* stride3,
                         const int* pad3, long long* out_keys, int* n_out, void* workspace, long long workspace_bytes, void* stream);
int gencomm_sp_rules_fwd(const long long* out_keys, int n_out, const long long* in_keys, int n_in, int B, const int* in_dims3,
                         const int* kernel3, const int* stride3, const int* pad3, int* nbr, void* stream);
long long gencomm_sp_prepared_floats(int K, int Cin, int Cout);
int gencomm_sp_prepare(const float* w, float* prepared, int K, int Cin, int Cout, int layout, void* stream);
int gencomm_sp_conv_fwd(const float* x, const int* nbr, const float* prepared, const float* scale, const float* shift, float* y,
                        int n_out, int K, int Cin, int Cout, int relu, void* stream);
int gencomm_sp_dense_fwd(const float* feat, const long long* keys, int n, int C, int B, const int* dims3, float* out, void* stream);
int gencomm_mean_vfe_fwd(const float* voxels, const int* num_points, const int* perm, float* out, int n, int max_points, int nfeat,
                         void* stream);
/* Training of the sparse layers (stage 1 trains the SECOND encoder): BatchNorm1d over the active rows [n][C] with batch statistics
 * (+ ReLU), forward and backward (as gencomm_bn2d_train_*; C in {16, 32, 64, 128}); gencomm_sp_rules_inv_fwd = inverse rulebook of
 * a strided layer (inv [K][n_in]: the output site that reads input site i through offset o); the input gradient is gencomm_sp_conv_fwd
 * on dy with weights prepared in layout 2 (channels swapped) + the inverse rulebook, or layout 3 (channels swapped, offsets mirrored)
 * + the forward rulebook for SubM layers; gencomm_sp_wgrad accumulates dW in the raw layout 0 [Cout][K][Cin] (<= 64 channels). */
int gencomm_bnrow_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y, float* save,
                            double* scratch, float momentum, float eps, int relu, int n, int C, void* stream);
int gencomm_bnrow_train_bwd(const float* x, const float* y, const float* dy, const float* save, const float* gamma, float* dx, float* dgamma,
                            float* dbeta, double* scratch, int relu, int n, int C, void* stream);
int gencomm_sp_rules_inv_fwd(const long long* in_keys, int n_in, const long long* out_keys, int n_out, int B, const int* in_dims3,
                             const int* kernel3, const int* stride3, const int* pad3, int* inv, void* stream);
int gencomm_sp_wgrad(const float* x, const float* dy, const int* nbr, float* dw, int n_out, int K, int Cin, int Cout, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Lift-Splat-Shoot camera encoder, ABI v12 (opencood/models/heter_encoders.py:83-241, sub_modules/lss_submodule.py:140-233,
 * utils/camera_utils.py:129-246). B agents x N cameras, D depth bins, an fH x fW feature map per camera, C image channels;
 * grid: lo3 = bx - dx / 2, dx3, nx3 = cells along (x, y, z), all three HOST arrays (float32, as the reference's tensors).
 *   gencomm_lss_splat_fwd   get_geometry + get_cam_feats' softmax / lift + voxel_pooling + QuickCumsum + griddify, without the
 *                           lifted tensor: depth_logit [B N][D][fH][fW], feat [B N][C][fH][fW] (image_head output), frustum
 *                           [D][fH][fW][3], rots / intrins / post_rots [B][N][3][3], trans / post_trans [B][N][3] (all device)
 *                           -> out [B][nz C][ny][nx] (channel z C + c, every element written: empty cells are 0);
 *                           cell [B N D fH fW] int32 (may be NULL): the reference's rank x (ny nz B) + y (nz B) + z B + b of each
 *                           frustum point (cell coordinates truncated toward zero, as .long()), -1 outside the grid.
 *                           Scratch: gencomm_lss_workspace_bytes. Three launches + the rocPRIM radix sort; deterministic.
 *   gencomm_lss_depth_target_fwd  depth_gt_indices of depth_supervision (CamEncode*.get_gt_depth_dist, eval mode): channel 3 of
 *                           imgs [BN][Cimg][H][W], clamp_max(d_max), bin_depths (mode 0 UD, 1 LID) picked at downsample / 2 ::
 *                           downsample -> indices int64 [BN][oH][oW] (clamped into [0, num_bins)), mask uint8 (may be NULL): 1
 *                           where the unclamped index was finite and inside [0, num_bins)
 *   gencomm_maxpool3x3s2_fwd  nn.MaxPool2d(3, stride 2, padding 1) on [N][C][H][W] (the ResNet stem)
 * -------------------------------------------------------------------------------------------- */
long long gencomm_lss_workspace_bytes(int B, int N, int D, int fH, int fW, int C, const int* nx3);
int gencomm_lss_splat_fwd(const float* depth_logit, const float* feat, const float* frustum, const float* rots, const float* trans,
                          const float* intrins, const float* post_rots, const float* post_trans, const float* lo3, const float* dx3,
                          const int* nx3, int B, int N, int D, int fH, int fW, int C, float* out, int* cell, void* workspace,
                          long long workspace_bytes, void* stream);
int gencomm_lss_depth_target_fwd(const float* imgs, int BN, int Cimg, int H, int W, int downsample, int mode, float d_min, float d_max,
                                 int num_bins, long long* indices, unsigned char* mask, void* stream);
int gencomm_maxpool3x3s2_fwd(const float* x, float* y, int N, int C, int H, int W, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Training the camera encoder (added within ABI v12).
 *   gencomm_lss_splat_bwd   gradients of gencomm_lss_splat_fwd with respect to depth_logit and feat from grad_out [B][nz C][ny][nx]:
 *                           fwd_workspace = the workspace of the forward call being differentiated (its softmax probabilities
 *                           and pixel-major feature rows are read from it: the caller keeps it untouched until the backward), cell =
 *                           that call's `cell` output -> d_depth_logit [B N][D][fH][fW], d_feat [B N][C][fH][fW] (every element
 *                           written). The camera matrices get no gradient (the reference's .long() cuts that path). D <= 256.
 *                           Scratch: gencomm_lss_splat_bwd_workspace_bytes (the cell-major copy of grad_out). Two launches, no sort,
 *                           no atomics, no memset, no host synchronisation: two runs are bit-identical.
 *   gencomm_maxpool3x3s2_bwd  dx [N][C][H][W] of gencomm_maxpool3x3s2_fwd from x and dy [N][C][Ho][Wo]: every window's dy goes to its
 *                           arg-max (first element in row-major window order with v > m || isnan(v), torch's tie rule); gather, no atomics
 *   gencomm_stem7x7_wgrad   weight gradient dw [Cout][Cin][7][7] of a 7x7 stride-2 pad-3 convolution (Cin <= 3, Cout a multiple of
 *                           64: the ResNet stem) from dy [N][Cout][Ho][Wo] and x [N][Cin][Hi][Wi]; scratch >=
 *                           gencomm_stem7x7_wgrad_scratch_floats floats (partial sums over pixel ranges, added in a fixed order)
 *   gencomm_depth_focal_loss  depth term of PointPillarDepthLoss (FocalLoss, point_pillar_depth_loss.py:105-185, no smoothing, no
 *                           foreground mask): *sum += scale * sum over pixels of -alpha (1 - p_t)^gamma log p_t (float64; the caller
 *                           zeroes it) and grad [BN][D][H][W] = d (that value) / d depth_logit, from depth_logit [BN][D][H][W] and
 *                           target int64 [BN][H][W]; scale = weight / (BN H W). One launch.
 * -------------------------------------------------------------------------------------------- */
long long gencomm_lss_splat_bwd_workspace_bytes(int B, int C, const int* nx3);
int gencomm_lss_splat_bwd(const float* grad_out, const void* fwd_workspace, long long fwd_workspace_bytes, const int* cell, const int* nx3,
                          int B, int N, int D, int fH, int fW, int C, float* d_depth_logit, float* d_feat, void* workspace,
                          long long workspace_bytes, void* stream);
int gencomm_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int N, int C, int H, int W, void* stream);
long long gencomm_stem7x7_wgrad_scratch_floats(int N, int Cin, int Hi, int Wi, int Cout);
int gencomm_stem7x7_wgrad(const float* dy, const float* x, float* dw, int N, int Cin, int Hi, int Wi, int Cout, float* scratch,
                          long long scratch_floats, void* stream);
int gencomm_depth_focal_loss(const float* depth_logit, const long long* target, float* grad, double* sum, int BN, int D, int H, int W,
                             float alpha, float gamma, float scale, void* stream);

/* ----------------------------------------------------------------------------------------------
 * The terms the HEAL and MPDA training criteria add to the detection-head loss (csrc/criteria_kernels.h). Value and gradient per call,
 * two launches each, no atomics: two runs give the same bits, and nothing has to be zeroed by the caller.
 *   gencomm_pyramid_occ_loss  calc_occ_loss of PointPillarPyramidLoss (point_pillar_pyramid_loss.py:69-103) over every pyramid level:
 *                           pos / neg [B][H][W][A] float32 (A >= 2; anchors 0 and 1 are read), occ / grad: host arrays of `levels`
 *                           (1..4) device pointers, level i [B][1][H / k_i][W / k_i] with k_i = relative_downsample[i] (host array;
 *                           max_pool2d floors), weight: host array [levels]. Labels of a level cell: positive if any cell of its
 *                           k x k window is positive on anchor 0 or 1, negative if every cell is negative on both; per (sample, level)
 *                           norm = max(#positive, 1); sigmoid focal loss (gamma, alpha) with cell weight (pos * pos_cls_weight + neg) /
 *                           norm; level loss = sum / B * weight[i]. sums: 5 + 8 B doubles (device): [0] total, [1..4] level losses
 *                           (0 beyond `levels`), the rest scratch. grad_i = d total / d occ_i, every element written once.
 *   gencomm_domain_bce_loss   the domain term of PointPillarMPDALoss (point_pillar_mpda_loss.py:124-150): x / grad [N][C][H][W]; target 1
 *                           for the agents named in source_index (host array [num_sources], the first agent of every scene), 0
 *                           elsewhere; sums: 1 + 32 N doubles (device): [0] mean over N C H W of max(x, 0) - x t + log1p(exp(-|x|)),
 *                           the rest scratch; grad = (sigmoid(x) - t) / (N C H W). N <= 1024.
 * -------------------------------------------------------------------------------------------- */
int gencomm_pyramid_occ_loss(const float* pos, const float* neg, const float* const* occ, float* const* grad, const int* relative_downsample,
                             const float* weight, int levels, int B, int H, int W, int A, float pos_cls_weight, float gamma, float alpha,
                             double* sums, void* stream);
int gencomm_domain_bce_loss(const float* x, const int* source_index, int num_sources, float* grad, double* sums, int N, int C, int H, int W,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GENCOMM_HIP_H */
