/*
 * libsatrender -- C ABI of the MI355X-native Sat-NeRF volumetric-rendering hot path.
 *
 * The reference (centreborelli/satnerf) is pure Python/PyTorch and has no FFI; each entry point below
 * replaces the ATen op sequence of the reference lines it cites (paths relative to the reference
 * repository root).  The host side (the satnerf_amd Python package) binds these with ctypes; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory owned by the caller (PyTorch); the library
 *     borrows it for the duration of the enqueue and allocates nothing;
 *   - all tensors fp32, contiguous, row-major unless stated; `ts` is int64;
 *   - `stream` is a hipStream_t (0 = default stream); calls only enqueue, they never synchronise;
 *   - return value 0 = ok, non-zero = error, text via sr_last_error() (thread-local);
 *   - gfx950 (MI355X) only.
 */
#ifndef SATRENDER_H
#define SATRENDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR_VERSION 200 /* major*10000 + minor*100 + patch; while major is 0 an incompatible signature change bumps minor */

/* numeric modes of the fused MLP (SURVEY.md section 7 "Hard parts") */
#define SR_MODE_BF16 1   /* single-pass bf16 MFMA, fp32 accumulate -- throughput mode            */
#define SR_MODE_BF16X3 3 /* hi*hi + lo*hi + hi*lo split on the same MFMA pipe -- parity mode (~2e-6) */
#define SR_MODE_F16 2    /* single-pass fp16 MFMA, fp32 accumulate: the throughput of SR_MODE_BF16 with 11-bit operands (~1.5e-4);
                            forward only -- weights and activations are O(1) here; the backward kernels stay bf16 -- widths 256 and 512,
                            stream_hi then holds fp16 (sr_pack_stream / sr_pack_all `n_f16`); the training workspaces keep their (bf16 / 8-bit) formats */

/* formats of the training workspaces the forward / dX / weight-gradient kernels exchange through HBM:
 * 16 = unorm16 phase / bf16 (the parity mode's backward), 8 = one byte per value (PHASE8 / micro-scaled int8): half the
 * bytes of a training step, used by the throughput mode */
#define SR_FMT16 16
#define SR_FMT8 8

int sr_version(void);
const char* sr_last_error(void);

/* ---- stream geometry (host-side, no GPU needed) -------------------------------------------------
 * The fused MLP consumes its weights as one linear "stream" of 1-KiB MFMA-A-fragment pieces in
 * consumption order.  These return the element counts the host packer
 * (satnerf_amd/packing.py) must produce for a given network shape; -1 on an unsupported shape. */
int64_t sr_fwd_stream_elems(int feat, int tau);  /* bf16 elements of the forward stream (per hi/lo plane) */
int64_t sr_bwd_stream_elems(int feat, int tau);  /* bf16 elements of the transposed (dX) stream          */
/* training workspaces, per 32-point tile, in 16-bit elements, for a workspace format `fmt` (below) */
int64_t sr_act_elems_per_tile(int feat, int fmt);   /* activations saved by the forward pass          */
int64_t sr_dpre_elems_per_tile(int feat, int fmt);  /* pre-activation gradients written by the dX pass */
/* tiles both workspaces must hold for n_points points: ceil(n_points / 32) rounded up to the 8 tiles of a workgroup -- the forward and
 * dX kernels run whole workgroups, and the waves past the last point still store their (unused) tile */
int64_t sr_workspace_tiles(int64_t n_points);
/* 16-bit elements of the WHOLE dpre workspace for n_points points = sr_workspace_tiles * sr_dpre_elems_per_tile, plus (SR_FMT8) the table
 * of exponent maxima the dX pass leaves behind the last tile for the weight-gradient pass: 16 bytes per 4 tiles, byte g = the largest MX8
 * exponent byte of scale group g over those tiles (csrc/mlp_layout.h), rounded up to whole KiB.  -1 on an unsupported shape. */
int64_t sr_dpre_workspace_elems(int64_t n_points, int feat, int fmt);

/* ---- weight packing:  replaces nothing in the reference (its weights feed addmm directly) ---------
 * out_hi[i] = bf16_rne(src[idx[i]] * scale[i]);  out_lo[i] = bf16_rne(src[idx[i]]*scale[i] - out_hi[i])
 * (out_lo may be NULL).  idx < 0 selects the constant 0. */
int sr_pack_stream(const float* src, const int32_t* idx, const float* scale, int64_t n,
                   uint16_t* out_hi, uint16_t* out_lo, int64_t n_f16, void* stream);
/* n_f16: the first n_f16 elements of out_hi are written as fp16 instead of bf16 (the forward stream of SR_MODE_F16; even) */
/* the same plus an fp32 gather (sr_gather_scale_f32) in ONE launch: the forward stream, the backward stream (concatenated
 * maps) and the fc_net.0 table are refreshed together after every optimizer step; `tick` (may be NULL) is a 1-float device
 * counter the launch increments: the step count sr_adam_step_graph reads later in the same captured graph */
int sr_pack_all(const float* src, const int32_t* idx, const float* scale, int64_t n, uint16_t* out_hi, uint16_t* out_lo,
                const int32_t* f32_idx, const float* f32_scale, int64_t n_f32, float* out_f32, float* tick, int64_t n_f16,
                void* stream);

/* out[i] = src[idx[i]] * scale[i] in fp32 (idx < 0 -> 0): builds the fc_net.0 table `l0` of sr_satnerf_mlp_fwd */
int sr_gather_scale_f32(const float* src, const int32_t* idx, const float* scale, int64_t n, float* out, void* stream);

/* grad[e] (+)= gscale[e] * (sum over the split-K slices of partial element gidx[e])  (gidx < 0: left untouched) -- reduces
 * the slices of sr_satnerf_wgrad (`blocks` = its planned job table, device) and scatters into the flat parameter-gradient
 * buffer (inverse of sr_pack_stream's gather) */
int sr_unpack_grads(const float* partial, const int32_t* gidx, const float* gscale, int64_t n_params, const int32_t* blocks,
                    float* grad, int accumulate, void* stream);

/* ---- stratified sampling: rendering.py:62-78 -----------------------------------------------------
 * rays (N, ray_stride>=8) with near at column 6, far at column 7; u (N,S) in [0,1) -> z_vals (N,S). */
int sr_ray_sample_fwd(const float* rays, int ray_stride, const float* u, int64_t n_rays, int n_samples,
                      float* z_vals, void* stream);

/* ---- sky-colour head, once per ray: models/satnerf.py:138-143,201 ---------------------------------
 * sun (N, sun_stride) -> sky (N,3) = sigmoid(W2 relu(W1 sun + b1) + b2);  W1 (H,3) b1 (H) W2 (3,H) b2 (3) */
int sr_sky_fwd(const float* sun, int sun_stride, int64_t n, int hidden, const float* w1, const float* b1,
               const float* w2, const float* b2, float* sky, void* stream);

/* ---- fused SatNeRF MLP over points: models/satnerf.py:20-40 (repeat_interleave + chunk loop) and
 *      SatNeRF.forward models/satnerf.py:156-208 (+ Siren models/nerf.py:23-33) ------------------------
 * point p (0 <= p < n_points) belongs to row r = p / n_samples of the per-ray arrays:
 *   xyz   = org[r] + dir[r] * z[p]           (rendering.py:81; dir==NULL or z==NULL -> xyz = org[r])
 *   sun_d = sun[r],  t = temb[ts ? ts[r] : r]  (rendering.py:99-100, nn.Embedding lookup)
 * outputs (any may be NULL): albedo (P,3), sigma (P), sun_v (P), beta (P)   [models/satnerf.py:45-49]
 * stream_hi/lo: packed forward stream from sr_pack_stream (lo required iff mode == SR_MODE_BF16X3)
 * l0: (feat,4) fp32 rows [w_x, w_y, w_z, b] of fc_net.0, each multiplied by 30/(2*pi), in slot order
 * acts: NULL, or training workspace of sr_act_elems_per_tile(feat, act_fmt) * sr_workspace_tiles(P) 16-bit elements, written in the
 * format act_fmt (SR_FMT8 needs mode == SR_MODE_BF16; act_fmt is ignored when acts == NULL). */
typedef struct sr_mlp_inputs {
  const float* org;
  int org_stride;
  const float* dir;
  int dir_stride;
  const float* sun;
  int sun_stride;
  const float* z;
  const float* temb;
  const int64_t* ts;
  int64_t n_points;
  int n_samples;
} sr_mlp_inputs;

int sr_satnerf_mlp_fwd(const sr_mlp_inputs* in, int feat, int tau, int mode, const uint16_t* stream_hi,
                       const uint16_t* stream_lo, const float* l0, float* albedo, float* sigma, float* sun_v,
                       float* beta, uint16_t* acts, int act_fmt, void* stream);

/* ---- one-launch render pass (no grad): rendering.py:62-81 (stratified sampling) -> models/satnerf.py:20-49 (the MLP over
 *      every sample) -> models/satnerf.py:52-70 (compositing) + the per-ray sky head (:138-143) -- the same arithmetic as
 *      sr_ray_setup -> sr_satnerf_mlp_fwd -> sr_composite_fwd, bit for bit, with the per-point values handed from the MLP to
 *      the compositing through LDS: a workgroup owns sr_render_points_per_block(feat, mode) consecutive points = whole rays,
 *      so n_samples must divide that number (64 and 128 do; other S: use the three separate launches).
 * rays (N, ray_stride >= 11) = o d near far sun; ts (N) image indices into temb (vocab, tau).
 * depths: z_in (N,S) given (the fine pass), else stratified with jitter u (N,S), else (both NULL) with jitter drawn in the kernel:
 *   Philox keyed by `seed`, stepping with step_counter[0]; tick != 0: the launch advances that counter (see sr_ray_setup_rng).
 * noise (N,S) or NULL with noise_std; sky_*: the sky head's weights (hidden, 3), (hidden), (3, hidden), (3).
 * bank_chunks > 0: `rays` / `ts` are a resident bank of bank_chunks x N rows and the launch renders chunk
 *   (step_counter[0] mod bank_chunks) of it -- with tick, a captured launch walks the bank chunk by chunk, replay after
 *   replay, as eval_satnerf.py:46-66 walks an image, with no host work and no gather in between (outputs: the chunk's N rays).
 * outputs: z_out (N,S) [NULL ok], albedo (N,S,3), sun_v (N,S), beta (N,S), sigma (N,S) [NULL ok], sky (N,3), weights (N,S),
 *   transparency (N,S), depth (N), rgb (N,3) clamped to [0,1]. */
typedef struct sr_render_args {
  const float* rays;
  int ray_stride;
  const int64_t* ts;
  const float* temb;
  int64_t n_rays;
  int n_samples;
  const float* z_in;
  const float* u;
  uint64_t seed;
  float* step_counter;
  int tick;
  const float* noise;
  float noise_std;
  int sky_hidden;
  const float* sky_w1;
  const float* sky_b1;
  const float* sky_w2;
  const float* sky_b2;
  int64_t bank_chunks;
} sr_render_args;

typedef struct sr_render_outputs {
  float* z_vals;
  float* albedo;
  float* sigma;
  float* sun_v;
  float* beta;
  float* sky;
  float* weights;
  float* transparency;
  float* depth;
  float* rgb;
} sr_render_outputs;

int sr_satnerf_render_fwd(const sr_render_args* in, int feat, int tau, int mode, const uint16_t* stream_hi, const uint16_t* stream_lo,
                          const float* l0, const sr_render_outputs* out, void* stream);
/* points a workgroup of the fused kernel owns (256 / 128), or -1 when (feat, mode) has no fused build */
int sr_render_points_per_block(int feat, int mode);

/* ---- depth-only ("geometry") render pass in ONE launch: rendering.py:62-81 -> the model's sigma_only cut, models/satnerf.py:183-185
 *      (fc_net and sigma_from_xyz, no feats, no colour / sun / uncertainty head) -> the sigma -> alpha -> weights -> depth half of
 *      models/satnerf.py:52-67; no sky head (:138-143), no rgb.  With SR_MODE_BF16 / SR_MODE_F16 the launch runs the trunk-and-sigma core,
 *      which reads the SAME packed stream as sr_satnerf_render_fwd (it jumps over the feats pieces) and none of the sky weights (sky_* may
 *      be NULL); depth, weights, transparency, z_vals and sigma are those of sr_satnerf_render_fwd on the same inputs, bit for bit.
 *      SR_MODE_BF16X3, and every mode under SATNERF_FWD_V1=1, run the full kernel with the unused outputs NULL (then sky_* are required).
 * Reads and writes only these fields of `out`: z_vals (N,S) [NULL ok], sigma (N,S) [NULL ok], weights (N,S), transparency (N,S), depth (N).
 * Preconditions as sr_satnerf_render_fwd: n_samples >= 2 and n_samples divides sr_render_points_per_block(feat, mode); tick is 0 or 1. */
int sr_satnerf_render_depth(const sr_render_args* in, int feat, int tau, int mode, const uint16_t* stream_hi, const uint16_t* stream_lo,
                            const float* l0, const sr_render_outputs* out, void* stream);

/* ---- sigma of the fused MLP over points: SatNeRF.forward(..., sigma_only=True), models/satnerf.py:183-185, as the point launch
 *      sr_satnerf_mlp_fwd (same inputs, stream and l0) restricted to the trunk and the sigma row: sigma (P), bit-equal to that launch's. */
int sr_satnerf_mlp_sigma(const sr_mlp_inputs* in, int feat, int tau, int mode, const uint16_t* stream_hi, const uint16_t* stream_lo,
                         const float* l0, float* sigma, void* stream);

/* ---- the training forward in ONE launch: replaces main.py:60-75,127 + metrics.py:21-25,36-44,56-73 + autograd through the compositing ---
 * sr_satnerf_render_train = sr_ray_setup + sr_satnerf_mlp_fwd (saving the SR_FMT8 activations) + sr_render_loss: the render pass above
 * with, in its epilogue, the colour loss (SatNerfLoss; SNerfLoss while sched[2] != 0) and the closed-form compositing backward of every
 * ray by the wave that composited it (same per-ray function as sr_render_loss: bit-identical to the three launches).  n_samples <= 64,
 * SR_MODE_BF16 / SR_MODE_F16, widths 256 and 512.  `out`: albedo / sigma / sun_v / beta (N,S[,3]) and sky (N,3) are required (the dX
 * pass and the sky head's backward read them), z_vals optional, weights / transparency / depth / rgb unused.  `train` outputs: loss_parts
 * (one per workgroup = ceil(N * S / sr_render_points_per_block) floats: the loss is their sum), rgb (N,3) or NULL, d_sigma (N,S),
 * d_albedo (N,S,3), d_sun_v (N,S), g_beta (N,S), d_sky (N,3).  acts: the SR_FMT8 workspace of sr_satnerf_mlp_fwd.
 * r05, the batch sampler inside the launch (replaces the DataLoader of main.py:96-110 as sr_gather_batch does, without its launch):
 * gather_idx != NULL: `in->rays` (stride 11), `in->ts` and `target` are the RESIDENT RAY BANK, gather_idx holds the shuffled row indices
 * of a whole epoch = `batches` x N entries, and the launch trains on batch cursor[0] of it -- ray r of the launch is bank row
 * gather_idx[cursor[0] * N + r] -- then moves the cursor on modulo `batches` (cursor = a 4-float block as sr_gather_batch's).  The wave
 * that composites a ray also copies its row to out_rays (N,11) / out_rgbs (N,3) / out_ts (N): the batch as the later launches of the
 * step (sky-head and embedding gradients, solar-correction pass) read it.
 * in->tick == 2 ("tick first", training launches only): the launch advances the step counter as tick == 1 does AND draws its jitter for
 * the advanced value -- it is the first launch of a step that has no sr_pack_all in front of it to tick. */
typedef struct sr_train_args {
  const float* target;   /* (N,3), or the bank's colours (rows, 3) with gather_idx */
  const float* sched;    /* 4-float schedule block or NULL */
  float beta_min;
  float* loss_parts;
  float* rgb;
  float* d_sigma;
  float* d_albedo;
  float* d_sun_v;
  float* g_beta;
  float* d_sky;
  const int64_t* gather_idx;
  float* cursor;
  int64_t batches;
  float* out_rays;
  float* out_rgbs;
  int64_t* out_ts;
} sr_train_args;
int sr_satnerf_render_train(const sr_render_args* in, int feat, int tau, int mode, const uint16_t* stream_hi, const uint16_t* stream_lo,
                            const float* l0, const sr_render_outputs* out, const sr_train_args* train, uint16_t* acts, int act_fmt, void* stream);

/* ---- backward of the fused MLP: replaces autograd through SatNeRF.forward (models/satnerf.py:156-208) ------------
 * sr_satnerf_mlp_bwd: data-gradient chain.  Inputs: the forward's saved `acts`, its four outputs and the gradients of
 * those outputs (g_* may be NULL = 0); bwd_stream = packed transposed weights (sr_pack_stream with
 * packing.backward_maps).  Outputs: dpre (sr_dpre_workspace_elems(P, feat, fmt) 16-bit elements) and d_t (P,tau)
 * fp32, the gradient w.r.t. each point's embedding vector (NULL to skip).  `fmt` = format of BOTH workspaces.
 * sr_satnerf_wgrad: weight-gradient GEMMs dpre x acts over all points.  `blocks` (n_blocks x 12 int32, device) lists the job
 * blocks (rf0 nr0 rf1 nr1 | cf0 nc0 cf1 nc1 | col_kind n_slices first_slice -: up to two ranges of dpre row fragments and of
 * activation column fragments, <= 16 each; packing.backward_maps); every block is cut into n_slices contiguous ranges of
 * 32-point tiles (split-K), one workgroup each, writing slice s to partial + s * (256*256 + 256*32) floats; reduce with
 * sr_unpack_grads.
 * sr_wgrad_plan (host, no GPU work): fills n_slices / first_slice of a HOST copy of the table for n_points points and at
 * most n_wg workgroups (n_wg <= 0: the current device's CU count); *n_slices = total slices.  `fmt` = the workspace format of
 * the kernel that will run the plan: SR_FMT16 cuts every block into the same number of slices (that kernel's time per tile
 * does not depend on the block), SR_FMT8 hands the workgroups out by a per-block cost x tiles (equal costs for the default 4-wave
 * kernel; SATNERF_WGRAD_V1=1: the r02 kernel's decode work grows with the fragments a block moves). */
int sr_satnerf_mlp_bwd(int feat, int tau, int64_t n_points, const uint16_t* bwd_stream, const uint16_t* acts,
                       const float* albedo, const float* sigma, const float* sun_v, const float* beta, const float* g_albedo,
                       const float* g_sigma, const float* g_sun_v, const float* g_beta, uint16_t* dpre, float* d_t, int fmt,
                       void* stream);
int sr_wgrad_plan(int32_t* blocks, int n_blocks, int64_t n_points, int n_wg, int fmt, int* n_slices);
int sr_satnerf_wgrad(int feat, int tau, int64_t n_points, const uint16_t* dpre, const uint16_t* acts, const int32_t* blocks,
                     int n_blocks, int n_slices, float* partial, void* stream);
/* the same contraction from SR_FMT8 workspaces (autograd's grad_weight / grad_bias of every nn.Linear, models/satnerf.py:104-153).
 * Default kernel (csrc/wgrad9.hip): 4 waves per job block, each wave decodes its 8-bit double fragments in registers (PHASE8 -> fp16
 * sine, MX8 -> fp16 value scaled per workgroup) and contracts 128 x 128 register tiles with fp16 MFMAs; SATNERF_WGRAD_V1=1 (and
 * workspaces of 4 GiB or more) run the r02 kernel, which expands the fragments in the LDS to bf16.  `loads` (n_blocks x
 * sr_wgrad8_load_ints() int32, device; packing.wgrad8_loads) says which unit of which workspace each wave of a block fetches and where
 * it goes -- ints 0..19 for the r02 kernel, 20..112 the duty table, the exponent groups of the row pairs, the quadrant mask and the per-wave stream variants (r06: thin streams for one-row blocks) of the default one
 * (which reads the exponent maxima behind the dpre workspace: dpre must be the buffer sr_satnerf_mlp_bwd wrote, sr_dpre_workspace_elems long); `blocks` is
 * the same planned table.  sr_wgrad_plan hands the default kernel equal slices (it runs one instruction stream for every block) and the
 * r02 kernel cost-weighted ones.
 * plan_span = int 11 of the planned table's first row (sr_wgrad_plan): 0 = one slice per workgroup; > 0 = a stream-K plan (the 4-wave kernel
 * walks `plan_span` tile units of the block-major job list per workgroup, writing one partial block per block it touches). */
/* dpre_elems = 16-bit elements the caller's dpre buffer holds: rejected below sr_dpre_workspace_elems(n_points, feat, SR_FMT8) */
int sr_satnerf_wgrad8(int feat, int tau, int64_t n_points, const uint16_t* dpre, int64_t dpre_elems, const uint16_t* acts,
                      const int32_t* blocks, const int32_t* loads, int n_blocks, int n_slices, int plan_span, float* partial, void* stream);
int sr_wgrad8_load_ints(void);

/* parameter gradients of the sky head (atomicAdd into g_*; zero them first) and of the embedding table
 * g_emb[ts[r]] += sum_j d_t[r*S + j] (nn.Embedding backward, rendering.py:100) */
int sr_sky_bwd(const float* sun, int sun_stride, int64_t n, int hidden, const float* w1, const float* b1, const float* w2,
               const float* sky, const float* d_sky, float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* stream);
int sr_embedding_bwd(const float* d_t, const int64_t* ts, int64_t n_rays, int n_samples, int tau, float* g_emb, void* stream);

/* ---- fused fast-path launches of the training step (same arithmetic as the separate entry points) -------------------
 * sr_ray_setup = sr_ray_sample_fwd + sr_sky_fwd (rays need >= 11 columns);
 * sr_render_loss = sr_composite_fwd -> sr_satnerf_loss -> sr_composite_bwd for n_samples <= 64, one wave per ray:
 *   outputs the MLP-backward inputs d_sigma (N,S), d_albedo (N,S,3), d_sun_v (N,S), g_beta (N,S), the per-ray d_sky (N,3),
 *   the loss partial sums (ceil(N/4)) and optionally the rendered rgb (N,3). */
/* sr_depth_loss: metrics.DepthLoss for the coarse model (metrics.py:75-92; main.py:134-141): value = sum(loss_parts[0 ..
 * ceil(N/256))) = lambda_ds/3 * mean(w * (depth - target)^2), g_depth (N) its gradient; depths (N, stride) = [target, weight, ...],
 * use_weights = 0 is --ds_noweights. */
/* sr_sc_loss: the solar-correction terms of SNerfLoss / SatNerfLoss (metrics.py:27-34) for the pass rendered along the sun
 * direction (rendering.py:102-108): compositing of that pass (z_vals, sigma[, noise]) -> value = sum(loss_parts[0 .. ceil(N/4))) =
 * lambda_sc/3 * (mean_r sum_j (T_j - sun_j)^2 + mean_r (1 - sum_j w_j sun_j)), d_sun_v (N,S) its gradient (T, w detached). */
int sr_sc_loss(const float* z_vals, const float* sigma, const float* noise, float noise_std, const float* sun_v, int64_t n_rays,
               int n_samples, float lambda_sc, float* loss_parts, float* d_sun_v, void* stream);
int sr_depth_loss(const float* depth, const float* depths, int depths_stride, int use_weights, int64_t n_rays, float lambda_ds,
                  float* loss_parts, float* g_depth, void* stream);
int sr_ray_setup(const float* rays, int ray_stride, const float* u, int64_t n_rays, int n_samples, int hidden, const float* w1,
                 const float* b1, const float* w2, const float* b2, float* z_vals, float* sky, void* stream);
/* the same with the stratified jitter u ~ U[0,1) (rendering.py:77) drawn INSIDE the kernel: Philox-4x32-10 keyed by `seed`,
 * counter = (ray, sample, step) with the step read from the device counter `step_counter[0]` (NULL = 0; the counter
 * sr_pack_all ticks) -- a captured training step then needs no RNG launch.  tick != 0: this launch also advances the counter
 * (captured forward passes have no sr_pack_all): `step_counter` is then a 4-float block as `sched`, [0] += 1 once every
 * workgroup has read it, [3] is scratch (an arrival counter, zero-initialised by the caller) */
int sr_ray_setup_rng(const float* rays, int ray_stride, uint64_t seed, float* step_counter, int tick, int64_t n_rays, int n_samples,
                     int hidden, const float* w1, const float* b1, const float* w2, const float* b2, float* z_vals, float* sky,
                     void* stream);
int sr_render_loss(const float* z_vals, const float* sigma, const float* noise, float noise_std, const float* albedo,
                   const float* sun_v, const float* beta, const float* sky, const float* target, int64_t n_rays, int n_samples,
                   float beta_min, const float* sched, float* loss_parts, float* rgb, float* d_sigma, float* d_albedo, float* d_sun_v,
                   float* g_beta, float* d_sky, void* stream);

/* `sched` (NULL = none) is the DEVICE-side schedule block of a captured training step, 4 floats the host updates between graph
 * replays: [0] 1-based optimizer step (ticked by sr_pack_all), [1] learning rate (sr_adam_step_graph with lr < 0 reads it:
 * StepLR(gamma 0.9) per epoch, main.py:86-94 / train_utils.py:41-57), [2] != 0 while the SNerfLoss warm-up lasts (the colour loss
 * is then the plain MSE of metrics.SNerfLoss, main.py:128-131 -- no beta term, no beta gradient), [3] reserved.
 * sr_adam_step_graph = sr_adam_step with the 1-based step count read from the device (state[0], advanced by sr_pack_all's
 * `tick` earlier in the same step) so the launch can be replayed from a hipGraph. */
/* `pack` of the launches that also keep the weight streams current (r05; NULL or pack->map == NULL: none): the thread that updated
 * parameter i writes it to its (at most two) places in the packed streams, so the next step needs no sr_pack_all launch.  The value
 * written is param * scales[index], the element-wise arithmetic of sr_pack_all: the streams hold the same bits as a fresh sr_pack_all. */
typedef struct sr_pack_scatter {
  const int32_t* map; /* 2 int32 per parameter (packing.pack_scatter_map): position | scale index << 26 | (1 << 28: the fp32 table `l0`), -1 = none */
  uint16_t* hi;       /* the stream the positions address: bf16; fp16 below n_f16 */
  uint16_t* lo;       /* the bf16x3 remainder plane, or NULL */
  float* l0;          /* the fp32 fc_net.0 table */
  int64_t n_f16;      /* as sr_pack_all's n_f16 */
  float scales[4];
} sr_pack_scatter;
/* The gradient tail, the last launch of a training step: sr_unpack_grads + sr_sky_bwd + sr_embedding_bwd as three block ranges of ONE
 * launch.  sr_grad_tail_args holds what its four entries share. */
typedef struct sr_grad_tail_args {
  const float* partial;  /* the split-K slices sr_satnerf_wgrad[8] wrote */
  const int32_t* gidx;   /* (n_params) as sr_unpack_grads: where parameter i's sum lives in a slice; < 0 = no weight-gradient GEMM produces it */
  const float* gscale;   /* (n_params) as sr_unpack_grads: the factor on parameter i's sum */
  int64_t n_params;
  const int32_t* blocks; /* the planned job table (sr_wgrad_plan), device */
  int n_blocks;          /* its rows, >= 1 */
  float* grad;           /* (n_params) flat gradient buffer */
  int accumulate;        /* != 0: add to what `grad` holds (the solar-correction / depth-supervision passes of the step), 0: overwrite */
  const float* sun;      /* (n_rays, >= 3) sun directions of the batch, the sky head's input (sr_sky_bwd) */
  int sun_stride;        /* row stride of `sun` in floats */
  int64_t n_rays;        /* rays of the batch; <= 0: nothing is launched */
  int hidden;            /* width of the sky head */
  const float* w1;       /* sky head: (hidden, 3) */
  const float* b1;       /*           (hidden)    */
  const float* w2;       /*           (3, hidden) */
  const float* sky;      /* (n_rays, 3) the head's output */
  const float* d_sky;    /* (n_rays, 3) its gradient */
  float* g_w1;           /* the head's parameter gradients, added to (atomics, or in a fixed order by the _det entries) */
  float* g_b1;
  float* g_w2;
  float* g_b2;
  const float* d_t;      /* (n_rays * n_samples, tau) gradient w.r.t. each point's embedding vector (sr_satnerf_mlp_bwd) */
  const int64_t* ts;     /* (n_rays) embedding row of each ray */
  int n_samples;
  int tau;
  float* g_emb;          /* (rows, tau) g_emb[ts[r]] += sum_j d_t[r * n_samples + j] (sr_embedding_bwd) */
} sr_grad_tail_args;
/* The optimizer half of sr_grad_tail_adam[_det] = sr_grad_tail + sr_adam_step_graph in one launch (the single-GPU captured step): the
 * thread that reduces a parameter's slices applies torch.optim.Adam to it and zeroes its gradient slot. */
typedef struct sr_tail_adam_args {
  float* params;           /* flat buffers aligned with `grad`: element i of all four is parameter i */
  float* exp_avg;
  float* exp_avg_sq;
  const int32_t* late_idx; /* (n_late) flat indices relative to `grad` of the parameters whose gradients arrive from OTHER blocks (the sky head,
                              the embedding rows): the last of those blocks to finish updates them */
  int n_late;              /* >= 0; late_idx may be NULL only when it is 0 */
  float* state;            /* the 4-float schedule block: [0] 1-based step, [1] rate used when lr < 0, [3] arrival counter, zero between launches */
  float lr;                /* < 0: read state[1] */
  float beta1;
  float beta2;
  float eps;
  float grad_scale;
  const sr_pack_scatter* pack; /* NULL or pack->map == NULL: none; pack->map holds n_params x 2 words */
} sr_tail_adam_args;
int sr_grad_tail(const sr_grad_tail_args* args, void* stream);
int sr_grad_tail_adam(const sr_grad_tail_args* args, const sr_tail_adam_args* adam, void* stream);
int sr_adam_step_graph(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                       float beta2, float eps, float grad_scale, float* state, int zero_grad, void* stream);

/* ---- fixed-order sky and embedding gradients (deterministic training steps) ---------------------------------------------------------
 * sr_sky_bwd, sr_embedding_bwd and the two tail launches add per-block / per-ray sums into g_* with float atomics: the order the sums land
 * in, and so the last bits of these gradients, depend on scheduling.  The *_det twins below store the SAME sums into caller-provided scratch
 * and let the last block to arrive add them up in a fixed order -- fp32 adds only, no FMA:
 *   sky parameter i:            acc = 0.0f; for b = 0 .. n_sky_blocks-1: acc += sky_part[b][i];                        g[i] += acc
 *   embedding element (row, c): acc = 0.0f; for r = 0 .. n_rays-1, increasing, where ts[r] == row: acc += emb_part[r][c];  g_emb[row][c] += acc
 * Rows of g_emb that no ray names are not touched.  The arrival is the one the HIP memory model asks for (workgroup barrier, one thread's
 * agent-scope acq_rel fetch_add, barrier); the last arriver resets the counter.
 * Scratch, in 4-byte words (the library owns no memory: the caller allocates it 16-byte aligned, zeroes word 0 ONCE and may reuse the buffer
 * for every launch; launches sharing a scratch must be ordered, e.g. on one stream):
 *   [0]      arrival counter (uint32; zero between launches), [1..3] padding to 16 bytes
 *   sky_part n_sky_blocks = ceil(n_rays / 32) rows of 7 * hidden + 3 floats; row b = the sums of rays [32 b, 32 b + 32) in the order of the
 *            head's parameters: g_w1 (hidden x 3, row-major) | g_b1 (hidden) | g_w2 (3 x hidden, row-major) | g_b2 (3)
 *   emb_part n_rays x tau floats: emb_part[r][c] = sum_j d_t[r][j][c]
 *   first    n_rays uint32: 1 where no earlier ray of the batch names ray r's row (where the reduction starts that row's chain), else 0
 * sr_late_grad_scratch_bytes (host only) = 4 * (4 + n_sky_blocks * (7 * hidden + 3) + n_rays * tau + n_rays); -1 for n_rays < 0, hidden < 1
 * or tau < 1.  Every word behind the counter is rewritten by each launch.
 * sr_sky_bwd_det / sr_embedding_bwd_det replace sr_sky_bwd / sr_embedding_bwd (same arguments, plus the scratch and its size in bytes).  A
 * stand-alone launch has only its own part: sr_sky_bwd_det reads the scratch as [counter | sky_part], sr_embedding_bwd_det as [counter |
 * emb_part | first]; a buffer of sr_late_grad_scratch_bytes is large enough for either.
 * sr_grad_tail_det replaces sr_grad_tail: the same three block ranges, the sky and embedding ranges storing partials; the last of THEIR blocks
 * to arrive (counter: scratch word 0) reduces in order into g_*.  The split-K range is sr_grad_tail's.
 * sr_grad_tail_adam_det replaces sr_grad_tail_adam: the last arriver (counter: state[3], as sr_grad_tail_adam; scratch word 0 is not used)
 * reduces in order and then updates the `late_idx` parameters from the reduced gradients; the split-K / Adam / re-pack range is
 * sr_grad_tail_adam's.  Results repeat bit for bit per box and per switch setting (sr_wgrad_plan depends on the CU count). */
int64_t sr_late_grad_scratch_bytes(int64_t n_rays, int hidden, int tau);
int sr_sky_bwd_det(const float* sun, int sun_stride, int64_t n, int hidden, const float* w1, const float* b1, const float* w2,
                   const float* sky, const float* d_sky, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* scratch,
                   int64_t scratch_bytes, void* stream);
int sr_embedding_bwd_det(const float* d_t, const int64_t* ts, int64_t n_rays, int n_samples, int tau, float* g_emb, float* scratch,
                         int64_t scratch_bytes, void* stream);
int sr_grad_tail_det(const sr_grad_tail_args* args, float* scratch, int64_t scratch_bytes, void* stream);
int sr_grad_tail_adam_det(const sr_grad_tail_args* args, const sr_tail_adam_args* adam, float* scratch, int64_t scratch_bytes,
                          void* stream);
/* sr_adam_step_graph that also re-packs (r06: the data-parallel step = the single-GPU step + one collective): Adam on all n elements of
 * the flat buffers, and each of the first n_packed parameters (the coarse model's; `pack->map` holds n_packed x 2 words) written into its
 * places of the weight streams as sr_grad_tail_adam does.  Sequence at N > 1: ... sr_grad_tail | all-reduce of `grads` | sr_adam_step_pack
 * -- no sr_pack_all, no separate update launch.  pack may be NULL (n_packed 0): plain sr_adam_step_graph arithmetic. */
int sr_adam_step_pack(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                      float eps, float grad_scale, float* state, int zero_grad, int64_t n_packed, const sr_pack_scatter* pack,
                      void* stream);

/* ---- layer-by-layer path for widths the fused kernel does not cover (fc_units != 256; opt.py:50 defaults to 512) ----
 * One nn.Linear of models/satnerf.py:104-153 per call, its input being the concatenation of one or two sources with the
 * PREVIOUS layer's activation applied on load (tensors between layers are pre-activations):
 *   acat[p][f] = act_s(src_s.x[(p / row_div_s) * ld_s + f - off_s]),  act = none | sin(w0 x) (Siren, models/nerf.py:23-33) | relu
 *   sr_linear_fwd:        y[p][n] = out_act(sum_f acat[p][f] * weight[n][f] + bias[n])          (weight (n_out, K) row-major)
 *   sr_linear_bwd_input:  d_src[p][k] = (sum_n G[p][n] * weight[n][col0 + k]) * act'(target.x[p][k])   (autograd grad_input)
 *   sr_linear_bwd_weight: d_weight[n][f] += sum_p G[p][n] * acat[p][f],  d_bias[n] += sum_p G[p][n]     (fp32 atomics)
 * with G[p][n] = gy[p][n] * out_act'(y[p][n]) (y = the activated forward output; may be NULL for SR_OUT_NONE).
 * out_act: softplus (sigma, beta), sigmoid (sun), sigmoid*1.002-0.001 (rgb, models/satnerf.py:195-196).
 * fp32 in / fp32 out, bf16 hi/lo split 3-pass MFMA inside (~1e-6 relative).  sr_points_along: xyz[p] = o + d * z. */
enum { SR_ACT_NONE = 0, SR_ACT_SIN = 1, SR_ACT_RELU = 2 };
enum { SR_OUT_NONE = 0, SR_OUT_SOFTPLUS = 1, SR_OUT_SIGMOID = 2, SR_OUT_SIGMOID_RGB = 3 };
typedef struct sr_linear_src {
  const float* x; /* (ceil(P / row_div), >= k) fp32 */
  int ld;         /* row stride in floats */
  int k;          /* columns taken from this source */
  int act;        /* SR_ACT_* applied on load */
  float w0;       /* sin(w0 * x) */
  int row_div;    /* point p reads row p / row_div: 1 = per point, n_samples = per ray */
} sr_linear_src;
int sr_linear_fwd(const sr_linear_src* src, int n_src, const float* weight, const float* bias, int64_t n_points, int n_out,
                  int out_act, float* y, int ldy, void* stream);
int sr_linear_bwd_input(const float* gy, int ldg, const float* y, int ldy, int out_act, const float* weight, int k_total, int col0,
                        const sr_linear_src* target, int64_t n_points, int n_out, float* d_src, int ldd, void* stream);
int sr_linear_bwd_weight(const float* gy, int ldg, const float* y, int ldy, int out_act, const sr_linear_src* src, int n_src,
                         int64_t n_points, int n_out, float* d_weight, float* d_bias, void* stream);
int sr_points_along(const float* rays, int ray_stride, int dir_col, const float* z_vals, int64_t n_rays, int n_samples, float* xyz,
                    void* stream);
/* Mapping.forward of the classic nerf (models/nerf.py:36-69): x (rows, dim) -> out (rows, 2*n_freqs*dim) =
 * [sin(2^0 x), cos(2^0 x), sin(2^1 x), cos(2^1 x), ...], no identity term */
int sr_positional_map(const float* x, int ld, int dim, int64_t rows, int n_freqs, float* out, void* stream);

/* ---- fused classic NeRF forward (csrc/nerf_fwd.inc): inference, width 256, single-pass bf16 operands with fp32 accumulation ----------
 * The model of models/__init__.py:8: mapping_sizes [10, 4], 8 layers of 256, skip at layer 4.  `stream_hi` = the weights packed by
 * sr_pack_stream with the gather maps of satnerf_amd/packing.py: nerf_forward_maps; sr_nerf_stream_elems(feat) = its bf16 element count,
 * -1 for a width this build does not serve.
 *
 * sr_nerf_mlp_fwd replaces NeRF.forward with both Mapping.forward calls (models/nerf.py:184-227) for n_points points:
 *   xyz (P, xyz_stride >= 3) per point, dirs read at row p / row_div (1 = a direction per point, n_samples = per ray);
 *   rgb (P,3) = sigmoid(.) * 1.002 - 0.001, sigma (P) = softplus(.).
 * sr_nerf_render_fwd replaces one pass of models/nerf.py:71-133 with the sampling in front of it (rendering.py:62-81,110-112,153-154) for
 * n_rays rays (N, ray_stride >= 8) = o d near far: depths = the stratified depths of sr_ray_sample_fwd from u (N,S), bit for bit, or z_in
 * (N,S) as given (exactly one of the two); points o + d z; the network; classic compositing = sr_composite_fwd without sun, sky and clamp
 * (noise (N,S) may be NULL).  Writes weights, transparency (N,S) and, where not NULL, z_out (N,S), rgb (N,3), depth (N).
 * A workgroup composites whole rays of its 256 points: 2 <= n_samples <= sr_nerf_render_max_samples().
 * Unsupported arguments return an error and launch nothing; zero points / rays return 0 without a launch. */
int64_t sr_nerf_stream_elems(int feat);
int sr_nerf_render_max_samples(void);
int sr_nerf_mlp_fwd(const float* xyz, int xyz_stride, const float* dirs, int dir_stride, int row_div, int64_t n_points, int feat,
                    const uint16_t* stream_hi, float* rgb, float* sigma, void* stream);
int sr_nerf_render_fwd(const float* rays, int ray_stride, int64_t n_rays, int n_samples, const float* u, const float* z_in,
                       const float* noise, float noise_std, int feat, const uint16_t* stream_hi, float* z_out, float* rgb, float* depth,
                       float* weights, float* transparency, void* stream);

/* ---- whole-image evaluation -------------------------------------------------------------
 * sr_composite_image: compositing (models/satnerf.py:52-70) that keeps per ray only what
 * eval_satnerf.save_nerf_output_to_images writes per pixel (eval_satnerf.py:106-146): image (N,13) =
 * [rgb(3) clamped, depth, sum w, sum w*sun, sum w*albedo(3), sum w*beta, sum w*sky(3)] -- 52 B/ray instead of 2,576 B.
 * sr_latlonalt_from_depth: SatelliteDataset.get_latlonalt_from_nerf_prediction (datasets/satellite.py:246-275) with
 * sat_utils.ecef_to_latlon_custom (sat_utils.py:76-95), in fp64: point = (o + d*depth) * range + center (ECEF, `center` =
 * 3 HOST doubles) -> lat, lon (degrees), alt (m), each (N,) fp64 on the device. */
int sr_composite_image(const float* z_vals, const float* sigma, const float* noise, float noise_std, const float* albedo,
                       const float* sun_v, const float* beta, const float* sky, int64_t n_rays, int n_samples, float* image,
                       void* stream);
int sr_latlonalt_from_depth(const float* rays, int ray_stride, const float* depth, int64_t n_rays, const double* center,
                            double range, double* lat, double* lon, double* alt, void* stream);

/* ---- RPC ray generation: datasets/satellite.py:18-65 get_rays + :218-227 normalize_rays + :229-244 sun -------
 * `rpc` = 90 HOST doubles of the image's RPC00B camera in rpcm's dict order: row_num[20], row_den[20], col_num[20], col_den[20],
 * row_offset, col_offset, lat_offset, lon_offset, alt_offset, row_scale, col_scale, lat_scale, lon_scale, alt_scale (apply
 * sat_utils.rescale_rpc for a down-scaled image first).  Pixel i = (col i % width, row i / width) is localised at max_alt (ray
 * origin) and min_alt in fp64 (Newton on the projection to rpcm's 1e-18 tolerance), converted to ECEF, and written as
 * rays8 (H*W, 8) fp32 = the reference's <cache_dir>/<img_id>.data content [o(3) d(3) near=0 far] and / or rays11 (H*W, 11) = the
 * same normalised by `center` (3 HOST doubles) / `range` in fp32 with the image's sun direction appended; either may be NULL. */
int sr_rpc_rays(const double* rpc, int width, int height, double min_alt, double max_alt, const double* center, double range,
                double sun_elevation_deg, double sun_azimuth_deg, float* rays11, float* rays8, void* stream);

/* ---- ECEF bounds of one image's rays: SatelliteDataset.init_scaling_params (datasets/satellite.py:139-151) ---
 * replaces the host loop that builds every ray of every image with numpy and rpcm and takes the extremes of their near and far points
 * for scene.loc.  `rpc`, width, height, min_alt, max_alt as for sr_rpc_rays.  Per pixel: sr_rpc_rays' rays8 row, near point = o, far
 * point = o + far * d in fp32 (separate multiply and add, as the reference's tensor ops :149-150); bounds6 (6 DEVICE floats) = {xmin,
 * xmax, ymin, ymax, zmin, zmax} over both.  A pixel with a non-finite coordinate contributes to no bound and adds 1 to *n_bad (1 DEVICE
 * int64); with no finite pixel the bounds are +inf / -inf.  Integer atomics on order-preserving keys: bitwise repeatable.  No host
 * synchronisation: capturable. */
int sr_rpc_scene_bounds(const double* rpc, int width, int height, double min_alt, double max_alt, float* bounds6, int64_t* n_bad,
                        void* stream);

/* ---- depth supervision from tie points: SatelliteDataset_depth (datasets/satellite_depth.py:51-129) ---------
 * `rpc` = 90 HOST doubles as for sr_rpc_rays (the full-resolution camera); colrow = n (col, row) DEVICE fp64 pairs (the JSON's
 * keypoints.2d_coordinates); pts3d = n_pts x 3 DEVICE fp64 ECEF tie points (pts3d.npy); pts3d_idx = n DEVICE int64 rows of pts3d
 * (keypoints.pts3d_indices; an index outside 0..n_pts-1 yields NaN and is never scattered).  No host synchronisation: capturable.
 * sr_rpc_rays_at: get_rays + normalize_rays + sun at the keypoints (satellite_depth.py:64-75; datasets/satellite.py:18-65,218-244):
 * sr_rpc_rays' per-pixel arithmetic at arbitrary (col, row), rays11 (n, 11) fp32 DEVICE; `center` = 3 HOST doubles.
 * sr_reprojection_errors: satellite_depth.py:116-122 -- sat_utils.ecef_to_latlon_custom of pts3d[idx], rpc.projection, and the fp64
 * pixel distance to colrow, err (n,) fp32 DEVICE (the reference stores it in a float32 matrix).
 * sr_keypoint_weights_scratch: HOST only; bytes of caller-owned scratch sr_keypoint_weights needs for n_pts points and n_cams cameras.
 * sr_keypoint_weights: satellite_depth.py:123-129 over all n observations of the dataset: cam (n,) DEVICE int64 = the image of each
 * observation (0..n_cams-1), err = the sr_reprojection_errors of all of them.  Per (point, camera) the observation with the largest
 * index wins (numpy's assignment keeps the last), e (n_pts,) fp32 DEVICE = its errors summed over cameras in camera order, e_mean (1
 * fp32 DEVICE) = the mean of e over all n_pts points (unobserved points count with 0), w (n_pts,) fp32 DEVICE = exp(-(e / e_mean)^2).
 * Sums accumulate in fp64 and are rounded to fp32 once (the reference sums in fp32); partials in a fixed order: bitwise repeatable.
 * sr_tie_point_depths: satellite_depth.py:77-91 -- depths (n, 2) fp32 DEVICE = [|(fp32(pts3d[idx]) - center) / range - origin|, w[idx]]
 * in fp32, origin = columns 0..2 of rays11 (sr_rpc_rays_at's output); w (n_pts DEVICE floats) may be NULL (column 1 = 0). */
int sr_rpc_rays_at(const double* rpc, const double* colrow, int64_t n, double min_alt, double max_alt, const double* center, double range,
                   double sun_elevation_deg, double sun_azimuth_deg, float* rays11, void* stream);
int sr_reprojection_errors(const double* rpc, const double* colrow, const int64_t* pts3d_idx, int64_t n, const double* pts3d,
                           int64_t n_pts, float* err, void* stream);
int sr_keypoint_weights_scratch(int64_t n_pts, int n_cams, int64_t* bytes);
int sr_keypoint_weights(const int64_t* pts3d_idx, const int64_t* cam, const float* err, int64_t n, int64_t n_pts, int n_cams,
                        void* scratch, int64_t scratch_bytes, float* e, float* w, float* e_mean, void* stream);
int sr_tie_point_depths(const float* rays11, const double* pts3d, const int64_t* pts3d_idx, int64_t n, int64_t n_pts,
                        const double* center, double range, const float* w, float* depths, void* stream);

/* ---- tie-point interpolation: study_depth_supervision.idw_interpolation (:64-103) and the
 * scipy.ndimage.gaussian_filter(mode="reflect") of save_heatmap_of_reprojection_error (:18-61), the interpolation behind
 * check_depth_supervision_points (:105-203) ------------------------------------------------------------------------------------
 * sr_idw_grid_scratch: HOST only; bytes of caller-owned scratch sr_idw_interpolate needs for k points and n_neighbors (1..32,
 * n_neighbors <= k <= 2^30).
 * sr_idw_interpolate: pts2d = k DEVICE fp64 (col, row) pairs carrying z (k DEVICE fp32); queries = n_query DEVICE fp64 (col, row)
 * pairs, or with query NULL every pixel (col i % width, row i / width) of the height x width raster (n_query ignored).  Per query the
 * n_neighbors nearest points by fp64 d^2 = dx*dx + dy*dy, ties to the lower index (an exhaustive search's answer: a grid over the
 * points, rings of cells until no unvisited cell can be nearer); out (DEVICE fp64) = z[nearest] when n_neighbors is 1 or the
 * nearest distance is < 1e-10, else sum((1/d_i) / sum(1/d_j) z_i) in fp64 in increasing distance.  Optional (NULL to skip): nn_idx
 * (n_query x n_neighbors DEVICE ints, the chosen indices in that order) and visited (n_query DEVICE ints, points examined).  Points
 * must be finite: a non-finite one is never chosen, and a query with fewer than n_neighbors finite points gets NaN and index -1.  No
 * float atomics, no host synchronisation; bitwise repeatable.
 * sr_gaussian_filter_f64: scipy.ndimage.gaussian_filter(in, sigma) with mode "reflect" on a row-major h x w DEVICE fp64 raster (each
 * side 1..65535): taps0 / taps1 = the 2 r + 1 DEVICE fp64 taps of axis 0 / 1 (scipy's _gaussian_kernel1d, symmetric, r <= 200), radius
 * -1 leaves that axis as it is (sigma <= 1e-15).  Axis 0 first into tmp (h x w DEVICE fp64, needed only when both axes are
 * filtered), then axis 1 into out; each output = x[i] w[0] + sum for k = r .. 1 of (x[i-k] + x[i+k]) w[k] in fp64 (correlate1d's
 * order), indices outside the axis reflected (period 2n).  in, tmp and out must not overlap. */
int sr_idw_grid_scratch(int64_t k, int n_neighbors, int64_t* bytes);
int sr_idw_interpolate(const double* pts2d, const float* z, int64_t k, const double* query, int64_t n_query, int height, int width,
                       int n_neighbors, void* scratch, int64_t scratch_bytes, double* out, int* nn_idx, int* visited, void* stream);
int sr_gaussian_filter_f64(const double* in, int h, int w, const double* taps0, int radius0, const double* taps1, int radius1,
                           double* tmp, double* out, void* stream);

/* ---- DSM extraction: SatelliteDataset.get_dsm_from_nerf_prediction (datasets/satellite.py:277-338) -------------
 * sr_utm_zone: utm.latlon_to_zone_number + utm.latitude_to_zone_letter as sat_utils.utm_from_latlon uses them (sat_utils.py:105-106),
 * HOST only: lon normalised to [-180, 180), Norway (zone 32) and Svalbard (31/33/35/37) exceptions, letter = ASCII code of
 * "CDEFGHJKLMNPQRSTUVWXX"[int(lat + 80) >> 3]; error unless -80 <= lat <= 84 and lon is finite.
 * sr_utm_from_latlon: sat_utils.utm_from_latlon (sat_utils.py:97-113) for a given zone (1..60): transverse Mercator (Krueger's series
 * to n^6, WGS84, k0 0.9996, false easting 500 km, false northing 0 in both hemispheres -- the reference's projection string has no
 * +south), lat / lon degrees (N,) fp64 -> east / north metres (N,) fp64.
 * sr_depth_to_utm: datasets/satellite.py:292-294 -- sr_latlonalt_from_depth's arithmetic (same `center` = 3 HOST doubles) followed by
 * the projection above, east / north / alt (N,) fp64.  zone 0 takes the zone of ray 0's point (sat_utils.py:105-106), 1..60 overrides
 * it; zone_out (2 DEVICE ints) receives {zone number, letter of ray 0's latitude}, number 0 when ray 0's point is unusable (then
 * east / north are NaN).
 * sr_dsm_bounds: datasets/satellite.py:303-304 -- bounds (4 DEVICE doubles) = {min east, max east, min north, max north} over the usable
 * points (finite east, north, alt and |alt| <= 2^20 m), NaN when there are none.
 * sr_dsm_rasterize: plyflatten(cloud, xoff, yoff, resolution, xsize, ysize, radius, sigma) (datasets/satellite.py:316) by this project's
 * own convention (not checked against plyflatten): column c covers east [xoff + c r, xoff + (c+1) r), row j
 * covers north (yoff - (j+1) r, yoff - j r]; each usable in-grid point adds weight w = 1 (sigma = inf) or exp(-d^2 / (2 sigma^2))
 * (d = cells from the point to the target centre) to every in-grid cell within `radius` (0..4) rows and columns.  dsm (ysize, xsize)
 * fp32 = sum w alt / sum w (NaN where sum w = 0), weight = sum w.  acc = 2 * xsize * ysize uint64 of caller-owned scratch (64-bit
 * fixed point, zeroed here): the result is bitwise independent of point order for every sigma. */
int sr_utm_zone(double lat, double lon, int* zone, int* letter);
int sr_utm_from_latlon(const double* lat, const double* lon, int64_t n, int zone, double* east, double* north, void* stream);
int sr_depth_to_utm(const float* rays, int ray_stride, const float* depth, int64_t n_rays, const double* center, double range,
                    int zone, double* east, double* north, double* alt, int* zone_out, void* stream);
int sr_dsm_bounds(const double* east, const double* north, const double* alt, int64_t n, double* bounds, void* stream);
int sr_dsm_rasterize(const double* east, const double* north, const double* alt, int64_t n, double xoff, double yoff,
                     double resolution, int xsize, int ysize, int radius, double sigma, uint64_t* acc, float* dsm, float* weight,
                     void* stream);

/* ---- nadir DSM: eval_s2p.lonlat_from_utm (eval_s2p.py:37-44) and one vertical ray per DSM cell ---------------
 * sr_utm_to_latlon: the inverse of sr_utm_from_latlon for a given zone (1..60): east / north metres (N,) DEVICE fp64 -> lat / lon
 * degrees (N,) DEVICE fp64 by Krueger's inverse series to n^6 (Karney 2011 eqs. 11, 15) and a fixed six Newton steps from the
 * conformal to the geodetic latitude (eqs. 19-21); WGS84, k0 0.9996, false easting 500 km, false northing 0 in both hemispheres
 * (southern points carry negative northings, as sr_utm_from_latlon writes them).  lon = central meridian + an angle in (-180, 180],
 * not wrapped.  A non-finite east or north gives NaN lat and lon.  n <= 0 launches nothing.
 * sr_ortho_rays: get_rays + normalize_rays (datasets/satellite.py:18-65,218-227) for a camera that looks straight down every cell of
 * a DSM grid, the RPC localisation replaced by the grid's own lon / lat.  Cell i = (row j = i / xsize, column c = i % xsize), row 0
 * at the top (sr_dsm_rasterize's layout); its centre E = xoff + (c + 0.5) r, N = yoff - (j + 0.5) r; (phi, lambda) = sr_utm_to_latlon
 * of (E, N).  Row i of rays (DEVICE fp32, row_stride >= 11 floats between rows, columns beyond 10 untouched):
 *   0..2  origin (ECEF(phi, lambda, max_alt) - center) / range, evaluated in fp64 and rounded to fp32 ONCE (the reference casts the
 *         ECEF origin to fp32 before subtracting the centre: ~0.4 m of error this does not have)
 *   3..5  direction -(cos phi cos lambda, cos phi sin lambda, sin phi), the inward ellipsoid normal in closed form
 *   6, 7  near = 0, far = (max_alt - min_alt) / range
 *   8..10 sun_d (3 HOST floats) as given
 * so the point at depth t along ray i has altitude max_alt - t range over the cell centre.  center = 3 HOST doubles.  latlon
 * (xsize * ysize, 2) DEVICE fp64 = (lat, lon) degrees per cell, may be NULL.  Errors (nothing is launched): zone outside 1..60,
 * min_alt >= max_alt, range <= 0, resolution <= 0, xsize or ysize < 1, xsize * ysize >= 2^31, row_stride < 11, any of them not
 * finite.  Neither entry synchronises with the host: capturable. */
int sr_utm_to_latlon(const double* east, const double* north, int64_t n, int zone, double* lat, double* lon, void* stream);
int sr_ortho_rays(double xoff, double yoff, double resolution, int xsize, int ysize, int zone, double min_alt, double max_alt,
                  const double* center, double range, const float* sun_d, float* rays, int row_stride, double* latlon, void* stream);

/* ---- geometric sun visibility: the ray from a rendered surface point towards the sun ---------------------------
 * The solar correction (metrics.py:27-33) trains the sun_v head towards the transparency the density leaves along a ray towards the
 * sun.  The reference's own sun rays (the `sc` pass, rendering.py:102-108) cannot serve to compute it: they add the east / north / up
 * vector of rays[:, 8:11] to an ECEF origin (a mixed frame) and start at the camera ray's origin, not at the surface.  sr_sun_rays
 * writes that ray in the scene's normalised ECEF frame; rendering it with sr_satnerf_render_depth and keeping the transparency in
 * front of the last sample (models/satnerf.py:52-63, column -1) gives the visibility; sr_sun_shade relights with it.
 * sr_sun_rays, per primary ray i: r = row i of rays (DEVICE fp32, ray_stride >= 11), t = depth[i] (DEVICE fp32), s = sun_d (3 HOST
 * floats: the call's one sun vector) or, with sun_d NULL, r[8..10]; s is (east, north, up) and need not be a unit vector.  In fp64
 * with contraction off, rounded to fp32 once:
 *   s^ = s / |s|;  P = o + d t;  E = P range + center (`center` = 3 HOST doubles);  (phi, lambda, alt) = sr_latlonalt_from_depth's
 *   dir  = s^_e e + s^_n n + s^_u u,  e = (-sin l, cos l, 0), n = (-sin p cos l, -sin p sin l, cos p), u = (cos p cos l, cos p sin l, sin p)
 *   L    = (max_alt - alt) / (s^_u range): where the ray reaches max_alt (metres) on the local tangent plane
 *   near = bias_abs + bias_rel (r[7] - r[6]), far = max(near, L); the bias keeps the ray from starting inside the surface it leaves
 * Row i of out (DEVICE fp32, out_stride >= 11, columns beyond 10 untouched) = [P(3) dir(3) near far sun(3)], sun = r[8..10] unchanged or
 * the call's sun_d as given (not normalised).  A ray is invalid when t or E is not finite, |s| is zero or not finite, or s^_u <= 0:
 * valid[i] (DEVICE uint8) = 0 and the row is [o(3) d(3) 0 0 sun(3)], a finite zero-length ray; otherwise valid[i] = 1.  latlonalt
 * ((3, n) DEVICE fp64: lat, lon in degrees, alt in metres; may be NULL) holds sr_latlonalt_from_depth's values bit for bit.  out
 * must not overlap rays.  Errors (nothing is launched): a stride < 11, range not finite or <= 0, max_alt or center not finite, a bias
 * negative or not finite, a call-level sun_d that is not finite, zero or has up <= 0, a null pointer with n > 0.  n <= 0 launches nothing.
 * sr_sun_shade: a per-pixel relighting of the composited albedo (it does not re-composite per sample).  With v = vis[i] (DEVICE fp32)
 * and c = 0..2, in fp32 in this order with contraction off: q = 1 - v, k = q sky[i][c], irr = v + k, x = albedo[i][c] irr,
 * rgb[i][c] = x clamped to [0, 1]; a NaN x stays NaN.  albedo / sky / rgb are DEVICE fp32 rows with strides >= 3 floats.
 * Neither entry synchronises with the host: capturable. */
int sr_sun_rays(const float* rays, int ray_stride, const float* depth, int64_t n, const double* center, double range, double max_alt,
                const float* sun_d, double bias_abs, double bias_rel, float* out, int out_stride, uint8_t* valid, double* latlonalt,
                void* stream);
int sr_sun_shade(const float* albedo, int albedo_stride, const float* sky, int sky_stride, const float* vis, int64_t n, float* rgb,
                 int rgb_stride, void* stream);

/* ---- ray casting against a DSM raster: the raster as geometry -----------------------------------------------------
 * hgt (ysize, xsize) DEVICE fp32 is a DSM raster in sr_dsm_rasterize's layout, a value that is not finite = no surface.  Grid frame, fp64
 * metres: a point (E, N, alt) has x = E - xoff, y = yoff - N, z = alt; cell (j, c) is x in [c r, (c+1) r), y in [j r, (j+1) r); a
 * finite cell is the solid column z <= h over that square, any other cell is empty and passed through.
 * The walk, one lane per ray, all fp64 with contraction off.  A ray is the straight segment A -> B, s in [0, 1], clipped to the grid's
 * rectangle first (a segment that misses it is a miss).  Cells are visited in order of s.  The parameter of the crossing of the
 * line x = k r is (k r - xA) / (xB - xA), computed from the absolute index k, never accumulated; rows likewise.  The cell the segment
 * is in at a parameter s is defined by these values alone (for xB > xA the largest c whose line is crossed at or before s, the
 * smallest for xB < xA, and the c with c r <= xA < (c+1) r for xB = xA): where a position is floored, at the entry, the index is
 * corrected against them, so a result does not depend on how the walk got there.  On a tie (both crossings at the same s) both
 * indices step: the two cells touched at a point are not visited.  Hit rule for a visited finite cell entered at s_in and left at
 * s_out = min(its next crossing, 1), with z(s) = zA + s (zB - zA): z(s_in) <= h hits at s_in (a wall, or a start inside the column);
 * otherwise z(s_out) <= h hits at (h - zA) / (zB - zA) (the top); otherwise the walk goes on.  The first hit ends it; reaching s = 1
 * or leaving the grid is a miss.  Crossing values of neighbouring lines must differ (r far above the spacing of the coordinates).
 * sr_heightfield_blockmax: blockmax (ceil(ysize / 16), ceil(xsize / 16)) DEVICE fp32 = the maximum of the finite cells of each 16 x 16
 * block, -inf where there is none; gmax (1 DEVICE fp32) = the maximum of the raster, -inf likewise.  Two launches, no atomics.
 * sr_heightfield_cast: n rays, given either in the scene frame -- rays (DEVICE fp32 rows, ray_stride >= 8: o(3) d(3) near far), center
 * (3 HOST doubles), range, zone (1..60), xoff, yoff; A and B are the UTM images of o + d near and o + d far by exactly
 * sr_depth_to_utm's arithmetic, the path between them is taken as the chord (sag <= run^2 / (8 R)), and t = near + s (far - near) --
 * or as grid-frame segments seg_a, seg_b ((n, 3) DEVICE fp64; then rays is NULL, center .. yoff are ignored and t = s).  Outputs:
 * depth (n,) fp32 = t evaluated in fp64 and rounded once, NaN on a miss; cell (n,) int32 = j xsize + c, -1 on a miss; s (n,) fp64,
 * NaN on a miss, may be NULL; seg (n, 6) DEVICE fp64 = (E, N, alt) of A and of B as sr_depth_to_utm gives them: required in the ray
 * form, where a first launch writes it and the walk reads it (the segment that was walked), and NULL with segments.
 * A ray with an endpoint that is not finite, or with far < near, is a miss, never a fault.
 * sr_heightfield_shadow: out (ysize, xsize) DEVICE fp32 = 1 lit, 0 shadowed, NaN where the cell is empty, the grid frame taken as flat.
 * For every finite cell A = (cell centre, h + bias), bias >= 0 metres; the direction is the unit vector of sun_d (3 HOST doubles:
 * east, north, up, up > 0), i.e. (uE, -uN, uU) in the grid frame; B is where the ray reaches gmax, above which nothing can block; a
 * start at or above gmax is lit.  The walk is sr_heightfield_cast's, with the start cell passed through whatever its height: the ray
 * leaves the surface it stands on (a rule, not a tuned bias).
 * accelerate = 1 (cast and shadow) takes the two-level walk: block by block, descending into a block's cells only where the segment's
 * lowest altitude over the block is <= the block's maximum, and ending a rising ray once it is above gmax; it then needs blockmax
 * and gmax of sr_heightfield_blockmax (the shadow needs gmax always).  Its results are bit-identical to accelerate = 0.
 * Errors (nothing is launched): xsize or ysize < 1, xsize * ysize >= 2^31, resolution not finite or <= 0, a null pointer, accelerate
 * outside {0, 1}, both or neither of rays and seg_a / seg_b, seg with segments, ray_stride < 8, zone outside 1..60, range not finite
 * or <= 0, xoff / yoff / center not finite, a bias negative or not finite, a sun_d that is not finite, zero or has up <= 0.  n <= 0
 * launches nothing.  No entry synchronises with the host: capturable. */
int sr_heightfield_blockmax(const float* hgt, int xsize, int ysize, float* blockmax, float* gmax, void* stream);
int sr_heightfield_cast(const float* hgt, int xsize, int ysize, double resolution, const float* blockmax, const float* gmax, int accelerate,
                        const float* rays, int ray_stride, const double* center, double range, int zone, double xoff, double yoff,
                        const double* seg_a, const double* seg_b, int64_t n, float* depth, int* cell, double* s, double* seg, void* stream);
int sr_heightfield_shadow(const float* hgt, int xsize, int ysize, double resolution, const float* blockmax, const float* gmax,
                          int accelerate, const double* sun_d, double bias, float* out, void* stream);

/* ---- orthorectification onto a DSM raster: a view's pixels brought to the DSM's cells ----------------------------
 * hgt, xsize, ysize, resolution, blockmax, gmax, accelerate: the raster of section 7.15 and sr_heightfield_blockmax's maxima (gmax is
 * always needed, blockmax with accelerate = 1); xoff, yoff, zone (1..60): its place in UTM, cell (j, c) centred at E = xoff + (c + 0.5) r,
 * N = yoff - (j + 0.5) r.  rpc = the 90 HOST doubles of sr_rpc_rays.  image = DEVICE pixels, fmt 0 uint8 (value v / 255) or 1 fp32
 * (value v), pixel (row, col) channel ch at element row row_stride + col pix_stride + ch, channels 1..4, pix_stride >= channels,
 * row_stride >= (width - 1) pix_stride + channels.  Pixel centres sit at integer (col, row), as sr_rpc_rays places them.
 * Per cell i = j xsize + c, fp64 with contraction off:
 *   h not finite: status 0 (empty), colour NaN, colrow NaN.
 *   (col, row) = the RPC projection of (sr_utm_to_latlon's (lat, lon) of the cell centre, altitude h): colrow[i] = (col, row), always.
 *   (col, row) not finite or outside [0, width - 1] x [0, height - 1]: status 3 (outside), colour NaN.
 *   line of sight: A = (cell centre, h + bias), bias >= 0 metres.  h + bias >= gmax: visible.  Else B = the UTM image of the camera's
 *   localisation of (col, row) at altitude gmax (sr_rpc_rays' Newton iteration), at altitude gmax, and A -> B is walked in the grid
 *   frame by sr_heightfield_cast's walk with cell i itself passed through (the chord, the grid taken as flat): a hit gives status 2
 *   (occluded), colour NaN; a miss status 1 (visible).  accelerate = 1 takes the two-level walk: the same bits.
 *   a visible cell's colour[i][ch], mode 0 nearest: pixel (floor(row + 0.5), floor(col + 0.5)); mode 1 bilinear: with x0 = floor(col),
 *   fx = col - x0 (rows likewise) ((1 - fx) p00 + fx p01) (1 - fy) + ((1 - fx) p10 + fx p11) fy; mode 2 bicubic: Keys' kernel with
 *   a = -0.5 over the 4 x 4 taps x0 - 1 .. x0 + 2, weights w(1 + fx), w(fx), w(1 - fx), w(2 - fx), each row's columns summed first in
 *   increasing index order, then the rows likewise.  Neighbour indices are clamped to the image (edge replicate).  Weights and sums
 *   in fp64, rounded to fp32 once.  A NaN pixel under a tap propagates.
 * Outputs: color (ysize, xsize, channels) DEVICE fp32, status (ysize, xsize) DEVICE uint8, colrow (ysize, xsize, 2) DEVICE fp64.
 * Fusion: sum ((ysize, xsize, channels) DEVICE fp64) and count ((ysize, xsize) DEVICE int32), both or neither: a visible cell adds
 * its fp32 colour to sum and 1 to count.  One lane owns one cell and calls follow one another on the stream: no atomics, the
 * accumulation of several views is bitwise repeatable and in call order.  The caller zeroes them and divides.
 * Two launches: the projection writes colrow and, into scratch, the status it decides and B; the second walks, samples and
 * accumulates.  scratch: caller-owned DEVICE bytes (8-byte aligned), at least sr_orthorectify_scratch(xsize, ysize) (HOST only).
 * stages 0 runs both, 1 the projection alone, 2 the second launch alone on the colrow and scratch a stages = 1 call with the same
 * raster, camera and bias left (another image, mode or walk without projecting again; timing).
 * Errors (nothing is launched): xsize or ysize < 1, xsize * ysize >= 2^31, resolution not finite or <= 0, xoff / yoff not finite, zone
 * outside 1..60, accelerate outside {0, 1}, a null pointer, width or height < 1, channels outside 1..4, fmt outside {0, 1}, strides
 * that overlap, mode outside 0..2, a bias negative or not finite, stages outside 0..2, one accumulator without the other, a zero RPC
 * scale, scratch too small or misaligned.  Neither entry synchronises with the host: capturable. */
int sr_orthorectify_scratch(int xsize, int ysize, int64_t* bytes);
int sr_orthorectify(const float* hgt, int xsize, int ysize, double resolution, double xoff, double yoff, int zone, const float* blockmax,
                    const float* gmax, int accelerate, const double* rpc, const void* image, int fmt, int width, int height, int channels,
                    int64_t row_stride, int64_t pix_stride, int mode, double bias, int stages, void* scratch, int64_t scratch_bytes,
                    float* color, uint8_t* status, double* colrow, double* sum, int* count, void* stream);

/* ---- cloud fusion: eval_s2p.project_cloud_into_utm_grid (eval_s2p.py:175-226) ---------------------------------
 * sr_cloud_grid bins a UTM cloud (east / north / alt (N,) DEVICE fp64, sr_depth_to_utm's outputs) into a map_h x map_w grid and keeps
 * per cell the min (mode 0), max (1), mean (2) or median (3) of the altitudes that landed in it: out (map_h, map_w) DEVICE fp64, NaN
 * where no point landed, count (map_h, map_w) DEVICE int32.
 * rule 0 (nearest, the reference's): col = rint((east - x0) / definition), row = rint((north - y0) / definition) in IEEE fp64 with
 * round-half-to-even (np.round), kept when 0 <= col < map_w and 0 <= row < map_h (-0 is column 0), written to output row
 * map_h - 1 - row (the reference's flipud: row 0 is north); (x0, y0) = (bb[0], bb[2]).
 * rule 1 (floor, sr_dsm_rasterize's cell): col = floor((east - x0) / definition), row = floor((y0 - north) / definition), (x0, y0) =
 * (xoff, yoff) of the DSM grid, output row = row.
 * Departure: a point whose east, north or alt is not finite contributes nothing (the reference lets a NaN altitude poison avg / med).
 * Stages, all on `stream` with no host round trip: (1) cell key per point + 32-bit integer histogram, (2) exclusive scan (block sums,
 * their scan, add), (3) scatter into per-cell segments by an integer cursor, (4) in-place sort of every segment on an order-preserving
 * 64-bit key (one wave up to 64 keys, one workgroup beyond), (5) reduce: min = first, max = last, med = the middle key or (a + b) / 2
 * of the two middle ones (np.median bit for bit), avg = the ascending fp64 sum / count.  Every mode reads the sorted segment and no
 * float atomic is used: the result is bitwise independent of point and arrival order, avg included.
 * scratch: caller-owned DEVICE bytes (8-byte aligned), at least sr_cloud_grid_scratch(n, map_w, map_h) (HOST only); it need not be
 * initialised.  stages = 0 runs everything; 1..4 stops after that stage (timing only: out is then not written).  n and map_w * map_h
 * must each be <= 2^31 - 4096 (int32 offsets), else an error is returned. */
int sr_cloud_grid_scratch(int64_t n, int map_w, int map_h, int64_t* bytes);
int sr_cloud_grid(const double* east, const double* north, const double* alt, int64_t n, double x0, double y0, double definition,
                  int map_w, int map_h, int rule, int mode, void* scratch, int64_t scratch_bytes, double* out, int* count, int stages,
                  void* stream);

/* ---- DSM registration: dsmr.compute_shift / dsmr.apply_shift (dsmr.py:6-148,163-215), the XY + Z
 * registration of sat_utils.dsm_pointwise_diff (sat_utils.py:172-177) --------------------------------------------------------------
 * u (hu, wu) is the reference DSM (the ground truth), v (hv, wv) the secondary (the prediction): row-major DEVICE fp64 (exact
 * widenings of fp32 rasters), shapes may differ, every side in 1..16384.  A pixel counts only when finite; reads outside v are NaN.
 * sr_dsm_register_scratch: HOST only; bytes of caller-owned scratch sr_dsm_compute_shift needs, and the number of levels (1 + the
 * halvings while min(h, w) of u > 100, recursive_ncc dsmr.py:121-135).
 * sr_dsm_downsample2x: downsample2x_ (dsmr.py:17-48), out ((h+1)/2, (w+1)/2) fp64: cell (J, I) = the mean of the finite in-bounds
 * pixels of the 2x2 window at (min(2J+1, h-1), min(2I+1, w-1)) (the reference's last write wins), summed in the order (j,i),
 * (j+1,i), (j,i+1), (j+1,i+1), NaN if none; bitwise the reference's.  The kernel compute_shift uses for every level.
 * sr_dsm_compute_shift: recursive_ncc with irange (1..16) and compute_shift's coefficients (dsmr.py:102-135,184-188).  At each level
 * every shift (x, y) = start +- irange gets mean_std's two-pass fp64 statistics (dsmr.py:50-88) and ncc = xcorr / (sig_u sig_v);
 * the first strict maximum scanning y outer, x inner wins and the next finer level starts at twice it.  Departure: a shift with
 * no valid pair or zero variance (where the reference raises ZeroDivisionError) gets ncc NaN and is never chosen; a level without a
 * finite ncc keeps its start.  Writes shift (2 DEVICE ints) = (dx, dy) and coef (8 DEVICE doubles) = {a, b, mu_u, mu_v, sig_u,
 * sig_v, xcorr, count} at that shift, a = sig_u / sig_v if scaling else 1, b = mu_u - mu_v a; count 0 means no answer.  Optional
 * (NULL to skip): ncc_levels (levels x (2 irange + 1)^2 DEVICE doubles, level 0 the finest, [y][x]) and start_levels (levels x 2
 * DEVICE ints).  The running shift lives in scratch: no host synchronisation, capturable.  Partials are summed in a fixed order
 * set by the shapes alone, so results are bitwise repeatable.
 * sr_dsm_apply_shift: apply_shift_ (dsmr.py:138-148) over v's extent: out[j, i] = a v[j + dy, i + dx] + b in fp64 (NaN outside v),
 * stored fp32 (hv, wv); (dx, dy) and (a, b) are read from the DEVICE shift / coef of sr_dsm_compute_shift. */
int sr_dsm_register_scratch(int hu, int wu, int hv, int wv, int irange, int64_t* bytes, int* levels);
int sr_dsm_downsample2x(const double* in, int h, int w, double* out, void* stream);
int sr_dsm_compute_shift(const double* u, int hu, int wu, const double* v, int hv, int wv, int irange, int scaling, void* scratch,
                         int64_t scratch_bytes, int* shift, double* coef, double* ncc_levels, int* start_levels, void* stream);
int sr_dsm_apply_shift(const double* v, int hv, int wv, const int* shift, const double* coef, float* out, void* stream);

/* ---- image metrics: metrics.mse / metrics.psnr / metrics.ssim (metrics.py:105-121), the PSNR and SSIM of
 * eval_satnerf.py:288-290 and main.py:194-195 -----------------------------------------------------------------------------------------
 * Both reductions accumulate in fp64 and write out (2 DEVICE doubles) = {sum, count}.  Each workgroup's partial goes to caller-owned
 * scratch and a second launch adds the partials in a fixed order; the grid depends on the shapes alone, so results are bitwise
 * repeatable.  No host synchronisation: capturable.
 * sr_image_metrics_scratch: HOST only; bytes of scratch that both sr_image_sse over n elements and sr_ssim_sum over (planes, h, w) need
 * (planes 0: the SSE alone).
 * sr_image_sse: metrics.mse's sum (metrics.py:105-112): sum of (pred - gt)^2 over n fp32 DEVICE elements, the difference and square
 * in fp64.  mask (optional, n / mask_div DEVICE bytes, n a multiple of mask_div): element i counts when mask[i / mask_div] != 0
 * (mask_div 1: per element; the trailing size: a mask over the leading dimensions, as torch boolean indexing).  count = the
 * elements used, so mse = sum / count (NaN when nothing is used).
 * sr_ssim_sum: the sum of kornia 0.5.3's losses.ssim map (metrics.py:116-121, window 3, max_val 1) over `planes` contiguous fp32
 * (h, w) planes of each image (NCHW, planes = B * C, 2 <= h, w): the 3x3 Gaussian (sigma 1.5) moments with reflect borders
 * (-1 -> 1, h -> h - 2), sigma = f(x^2) - mu^2 etc., map = ((2 mu1 mu2 + C1)(2 sigma12 + C2)) / ((mu1^2 + mu2^2 + C1)(sigma1^2 +
 * sigma2^2 + C2) + 1e-12), C1 = 0.01^2, C2 = 0.03^2, all in fp64.  count = planes * h * w, so ssim = sum / count. */
int sr_image_metrics_scratch(int64_t n, int64_t planes, int h, int w, int64_t* bytes);
int sr_image_sse(const float* pred, const float* gt, int64_t n, const uint8_t* mask, int64_t mask_div, void* scratch,
                 int64_t scratch_bytes, double* out, void* stream);
int sr_ssim_sum(const float* img1, const float* img2, int64_t planes, int h, int w, void* scratch, int64_t scratch_bytes, double* out,
                void* stream);

/* ---- a dataset's colours: load_tensor_from_rgb_geotiff (datasets/satellite.py:67-80) from the 8-bit image ------
 * src: DEVICE bytes of a 3-channel (src_h, src_w) image addressed as src[r * row_stride + c * pix_stride + k * chan_stride] (strides in
 * bytes, all >= 1: a dense HWC image is (3 w, 3, 1), a dense CHW image (w, 1, h w)); out: (out_h * out_w, 3) fp32 DEVICE rows,
 * out[(r * out_w + c) * 3 + k].  Values are v = (float)u8 / 255.0f, which is the reference's float32(float64(u8) / 255.) for all 256 bytes.
 * out_h == src_h and out_w == src_w: the plain conversion.  Any other size: torchvision's tensor Resize(BICUBIC) = ATen's
 * upsample_bicubic2d with align_corners=False and no antialias, all in fp32 with every product and sum rounded (no fma).  Per axis:
 * scale = (float)n_in / (float)n_out, src = scale * ((float)dst + 0.5f) - 0.5f, i0 = floorf(src), t = src - i0, taps i0 - 1 .. i0 + 2
 * clamped to [0, n_in - 1], with the cubic-convolution weights (A = -0.75) w(x) = ((A + 2) x - (A + 3)) x^2 + 1 for |x| <= 1 and
 * ((A x - 5 A) x + 8 A) x - 4 A for 1 < |x| < 2 at x = t + 1, t, 1 - t, 2 - t.  An output value is the 4 x 4 weighted sum (columns, then
 * rows) and is not clamped to [0, 1].  Both layouts of one image give the same bits.  out_h * out_w == 0: nothing is launched.  No
 * scratch and no host synchronisation: capturable. */
int sr_image_colors(const uint8_t* src, int src_h, int src_w, int64_t row_stride, int64_t pix_stride, int64_t chan_stride, int out_h,
                    int out_w, float* out, void* stream);

/* ---- a Blender scene's colours and rays: BlenderDataset (datasets/blender.py:12-209) after the PNG decode ------
 * sr_blender_colors: Pillow's 8-bit Image.resize((out_w, out_h), Image.LANCZOS) of one RGBA image, byte for byte, then ToTensor and the
 * blend onto white.  src: DEVICE bytes of a 4-channel (src_h, src_w) image addressed as src[r * row_stride + c * pix_stride + k *
 * chan_stride] (strides in bytes, all >= 1: dense HWC is (4 w, 4, 1), dense CHW (w, 1, h w)); both layouts give the same bits.  Sides:
 * source 1..65536, output 0..65536; out_h * out_w == 0 launches nothing.
 * Premultiply on load: c' = MULDIV255(c, a): t = c * a + 128, c' = ((t >> 8) + t) >> 8; alpha unchanged.
 * Coefficients, per axis, built on the HOST in fp64 and passed as DEVICE int32 tables coef (n_out, ksize), rows zero-padded
 * (coef_w: src_w -> out_w, coef_h: src_h -> out_h; NULL for an axis whose size does not change): scale = n_in / n_out, fs =
 * max(scale, 1), support = 3 fs, ksize = 2 ceil(support) + 1; for output index xx: center = (xx + 0.5) scale, xmin = max((int)(center -
 * support + 0.5), 0), xmax = min((int)(center + support + 0.5), n_in) - xmin, w[x] = L((x + xmin - center + 0.5) / fs) for x < xmax, L(x)
 * = sinc(x) sinc(x / 3) on -3 <= x < 3 and 0 elsewhere, sinc(0) = 1, else sinc(x) = sin(pi x) / (pi x); w is divided by its running sum
 * taken in index order; k = (int)(w 2^22 + 0.5) for w >= 0, (int)(w 2^22 - 0.5) for w < 0 (truncation toward zero).  xmin and xmax
 * are recomputed on the device from the same fp64 expressions (clamped to the source and to ksize), so there is no bounds table;
 * ksize_w / ksize_h must be the ksize above for the sizes given.
 * Each pass: acc = 2^21 + sum_x pixel[xmin + x] k[x] in int32 per band, output = clamp(acc >> 22, 0, 255) as u8.  Horizontal first,
 * over the four premultiplied bands, into scratch (src_h, out_w, 4) u8; the vertical pass runs over that.  A pass with n_out == n_in is
 * skipped; with both skipped the bytes are the source's own (no premultiply round trip).
 * Un-premultiply (after a pass ran): a == 0 or a == 255 keeps the colour bytes, else c = min(255 c' / a, 255), integer division.
 * Outputs (DEVICE): rgbs (out_h * out_w, 3) fp32 = v_c v_a + (1.0f - v_a) with v = (float)u8 / 255.0f, every product, difference and sum
 * rounded, not clamped (datasets/blender.py:139); valid_mask (out_h * out_w) u8 = a > 0, may be NULL; rgba (out_h * out_w, 4) u8, the
 * resized image, 4-byte aligned, may be NULL.
 * scratch: caller-owned DEVICE bytes, 4-byte aligned, at least sr_blender_colors_scratch (HOST only; 0 unless both passes run).
 * stages = 0 runs everything; 1 stops after the horizontal pass when a vertical one follows (timing only: no output is written).
 * Errors (null pointers with a non-empty output, strides < 1, sides out of range, a ksize that does not fit n_in -> n_out, scratch too
 * small or misaligned) return before anything touches the device.  No host synchronisation: capturable.
 * sr_pinhole_rays: get_ray_directions + get_rays + near / far (datasets/blender.py:12-59,142-149): out (h * w, 8) fp32 DEVICE rows
 * [o (3), d (3), near, far], 16-byte aligned, pixel (r, c) at row r * w + c.  fx, fy, cx, cy, near, far and c2w (HOST, 12 floats, row-major
 * (3, 4) = [R | o]) are fp32 as the reference's tensors hold them.  Per pixel in fp64, every operation rounded: dx = (c - cx) / fx, dy =
 * -((r - cy) / fy), dz = -1, w_k = (dx R[k][0] + dy R[k][1]) + dz R[k][2], n = sqrt((w_0^2 + w_1^2) + w_2^2), d_k = w_k / n rounded to
 * fp32 once; o = c2w[:, 3].  h * w == 0 launches nothing.  No scratch, no host synchronisation: capturable.
 * sr_blender_perturb: add_perturbation (datasets/blender.py:61-79) of one RGBA image, in front of sr_blender_colors.  src and dst: DEVICE
 * bytes of (h, w) images addressed with the same three byte strides as above (each 1..2^40); dst may be src (in place) or must not
 * overlap it.
 * Per pixel: every band's byte v becomes lut[k * 256 + v] (lut: HOST, 4 x 256 bytes, NULL = unchanged), then for i = 0 .. n_rects - 1 in
 * order a pixel with x0 <= c <= x1 and y0 <= r <= y1 (rects: HOST (n_rects, 4) int32 [x0, y0, x1, y1], both corners inside, any
 * integers: a rectangle is clipped to the image, one outside it or with x1 < x0 or y1 < y0 draws nothing) takes the four bytes
 * fills[4 i ..] (HOST (n_rects, 4) u8, RGBA); a later rectangle wins.  n_rects 0..16; rects and fills may be NULL when it is 0.  The
 * table and the rectangles are copied into the kernel's arguments: no upload, the host arrays are free on return.  One launch; a dense
 * 4-byte-aligned HWC image moves as one dword per pixel, anything else as bytes, with the same result.  Errors (null image, sides
 * outside 1..65536, strides outside 1..2^40, n_rects out of range, null rects or fills with n_rects > 0, partial overlap) return before anything
 * touches the device.  No scratch, no host synchronisation: capturable. */
int sr_blender_colors_scratch(int src_h, int src_w, int out_h, int out_w, int64_t* bytes);
int sr_blender_colors(const uint8_t* src, int src_h, int src_w, int64_t row_stride, int64_t pix_stride, int64_t chan_stride, int out_h,
                      int out_w, const int32_t* coef_w, int ksize_w, const int32_t* coef_h, int ksize_h, void* scratch,
                      int64_t scratch_bytes, float* rgbs, uint8_t* valid_mask, uint8_t* rgba, int stages, void* stream);
int sr_pinhole_rays(int h, int w, float fx, float fy, float cx, float cy, const float* c2w, float near, float far, float* out,
                    void* stream);
int sr_blender_perturb(const uint8_t* src, uint8_t* dst, int h, int w, int64_t row_stride, int64_t pix_stride, int64_t chan_stride,
                       const uint8_t* lut, const int32_t* rects, const uint8_t* fills, int n_rects, void* stream);

/* ---- evaluation image products: what study_solar_interpolation.py and train_utils.visualize_depth do to
 * rendered images ---------------------------------------------------------------------------------------------------------------------
 * Every image is DEVICE fp32 addressed as image[r * row_stride + c * col_stride] (strides in ELEMENTS, all >= 1): a dense (h, w) image
 * is (w, 1), column k of the (N, 13) buffer of the image render is image + k with (13 w, 13), and a crop window starting at (r0, c0)
 * is image + r0 * row_stride + c0 * col_stride with the window's sides.  The reference's window is rows int(h / 4) .. int(3 h / 4),
 * columns int(w / 4) .. int(3 w / 4).  Every entry returns its errors (null pointers with a non-empty image, sides or strides out of
 * range, a window that does not fit its strip, scratch too small or misaligned) before anything touches the device, launches nothing
 * for an empty image, and does no host synchronisation: capturable.
 *
 * sr_nearest_fill: quickly_interpolate_nans_from_singlechannel_img (study_solar_interpolation.py:53-68), i.e. scipy's
 * griddata(method="nearest"), on an (h, w) image with sides 0..8192.  A pixel is missing iff it is NaN (infinities and -0 are valid).
 * out (h, w) dense fp32: a valid pixel is copied bit for bit; a missing pixel (r, c) takes the bits of the valid pixel (r', c') that
 * minimises ((r - r')^2 + (c - c')^2, r', c') in lexicographic order -- the squared distance is an exact integer, and of several
 * pixels at the least distance the one in the smallest row, then the smallest column, wins (scipy leaves that choice to its KD-tree).
 * An image without a valid pixel comes back as it is, all NaN (scipy raises there).  index (optional, (h, w) int32, NULL to skip) =
 * r' * w + c' of the pixel taken (a valid pixel's own position), -1 where there is none.  out must not overlap image.  scratch:
 * caller-owned DEVICE bytes, 2-byte aligned, at least sr_nearest_fill_scratch (HOST only).  Two launches: a column pass (nearest
 * valid row per pixel and column, ties to the upper row) and a row pass (minimum of the packed key over the row's columns).
 *
 * sr_colorize: train_utils.visualize_depth (train_utils.py:59-72) and hstack_dsm_tifs_v1 after its fill
 * (study_solar_interpolation.py:85-93) over a (rows, cols) window, sides 0..65535.
 *   1. nan_to_zero = 1 (visualize_depth's np.nan_to_num): NaN -> 0, +-inf -> +-FLT_MAX.  nan_to_zero = 0: values are taken as they are.
 *   2. mi = vmin if bounds & 1 else the minimum over the window, ma = vmax if bounds & 2 else the maximum, both after step 1 and with
 *      NaN skipped; held as integer keys, so no arrival order changes them (a window of NaN only: mi = +inf, ma = -inf).  With
 *      bounds != 0, x is clipped: x < mi -> mi, then x > ma -> ma (a NaN stays).
 *   3. q = (x - mi) / d, y = 255.0f * q, index = (uint8_t)y by truncation; each a single correctly rounded fp32 operation.  d =
 *      (ma - mi) + 1e-8f, two rounded fp32 operations, unless bounds == 3: then d = denom, which the caller computes as the reference
 *      does from two Python floats, (float)((double)vmax - (double)vmin + 1e-8).  (numpy 2 keeps a Python float weak beside an fp32
 *      value, so with a measured bound the sum is fp32.)  Outside the reference's domain: a NaN or infinite y gives index 0, a finite
 *      y is clamped to 0..255.
 *   4. Outputs, any subset, NULL to skip: index_out (rows, cols) u8; strip: lut[index]'s three bytes at strip[(r * strip_cols +
 *      strip_col0 + c) * 3 + k], a caller's (rows, strip_cols, 3) u8 image (this placement is the reference's np.hstack); chw (3, rows,
 *      cols) fp32 = (float)lut[index][k] / 255.0f, torchvision's ToTensor and the expression of sr_image_colors.  lut: 256 x 3 DEVICE
 *      bytes, in the channel order the caller wants out.
 * scratch: 4-byte aligned DEVICE bytes, at least sr_colorize_scratch(bounds) (HOST only; 0 when both bounds are given).
 *
 * sr_unit_to_u8: hstack_sun_tifs / hstack_rgb_tifs (study_solar_interpolation.py:23-51): strip[(r * strip_cols + strip_col0 + c) *
 * channels + k] = (uint8_t)(image[r * row_stride + c * col_stride + k * chan_stride] * 255.0f), one rounded multiply, then truncation;
 * channels 1 or 3.  Composited sigmoid outputs lie in [0, 1]; outside it numpy's cast is undefined, and this kernel clamps to 0..255
 * with NaN -> 0. */
int sr_nearest_fill_scratch(int h, int w, int64_t* bytes);
int sr_nearest_fill(const float* image, int h, int w, int64_t row_stride, int64_t col_stride, void* scratch, int64_t scratch_bytes,
                    float* out, int32_t* index, void* stream);
int sr_colorize_scratch(int bounds, int64_t* bytes);
int sr_colorize(const float* image, int rows, int cols, int64_t row_stride, int64_t col_stride, int nan_to_zero, int bounds, float vmin,
                float vmax, float denom, const uint8_t* lut, uint8_t* index_out, uint8_t* strip, int64_t strip_cols, int64_t strip_col0,
                float* chw, void* scratch, int64_t scratch_bytes, void* stream);
int sr_unit_to_u8(const float* image, int rows, int cols, int channels, int64_t row_stride, int64_t col_stride, int64_t chan_stride,
                  uint8_t* strip, int64_t strip_cols, int64_t strip_col0, void* stream);

/* ---- training-step kernels --------------------------------------------------------------
 * sr_satnerf_loss: metrics.SatNerfLoss for the coarse model (metrics.py:21-25,56-73): value = sum of
 * loss_parts[0 .. ceil(N/4)), and grad_scale * dLoss/d{rgb (N,3), weights (N,S), beta (N,S)} in g_*.
 * sr_adam_step: torch.optim.Adam update (main.py:84) over a flat buffer; `step` is the 1-based step count; grads are
 * multiplied by grad_scale first and zeroed afterwards when zero_grad != 0. */
int sr_satnerf_loss(const float* rgb, const float* weights, const float* beta, const float* target, int64_t n_rays,
                    int n_samples, float beta_min, float grad_scale, const float* sched, float* loss_parts, float* g_rgb,
                    float* g_weights, float* g_beta, void* stream);
/* batch gather from a GPU-resident ray bank: rows idx[0..n) of rays (.,11), rgbs (.,3), ts (.) -> contiguous batch tensors
 * (replaces DataLoader collate + host-to-device copy, main.py:96-110).  cursor != NULL (a zero-initialised 4-float device
 * block, [3] scratch): idx holds the shuffled indices of a whole epoch = `batches` x n entries, the launch gathers batch
 * cursor[0] and advances the cursor modulo `batches` -- inside a captured training step the sampler needs no host work */
int sr_gather_batch(const float* rays, const float* rgbs, const int64_t* ts, const int64_t* idx, int64_t n, float* out_rays,
                    float* out_rgbs, int64_t* out_ts, float* cursor, int64_t batches, void* stream);
/* sr_gather_batch + sr_ray_setup_rng in ONE launch (one wave per ray) for captured steps that sample for themselves: the rows go to
 * the static batch tensors, z_vals (n, n_samples) and sky (n,3) are computed from the row just read; the jitter step is
 * step_counter[0] + step_offset (the launch runs before sr_pack_all ticks that counter: offset 1 reproduces sr_ray_setup_rng's draws) */
int sr_gather_setup(const float* rays, const float* rgbs, const int64_t* ts, const int64_t* idx, int64_t n, float* out_rays,
                    float* out_rgbs, int64_t* out_ts, float* cursor, int64_t batches, int n_samples, int hidden, const float* w1,
                    const float* b1, const float* w2, const float* b2, float* z_vals, float* sky, uint64_t seed,
                    const float* step_counter, int step_offset, void* stream);
int sr_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                 float beta2, float eps, float grad_scale, int64_t step, int zero_grad, void* stream);

/* ---- sigma -> alpha compositing: models/satnerf.py:52-70 ------------------------------------------
 * noise may be NULL (== noise_std 0).  sky is per ray (N,3).  Outputs: weights, transparency (N,S),
 * depth (N), rgb (N,3) (clamped to [0,1] when clamp_rgb != 0; the classic nerf variant does not clamp,
 * models/nerf.py:128, and passes sun_v = sky = NULL). */
int sr_composite_fwd(const float* z_vals, const float* sigma, const float* noise, float noise_std,
                     const float* albedo, const float* sun_v, const float* sky, int64_t n_rays, int n_samples,
                     int clamp_rgb, float* weights, float* transparency, float* depth, float* rgb, void* stream);

/* closed-form backward of sr_composite_fwd.  Upstream grads g_* may be NULL (=0).
 * Produces d_sigma (N,S), d_albedo (N,S,3), d_sun_v (N,S), d_sky (N,3); any output may be NULL. */
int sr_composite_bwd(const float* z_vals, const float* sigma, const float* noise, float noise_std,
                     const float* albedo, const float* sun_v, const float* sky, const float* weights,
                     const float* transparency, const float* rgb_unclamped_or_null, int64_t n_rays, int n_samples,
                     int clamp_rgb, const float* g_rgb, const float* g_depth, const float* g_weights,
                     const float* g_transparency, float* d_sigma, float* d_albedo, float* d_sun_v, float* d_sky,
                     void* stream);

/* ---- importance resampling + merge: rendering.py:10-49 and :121-125 -------------------------------
 * z_coarse (N,S) sorted, weights_coarse (N,S), u (N,I) -> z_fine (N,S+I) = sort(cat(z_coarse, z_new)). */
int sr_sample_pdf_merge(const float* z_coarse, const float* weights_coarse, const float* u, int64_t n_rays,
                        int n_samples, int n_importance, float eps, float* z_fine, void* stream);
/* stand-alone rendering.sample_pdf (rendering.py:10-49): bins (N,nb), weights (N,nb-1), u (N,I) -> samples (N,I) */
int sr_sample_pdf(const float* bins, const float* weights, const float* u, int64_t n_rays, int n_bins, int n_importance,
                  float eps, float* samples, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SATRENDER_H */
