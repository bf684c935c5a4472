// C ABI of the fused forward MLP.  One table (kFwdUnits) says which (width, mode) units exist and what each one launches; one routine
// (fwd_request) checks a request of any of the five entries, fills the parameter block and reaches the unit's launcher.  A new
// (width, mode) unit is one table row; a new entry is one call of fwd_request and, where it differs, one block there.
#include "common.h"
#include "mlp_layout.h"
#include "mlp_params.h"
using namespace sr;

// (width, mode) -> the translation units' entries (declared in mlp_params.h), indexed by aux steps - 1
struct FwdUnit {
  int feat, mode;
  int waves;              // per workgroup, each one 32-point tile
  FwdLaunch full[2];
  FwdGeomLaunch geom[2];  // null: a sigma-only request runs the full kernel with the unused outputs null (the parity mode)
  long (*pieces[2])();    // 512-byte pieces of the width's forward stream
};
static const FwdUnit kFwdUnits[] = {
    {kFeat, SR_MODE_BF16, kFwdWaves256, {launch_fwd_p1a1, launch_fwd_p1a2}, {launch_fwd_geom_p1a1, launch_fwd_geom_p1a2},
     {FwdStream<1>::total_pieces, FwdStream<2>::total_pieces}},
    {kFeat, SR_MODE_F16, kFwdWaves256, {launch_fwd_h1a1, launch_fwd_h1a2}, {launch_fwd_geom_h1a1, launch_fwd_geom_h1a2},
     {FwdStream<1>::total_pieces, FwdStream<2>::total_pieces}},
    {kFeat, SR_MODE_BF16X3, kFwdWavesParity, {launch_fwd_p3a1, launch_fwd_p3a2}, {nullptr, nullptr},
     {FwdStream<1>::total_pieces, FwdStream<2>::total_pieces}},
    {512, SR_MODE_BF16, kFwdWaves512, {launch_fwd512_p1a1, launch_fwd512_p1a2}, {launch_fwd512_geom_p1a1, launch_fwd512_geom_p1a2},
     {fwd512_stream_pieces_a1, fwd512_stream_pieces_a2}},
    {512, SR_MODE_F16, kFwdWaves512, {launch_fwd512_h1a1, launch_fwd512_h1a2}, {launch_fwd512_geom_h1a1, launch_fwd512_geom_h1a2},
     {fwd512_stream_pieces_a1, fwd512_stream_pieces_a2}},
};

// the row of (feat, mode); null: no fused kernel
static const FwdUnit* fwd_unit(int feat, int mode) {
  for (const FwdUnit& u : kFwdUnits)
    if (u.feat == feat && u.mode == mode) return &u;
  return nullptr;
}

extern "C" int64_t sr_fwd_stream_elems(int feat, int tau) {
  if (tau < 1 || tau > 24) return -1;
  for (const FwdUnit& u : kFwdUnits)
    if (u.feat == feat) return u.pieces[aux_steps(tau) - 1]() * 512;  // one stream layout per width, whatever the mode
  return -1;
}

extern "C" int sr_render_points_per_block(int feat, int mode) {
  const FwdUnit* unit = fwd_unit(feat, mode);
  return unit != nullptr ? unit->waves * 32 : -1;
}

// Every entry's request: a point launch (pt; out names the per-point outputs) or a render pass (pt == NULL: in, out, and tr for the
// training launch); geom = sigma and what follows from it alone.  All checks come before the empty return, so a bad empty request
// is refused too.  The two families word their common checks differently, as they always have.
static int fwd_request(const char* who, const sr_mlp_inputs* pt, const sr_render_args* in, const sr_render_outputs* out, const sr_train_args* tr,
                       uint16_t* acts, int act_fmt, bool geom, int feat, int tau, int mode, const uint16_t* stream_hi,
                       const uint16_t* stream_lo, const float* l0, void* stream) {
  const bool render = pt == nullptr;
  const FwdUnit* unit = fwd_unit(feat, mode);
  const bool lo_ok = mode != SR_MODE_BF16X3 || stream_lo;
  if (render) {
    SR_REQUIRE(in != nullptr && out != nullptr, "%s: null argument block", who);
    SR_REQUIRE(unit != nullptr, "%s: no fused kernel for feat=%d mode=%d (256: every mode; 512: SR_MODE_BF16 / SR_MODE_F16)", who, feat, mode);
  } else {
    SR_REQUIRE(feat == kFeat || feat == 512, "%s: feat=%d unsupported (this build handles %d and 512)", who, feat, kFeat);
    SR_REQUIRE(mode == SR_MODE_BF16 || mode == SR_MODE_BF16X3 || mode == SR_MODE_F16, "%s: bad mode %d", who, mode);
    if (geom) {
      SR_REQUIRE(unit != nullptr, "%s: feat=512 runs the fused kernel in SR_MODE_BF16 / SR_MODE_F16 (parity mode: layer by layer)", who);
    } else {
      SR_REQUIRE(unit != nullptr && (feat == kFeat || acts == nullptr || act_fmt == SR_FMT8),
                 "%s: feat=512 runs the fused kernel in SR_MODE_BF16 / SR_MODE_F16, saving activations in SR_FMT8 only (parity mode: layer by layer)", who);
    }
  }
  SR_REQUIRE(tau >= 1 && tau <= 24, "%s: tau=%d unsupported (1..24)", who, tau);
  if (render) {
    const int per_block = unit->waves * 32;
    SR_REQUIRE(in->n_samples >= 2 && per_block % in->n_samples == 0, "%s: n_samples=%d must be >= 2 and divide %d (sr_render_points_per_block)", who,
               in->n_samples, per_block);
    SR_REQUIRE(in->rays && in->ts && in->temb && in->ray_stride >= 11, "%s: rays (stride >= 11), ts and temb are required", who);
    SR_REQUIRE(stream_hi && l0 && lo_ok, "%s: null weight stream", who);
    const bool sky_ok = in->sky_w1 && in->sky_b1 && in->sky_w2 && in->sky_b2 && in->sky_hidden >= 1;
    if (geom) {
      SR_REQUIRE(out->weights && out->transparency && out->depth, "%s: weights, transparency and depth outputs are required", who);
      SR_REQUIRE(in->tick == 0 || in->tick == 1, "%s: tick must be 0 or 1", who);
    } else {
      SR_REQUIRE(sky_ok, "%s: the sky head's weights are required", who);
      SR_REQUIRE(tr != nullptr || (out->weights && out->transparency), "%s: weights and transparency outputs are required", who);
    }
    SR_REQUIRE(!in->tick || in->step_counter, "%s: tick needs the 4-float step counter block", who);
    SR_REQUIRE(in->bank_chunks >= 0 && (in->bank_chunks == 0 || in->step_counter), "%s: bank_chunks needs the step counter", who);
    if (geom) {
      // the geometry core reads no sky weight; the full kernel that serves the request elsewhere evaluates the sky head whatever is stored
      const bool full_kernel = unit->geom[0] == nullptr || fwd_v1_forced();
      SR_REQUIRE(!full_kernel || sky_ok,
                 "%s: this configuration runs the full kernel (parity mode or SATNERF_FWD_V1), which needs the sky head's weights", who);
    } else {
      if (tr != nullptr) {
        SR_REQUIRE(mode == SR_MODE_BF16 || mode == SR_MODE_F16, "%s: the fused training forward exists for SR_MODE_BF16 / SR_MODE_F16 (8-bit saved state)", who);
        SR_REQUIRE(acts != nullptr && act_fmt == SR_FMT8, "%s: needs the SR_FMT8 activation workspace", who);
        SR_REQUIRE(in->n_samples <= 64, "%s: n_samples=%d unsupported (one wave per ray: <= 64); use the separate launches", who, in->n_samples);
        SR_REQUIRE(tr->target && tr->loss_parts && tr->d_sigma && tr->d_albedo && tr->d_sun_v && tr->g_beta && tr->d_sky && out->sky, "%s: null training output", who);
        SR_REQUIRE(out->albedo && out->sigma && out->sun_v && out->beta, "%s: the four per-point outputs are required (the dX pass reads them)", who);
        if (tr->gather_idx != nullptr) {
          SR_REQUIRE(tr->cursor && tr->batches >= 1 && tr->batches < (1 << 24), "%s: the in-launch sampler needs a cursor block and 1 <= batches < 2^24", who);
          SR_REQUIRE(tr->out_rays && tr->out_rgbs && tr->out_ts, "%s: the in-launch sampler needs out_rays / out_rgbs / out_ts", who);
          SR_REQUIRE(in->ray_stride == 11 && in->bank_chunks == 0 && in->z_in == nullptr && in->u == nullptr && in->noise == nullptr,
                     "%s: the in-launch sampler takes a bank of 11-float rows and draws its own jitter (no z_in / u / noise / bank_chunks)", who);
        }
      }
      SR_REQUIRE(in->tick != 2 || (tr != nullptr && in->bank_chunks == 0), "%s: tick == 2 (tick first) is a training-launch option", who);
      SR_REQUIRE(in->tick >= 0 && in->tick <= 2, "%s: tick must be 0, 1 or 2", who);
    }
    if (in->n_rays <= 0) return 0;
  } else {
    SR_REQUIRE(stream_hi && l0 && pt->org && pt->sun && pt->temb, "%s: null pointer argument", who);
    SR_REQUIRE(lo_ok, "%s: BF16X3 needs the lo plane", who);
    SR_REQUIRE(pt->n_samples >= 1, "%s: n_samples must be >= 1", who);
    SR_REQUIRE(acts == nullptr || act_fmt == SR_FMT16 || act_fmt == SR_FMT8, "%s: act_fmt must be 16 or 8 (got %d)", who, act_fmt);
    if (pt->n_points <= 0) return 0;
  }

  FwdParams p{};  // no render pass, no training epilogue
  if (render) {
    p.in.org = in->rays, p.in.org_stride = in->ray_stride;
    p.in.dir = in->rays + 3, p.in.dir_stride = in->ray_stride;
    p.in.sun = in->rays + 8, p.in.sun_stride = in->ray_stride;
    p.in.temb = in->temb, p.in.ts = in->ts;
    p.in.n_points = in->n_rays * in->n_samples, p.in.n_samples = in->n_samples;
    RenderParams& r = p.rend;
    r.rays = in->rays, r.ray_stride = in->ray_stride, r.z_in = in->z_in, r.u = in->u, r.seed = in->seed, r.step_counter = in->step_counter;
    r.tick = in->tick, r.noise = in->noise, r.noise_std = in->noise_std, r.sky_hidden = in->sky_hidden;
    r.w1 = in->sky_w1, r.b1 = in->sky_b1, r.w2 = in->sky_w2, r.b2 = in->sky_b2;
    r.z_out = out->z_vals, r.weights = out->weights, r.transp = out->transparency, r.depth = out->depth;
    if (!geom) r.sky = out->sky, r.rgb = out->rgb;
    r.n_rays = in->n_rays, r.bank_chunks = in->bank_chunks;
  } else {
    p.in = *pt;
  }
  if (tr != nullptr) {
    TrainParams& t = p.train;
    t.target = tr->target, t.sched = tr->sched, t.beta_min = tr->beta_min, t.loss_parts = tr->loss_parts, t.rgb = tr->rgb;
    t.d_sigma = tr->d_sigma, t.d_albedo = tr->d_albedo, t.d_sun = tr->d_sun_v, t.g_beta = tr->g_beta, t.d_sky = tr->d_sky;
    t.gather_idx = (const long long*)tr->gather_idx, t.cursor = tr->cursor, t.batches = (unsigned)tr->batches;
    t.out_rays = tr->out_rays, t.out_rgbs = tr->out_rgbs, t.out_ts = (long long*)tr->out_ts;
  }
  p.stream_hi = (const char*)stream_hi, p.stream_lo = (const char*)stream_lo, p.l0 = (const float4*)l0;
  p.sigma = out->sigma;
  if (!geom) p.albedo = out->albedo, p.sun_v = out->sun_v, p.beta = out->beta;  // a geometry request leaves what it does not name null
  p.acts = (uint4*)acts, p.tau = tau;
  const int a = aux_steps(tau) - 1;
  if (geom && unit->geom[a] != nullptr) return unit->geom[a](p, (hipStream_t)stream);
  return unit->full[a](p, acts != nullptr ? act_fmt : 0, (hipStream_t)stream);
}

extern "C" int sr_satnerf_mlp_fwd(const sr_mlp_inputs* in, int feat, int tau, int mode, const uint16_t* stream_hi,
                                  const uint16_t* stream_lo, const float* l0, float* albedo, float* sigma, float* sun_v, float* beta,
                                  uint16_t* acts, int act_fmt, void* stream) {
  SR_REQUIRE(in != nullptr, "sr_satnerf_mlp_fwd: null inputs");
  sr_render_outputs out{};
  out.albedo = albedo, out.sigma = sigma, out.sun_v = sun_v, out.beta = beta;
  return fwd_request("sr_satnerf_mlp_fwd", in, nullptr, &out, nullptr, acts, act_fmt, false, feat, tau, mode, stream_hi, stream_lo, l0, stream);
}

extern "C" int sr_satnerf_mlp_sigma(const sr_mlp_inputs* in, int feat, int tau, int mode, const uint16_t* stream_hi, const uint16_t* stream_lo,
                                    const float* l0, float* sigma, void* stream) {
  SR_REQUIRE(in != nullptr && sigma != nullptr, "sr_satnerf_mlp_sigma: null inputs or output");
  sr_render_outputs out{};
  out.sigma = sigma;
  return fwd_request("sr_satnerf_mlp_sigma", in, nullptr, &out, nullptr, nullptr, 0, true, feat, tau, mode, stream_hi, stream_lo, l0, stream);
}

extern "C" int sr_satnerf_render_fwd(const sr_render_args* in, int feat, int tau, int mode, const uint16_t* stream_hi, const uint16_t* stream_lo,
                                     const float* l0, const sr_render_outputs* out, void* stream) {
  return fwd_request("sr_satnerf_render_fwd", nullptr, in, out, nullptr, nullptr, 0, false, feat, tau, mode, stream_hi, stream_lo, l0, stream);
}

extern "C" int sr_satnerf_render_depth(const sr_render_args* in, int feat, int tau, int mode, const uint16_t* stream_hi, const uint16_t* stream_lo,
                                       const float* l0, const sr_render_outputs* out, void* stream) {
  return fwd_request("sr_satnerf_render_depth", nullptr, in, out, nullptr, nullptr, 0, true, feat, tau, mode, stream_hi, stream_lo, l0, stream);
}

extern "C" int sr_satnerf_render_train(const sr_render_args* in, int feat, int tau, int mode, const uint16_t* stream_hi, const uint16_t* stream_lo,
                                       const float* l0, const sr_render_outputs* out, const sr_train_args* train, uint16_t* acts, int act_fmt,
                                       void* stream) {
  SR_REQUIRE(train != nullptr, "sr_satnerf_render_train: null training argument block");
  return fwd_request("sr_satnerf_render_train", nullptr, in, out, train, acts, act_fmt, false, feat, tau, mode, stream_hi, stream_lo, l0, stream);
}
