// the geometry (trunk + sigma) build of the fused forward kernel, fp16 operands (SR_MODE_F16): both aux sizes, a translation unit of its own
// (two short streams weigh about what one full unit does in the parallel build)
#define SR_F16 1
#include "mlp_fwd2.inc"
namespace sr {
int launch_fwd_geom_h1a1(const FwdParams& p, hipStream_t st) { return launch_fwd_geom<1>(p, st, launch_fwd_h1a1); }
int launch_fwd_geom_h1a2(const FwdParams& p, hipStream_t st) { return launch_fwd_geom<2>(p, st, launch_fwd_h1a2); }
}  // namespace sr
