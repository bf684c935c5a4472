// the geometry (trunk + sigma) build of the fused forward kernel, bf16 operands: both aux sizes, a translation unit of its own
// (two short streams weigh about what one full unit does in the parallel build)
#include "mlp_fwd2.inc"
namespace sr {
int launch_fwd_geom_p1a1(const FwdParams& p, hipStream_t st) { return launch_fwd_geom<1>(p, st, launch_fwd_p1a1); }
int launch_fwd_geom_p1a2(const FwdParams& p, hipStream_t st) { return launch_fwd_geom<2>(p, st, launch_fwd_p1a2); }
}  // namespace sr
