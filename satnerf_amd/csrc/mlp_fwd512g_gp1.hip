// the geometry (trunk + sigma) build of the 512-wide fused forward kernel, bf16 operands: both aux sizes
#define SR_FEAT 512
#include "mlp_fwd512g.inc"
namespace sr {
int launch_fwd512_geom_p1a1(const FwdParams& p, hipStream_t st) { return launch_fwd512_geom<1>(p, st, launch_fwd512_p1a1); }
int launch_fwd512_geom_p1a2(const FwdParams& p, hipStream_t st) { return launch_fwd512_geom<2>(p, st, launch_fwd512_p1a2); }
}  // namespace sr
