// one-plane fp16 instantiations of the fused edge-layer kernel (edge_layer_kernel.h): precision DIFUSCO_PREC_FP16X1.
#include "edge_layer_kernel.h"

namespace difusco {
hipError_t launch_fused_fp16x1(int kind, const FusedLayerArgs& a) { return launch_fused_kind<FFp16x1>(kind, a); }
}  // namespace difusco
