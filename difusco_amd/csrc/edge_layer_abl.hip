// Profiling-only variants of the fp16 middle-layer kernel (edge_layer_kernel.h): compile-time ablation masks selected
// with difusco_debug_set(0, mask).  Results are WRONG for every mask except 16 (production code + phase timestamps).
#include "edge_layer_kernel.h"

namespace difusco {
hipError_t launch_fused_ablation(int mask, const FusedLayerArgs& a) {
  switch (mask) {
    case 1: return launch_fused_t<FFp16, 1, FUSED_NW>(a);      // no neighbour-table gathers
    case 2: return launch_fused_t<FFp16, 2, FUSED_NW>(a);      // no neighbour sum
    case 4: return launch_fused_t<FFp16, 4, FUSED_NW>(a);      // no LayerNorm / activation math
    case 8: return launch_fused_t<FFp16, 8, FUSED_NW>(a);      // no GEMM 2
    case 15: return launch_fused_t<FFp16, 15, FUSED_NW>(a);    // GEMM 1 + weight streaming only
    case 16: return launch_fused_t<FFp16, 16, FUSED_NW>(a);    // production code + phase timestamps
    case 17: return launch_fused_t<FFp16, 15, FUSED_NW, false, false, 0, FUSED_OPT_R2>(a);   // 15 with the production options
    case 18: return launch_fused_t<FFp16, 16, FUSED_NW, false, false, 0, FUSED_OPT>(a);   // 16 (phase stamps), production options (full-line gathers)
    case 19: return launch_fused_t<FFp16, 16, FUSED_NW, false, false, 0, FUSED_OPT_R2>(a);   // stamps, round 2's options (register gathers)
    case 34: return launch_fused_t<FFp16, 16 + 1024, FUSED_NW, false, false, 0, FUSED_OPT>(a);   // stamps, gather requests never waited for
    case 35: return launch_fused_t<FFp16, 16 + 1024 + 2048, FUSED_NW, false, false, 0, FUSED_OPT>(a);   // stamps, no gather requests, no waits
    case 36: return launch_fused_t<FFp16, 1024, FUSED_NW, false, false, 0, FUSED_OPT>(a);   // (no stamps) gather requests never waited for
    case 37: return launch_fused_t<FFp16, 1024 + 2048, FUSED_NW, false, false, 0, FUSED_OPT>(a);   // (no stamps) no gather requests, no waits
    // round 6, traffic attribution (profiles/r06/reread_attribution.txt): ONE access class off at a time, production options, no stamps
    case 38: return launch_fused_t<FFp16, 16384, FUSED_NW, false, false, 0, FUSED_OPT>(a);   // no weight-stage refills / barriers (stale LDS)
    case 39: return launch_fused_t<FFp16, 32768, FUSED_NW, false, false, 0, FUSED_OPT>(a);   // no e stream into GEMM 1
    case 40: return launch_fused_t<FFp16, 32, FUSED_NW, false, false, 0, FUSED_OPT>(a);      // no residual read, no e store
    case 41: return launch_fused_t<FFp16, 128, FUSED_NW, false, false, 0, FUSED_OPT>(a);     // no B h[i] loads
    case 42: return launch_fused_t<FFp16, 128 + 1024 + 2048, FUSED_NW, false, false, 0, FUSED_OPT>(a);   // no node-table access at all
    case 22: return launch_fused_t<FFp16, 16 + 32768, FUSED_NW, false, false, 0, FUSED_OPT_R2>(a);   // stamps, no e stream
    case 23: return launch_fused_t<FFp16, 16 + 16384, FUSED_NW, false, false, 0, FUSED_OPT_R2>(a);   // stamps, no stage refills / barriers
    case 24: return launch_fused_t<FFp16, 16 + 1, FUSED_NW, false, false, 0, FUSED_OPT_R2>(a);       // stamps, no gathers
    case 27: return launch_fused_t<FFp16, 16 + 65536, FUSED_NW, false, false, 0, FUSED_OPT_R2>(a);     // stamps, stage requests not waited for
    case 28: return launch_fused_t<FFp16, 16 + 131072, FUSED_NW, false, false, 0, FUSED_OPT_R2>(a);    // stamps, no stage barrier
    case 29: return launch_fused_t<FFp16, 16 + 196608, FUSED_NW, false, false, 0, FUSED_OPT_R2>(a);    // stamps, neither (requests still issued)
    case 30: return launch_fused_t<FFp16, 16 + 128, FUSED_NW, false, false, 0, FUSED_OPT_R2>(a);       // stamps, no B h[i] gathers
    case 31: return launch_fused_t<FFp16, 16 + 256, FUSED_NW, false, false, 0, FUSED_OPT_R2>(a);       // stamps, no A h[j] / V h[j] gathers
    case 32:      // stamps, LAST layer of a TSP step (no V gathers / gate / neighbour sum; GroupNorm partial sums go to `part`)
    {
      FusedLayerArgs t = a;
      t.gn_tile = a.part, t.etmax_out = nullptr;
      return launch_fused_t<FFp16, 16, FUSED_NW, false, true, 1, FUSED_OPT_R2>(t);
    }
    case 33:      // stamps, FIRST layer (two-row table instead of e and GEMM 1; the table rows are taken from b_c .. for timing only)
    {
      FusedLayerArgs t = a;
      t.l0_table = a.node4;
      return launch_fused_t<FFp16, 16, FUSED_NW, true, false, 0, FUSED_OPT_R2>(t);
    }
    default: return hipErrorInvalidValue;
  }
}
}  // namespace difusco
