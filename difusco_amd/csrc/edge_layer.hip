// Fused edge pass of one DIFUSCO GNN layer for gfx950 (H = 256): the launcher (one entry, launch_edge_layer_fused, taking a
// FusedLayerArgs record), the node update that follows the edge pass, and the fp16 production instantiations of the kernel
// template in edge_layer_kernel.h.
#include "edge_layer_kernel.h"

namespace difusco {

// ------------------------------------------------------------------------------------------------
// node update after the fused edge pass:  h_i += ReLU(LN_h(Uh_i + sum_j gate*Vh_j)) (+ t, MIS)
// (gnn_encoder.py:115,123,134,447-448).  One wavefront per node; the neighbour sum is assembled from the
// per-tile pieces written by edge_layer_fused_kernel, in tile order.  agg_mode 1 (aggregation = "mean",
// gnn_encoder.py:170-171,184-185): the sum is divided by the number of edges of the row (empty row: 0); agg_mode 2 ("max",
// :172-173,187-188): the pieces are maxima and are combined by maximum (empty row: 0).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void node_finalize_kernel(int n_nodes, int n_edges, const int* __restrict__ rowptr,
                                                            const float* __restrict__ node4,
                                                            const float* __restrict__ part,
                                                            const float* __restrict__ direct, float* h,
                                                            const float* __restrict__ nh_w,
                                                            const float* __restrict__ nh_b,
                                                            const float* __restrict__ tbias, int time_on_edge,
                                                            float* __restrict__ row_scale, const float* h_in,
                                                            int agg_mode) {
  constexpr int H = 256;
  const int lane = threadIdx.x & 63;
  const int f = lane * 4;
  const int i = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (i >= n_nodes) return;
  const int a = rowptr[i], b = rowptr[i + 1];
  const bool agg_mean = agg_mode == 1, agg_max = agg_mode == 2 && b > a;      // (wave uniform)
  v4f agg = {0.0f, 0.0f, 0.0f, 0.0f};
  if (agg_max) agg = v4f{-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  if (b > a) {
    const int t0 = a >> 5, t1 = (b - 1) >> 5;
    for (int t = t0; t <= t1; ++t) {
      const int first = 32 * t;
      int last = first + 31;
      last = last < n_edges ? last : n_edges - 1;
      // (a single-segment tile writes part[tile][0] only: a row that covers the whole tile takes the first branch; in the last
      //  tile `last` is the launch's last edge, whose row the pad lanes extend)
      const float* src;
      if (a <= first) src = part + ((long long)t * 2 + 0) * H;          // owns the tile's first edge
      else if (b > last) src = part + ((long long)t * 2 + 1) * H;       // owns the tile's last edge
      else src = direct + (long long)i * H;                              // strictly inside the tile
      const v4f piece = *reinterpret_cast<const v4f*>(src + f);
      if (agg_max) {      // (the pieces are maxima: kinds 8, 9, 11 of the fused kernel)
#pragma unroll
        for (int q = 0; q < 4; ++q) agg[q] = __builtin_fmaxf(agg[q], piece[q]);
      } else {
        agg += piece;
      }
    }
    if (agg_mean) {      // (wave uniform) true divisions: the value of sum / count
      const float cnt = (float)(b - a);
#pragma unroll
      for (int q = 0; q < 4; ++q) agg[q] = agg[q] / cnt;
    }
  }
  const v4f uh = *reinterpret_cast<const v4f*>(node4 + (long long)i * 4 * H + f);
  v4f x = uh + agg;
  constexpr float inv_h = 1.0f / 256.0f;
  const float mean = wave_sum(x[0] + x[1] + x[2] + x[3]) * inv_h;
  v4f d = x - mean;
  const float rstd = 1.0f / sqrtf(wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) * inv_h + 1e-5f);
  const v4f gw = *reinterpret_cast<const v4f*>(nh_w + f), gb = *reinterpret_cast<const v4f*>(nh_b + f);
  const v4f tb = *reinterpret_cast<const v4f*>(tbias + f);
  float* hp = h + (long long)i * H + f;
  v4f hv = *reinterpret_cast<const v4f*>(h_in + (long long)i * H + f);      // (h_in == h: in place)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float y = d[q] * rstd * gw[q] + gb[q];
    y = y > 0.0f ? y : 0.0f;
    if (!time_on_edge) y += tb[q];
    hv[q] += y;
  }
  *reinterpret_cast<v4f*>(hp) = hv;
  if (row_scale != nullptr) {      // power-of-two operand scale of this row for the next node-row linear (fp16 planes)
    float m = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(hv[0]), __builtin_fabsf(hv[1])),
                              __builtin_fmaxf(__builtin_fabsf(hv[2]), __builtin_fabsf(hv[3])));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, off, 64));
    float inv;
    const float sc = pow2_scale_for(m, inv);
    if (lane == 0) row_scale[i] = sc;
  }
}

#ifdef DIFUSCO_PROFILING
// process-wide knobs of the PROFILING library (libdifusco_hip_prof.so, difusco_debug_set); the production library has none
int g_fused_ablate = 0;   // ablation mask (difusco_debug_set key 0): wrong results by construction, timing only
int g_fused_lds_pad = 0;  // extra dynamic LDS bytes: occupancy probe (key 6)
int g_fused_start_delay = 0;   // cycles by which the second-slot workgroups of the first generation start late (key 9)
int g_fused_opt = FUSED_OPT;   // key 7: A/B variants of the scheduling options
unsigned long long* g_fused_dbg = nullptr;   // device buffer for phase timestamps, [n_tiles][16]
#endif

hipError_t launch_fused_fp16(int kind, const FusedLayerArgs& a) { return launch_fused_kind<FFp16>(kind, a); }

// The one launcher of the fused edge pass (kernels.h: FusedKind, FusedLayerArgs, mode, variant).
hipError_t launch_edge_layer_fused(int mode, FusedKind fk, int variant, const FusedLayerArgs& a) {
  if (a.n_edges <= 0) return hipSuccess;
#ifdef DIFUSCO_PROFILING
  // profiling-only variants exist for the fp16 middle layer
  if (fk == FusedKind::Middle && mode == 3 && g_fused_ablate != 0) return launch_fused_ablation(g_fused_ablate, a);
#endif
  int kind = (int)fk;      // kinds of launch_fused_kind: + 4 register gathers, + 8 max aggregation
  if (variant & 2) {
    if (variant & 1) return hipErrorInvalidValue;
    if (fk != FusedKind::TailTsp) kind += 8;      // (the last layer of a TSP step has no neighbour aggregation)
  } else if (variant & 1) {
    kind += 4;
  }
  if (mode == 1) return launch_fused_bf16(kind, a);     // DIFUSCO_PREC_BF16X3
  if (mode == 3) return launch_fused_fp16(kind, a);     // DIFUSCO_PREC_FP16X3
  if (mode == 4) return launch_fused_fp16x1(kind, a);   // DIFUSCO_PREC_FP16X1
  return hipErrorInvalidValue;
}

// The reference's node rows -> the fused kernel's log2(e) domain (only the stand-alone layer entry difusco_edge_layer_fused needs
// this pass: the step driver's node linear writes the rows in that form).  One thread per float4.
__global__ __launch_bounds__(256) void fuse_node_tables_kernel(const float* __restrict__ node4, const float* __restrict__ b_c,
                                                               long long n_vec, float* __restrict__ out) {
  constexpr float kLog2e = 1.4426950408889634f;
  const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_vec) return;
  const int c = (int)(v & 255) * 4;      // column inside the 1024-float row
  v4f x = *reinterpret_cast<const v4f*>(node4 + v * 4);
  if (c >= 512) {
    if (c < 768) x += *reinterpret_cast<const v4f*>(b_c + (c - 512));
    x = x * kLog2e;
  }
  *reinterpret_cast<v4f*>(out + v * 4) = x;
}

hipError_t launch_fuse_node_tables(const float* node4, const float* b_c, int n_nodes, float* out, hipStream_t stream) {
  if (n_nodes <= 0) return hipSuccess;
  const long long n_vec = (long long)n_nodes * 256;
  hipLaunchKernelGGL(fuse_node_tables_kernel, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0, stream, node4, b_c, n_vec, out);
  return hipGetLastError();
}

hipError_t launch_node_finalize(int n_nodes, int n_edges, const int* rowptr, const float* node4, const float* part,
                                const float* direct, float* h, const float* nh_w, const float* nh_b,
                                const float* tbias, int time_on_edge, float* row_scale, hipStream_t stream,
                                const float* h_in, int agg_mode) {
  if (n_nodes <= 0) return hipSuccess;
  if (agg_mode < 0 || agg_mode > 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(node_finalize_kernel, dim3((unsigned)((n_nodes + 3) / 4)), dim3(256), 0, stream, n_nodes, n_edges,
                     rowptr, node4, part, direct, h, nh_w, nh_b, tbias, time_on_edge, row_scale, h_in ? h_in : h, agg_mode);
  return hipGetLastError();
}

}  // namespace difusco
