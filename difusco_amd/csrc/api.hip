// C ABI of libdifusco_hip.so (declared in include/difusco_hip.h) and the step driver that strings the
// gfx950 kernels into one reverse-diffusion step.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/difusco_hip.h"
#include "kernels.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(DIFUSCO_EHIP, "%s: %s", #expr, hipGetErrorString(e_));  \
  } while (0)

}  // namespace

namespace difusco {
// error reporting for the other translation units of the library (same thread-local message buffer)
int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace difusco

namespace {

constexpr int64_t kAlignFloats = 64;  // every packed tensor starts on a 256-byte boundary

int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

struct Layout {
  std::vector<int64_t> off;
  int64_t total = 0;
  int64_t layer_stride = 0;  // floats between the same tensor of consecutive layers
};

// the step's buffer resets: a zero-fill kernel (no memset node when the step is captured into a hipGraph; zero bytes is a no-op)
hipError_t zero_async(void* p, size_t bytes, hipStream_t st) { return difusco::launch_zero_words(p, bytes, st); }

bool hidden_ok(int h) { return h == 64 || h == 128 || h == 256; }

Layout make_layout(int H, int L, int C) {
  Layout lo;
  const int64_t T2 = H / 2;
  int64_t cur = 0;
  auto push = [&](int64_t n) {
    lo.off.push_back(cur);
    cur = align_up(cur + n, kAlignFloats);
  };
  push((int64_t)H * H); push(H);          // node_embed
  push((int64_t)H * H); push(H);          // edge_embed
  push(T2 * H); push(T2);                 // time_embed.0
  push(T2 * T2); push(T2);                // time_embed.2
  push(H); push(H);                       // out.0 (GroupNorm affine)
  push((int64_t)C * H); push(C);          // out.2 (1x1 conv)
  push(T2); push(T2); push(H);            // freqs, dimt_pos, dimt_scalar
  push((int64_t)5 * H * H / 2 + H);       // edge_embed split planes (3 bf16 + 2 fp16 planes of H*H) + fp16 row inverse scales
  const int64_t layer0 = cur;
  for (int l = 0; l < L; ++l) {
    push((int64_t)4 * H * H); push((int64_t)4 * H);  // node4 = U|V|A|B
    push((int64_t)H * H); push(H);                    // C
    push(H); push(H); push(H); push(H);               // norm_h, norm_e
    push((int64_t)H * T2); push(H);                   // time layer
    push(H); push(H);                                 // per_layer_out LN
    push((int64_t)H * H); push(H);                    // per_layer_out linear
    push((int64_t)5 * H * H / 2 + H); push((int64_t)5 * H * H / 2 + H);  // split planes of C and per_layer_out (+ inverse scales)
    push((int64_t)5 * 4 * H * H / 2 + 4 * H);                             // split planes of the node linear (+ inverse scales)
    push(8);                                                               // operand scales of the fused edge kernel
    push((int64_t)4 * H); push((int64_t)8 * H);                            // node linear, fused path: bias, column scales (fp16 | bf16 planes)
    if (l == 0) lo.layer_stride = cur - layer0;
  }
  lo.total = cur;
  return lo;
}

// ---- named views of the packed weight blob --------------------------------------------------------
// A split weight record of an [n_out, k] matrix: 3 bf16 planes, 2 fp16 planes (16-bit elements), then the fp32 inverse scales of
// the fp16 planes.  The planes of one precision and their inverse scales (null for bf16: unscaled).
struct SplitPlanes {
  const unsigned short* planes;
  const float* w_inv;
};
SplitPlanes split_planes(const void* record, long long n_out, long long k, bool f16) {
  const long long nk = n_out * k;
  return {reinterpret_cast<const unsigned short*>(record) + (f16 ? 3 * nk : 0),
          f16 ? reinterpret_cast<const float*>(record) + 5 * nk / 2 : nullptr};
}
// fp16 planes (FP16X3, and FP16X1: the hi plane of FP16X3's pair)?
bool f16_planes(int precision) { return precision == DIFUSCO_PREC_FP16X3 || precision == DIFUSCO_PREC_FP16X1; }

// the tensors of layer l (DIFUSCO_WL_*)
struct LayerW {
  const float *node4_w, *node4_b, *c_w, *c_b, *norm_h_w, *norm_h_b, *norm_e_w, *norm_e_b, *out_ln_w, *out_ln_b, *out_w, *out_b,
      *c_planes, *out_planes, *node4_planes, *fused_scales, *node4_fused_b, *node4_fused_s;
};
struct Weights {
  Layout lo;
  const float* base;
  Weights(const float* w, int H, int L, int C) : lo(make_layout(H, L, C)), base(w) {}
  const float* g(int id) const { return base + lo.off[id]; }      // DIFUSCO_W_*
  LayerW layer(int l) const {
    const int64_t* o = lo.off.data() + DIFUSCO_W_GLOBAL_COUNT + l * DIFUSCO_WL_COUNT;
    auto at = [&](int id) { return base + o[id]; };
    return {at(DIFUSCO_WL_NODE4_W), at(DIFUSCO_WL_NODE4_B), at(DIFUSCO_WL_C_W), at(DIFUSCO_WL_C_B), at(DIFUSCO_WL_NORM_H_W),
            at(DIFUSCO_WL_NORM_H_B), at(DIFUSCO_WL_NORM_E_W), at(DIFUSCO_WL_NORM_E_B), at(DIFUSCO_WL_OUT_LN_W),
            at(DIFUSCO_WL_OUT_LN_B), at(DIFUSCO_WL_OUT_W), at(DIFUSCO_WL_OUT_B), at(DIFUSCO_WL_C_PLANES),
            at(DIFUSCO_WL_OUT_PLANES), at(DIFUSCO_WL_NODE4_PLANES), at(DIFUSCO_WL_FUSED_SCALES),
            at(DIFUSCO_WL_NODE4_FUSED_B), at(DIFUSCO_WL_NODE4_FUSED_S)};
  }
};

// hands out consecutive pieces of a buffer, each on a 256-byte boundary (null base: sizes only)
struct Carver {
  char* base;
  size_t cur = 0;
  template <typename T = float>
  T* take(size_t bytes) {
    const size_t at = cur;
    cur = (cur + bytes + 255) / 256 * 256;
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
};

struct Workspace {
  float *h, *node4, *e, *tmp, *tbias, *table_in, *table, *stats, *part, *direct, *gn_tile, *etmax, *hscale, *escale;
  double* partial;
  size_t bytes;
};

// pieces of the neighbour sum written by the fused edge kernel: 2 per 32-edge tile (8 tiles per workgroup)
size_t fused_part_floats(int64_t E) { return (size_t)((E + 255) / 256) * 8 * 2 * 256; }

Workspace carve(void* base, int H, int L, int64_t N, int64_t E, int S, int nblk) {
  Workspace w;
  Carver c{(char*)base};
  w.h = c.take(sizeof(float) * N * H);
  w.node4 = c.take(sizeof(float) * N * 4 * H);
  w.e = c.take(sizeof(float) * (H == 256 ? (E + 255) / 256 * 256 : E) * H);   // fused path: tiles of 256 edges
  w.tmp = c.take(sizeof(float) * (E > 2 ? E : 2) * H);
  w.tbias = c.take(sizeof(float) * L * H);
  w.table_in = c.take(sizeof(float) * 2 * H);
  w.table = c.take(sizeof(float) * 4 * H);      // rows 0,1: edge-input table; rows 2,3: C of layer 0 applied to them
  w.stats = c.take(sizeof(float) * S * 64);
  w.partial = c.take<double>(sizeof(double) * (size_t)S * (nblk < 256 ? 256 : nblk) * 64);
  w.part = c.take(H == 256 ? sizeof(float) * fused_part_floats(E) : 0);
  w.direct = c.take(H == 256 ? sizeof(float) * N * H : 0);
  w.gn_tile = c.take(H == 256 ? sizeof(float) * ((E + 255) / 256 * 8) * 96 : 0);   // per 32-edge tile: 32 x (sum, sumsq of x - pivot), 32 pivots
  // operand scales of the fp16 split path: max |e| per 32-edge tile (fused kernel), one power of two per node row / edge row
  w.etmax = c.take(H == 256 ? sizeof(float) * ((E + 255) / 256 * 8) : 0);
  w.hscale = c.take(sizeof(float) * N);
  w.escale = c.take(sizeof(float) * E);
  w.bytes = c.cur;
  return w;
}

// Prepared state of a TSP call shape (difusco_step_args.prepared): what a step computes from (weights, points) alone.
struct Prepared {
  float *h0, *node4_0, *table;      // [N,H], [N,4H], [4,H]
  size_t bytes;
};
Prepared carve_prepared(void* base, int H, int64_t N) {
  Prepared p;
  Carver c{(char*)base};
  p.h0 = c.take(sizeof(float) * N * H);
  p.node4_0 = c.take(sizeof(float) * N * 4 * H);
  p.table = c.take(sizeof(float) * 4 * H);
  p.bytes = c.cur;
  return p;
}

// ---- optional in-library profiler: HIP events around every kernel launch, per category ----------
// (bench.py needs the average duration of the dominant kernel measured on the launch stream inside
// the timed region; the launches happen inside difusco_denoise_step, so the brackets live here.)
enum { PROF_LINEAR_EDGE = 0, PROF_LINEAR_NODE, PROF_GATE, PROF_HEAD, PROF_EMBED, PROF_NCAT };
// (process-wide, like the HIP events it owns; every access goes through g_prof_mu, so that two engines driven from two
// host threads cannot corrupt it - their brackets simply share the category totals)
std::mutex g_prof_mu;
struct Profiler {
  bool on = false;
  bool dominant_only = false;   // bracket category 0 (the E-row / fused edge-layer launches) only
  std::vector<hipEvent_t> ev;   // pairs
  std::vector<int> cat;
  size_t used = 0;              // pairs in use
} g_prof;

struct ProfScope {
  hipStream_t st;
  bool active;
  hipEvent_t end;      // handle copied while the lock is held: the destructor never touches the shared vectors
  ProfScope(int category, hipStream_t s) : st(s), active(false), end(nullptr) {      // category < 0: no bracket
    if (category < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof.on || (g_prof.dominant_only && category != PROF_LINEAR_EDGE) || g_prof.used * 2 + 2 > g_prof.ev.size()) return;
    const size_t slot = g_prof.used++;
    g_prof.cat[slot] = category;
    end = g_prof.ev[2 * slot + 1];
    active = hipEventRecord(g_prof.ev[2 * slot], st) == hipSuccess;
  }
  ~ProfScope() {
    if (active) (void)hipEventRecord(end, st);
  }
};

#ifdef DIFUSCO_PROFILING
int g_step_skip = 0;      // difusco_debug_set key 11 (profiling library): launches of the step that are skipped for an upper-bound timing
#endif

// PROF(category, call): HIP_TRY(call), bracketed by a pair of HIP events on `st` when profiling is on.
// PROF_IF(on, ..): the same inside the helpers that difusco_prepare shares with the step - its launches are never bracketed.
#define PROF_IF(on, cat, call) { ProfScope ps_((on) ? (cat) : -1, st); HIP_TRY(call); }
#define PROF(cat, call) PROF_IF(true, cat, call)
#define STAGE(call) do { const int rc_ = (call); if (rc_ != DIFUSCO_OK) return rc_; } while (0)

using namespace difusco;

// ---- the launch plan of a step ---------------------------------------------------------------------
// the header of a difusco_step_args block: struct size, ABI, model shape, precision (the step and difusco_prepare)
int validate_header(const difusco_step_args* a) {
  if (a->struct_size != sizeof(difusco_step_args) || a->abi_version != DIFUSCO_ABI_VERSION)
    return fail(DIFUSCO_EINVAL, "ABI mismatch: struct_size %u (want %zu), abi %u (want %d)", a->struct_size,
                sizeof(difusco_step_args), a->abi_version, DIFUSCO_ABI_VERSION);
  if (!hidden_ok(a->hidden)) return fail(DIFUSCO_EINVAL, "hidden must be 64, 128 or 256 (got %d)", a->hidden);
  if (a->n_layers < 1) return fail(DIFUSCO_EINVAL, "n_layers must be >= 1");
  if (a->out_channels != 1 && a->out_channels != 2) return fail(DIFUSCO_EINVAL, "out_channels must be 1 or 2 (got %d)", a->out_channels);
  if (a->precision < DIFUSCO_PREC_FP32 || a->precision > DIFUSCO_PREC_FP16X1) return fail(DIFUSCO_EINVAL, "unknown precision %d", a->precision);
  return DIFUSCO_OK;
}

// Every path decision and derived size of a step, computed once from the argument block: after make_plan nothing in the driver
// re-derives one.
struct StepPlan {
  int H, L, C;
  int64_t N, E, out_rows, E_pad, n_tiles_pad;      // fused path: e is kept in tiles of 256 edges (32-edge tiles: n_tiles_pad)
  bool tsp, head_only;
  int nprec;                       // precision of every matrix product but the edge-row GEMMs of the layers
  bool f16;                        // fp16 planes (FP16X3 or FP16X1): operand scales are kept
  bool fused;
  int fused_variant;               // launch_edge_layer_fused: bit 0 register gathers, bit 1 max aggregation
  bool l0_fold, tail_fold, gn_fold, use_prep;
};

StepPlan make_plan(const difusco_step_args* a) {
  StepPlan p;
  p.H = a->hidden, p.L = a->n_layers, p.C = a->out_channels;
  p.N = a->n_nodes, p.E = a->n_edges;
  p.tsp = a->task == DIFUSCO_TASK_TSP;
  p.out_rows = p.tsp ? p.E : p.N;
  p.head_only = a->gn_phase == 2;   // everything up to the statistics was done by the phase-1 call
  // FP16X1: only the edge-row GEMMs of the layers (C, per_layer_out[l][2]) take the one-product form; every other matrix product
  // (edge embedding, node linears) runs as FP16X3 - nprec is the precision of those
  p.nprec = a->precision == DIFUSCO_PREC_FP16X1 ? DIFUSCO_PREC_FP16X3 : a->precision;
  p.f16 = p.nprec == DIFUSCO_PREC_FP16X3;
  // fused edge-layer path: H = 256, 16-bit split planes, one GroupNorm statistic segment; e is then kept in the
  // tiled layout (kernels.h: edge_tiled_offset) from the embedding to the head
  // (per-sample statistic segments - the dense mode of TSP-50 / 100 with parallel_sampling > 1 - run the same fused layers;
  // only the head differs: masked per-segment statistics and a per-row segment look-up, launch_head_tiled)
  // the full-line neighbour-table gathers address node rows by 32-bit byte offsets (4 KB per node): calls with 2^20 nodes or
  // more take the register-gather instantiation of the same kernel (64-bit addresses, bit-identical results, ~3 % slower)
  const int reg_gather = p.N >= (1 << 20) ? 1 : 0;
  // aggregation = max has fused instantiations of its own (the per-tile pieces are maxima) for the full-line gather form only:
  // with 2^20 nodes or more it takes the unfused sequence
  const bool agg_max = a->aggregation == DIFUSCO_AGG_MAX;
  p.fused = p.H == 256 && !a->no_fusion && p.E > 0 && !(agg_max && reg_gather) &&
            (a->precision == DIFUSCO_PREC_BF16X3 || a->precision == DIFUSCO_PREC_FP16X3 ||
             a->precision == DIFUSCO_PREC_FP16X1);
  p.fused_variant = reg_gather | (agg_max ? 2 : 0);
  p.E_pad = (p.E + 255) / 256 * 256;
  p.n_tiles_pad = p.E_pad / 32;
#ifdef DIFUSCO_PROFILING
  const bool ablating = difusco::g_fused_ablate != 0;      // (the ablation variants exist for the middle layer only: no folds)
#else
  const bool ablating = false;
#endif
  // first layer: when the edge input is a table lookup (categorical TSP: embedding of the bit; MIS: zeros) the fused
  // kernel takes it from the table and the pass that would write e0 to HBM is skipped
  p.l0_fold = p.fused && (a->flags & DIFUSCO_FLAG_NO_L0_FOLD) == 0 && !ablating && (p.tsp ? a->xt_is_binary != 0 : true);
  // last layer (at least two layers).  TSP: the fused kernel also emits the head's GroupNorm partial sums per tile and
  // skips the node update nobody reads; MIS: it skips the edge output nobody reads.
  p.tail_fold = p.fused && p.L >= 2 && (a->flags & DIFUSCO_FLAG_NO_TAIL_FOLD) == 0 && !ablating;
  p.gn_fold = p.tail_fold && p.tsp;
  // prepared state (TSP, fused path only; anything else recomputes - the stateless step is always correct)
  p.use_prep = a->prepared != nullptr && p.fused && p.tsp && !ablating;
  return p;
}

// ---- pieces that difusco_prepare shares with the step: the same kernels on the same operands, `dst` in the workspace or in the
// prepared buffer ------------------------------------------------------------------------------------
// per-layer time bias rows of n_t diffusion times (HOST array): tbias[i][l][:] = time_layer_l(time_embed(timestep_embedding(t_i)))
hipError_t time_bias_rows(const Weights& w, int H, int L, const float* t_host, int n_t, float* out, hipStream_t st) {
  const int64_t* l0 = w.lo.off.data() + DIFUSCO_W_GLOBAL_COUNT;      // layer 0's tensors; the others follow at layer_stride
  return difusco::launch_time_bias(t_host, n_t, H, L, w.g(DIFUSCO_W_TIME_FREQS), w.g(DIFUSCO_W_TIME0_W), w.g(DIFUSCO_W_TIME0_B),
                                   w.g(DIFUSCO_W_TIME2_W), w.g(DIFUSCO_W_TIME2_B), w.base + l0[0], w.lo.layer_stride,
                                   l0[DIFUSCO_WL_TIME_W] - l0[0], l0[DIFUSCO_WL_TIME_B] - l0[0], out, st);
}

// h0 = node_embed(pos_embed(points))  (gnn_encoder.py:394); `feat`: [N,H] scratch for the sinusoidal features
int embed_tsp_nodes(const Weights& w, int H, int64_t N, const float* points, float* feat, float* h0, hipStream_t st, bool prof) {
  PROF_IF(prof, PROF_EMBED, launch_pos_embed(points, w.g(DIFUSCO_W_DIMT_POS), (int)N, H, feat, st))
  PROF_IF(prof, PROF_LINEAR_NODE, linear_rows(feat, w.g(DIFUSCO_W_NODE_EMBED_W), w.g(DIFUSCO_W_NODE_EMBED_B), nullptr, h0, N, H, H, H, st))
  return DIFUSCO_OK;
}

// U | V | A | B rows of h for one layer -> dst [N,4H].  scale_pass: compute the row scales of h (fp16 planes) here - they are left by
// node_finalize of the previous layer on the fused path.  fused_domain: the rows are read by the fused edge kernel, i.e. A | B in
// its log2(e) domain with b_C folded into the A rows (difusco_hip.h, ABI 11 note): the node linear of a precision with a fused
// path writes them so (fused bias / column-scale vectors); any other precision computes the reference's rows and converts them in
// place, so that a prepared buffer is in the kernel's domain WHATEVER precision prepared it.
int node_rows(int precision, int H, int64_t N, const LayerW& lw, const float* h, float* hscale, bool scale_pass, bool fused_domain,
              float* dst, hipStream_t st, bool prof) {
  const int nprec = precision == DIFUSCO_PREC_FP16X1 ? DIFUSCO_PREC_FP16X3 : precision;
  const bool f16 = nprec == DIFUSCO_PREC_FP16X3;
  bool converted = false;      // rows already in the fused kernel's domain
  if (precision != DIFUSCO_PREC_FP32 && H == 256) {   // node rows on the same split-precision matrix-core path
    const SplitPlanes np = split_planes(lw.node4_planes, 4 * H, H, f16);
    SplitScale sc;
    if (f16) {
      if (scale_pass) PROF_IF(prof, PROF_LINEAR_NODE, launch_row_pow2_scale(h, N, H, hscale, st))
      sc.row_scale = hscale;
      sc.w_inv = np.w_inv;
    }
    converted = fused_domain && (nprec == DIFUSCO_PREC_BF16X3 || nprec == DIFUSCO_PREC_FP16X3);
    if (converted) sc.w_inv = lw.node4_fused_s + (f16 ? 0 : 4 * H);
    PROF_IF(prof, PROF_LINEAR_NODE, linear_rows_split(h, np.planes, (long long)4 * H * H, nprec, converted ? lw.node4_fused_b : lw.node4_b,
                                                      nullptr, dst, N, H, 4 * H, 4 * H, st, 0, sc))
  } else {
    PROF_IF(prof, PROF_LINEAR_NODE, linear_rows(h, lw.node4_w, lw.node4_b, nullptr, dst, N, H, 4 * H, 4 * H, st))
  }
  if (fused_domain && !converted && H == 256) PROF_IF(prof, PROF_LINEAR_NODE, launch_fuse_node_tables(dst, lw.c_b, (int)N, dst, st))
  return DIFUSCO_OK;
}

// C of layer 0 on the two rows of the edge-input table (table rows 0, 1 -> rows 2, 3; layer-0 fold of the fused step and
// difusco_prepare).  Exact fp32, except under FP16X1: there the one-product fp16 linear that the fused kernel's GEMM 1 applies to
// an e tile (each row scaled by its power of two, the hi plane of C), so that folding layer 0 keeps the precision's contract.
// scale2: two floats of scratch.
hipError_t table_c_rows(int precision, int H, float* table, const LayerW& lw, float* scale2, hipStream_t st) {
  if (precision != DIFUSCO_PREC_FP16X1) return launch_two_rows_linear(H, table, lw.c_w, nullptr, table + 2 * H, st);
  hipError_t er = launch_row_pow2_scale(table, 2, H, scale2, st);
  if (er != hipSuccess) return er;
  const SplitPlanes cp = split_planes(lw.c_planes, H, H, true);
  SplitScale sc;
  sc.row_scale = scale2;
  sc.w_inv = cp.w_inv;
  return linear_rows_split(table, cp.planes, (long long)H * H, DIFUSCO_PREC_FP16X1, nullptr, nullptr, table + 2 * H, 2, H, H, H, st, 0, sc);
}

// two-row edge-input table of a categorical TSP step (the embedding of the bit x_t, gnn_encoder.py:395) -> table rows 0, 1;
// with_c: C of layer 0 applied to it -> rows 2, 3.  table_in: [2,H] scratch.
int edge_input_table(int precision, int H, const Weights& w, float* table_in, float* table, bool with_c, hipStream_t st, bool prof) {
  PROF_IF(prof, PROF_EMBED, launch_scalar_embed(nullptr, nullptr, w.g(DIFUSCO_W_DIMT_SCALAR), 2, H, table_in, st))
  PROF_IF(prof, PROF_EMBED, launch_two_rows_linear(H, table_in, w.g(DIFUSCO_W_EDGE_EMBED_W), w.g(DIFUSCO_W_EDGE_EMBED_B), table, st))
  if (with_c) PROF_IF(prof, PROF_EMBED, table_c_rows(precision, H, table, w.layer(0), table_in, st))
  return DIFUSCO_OK;
}

// ---- one step: what every stage reads, and the stages in launch order ------------------------------------
struct Step {
  const difusco_step_args* a;
  StepPlan p;
  int H;
  Workspace ws;
  Prepared prep;
  Weights w;
  const float* tbias;      // [L,H] time-bias rows of this t: the caller's, or ws.tbias
  const float* table;      // two-row edge-input table (+ C of layer 0 applied to it): prepared or ws.table
  hipStream_t st;

  // E-row linear of the unfused sequence: exact fp32 MFMA or split planes, same contract (mode: the precision of this product)
  hipError_t edge_linear(int mode, const float* x, const float* w, const float* planes, const float* b,
                         const float* res, float* y) const {
    if (mode == DIFUSCO_PREC_FP32) return linear_rows(x, w, b, res, y, p.E, H, H, H, st);
    const SplitPlanes sp = split_planes(planes, H, H, f16_planes(mode));
    SplitScale sc;
    if (f16_planes(mode)) {
      // fp16 planes: per-row power-of-two scale of x (one extra pass over x on this unfused path), weight inverse scales
      hipError_t er = launch_row_pow2_scale(x, p.E, H, ws.escale, st);
      if (er != hipSuccess) return er;
      sc.row_scale = ws.escale;
      sc.w_inv = sp.w_inv;
    }
    return linear_rows_split(x, sp.planes, (long long)H * H, mode, b, res, y, p.E, H, H, H, st, 0, sc);
  }

  // the pad lanes of e's last tiles must read as zero in every later kernel of the fused path (zero bytes when E fills its tiles)
  hipError_t zero_pad_tail() const {
    const int64_t done = (p.E / 32) * 32;
    return zero_async(ws.e + done * H, sizeof(float) * (p.E_pad - done) * H, st);
  }

  // input embeddings of a TSP step (gnn_encoder.py:394-395).  ws.node4 doubles as scratch for the sinusoidal node features before
  // the first layer overwrites it.
  int embed_tsp() const {
    if (!p.use_prep) STAGE(embed_tsp_nodes(w, H, p.N, a->points, ws.node4, ws.h, st, true));
    if (p.fused) PROF(PROF_EMBED, zero_pad_tail())
    if (a->xt_is_binary) {
      // (l0_fold: e0 and C e0 are read from the table by the first fused layer)
      if (!p.use_prep) STAGE(edge_input_table(a->precision, H, w, ws.table_in, ws.table, p.l0_fold, st, true));
      if (p.l0_fold) return DIFUSCO_OK;
      if (p.fused) {
        PROF(PROF_EMBED, launch_table_rows_tiled(a->xt, a->perm, table, p.E, ws.e, st))
        if (p.f16) PROF(PROF_EMBED, launch_tile_absmax_tiled(ws.e, p.n_tiles_pad, ws.etmax, st))
      } else {
        PROF(PROF_EMBED, launch_table_rows(a->xt, a->perm, table, p.E, H, ws.e, st))
      }
    } else if (p.fused) {   // sinusoidal features generated inside the linear: the E x H embedding never exists in memory
      const SplitPlanes ep = split_planes(w.g(DIFUSCO_W_EDGE_EMBED_PLANES), H, H, p.f16);
      PROF(PROF_EMBED, launch_edge_embed_tiled(a->xt, a->perm, w.g(DIFUSCO_W_DIMT_SCALAR), ep.planes, (long long)H * H, p.nprec, ep.w_inv,
                                               w.g(DIFUSCO_W_EDGE_EMBED_B), ws.e, p.E, p.f16 ? ws.etmax : nullptr, st, a->gen_table,
                                               a->gen_table ? reinterpret_cast<int*>(ws.escale) : nullptr))      // (escale: unfused path only - free here)
    } else {
      PROF(PROF_EMBED, launch_scalar_embed(a->xt, a->perm, w.g(DIFUSCO_W_DIMT_SCALAR), p.E, H, ws.tmp, st))
      PROF(PROF_LINEAR_EDGE, edge_linear(p.nprec, ws.tmp, w.g(DIFUSCO_W_EDGE_EMBED_W), w.g(DIFUSCO_W_EDGE_EMBED_PLANES),
                                         w.g(DIFUSCO_W_EDGE_EMBED_B), nullptr, ws.e))
    }
    return DIFUSCO_OK;
  }

  // input embeddings of a MIS step (gnn_encoder.py:405-407): h from x_t, e = zeros
  int embed_mis() const {
    PROF(PROF_EMBED, launch_scalar_embed(a->xt, nullptr, w.g(DIFUSCO_W_DIMT_SCALAR), p.N, H, ws.node4, st))
    PROF(PROF_LINEAR_NODE, linear_rows(ws.node4, w.g(DIFUSCO_W_NODE_EMBED_W), w.g(DIFUSCO_W_NODE_EMBED_B), nullptr, ws.h, p.N, H, H, H, st))
    if (p.l0_fold) {   // e = zeros comes from an all-zero table; only the pad tail must read as zero
      PROF(PROF_EMBED, zero_async(ws.table, sizeof(float) * 4 * H, st))
      PROF(PROF_EMBED, zero_pad_tail())
    } else if (p.E > 0) {
      PROF(PROF_EMBED, zero_async(ws.e, sizeof(float) * (p.fused ? p.E_pad : p.E) * H, st))
      if (p.fused && p.f16) PROF(PROF_EMBED, zero_async(ws.etmax, sizeof(float) * p.n_tiles_pad, st))
    }
    return DIFUSCO_OK;
  }

  // edge pass + node update of layer l on the fused path: one launch record, the kind says what the step still needs from the layer
  int fused_layer(int l, const LayerW& lw, const float* node4, const float* h_in) const {
    const float* tb = tbias + (size_t)l * H;
    FusedLayerArgs fa;
    fa.e = ws.e, fa.node4 = node4, fa.row = a->row, fa.col = a->col, fa.n_edges = (int)p.E;
    fa.c_planes = split_planes(lw.c_planes, H, H, p.f16).planes;      // (FP16X1: the hi plane of FP16X3's pair)
    fa.o_planes = split_planes(lw.out_planes, H, H, p.f16).planes;
    fa.plane_stride = (long long)H * H;
    fa.b_c = lw.c_b, fa.g_e = lw.norm_e_w, fa.b_e = lw.norm_e_b, fa.tbias = tb;
    fa.g_o = lw.out_ln_w, fa.b_o = lw.out_ln_b, fa.b_out = lw.out_b;
    fa.time_on_edge = p.tsp ? 1 : 0;
    fa.part = ws.part, fa.direct = ws.direct, fa.scales = lw.fused_scales, fa.stream = st;
    FusedKind kind = FusedKind::Middle;
    if (l == 0 && p.l0_fold) {
      kind = FusedKind::FirstFromTable;
      fa.l0_table = table, fa.l0_x = p.tsp ? a->xt : nullptr, fa.l0_perm = p.tsp ? a->perm : nullptr;
      fa.etmax_out = ws.etmax;
    } else if (p.tail_fold && l == p.L - 1) {
      kind = p.tsp ? FusedKind::TailTsp : FusedKind::TailMis;
      fa.gn_tile = ws.gn_tile, fa.etmax_in = ws.etmax;
    } else {
      fa.etmax_in = fa.etmax_out = ws.etmax;
    }
    PROF(PROF_LINEAR_EDGE, launch_edge_layer_fused(a->precision, kind, p.fused_variant, fa))
    if (p.gn_fold && l == p.L - 1) return DIFUSCO_OK;     // TSP: h is not read after the last layer
#ifdef DIFUSCO_PROFILING
    if (g_step_skip & 1) return DIFUSCO_OK;      // (timing only, WRONG results: what any fold of node_finalize could save at most)
#endif
    PROF(PROF_GATE, launch_node_finalize((int)p.N, (int)p.E, a->rowptr, node4, ws.part, ws.direct, ws.h, lw.norm_h_w, lw.norm_h_b, tb,
                                         p.tsp ? 1 : 0, p.f16 ? ws.hscale : nullptr, st, h_in, a->aggregation))
    return DIFUSCO_OK;
  }

  // the same layer as three launches: C e, gate + aggregation + norms, per_layer_out (+ residual)
  int unfused_layer(int l, const LayerW& lw) const {
    PROF(PROF_LINEAR_EDGE, edge_linear(a->precision, ws.e, lw.c_w, lw.c_planes, lw.c_b, nullptr, ws.tmp))
    PROF(PROF_GATE, launch_edge_gate_aggregate(H, (int)p.N, a->rowptr, a->col, ws.node4, ws.tmp, ws.h, lw.norm_h_w, lw.norm_h_b,
                                               lw.norm_e_w, lw.norm_e_b, lw.out_ln_w, lw.out_ln_b, tbias + (size_t)l * H,
                                               p.tsp ? 1 : 0, st, a->aggregation))
    PROF(PROF_LINEAR_EDGE, edge_linear(a->precision, ws.tmp, lw.out_w, lw.out_planes, lw.out_b, ws.e, ws.e))
    return DIFUSCO_OK;
  }

  // the GNN layers (gnn_encoder.py:425-449)
  int run_layers() const {
    for (int l = 0; l < p.L; ++l) {
      const LayerW lw = w.layer(l);
      // layer 0 of a step with prepared state: U|V|A|B of h0 and h0 itself come from the prepared buffer
      const bool prep_l = p.use_prep && l == 0;
      bool node_linear = !prep_l;
#ifdef DIFUSCO_PROFILING
      if ((g_step_skip & 2) && l >= 2) node_linear = false;      // (timing only, WRONG results: no node-linear launches from layer 2 on)
#endif
      if (node_linear)
        STAGE(node_rows(a->precision, H, p.N, lw, ws.h, ws.hscale, !p.fused || l == 0, p.fused, ws.node4, st, true));
      STAGE(p.fused ? fused_layer(l, lw, prep_l ? prep.node4_0 : ws.node4, prep_l ? prep.h0 : nullptr) : unfused_layer(l, lw));
    }
    return DIFUSCO_OK;
  }

  // head + posterior (gnn_encoder.py:400-401 / :412-413, pl_tsp_model.py:133-137, pl_meta_model.py:102-175)
  int run_head(const uint64_t* offset_shift) const {
    RandInstances ri;
    if (a->rand_mode == DIFUSCO_RAND_PHILOX_INSTANCES) ri = RandInstances{a->n_instances, a->instance_rows, a->instance_seeds};
    const int* seg_ptr = a->n_segments > 1 ? a->seg_ptr : nullptr;
    const int nblk = gn_blocks_for(p.out_rows);
    if (p.fused && p.tsp) {
      PROF(PROF_HEAD, launch_head_tiled(p.C, ws.e, p.E, nblk < 8 ? 8 : nblk / 8 * 8, ws.partial, ws.stats, w.g(DIFUSCO_W_OUT_GN_W),
                                        w.g(DIFUSCO_W_OUT_GN_B), w.g(DIFUSCO_W_OUT_CONV_W), w.g(DIFUSCO_W_OUT_CONV_B), a->perm, a->xt,
                                        a->post, a->rand_mode, a->rand, a->seed, a->offset, a->xt_out, a->pred_out, a->prob_out, st,
                                        p.gn_fold ? ws.gn_tile : nullptr, a->gn_phase, a->gn_sums, seg_ptr, a->n_segments, ri,
                                        offset_shift))
      return DIFUSCO_OK;
    }
    PROF(PROF_HEAD, launch_head(H, p.C, p.tsp ? ws.e : ws.h, seg_ptr, a->n_segments, p.out_rows, nblk, ws.partial, ws.stats,
                                w.g(DIFUSCO_W_OUT_GN_W), w.g(DIFUSCO_W_OUT_GN_B), w.g(DIFUSCO_W_OUT_CONV_W), w.g(DIFUSCO_W_OUT_CONV_B),
                                p.tsp ? a->perm : nullptr, a->xt, a->post, a->rand_mode, a->rand, a->seed, a->offset, a->xt_out,
                                a->pred_out, a->prob_out, st, a->gn_phase, a->gn_sums, ri, offset_shift))
    return DIFUSCO_OK;
  }

  // DIFUSCO_FLAG_CHECK_FINITE: count inf / nan in the outputs (the statistics scratch is free after the head), synchronise
  int check_finite() const {
    if ((a->flags & DIFUSCO_FLAG_CHECK_FINITE) == 0 || a->gn_phase == 1) return DIFUSCO_OK;
    unsigned* cnt = reinterpret_cast<unsigned*>(ws.partial);
    HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned), st));
    HIP_TRY(launch_count_nonfinite(a->xt_out, p.out_rows, cnt, st));
    // head GroupNorm mean / rstd: nan as soon as the final state holds one (a sampled bit hides it)
    HIP_TRY(launch_count_nonfinite(ws.stats, (long long)a->n_segments * 64, cnt, st));
    HIP_TRY(launch_count_nonfinite(a->pred_out, p.out_rows * p.C, cnt, st));
    HIP_TRY(launch_count_nonfinite(a->prob_out, a->diffusion == DIFUSCO_CATEGORICAL ? p.out_rows : 0, cnt, st));
    unsigned bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, cnt, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(DIFUSCO_ENONFINITE, "denoise step produced %u non-finite output values", bad);
    return DIFUSCO_OK;
  }
};

}  // namespace

extern "C" {

int difusco_abi_version(void) { return DIFUSCO_ABI_VERSION; }

const char* difusco_last_error(void) { return g_err; }

int difusco_weights_layout(int hidden, int n_layers, int out_channels, int64_t* offsets, int max_entries,
                           int64_t* total_floats) {
  if (!hidden_ok(hidden)) return fail(DIFUSCO_EINVAL, "hidden must be 64, 128 or 256 (got %d)", hidden);
  if (n_layers < 1 || (out_channels != 1 && out_channels != 2))
    return fail(DIFUSCO_EINVAL, "n_layers >= 1 and out_channels in {1,2} required");
  Layout lo = make_layout(hidden, n_layers, out_channels);
  const int n = (int)lo.off.size();
  if (offsets) {
    if (max_entries < n) return fail(DIFUSCO_EINVAL, "offset array too small: need %d", n);
    std::memcpy(offsets, lo.off.data(), sizeof(int64_t) * n);
  }
  if (total_floats) *total_floats = lo.total;
  return n;
}

int difusco_csr_from_coo_host(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, int32_t* rowptr,
                              int32_t* col, int32_t* row, int32_t* perm, int* identity) {
  if (!edge_index || !rowptr || !col || !row || !perm) return fail(DIFUSCO_EINVAL, "null pointer");
  if (n_edges < 0 || n_nodes < 0 || n_edges > INT32_MAX || n_nodes >= INT32_MAX)
    return fail(DIFUSCO_EINVAL, "sizes out of int32 range");
  const int64_t* r = edge_index;
  const int64_t* c = edge_index + n_edges;
  for (int64_t i = 0; i <= n_nodes; ++i) rowptr[i] = 0;
  for (int64_t k = 0; k < n_edges; ++k) {
    if (r[k] < 0 || r[k] >= n_nodes || c[k] < 0 || c[k] >= n_nodes)
      return fail(DIFUSCO_EINVAL, "edge %lld = (%lld,%lld) out of range [0,%lld)", (long long)k, (long long)r[k],
                  (long long)c[k], (long long)n_nodes);
    rowptr[r[k] + 1]++;
  }
  for (int64_t i = 0; i < n_nodes; ++i) rowptr[i + 1] += rowptr[i];
  std::vector<int32_t> fill(rowptr, rowptr + n_nodes);
  int ident = 1;
  for (int64_t k = 0; k < n_edges; ++k) {  // stable counting sort by centre node
    const int32_t s = fill[r[k]]++;
    col[s] = (int32_t)c[k];
    row[s] = (int32_t)r[k];
    perm[s] = (int32_t)k;
    if (s != k) ident = 0;
  }
  if (identity) *identity = ident;
  return DIFUSCO_OK;
}

size_t difusco_workspace_bytes(int hidden, int n_layers, int n_nodes, int n_edges, int n_segments) {
  if (!hidden_ok(hidden) || n_layers < 1 || n_nodes < 0 || n_edges < 0 || n_segments < 1) return 0;
  const long long rows = n_edges > n_nodes ? n_edges : n_nodes;
  return carve(nullptr, hidden, n_layers, n_nodes, n_edges, n_segments, difusco::gn_blocks_for(rows)).bytes;
}

int difusco_denoise_step(const difusco_step_args* a) { return difusco_denoise_step_shifted(a, nullptr); }

int difusco_denoise_step_shifted(const difusco_step_args* a, const uint64_t* offset_shift) {
  if (!a) return fail(DIFUSCO_EINVAL, "null args");
  STAGE(validate_header(a));
  if (a->task != DIFUSCO_TASK_TSP && a->task != DIFUSCO_TASK_MIS) return fail(DIFUSCO_EINVAL, "unknown task %d", a->task);
  if (a->diffusion != DIFUSCO_CATEGORICAL && a->diffusion != DIFUSCO_GAUSSIAN)
    return fail(DIFUSCO_EINVAL, "unknown diffusion %d", a->diffusion);
  if (a->out_channels != (a->diffusion == DIFUSCO_CATEGORICAL ? 2 : 1))
    return fail(DIFUSCO_EINVAL, "out_channels %d does not match diffusion type", a->out_channels);
  const int64_t N = a->n_nodes, E = a->n_edges;
  if (N <= 0 || E < 0) return fail(DIFUSCO_EINVAL, "n_nodes must be > 0, n_edges >= 0");
  if (!a->weights || !a->rowptr || (E > 0 && !a->col) || !a->xt || !a->xt_out || !a->workspace)
    return fail(DIFUSCO_EINVAL, "null device pointer (weights/rowptr/col/xt/xt_out/workspace)");
  if (a->task == DIFUSCO_TASK_TSP && !a->points && !a->prepared) return fail(DIFUSCO_EINVAL, "TSP needs points");
  if (a->task == DIFUSCO_TASK_TSP && E == 0) return fail(DIFUSCO_EINVAL, "TSP needs edges");
  if (a->n_segments < 1 || (a->n_segments > 1 && !a->seg_ptr))
    return fail(DIFUSCO_EINVAL, "n_segments >= 1, seg_ptr required when > 1");
  if (a->rand_mode == DIFUSCO_RAND_INJECTED && !a->rand) return fail(DIFUSCO_EINVAL, "injected randomness needs rand");
  if (a->rand_mode < 0 || a->rand_mode > DIFUSCO_RAND_PHILOX_INSTANCES)
    return fail(DIFUSCO_EINVAL, "unknown rand_mode %d", a->rand_mode);
  if (a->rand_mode == DIFUSCO_RAND_PHILOX_INSTANCES && (a->n_instances < 1 || !a->instance_rows || !a->instance_seeds))
    return fail(DIFUSCO_EINVAL, "rand_mode PHILOX_INSTANCES needs n_instances >= 1, instance_rows and instance_seeds");
  if (a->gn_phase < 0 || a->gn_phase > 2) return fail(DIFUSCO_EINVAL, "gn_phase must be 0, 1 or 2");
  if (a->aggregation < DIFUSCO_AGG_SUM || a->aggregation > DIFUSCO_AGG_MAX)
    return fail(DIFUSCO_EINVAL, "unknown aggregation %d (DIFUSCO_AGG_SUM / MEAN / MAX)", a->aggregation);
  if (a->gn_phase != 0 && (a->n_segments != 1 || !a->gn_sums))
    return fail(DIFUSCO_EINVAL, "gn_phase %d needs n_segments == 1 and a gn_sums buffer of 65 doubles", a->gn_phase);
  if (a->post[4] != 0.0f && a->rand_mode == DIFUSCO_RAND_NONE)
    return fail(DIFUSCO_EINVAL, "this step draws random numbers: rand_mode must not be NONE");

  const StepPlan p = make_plan(a);
  const Workspace ws = carve(a->workspace, p.H, p.L, N, E, a->n_segments, gn_blocks_for(E > N ? E : N));
  if (ws.bytes > a->workspace_bytes)
    return fail(DIFUSCO_EWORKSPACE, "workspace too small: %zu < %zu", a->workspace_bytes, ws.bytes);
  if (p.fused && !a->row) return fail(DIFUSCO_EINVAL, "the fused edge-layer kernel needs args->row");
  if (p.tsp && !a->points && !p.use_prep && !p.head_only)
    return fail(DIFUSCO_EINVAL, "TSP needs points (only a fused-path step with prepared state runs without them)");
  const Prepared prep = carve_prepared(const_cast<void*>(a->prepared), p.H, N);
  hipStream_t st = (hipStream_t)a->stream;
  const Step s{a, p, p.H, ws, prep, Weights(a->weights, p.H, p.L, p.C),
               a->tbias ? a->tbias : ws.tbias,      // (caller-prepared rows of this t, or computed here)
               p.use_prep ? prep.table : ws.table, st};

  if (!p.head_only) {      // (phase 2: e / h of the phase-1 call are still in the workspace)
    if (!a->tbias) PROF(PROF_EMBED, time_bias_rows(s.w, p.H, p.L, &a->t, 1, ws.tbias, st))
    STAGE(p.tsp ? s.embed_tsp() : s.embed_mis());
    STAGE(s.run_layers());
  }
  STAGE(s.run_head(offset_shift));
  return s.check_finite();
}

size_t difusco_prepared_bytes(int hidden, int n_nodes) {
  if (!hidden_ok(hidden) || n_nodes <= 0) return 0;
  return carve_prepared(nullptr, hidden, n_nodes).bytes;
}

int difusco_time_bias_rows(int hidden, int n_layers, int out_channels, const float* weights, const float* t_host, int n_t,
                           float* out, void* stream) {
  if (!hidden_ok(hidden) || n_layers < 1 || (out_channels != 1 && out_channels != 2))
    return fail(DIFUSCO_EINVAL, "hidden in {64,128,256}, n_layers >= 1, out_channels in {1,2} required");
  if (!weights || !t_host || !out || n_t < 1) return fail(DIFUSCO_EINVAL, "null pointer or n_t < 1");
  HIP_TRY(time_bias_rows(Weights(weights, hidden, n_layers, out_channels), hidden, n_layers, t_host, n_t, out, (hipStream_t)stream));
  return DIFUSCO_OK;
}

// e0 = edge_embed(ScalarEmbeddingSine(x_t)) for a general (Gaussian / non-binary) x_t, by the kernel the fused step uses (edge_embed.hip):
// exported for the parity tests (partial tiles, permuted inputs, |x_t| up to 6).
size_t difusco_gen_table_bytes(int hidden) {
  if (hidden != 256) return 0;
  // rows | build scratch: the sinusoidal features of the grid, the grid itself
  return sizeof(float) * ((size_t)2 * difusco::kGenRows * 256 + 1024);
}

int difusco_gen_table_build(int hidden, int n_layers, int out_channels, const float* weights, float* table, size_t table_bytes,
                            void* stream) {
  if (hidden != 256) return fail(DIFUSCO_EINVAL, "difusco_gen_table_build: hidden = 256 required");
  if (n_layers < 1 || (out_channels != 1 && out_channels != 2) || !weights || !table) return fail(DIFUSCO_EINVAL, "bad model shape / null pointer");
  if (table_bytes < difusco_gen_table_bytes(hidden)) return fail(DIFUSCO_EWORKSPACE, "gen table buffer too small: %zu < %zu", table_bytes, difusco_gen_table_bytes(hidden));
  const Weights w(weights, hidden, n_layers, out_channels);
  const int H = hidden;
  hipStream_t st = (hipStream_t)stream;
  float* feat = table + (size_t)kGenRows * H;
  float* grid = feat + (size_t)kGenRows * H;
  HIP_TRY(launch_gen_table_grid(grid, st));
  HIP_TRY(launch_scalar_embed(grid, nullptr, w.g(DIFUSCO_W_DIMT_SCALAR), kGenRows, H, feat, st));       // precise sin / cos of x / dim_t
  HIP_TRY(linear_rows(feat, w.g(DIFUSCO_W_EDGE_EMBED_W), w.g(DIFUSCO_W_EDGE_EMBED_B), nullptr, table, kGenRows, H, H, H, st));   // exact fp32 MFMA
  return DIFUSCO_OK;
}

int difusco_edge_embed(int hidden, int n_layers, int out_channels, const float* weights, int precision, const float* xt,
                       const int32_t* perm, int64_t n_edges, float* e_tiled, float* tile_max, const float* gen_table, void* stream) {
  if (hidden != 256) return fail(DIFUSCO_EINVAL, "difusco_edge_embed: the tiled kernel exists for hidden = 256");
  if (n_layers < 1 || (out_channels != 1 && out_channels != 2)) return fail(DIFUSCO_EINVAL, "n_layers >= 1, out_channels in {1,2} required");
  if (precision != DIFUSCO_PREC_BF16X3 && precision != DIFUSCO_PREC_FP16X3)
    return fail(DIFUSCO_EINVAL, "difusco_edge_embed: precision must be BF16X3 or FP16X3");
  if (!weights || !xt || !e_tiled || n_edges < 0 || n_edges > 0x7fffffff) return fail(DIFUSCO_EINVAL, "null pointer / bad n_edges");
  const Weights w(weights, hidden, n_layers, out_channels);
  const int H = hidden;
  const SplitPlanes ep = split_planes(w.g(DIFUSCO_W_EDGE_EMBED_PLANES), H, H, precision == DIFUSCO_PREC_FP16X3);
  // (stand-alone entry: the tile flags live in the table buffer's build scratch - enough for 581,632 edges; the step uses its workspace)
  int* flags = gen_table ? reinterpret_cast<int*>(const_cast<float*>(gen_table) + (size_t)kGenRows * H) : nullptr;
  if (gen_table && (n_edges + 127) / 128 * 4 > (int64_t)kGenRows * H)
    return fail(DIFUSCO_EINVAL, "difusco_edge_embed with a table: at most %d edges per call (use the step for larger inputs)", kGenRows * H * 32);
  HIP_TRY(launch_edge_embed_tiled(xt, perm, w.g(DIFUSCO_W_DIMT_SCALAR), ep.planes, (long long)H * H, precision, ep.w_inv,
                                  w.g(DIFUSCO_W_EDGE_EMBED_B), e_tiled, n_edges, tile_max, (hipStream_t)stream, gen_table, flags));
  return DIFUSCO_OK;
}

// The step-invariant part of a TSP step, by the helpers the stateless step itself calls (and therefore with its bits): node
// embedding, row scales, layer 0's node linear, the two-row edge-input table and C of layer 0 applied to it.
int difusco_prepare(const difusco_step_args* a, void* prepared, size_t prepared_bytes) {
  if (!a || !prepared) return fail(DIFUSCO_EINVAL, "null args / buffer");
  STAGE(validate_header(a));
  const int H = a->hidden, L = a->n_layers;
  if (a->task != DIFUSCO_TASK_TSP) return fail(DIFUSCO_EINVAL, "prepared state exists for TSP only (the MIS node embedding is a function of x_t)");
  const int64_t N = a->n_nodes, E = a->n_edges;
  if (N <= 0 || E < 0 || !a->weights || !a->points || !a->workspace) return fail(DIFUSCO_EINVAL, "null pointer / empty graph");
  const Prepared prep = carve_prepared(prepared, H, N);
  if (prep.bytes > prepared_bytes) return fail(DIFUSCO_EWORKSPACE, "prepared buffer too small: %zu < %zu", prepared_bytes, prep.bytes);
  const Workspace ws = carve(a->workspace, H, L, N, E, a->n_segments < 1 ? 1 : a->n_segments, gn_blocks_for(E > N ? E : N));
  if (ws.bytes > a->workspace_bytes) return fail(DIFUSCO_EWORKSPACE, "workspace too small: %zu < %zu", a->workspace_bytes, ws.bytes);
  const Weights w(a->weights, H, L, a->out_channels);
  hipStream_t st = (hipStream_t)a->stream;
  STAGE(embed_tsp_nodes(w, H, N, a->points, ws.node4, prep.h0, st, false));
  // the prepared rows are read by the fused edge kernel only (make_plan: use_prep requires the fused path): always in its domain
  STAGE(node_rows(a->precision, H, N, w.layer(0), prep.h0, ws.hscale, true, true, prep.node4_0, st, false));
  return edge_input_table(a->precision, H, w, ws.table_in, prep.table, true, st, false);
}

int difusco_linear_rows(const float* x, const float* w, const float* bias, const float* residual, float* y, int64_t m,
                        int k, int n_out, int64_t ldy, void* stream) {
  if (!x || !w || !y) return fail(DIFUSCO_EINVAL, "null pointer");
  if (!(k == 32 || k == 64 || k == 128 || k == 256) || n_out % 32 != 0 || n_out <= 0 || ldy < n_out)
    return fail(DIFUSCO_EINVAL, "k must be 32/64/128/256, n_out a positive multiple of 32, ldy >= n_out");
  HIP_TRY(difusco::linear_rows(x, w, bias, residual, y, m, k, n_out, ldy, (hipStream_t)stream));
  return DIFUSCO_OK;
}

int difusco_linear_rows_split(const float* x, const void* planes, int precision, const float* bias,
                              const float* residual, float* y, int64_t m, int k, int n_out, int64_t ldy,
                              float* row_scale_scratch, void* stream) {
  if (!x || !planes || !y) return fail(DIFUSCO_EINVAL, "null pointer");
  if (precision < DIFUSCO_PREC_BF16X3 || precision > DIFUSCO_PREC_FP16X1)
    return fail(DIFUSCO_EINVAL, "precision must be BF16X3, BF16X6, FP16X3 or FP16X1");
  if (!(k == 64 || k == 128 || k == 256) || (n_out != k && !(k == 256 && n_out > 0 && n_out % 256 == 0)) || ldy < n_out)
    return fail(DIFUSCO_EINVAL, "split path needs k in {64,128,256}, n_out == k (or a multiple of 256 for k = 256), ldy >= n_out");
  const SplitPlanes sp = split_planes(planes, n_out, k, f16_planes(precision));      // (FP16X1: the hi plane of the fp16 pair)
  difusco::SplitScale sc;
  sc.w_inv = sp.w_inv;
  if (sp.w_inv != nullptr && row_scale_scratch != nullptr) {
    HIP_TRY(difusco::launch_row_pow2_scale(x, m, k, row_scale_scratch, (hipStream_t)stream));
    sc.row_scale = row_scale_scratch;
  }
  HIP_TRY(difusco::linear_rows_split(x, sp.planes, (long long)n_out * k, precision, bias, residual, y, m, k, n_out, ldy,
                                     (hipStream_t)stream, 0, sc));
  return DIFUSCO_OK;
}

int difusco_edge_gate_aggregate_ex(int hidden, int n_nodes, const int32_t* rowptr, const int32_t* col, const float* node4,
                                   float* ce_act, float* h, const float* norm_h_w, const float* norm_h_b,
                                   const float* norm_e_w, const float* norm_e_b, const float* out_ln_w,
                                   const float* out_ln_b, const float* tbias, int time_on_edge, int aggregation,
                                   void* stream) {
  if (!hidden_ok(hidden)) return fail(DIFUSCO_EINVAL, "hidden must be 64, 128 or 256");
  if (!rowptr || !node4 || !h || !norm_h_w || !norm_h_b || !norm_e_w || !norm_e_b || !out_ln_w || !out_ln_b || !tbias)
    return fail(DIFUSCO_EINVAL, "null pointer");
  if (aggregation < DIFUSCO_AGG_SUM || aggregation > DIFUSCO_AGG_MAX)
    return fail(DIFUSCO_EINVAL, "aggregation must be DIFUSCO_AGG_SUM, _MEAN or _MAX");
  HIP_TRY(difusco::launch_edge_gate_aggregate(hidden, n_nodes, rowptr, col, node4, ce_act, h, norm_h_w, norm_h_b, norm_e_w,
                                              norm_e_b, out_ln_w, out_ln_b, tbias, time_on_edge, (hipStream_t)stream,
                                              aggregation));
  return DIFUSCO_OK;
}

int difusco_edge_gate_aggregate(int hidden, int n_nodes, const int32_t* rowptr, const int32_t* col, const float* node4,
                                float* ce_act, float* h, const float* norm_h_w, const float* norm_h_b,
                                const float* norm_e_w, const float* norm_e_b, const float* out_ln_w,
                                const float* out_ln_b, const float* tbias, int time_on_edge, void* stream) {
  return difusco_edge_gate_aggregate_ex(hidden, n_nodes, rowptr, col, node4, ce_act, h, norm_h_w, norm_h_b, norm_e_w, norm_e_b,
                                        out_ln_w, out_ln_b, tbias, time_on_edge, DIFUSCO_AGG_SUM, stream);
}

size_t difusco_fused_scratch_bytes(int n_nodes, int n_edges) {
  if (n_nodes < 0 || n_edges < 0) return 0;
  // pieces of the neighbour sum | direct rows | tile maxima | the node rows in the kernel's log2(e) domain (ABI 11)
  return sizeof(float) * (fused_part_floats(n_edges) + (size_t)n_nodes * 256 + (size_t)(n_edges + 255) / 256 * 8 + 64 + 64 +
                          (size_t)n_nodes * 1024) + 256;
}

int difusco_edge_layer_fused_ex(int precision, int n_nodes, int n_edges, const int32_t* rowptr, const int32_t* row,
                                const int32_t* col, const float* node4, float* e, float* h, const void* planes_c,
                                const void* planes_o, const float* b_c, const float* norm_h_w, const float* norm_h_b,
                                const float* norm_e_w, const float* norm_e_b, const float* out_ln_w,
                                const float* out_ln_b, const float* b_out, const float* tbias, int time_on_edge,
                                const float* scales, void* scratch, int aggregation, int reg_gather, void* stream) {
  if (aggregation < DIFUSCO_AGG_SUM || aggregation > DIFUSCO_AGG_MAX)
    return fail(DIFUSCO_EINVAL, "aggregation must be DIFUSCO_AGG_SUM, _MEAN or _MAX");
  if (reg_gather != 0 && reg_gather != 1) return fail(DIFUSCO_EINVAL, "reg_gather must be 0 or 1");
  if (reg_gather && aggregation == DIFUSCO_AGG_MAX)      // (launch_edge_layer_fused: no register-gather instantiation of the max kinds)
    return fail(DIFUSCO_EINVAL, "fused kernel: aggregation = max has no register-gather variant");
  if (precision != DIFUSCO_PREC_BF16X3 && precision != DIFUSCO_PREC_FP16X3 && precision != DIFUSCO_PREC_FP16X1)
    return fail(DIFUSCO_EINVAL, "fused kernel: precision must be BF16X3, FP16X3 or FP16X1");
  if (!rowptr || !row || !col || !node4 || !e || !h || !planes_c || !planes_o || !b_c || !norm_h_w || !norm_h_b ||
      !norm_e_w || !norm_e_b || !out_ln_w || !out_ln_b || !b_out || !tbias || !scratch)
    return fail(DIFUSCO_EINVAL, "null pointer");
  const bool f16 = f16_planes(precision);
  if (f16 && !scales)
    return fail(DIFUSCO_EINVAL, "fused kernel, FP16X3 / FP16X1: the operand-scale record of the layer is required");
  hipStream_t st = (hipStream_t)stream;
  const long long n_tiles_pad = ((long long)n_edges + 255) / 256 * 8;
  Carver sc{(char*)scratch};
  float* part = sc.take(sizeof(float) * fused_part_floats(n_edges));
  float* direct = sc.take(sizeof(float) * (size_t)n_nodes * 256);
  float* etmax = sc.take(sizeof(float) * n_tiles_pad);
  // The caller's node4 is the reference's U h | V h | A h | B h (gnn_encoder.py:94-103).  The kernel reads the A | B rows in its
  // log2(e) domain with b_C folded into the A rows (difusco_hip.h, ABI 11 note): converted copy in the scratch.  (The step driver
  // has no such pass: its node linear produces the rows in that form.)
  float* node4_k = sc.take(sizeof(float) * (size_t)n_nodes * 1024);
  HIP_TRY(difusco::launch_fuse_node_tables(node4, b_c, n_nodes, node4_k, st));
  if (f16)      // e-stream scale per tile: normally left by the producer of e
    HIP_TRY(difusco::launch_tile_absmax_tiled(e, n_tiles_pad, etmax, st));
  difusco::FusedLayerArgs fa;
  fa.e = e, fa.node4 = node4_k, fa.row = row, fa.col = col, fa.n_edges = n_edges;
  fa.c_planes = split_planes(planes_c, 256, 256, f16).planes;
  fa.o_planes = split_planes(planes_o, 256, 256, f16).planes;
  fa.plane_stride = 256LL * 256;
  fa.b_c = b_c, fa.g_e = norm_e_w, fa.b_e = norm_e_b, fa.tbias = tbias, fa.g_o = out_ln_w, fa.b_o = out_ln_b, fa.b_out = b_out;
  fa.time_on_edge = time_on_edge, fa.part = part, fa.direct = direct, fa.scales = scales;
  fa.etmax_in = fa.etmax_out = etmax, fa.stream = st;
  HIP_TRY(difusco::launch_edge_layer_fused(precision, difusco::FusedKind::Middle,
                                           reg_gather | (aggregation == DIFUSCO_AGG_MAX ? 2 : 0), fa));      // (as the step: fused_variant)
  // (node_finalize reads the U rows, which the conversion copies unchanged: either buffer would do)
  HIP_TRY(difusco::launch_node_finalize(n_nodes, n_edges, rowptr, node4, part, direct, h, norm_h_w, norm_h_b, tbias,
                                        time_on_edge, nullptr, st, nullptr, aggregation));
  return DIFUSCO_OK;
}

int difusco_edge_layer_fused(int precision, int n_nodes, int n_edges, const int32_t* rowptr, const int32_t* row,
                             const int32_t* col, const float* node4, float* e, float* h, const void* planes_c,
                             const void* planes_o, const float* b_c, const float* norm_h_w, const float* norm_h_b,
                             const float* norm_e_w, const float* norm_e_b, const float* out_ln_w,
                             const float* out_ln_b, const float* b_out, const float* tbias, int time_on_edge,
                             const float* scales, void* scratch, void* stream) {
  return difusco_edge_layer_fused_ex(precision, n_nodes, n_edges, rowptr, row, col, node4, e, h, planes_c, planes_o, b_c, norm_h_w,
                                     norm_h_b, norm_e_w, norm_e_b, out_ln_w, out_ln_b, b_out, tbias, time_on_edge, scales, scratch,
                                     DIFUSCO_AGG_SUM, n_nodes >= (1 << 20) ? 1 : 0, stream);
}

int difusco_categorical_posterior(const float* logits, const float* xt, const float* post, int rand_mode,
                                  const float* rand, uint64_t seed, uint64_t offset, float* xt_out, float* prob_out,
                                  int64_t n, void* stream) {
  if (rand_mode < DIFUSCO_RAND_NONE || rand_mode > DIFUSCO_RAND_PHILOX)
    return fail(DIFUSCO_EINVAL, "posterior: rand_mode must be 0, 1 or 2 (the per-instance mode needs a step)");
  if (!logits || !xt || !post || !xt_out) return fail(DIFUSCO_EINVAL, "null pointer");
  if (post[4] != 0.0f && (rand_mode == DIFUSCO_RAND_NONE || (rand_mode == DIFUSCO_RAND_INJECTED && !rand)))
    return fail(DIFUSCO_EINVAL, "this step draws random numbers: provide rand or use PHILOX");
  HIP_TRY(difusco::launch_categorical_posterior(logits, xt, post, rand_mode, rand, seed, offset, xt_out, prob_out, n,
                                                (hipStream_t)stream));
  return DIFUSCO_OK;
}

int difusco_gaussian_posterior(const float* pred, const float* xt, const float* post, int rand_mode, const float* rand,
                               uint64_t seed, uint64_t offset, float* xt_out, int64_t n, void* stream) {
  if (rand_mode < DIFUSCO_RAND_NONE || rand_mode > DIFUSCO_RAND_PHILOX)
    return fail(DIFUSCO_EINVAL, "posterior: rand_mode must be 0, 1 or 2 (the per-instance mode needs a step)");
  if (!pred || !xt || !post || !xt_out) return fail(DIFUSCO_EINVAL, "null pointer");
  if (post[4] != 0.0f && (rand_mode == DIFUSCO_RAND_NONE || (rand_mode == DIFUSCO_RAND_INJECTED && !rand)))
    return fail(DIFUSCO_EINVAL, "this step draws random numbers: provide rand or use PHILOX");
  HIP_TRY(difusco::launch_gaussian_posterior(pred, xt, post, rand_mode, rand, seed, offset, xt_out, n, (hipStream_t)stream));
  return DIFUSCO_OK;
}

#ifdef DIFUSCO_PROFILING
int difusco_debug_set_ptr(int key, void* p) {
  if (key == 1) { difusco::g_fused_dbg = reinterpret_cast<unsigned long long*>(p); return DIFUSCO_OK; }
  return fail(DIFUSCO_EINVAL, "unknown debug key %d", key);
}

int difusco_debug_set(int key, int value) {
  if (key == 0) { difusco::g_fused_ablate = value; return DIFUSCO_OK; }
  if (key == 6) { difusco::g_fused_lds_pad = value; return DIFUSCO_OK; }
  if (key == 9) { difusco::g_fused_start_delay = value; return DIFUSCO_OK; }
  if (key == 7) { difusco::g_fused_opt = value; return DIFUSCO_OK; }
  if (key == 10 && value >= 0 && value <= 31) { difusco::g_node_linear_ablate = value; return DIFUSCO_OK; }
  if (key == 11 && value >= 0 && value <= 3) { g_step_skip = value; return DIFUSCO_OK; }      // bit 0: no node_finalize launches, bit 1: no node linears from layer 2 on
  if (key == 8 && (value == 0 || value == 1 || value == 4)) { difusco::g_node_linear_depth = value; return DIFUSCO_OK; }
  return fail(DIFUSCO_EINVAL, "unknown debug key %d", key);
}
#endif  // DIFUSCO_PROFILING

int difusco_profile_enable(int on, int max_launches) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (on) {
    if (max_launches < 1) max_launches = 1;
    while (g_prof.ev.size() < (size_t)max_launches * 2) {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      g_prof.ev.push_back(e);
    }
    g_prof.cat.assign(g_prof.ev.size() / 2, 0);
    g_prof.used = 0;
  }
  g_prof.on = on != 0;
  g_prof.dominant_only = on == 2;   // 2: only the dominant category (0) is bracketed - the cheap mode bench.py uses
  return DIFUSCO_OK;
}

int difusco_profile_collect(double* ms, int64_t* launches, int n_categories) {
  if (!ms || !launches || n_categories < PROF_NCAT) return fail(DIFUSCO_EINVAL, "need %d categories", PROF_NCAT);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (int c = 0; c < n_categories; ++c) { ms[c] = 0.0; launches[c] = 0; }
  for (size_t i = 0; i < g_prof.used; ++i) {
    HIP_TRY(hipEventSynchronize(g_prof.ev[2 * i + 1]));
    float t = 0.0f;
    HIP_TRY(hipEventElapsedTime(&t, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
    ms[g_prof.cat[i]] += t;
    launches[g_prof.cat[i]] += 1;
  }
  const int used = (int)g_prof.used;
  g_prof.used = 0;
  return used;
}

}  // extern "C"
