// ndp_capi.inc -- host side of libndp_hip.so: argument checks, workspace layout, kernel
// launches.  Included at the end of ndp_kernels.hip (one translation unit).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <dlfcn.h>
#include <mutex>

#include "../../include/ndp.h"

namespace ndp {

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define NDP_CHECK_ARG(cond, ...) \
  do { if (!(cond)) return ndp::fail(NDP_E_ARG, __VA_ARGS__); } while (0)

static int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NDP_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return NDP_OK;
}

// ---------------------------------------------------------------- per-kernel HIP-event timing
// Off by default.  When enabled (per host thread) every kernel launch made through this
// library is bracketed by hipEvents recorded on the stream it is launched on, so that
// bench.py can report the duration of individual kernels of a step.  Not capturable.
struct TimedLaunch { const char* name; hipEvent_t t0, t1; };
struct TimingState {
  bool on = false;
  TimedLaunch ev[4096];
  int n = 0;
};
static thread_local TimingState g_timing;

// NDP_ROCTX=1: every launch is also bracketed by a roctx range carrying the kernel's label (rocprofv3 --marker-trace
// shows the host side of each launch under the label bench.py's tables use); libroctx64 is looked up at run time, the
// library does not link against it.
struct Roctx { int (*push)(const char*); int (*pop)(); bool on; };
static Roctx& roctx() {
  static Roctx r = [] {
    Roctx x = {nullptr, nullptr, false};
    const char* e = getenv("NDP_ROCTX");
    if (e && e[0] == '1') {
      void* h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
      if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
      if (h) {
        x.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        x.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        x.on = x.push && x.pop;
      }
    }
    return x;
  }();
  return r;
}

struct KTimer {
  hipStream_t st; int idx; bool range;
  KTimer(const char* name, hipStream_t s) : st(s), idx(-1), range(false) {
    if (roctx().on) { roctx().push(name); range = true; }
    TimingState& t = g_timing;
    if (!t.on || t.n >= 4096) return;
    idx = t.n++;
    t.ev[idx].name = name;
    hipEventCreate(&t.ev[idx].t0);
    hipEventCreate(&t.ev[idx].t1);
    hipEventRecord(t.ev[idx].t0, st);
  }
  ~KTimer() {
    if (idx >= 0) hipEventRecord(g_timing.ev[idx].t1, st);
    if (range) roctx().pop();
  }
};

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int64_t pad_rows(int64_t rows) { return (rows + NDP_ROW_PAD - 1) / NDP_ROW_PAD * NDP_ROW_PAD; }
static inline int64_t pad4(int64_t n) { return (n + 3) / 4 * 4; }
static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// ---------------------------------------------------------------- kernel variants
// One list per kernel: its instantiations (template arguments, function, dynamic LDS).  set_attrs() opts every entry in
// and the launch sites take theirs from the same list: no variant is launched without its opt-in.
template <typename Args>
struct Variant { int t[3]; void (*fn)(Args); int lds; };
#define NDP_GFWD(WA) {{WA, 0, 0}, k_g_fwd<WA, false>, g_fwd_lds_floats() * 4}, {{WA, 1, 0}, k_g_fwd<WA, true>, g_fwd_lds_floats() * 4}
static const Variant<GFwdArgs> kGFwd[] = {NDP_GFWD(1), NDP_GFWD(2), NDP_GFWD(4)};                      // (W1ALIGN, PK)
#undef NDP_GFWD
#define NDP_D(NP) {{NP, 0, 0}, k_d<NP, false>, d_lds_floats<NP>() * 4}, {{NP, 1, 0}, k_d<NP, true>, d_lds_floats<NP>() * 4}
static const Variant<DArgs> kD[] = {NDP_D(1), NDP_D(2)};                                               // (NP, PK)
#undef NDP_D
static const Variant<GBwdArgs> kGBwd[] = {{{0, 0, 0}, k_g_bwd<false>, g_bwd_lds_floats() * 4},         // (PK)
                                          {{1, 0, 0}, k_g_bwd<true>, g_bwd_lds_floats() * 4}};
static const Variant<WgradArgs> kWgrad[] = {{{0, 0, 0}, k_wgrad, wgrad_lds_floats() * 4},              // (WIDE jobs)
                                            {{1, 0, 0}, k_wgrad_wide, wgrad_wide_launch_lds_floats() * 4}};
// the phase kernels: (ring, NR, preload); the large ring first, then the small one per step_code_rows count
#define NDP_A(RG, NR) {{RG, NR, 0}, k_phase_a<true, RG, NR>, phase_a_lds_floats() * 4}
static const Variant<PhaseAArgs> kPhaseA[] = {NDP_A(96, 0), NDP_A(kPhaseASmallRing, 0), NDP_A(kPhaseASmallRing, 1),
                                              NDP_A(kPhaseASmallRing, 4)};
#undef NDP_A
#define NDP_B(RG, PRE, NR) {{RG, NR, PRE}, k_phase_b<true, RG, PRE, NR>, phase_b_lds_floats(PRE) * 4}
static const Variant<PhaseBArgs> kPhaseB[] = {NDP_B(96, true, 0), NDP_B(32, false, 0), NDP_B(32, false, 1), NDP_B(32, false, 4)};
#undef NDP_B
static const Variant<NdivArgs> kNdiv[] = {{{4, 2, 0}, k_ndiv<4, 2>, 64 * 1024}, {{16, 16, 0}, k_ndiv<16, 16>, 64 * 1024}};   // (MX, MZ)
static_assert(phase_a_lds_floats() * 4 * 3 <= 160 * 1024, "phase A: three workgroups per CU at large M");

// hipFuncSetAttribute applies to the CURRENT device's copy of the code object: one flag per device (a module on
// cuda:1 must not find the opt-in done "already" by cuda:0)
constexpr int kMaxDevices = 64;
static std::once_flag g_attr_once[kMaxDevices];
static std::once_flag& device_once(std::once_flag (&flags)[kMaxDevices]) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
  return flags[dev];
}

template <typename K>
static void allow_lds(K kernel, int bytes) {
  // dynamic LDS above 64 KiB must be opted into once per kernel
  hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}
template <typename Args, size_t N>
static void allow_lds(const Variant<Args> (&list)[N]) {
  for (const Variant<Args>& v : list) allow_lds(v.fn, v.lds);
}
static void set_attrs() {
  std::call_once(device_once(g_attr_once), [] {
    allow_lds(kGFwd); allow_lds(kD); allow_lds(kGBwd); allow_lds(kWgrad); allow_lds(kPhaseA); allow_lds(kPhaseB); allow_lds(kNdiv);
  });
}

// index of the list's variant with these template arguments, -1: none
template <typename Args, size_t N>
static int find_variant(const Variant<Args> (&list)[N], int t0, int t1 = 0) {
  for (size_t i = 0; i < N; ++i)
    if (list[i].t[0] == t0 && list[i].t[1] == t1) return (int)i;
  return -1;
}
// lds < 0: the variant's own
template <typename Args, size_t N>
static int launch_variant(const char* what, const Variant<Args> (&list)[N], int index, unsigned grid, int threads, int64_t lds,
                          hipStream_t st, const Args& a) {
  if (index < 0 || index >= (int)N) return fail(NDP_E_LAUNCH, "%s: no such kernel variant", what);
  set_attrs();
  hipLaunchKernelGGL(list[index].fn, dim3(grid), dim3(threads), (size_t)(lds < 0 ? list[index].lds : lds), st, a);
  return check_launch(what);
}

// ---------------------------------------------------------------- the two networks
// A network is its layers' widths, layer l being [width[l + 1] x width[l]]: parameter layout, packed copies, workspaces,
// pack specs and weight-gradient jobs derive from them.  code0: the first of fc1's 256 code columns (G: noise columns
// follow them, D: the action columns come first).
struct Mlp { int layers; int width[6]; int code0; };
constexpr Mlp g_mlp(int nz) { return Mlp{5, {CODE + nz, 128, 64, 128, 256, ADIM}, 0}; }
constexpr Mlp d_mlp() { return Mlp{4, {ADIM + CODE, 64, 128, 256, 1, 0}, ADIM}; }

struct MlpLayout { int64_t w[5], b[5], total; };
constexpr MlpLayout layout(const Mlp& n) {
  MlpLayout L = {};
  int64_t o = 0;
  for (int l = 0; l < n.layers; ++l) {
    L.w[l] = o; o += (int64_t)n.width[l + 1] * n.width[l];
    L.b[l] = o; o += n.width[l + 1];
  }
  L.total = o;
  return L;
}
// packed-copy layout (floats): the forward copies of every layer but the last (fc1: its code columns), then the
// data-gradient copies of those from fc2 on
struct PackOffsets { int fwd[4], dg[4], total; };
constexpr PackOffsets pack_offsets(const Mlp& n) {
  PackOffsets P = {};
  int o = 0;
  for (int l = 0; l + 1 < n.layers; ++l) { P.fwd[l] = o; o += n.width[l + 1] * (l ? n.width[l] : CODE); }
  P.dg[0] = -1;
  for (int l = 1; l + 1 < n.layers; ++l) { P.dg[l] = o; o += n.width[l + 1] * n.width[l]; }
  P.total = o;
  return P;
}
static_assert(pack_offsets(g_mlp(1)).total == 131072 && pack_offsets(d_mlp()).total == 98304, "packed copies the kernels index");

static GNet g_net(const float* p, int nz, const float* packed = nullptr) {
  const Mlp m = g_mlp(nz);
  const MlpLayout L = layout(m);
  const PackOffsets P = pack_offsets(m);
  GNet n;
  n.w1 = p + L.w[0]; n.b1 = p + L.b[0]; n.w2 = p + L.w[1]; n.b2 = p + L.b[1]; n.w3 = p + L.w[2]; n.b3 = p + L.b[2];
  n.w4 = p + L.w[3]; n.b4 = p + L.b[3]; n.w5 = p + L.w[4]; n.b5 = p + L.b[4];
  n.ld1 = m.width[0]; n.nz = nz;
  n.pf1 = n.pf2 = n.pf3 = n.pf4 = n.pg2 = n.pg3 = n.pg4 = nullptr;
  if (packed) {
    n.pf1 = packed + P.fwd[0]; n.pf2 = packed + P.fwd[1]; n.pf3 = packed + P.fwd[2]; n.pf4 = packed + P.fwd[3];
    n.pg2 = packed + P.dg[1]; n.pg3 = packed + P.dg[2]; n.pg4 = packed + P.dg[3];
  }
  return n;
}
static DNet d_net(const float* p, const float* packed = nullptr) {
  const MlpLayout L = layout(d_mlp());
  const PackOffsets P = pack_offsets(d_mlp());
  DNet n;
  n.w1 = p + L.w[0]; n.b1 = p + L.b[0]; n.w2 = p + L.w[1]; n.b2 = p + L.b[1]; n.w3 = p + L.w[2]; n.b3 = p + L.b[2];
  n.w4 = p + L.w[3]; n.b4 = p + L.b[3];
  n.pf1 = n.pf2 = n.pf3 = n.pg2 = n.pg3 = nullptr;
  if (packed) {
    n.pf1 = packed + P.fwd[0]; n.pf2 = packed + P.fwd[1]; n.pf3 = packed + P.fwd[2];
    n.pg2 = packed + P.dg[1]; n.pg3 = packed + P.dg[2];
  }
  return n;
}
static PackSpec pack_spec(const Mlp& n, float* packed) {
  const MlpLayout L = layout(n);
  const PackOffsets P = pack_offsets(n);
  PackSpec ps;
  memset(&ps, 0, sizeof(ps));
  for (int l = 0; l + 1 < n.layers; ++l) {
    PackLayer& p = ps.L[l];
    p.w_off = (int)L.w[l]; p.ld = n.width[l]; p.out = n.width[l + 1];
    p.main0 = l ? 0 : n.code0; p.main_in = l ? n.width[l] : CODE;
    p.fwd_off = P.fwd[l]; p.dg_off = P.dg[l];
  }
  ps.nl = n.layers - 1; ps.packed = packed;
  return ps;
}
static int launch_pack(const float* params, const Mlp& n, float* packed, hipStream_t st) {
  KTimer kt("k_pack", st);
  PackArgs a;
  a.params = params; a.n = (int)layout(n).total; a.ps = pack_spec(n, packed);
  hipLaunchKernelGGL(k_pack, dim3(blocks_of(a.n)), dim3(kThreads), 0, st, a);
  return check_launch("k_pack");
}

// ---------------------------------------------------------------- weight-gradient chunk counts
// the 64 x 64 (and skinny) jobs of a network with every layer in them; wide: without the 256 x 128 layer's eight
constexpr int job_count(const Mlp& n, bool wide) {
  int jobs = n.width[1] / 64 * (CODE / 64 + 1);           // fc1: the code column blocks and the narrow tail per 64 outputs
  for (int l = 1; l < n.layers; ++l) {
    const int out = n.width[l + 1], in = n.width[l];
    if (!(wide && out == 256 && in == 128)) jobs += (out < 64 ? 1 : out / 64) * (in / 64);
  }
  return jobs;
}
// split-K chunking of the weight-gradient rows
static int wgrad_chunks(int njobs, int64_t rows) {
  int64_t want = 512 / njobs;                          // jobs*chunks <= 512 = 2 workgroups per CU (64 KiB LDS each): one resident round
  if (want >= 8) want = want / 8 * 8;                  // whole chunks per XCD (k_wgrad deals chunk c to XCD c % 8)
  // With many rows the light jobs (K-deduplicated fc1 columns, the 1- and 4-wide layers) retire
  // early and leave their slots to the heavy ones: more, shorter chunks then balance better
  // (measured at B = 1024: 24/16 chunks 0.707 ms/step, 32/32 0.652; at B = 64 the opposite).
  if (rows >= 16384 && want < 32) want = 32;
  int64_t maxc = rows / 64;                             // at least 64 rows per chunk
  if (maxc < 1) maxc = 1;
  if (want > maxc) want = maxc;
  if (want > 64) want = 64;
  return (int)want;
}
// Large M: the 256 x 128 layer (D.fc3, G.fc4) as two LDS-staged 128 x 128 jobs per row chunk (k_wgrad_wide, WG_WIDE)
// instead of eight 64 x 64 jobs; their workgroups carry 4 x the work of a 64 x 64 job per row, so they get their own,
// larger chunk count (and as many slabs: that layer's parameters are a region of the slab sum).  0: not used.
static int wgrad_wide_chunks(int64_t rows) {
  // from 28,000 rows (below, the 64 x 64 jobs win: B = 512 / K = 6, 25,088 / 21,504 rows, 0.2869 vs 0.2929 ms; B = 384 / K = 6
  // 0.2254 vs 0.2347), a multiple of 32 chunks (56 chunks were 6 us slower than 64 at 28,672 rows),
  if (rows < 28000) return 0;
  // about 480 rows per chunk (two 128 x 128 jobs per chunk: ~30 slabs of 16 rows per workgroup).  Measured with the layer
  // split in two jobs (commit 2abfcda): B = 128 / K = 32 (29,568 / 28,672 rows) 64 chunks 0.3191 ms per
  // step (48: 0.3326, 80: 0.3212, 96: 0.3263, 128: 0.3542; without the WIDE jobs 0.3290), B = 1024 / K = 6 (50,176 rows)
  // 96 chunks 0.4963 (64: 0.5084; without 0.5158).  As ONE 256 x 128 job per chunk the layer needed 128-160 chunks
  // and the slab sums grew by 4 us each: 0.3247 / 0.5027.
  const int64_t want = (rows / 480 + 16) / 32 * 32;
  return (int)(want < 64 ? 64 : want);
}
// Chunk counts of a launch: `heavy` for the jobs that run a full 64 x 64 block over every row (fc2..fc4 of G,
// fc2 / fc3 of D), `light` for the K-deduplicated fc1 blocks and the 1..4-wide operands, which finish in half the
// time (stamps): at small M giving the heavy jobs more, shorter chunks and the light ones fewer keeps the launch
// within one resident round (<= 512 workgroups) and shortens its critical path.  heavy >= light; heavy is the slab
// count.  From 16,384 rows, or where the heavy count would leave a chunk fewer than 64 rows, both are wgrad_chunks.
// wide: wgrad_wide_chunks; slabs a launch may write: the 64 x 64 jobs' chunk count or the WIDE job's, whichever is larger.
struct NetPlan { int heavy, light, wide, slabs; };
static NetPlan wgrad_plan(bool is_g, int64_t rows) {
  // measured: G 24 at config 2; D (whose real pass is deduplicated: FLAT + M rows) 8 up to 4,096 rows -- 152 workgroups
  // and 8 slabs, 79.0 vs 80.3 us per step at B = 64, 75.2 vs 76.8 at B = 32 -- and 32 above (B = 128, 192)
  // (G's light jobs: 12 chunks, 12,788 vs 12,742 steps/s with 8 at config 2, three alternating runs each)
  const int h = is_g ? 24 : (rows <= 4096 ? 8 : 32), l = is_g ? 12 : 8;
  NetPlan p = {h, l, wgrad_wide_chunks(rows), 0};
  if (rows >= 16384 || rows / 64 < h) p.heavy = p.light = wgrad_chunks(job_count(is_g ? g_mlp(1) : d_mlp(), false), rows);
  p.slabs = p.heavy > p.wide ? p.heavy : p.wide;
  return p;
}
// a chunk may end up empty when rows_per_chunk rounds up; its slab must still be written
static unsigned wgrad_grid(int njobs, const NetPlan& p, int64_t nd_blocks) {
  return (unsigned)((p.wide ? 2 * p.wide : 0) + 8 * ((p.heavy + 7) / 8) * njobs + nd_blocks);
}

// ---------------------------------------------------------------- workspaces
// A workspace is a struct of float offsets into the buffer it lies in, from `at` to `end` (its size when at = 0).
// stack_rows: n consecutive [rows x width[i]] tensors from `at`; returns where they end.
static int64_t stack_rows(int64_t at, int64_t rows, const int* width, int n, int64_t* off) {
  for (int i = 0; i < n; ++i) { off[i] = at; at += rows * width[i]; }
  return at;
}
// G activations saved by the forward: h1 | h2 | h3 | h4, each [mpad x width]
struct GActs { int64_t h[4], end; };
static GActs g_acts(int64_t at, int64_t mpad) {
  const Mlp n = g_mlp(1);
  GActs a;
  a.end = stack_rows(at, mpad, n.width + 1, 4, a.h);
  return a;
}
// G backward scratch: dy1 | dy2 | dy3 | dy4 | dy5 | slabs
struct GBwdWs { int64_t dy[5], slabs, end; NetPlan plan; int64_t slab_stride; };
static GBwdWs g_bwd_ws(int64_t at, int64_t mpad, int nz) {
  const Mlp n = g_mlp(nz);
  GBwdWs w;
  w.slabs = stack_rows(at, mpad, n.width + 1, 5, w.dy);
  w.plan = wgrad_plan(true, mpad);
  w.slab_stride = pad4(layout(n).total);
  w.end = w.slabs + w.plan.slabs * w.slab_stride;
  return w;
}
// D backward scratch: xa | h1 | h2 | h3 | dy1 | dy2 | dy3 | dl | slabs | loss partials
// rows: all rows the weight-gradient jobs run over (the passes back to back)
struct DBwdWs { int64_t xa, h[3], dy[4], slabs, lossp, end; NetPlan plan; int64_t slab_stride; };   // dy[3]: dl
static DBwdWs d_bwd_ws(int64_t at, int64_t rows) {
  const Mlp n = d_mlp();
  DBwdWs w;
  w.xa = at;
  w.slabs = stack_rows(stack_rows(at + rows * ADIM, rows, n.width + 1, 3, w.h), rows, n.width + 1, 4, w.dy);
  w.plan = wgrad_plan(false, rows);
  w.slab_stride = pad4(layout(n).total);
  w.lossp = w.slabs + w.plan.slabs * w.slab_stride;
  w.end = w.lossp + pad4(rows / 16);
  return w;
}
// the workspaces' tensors in the kernel argument structs' named fields
template <typename Args, typename P> static void hand_g_acts(Args& a, P* base, const GActs& s) {
  a.h1 = base + s.h[0]; a.h2 = base + s.h[1]; a.h3 = base + s.h[2]; a.h4 = base + s.h[3];
}
template <typename Args, typename P> static void hand_g_acts_phase(Args& a, P* base, const GActs& s) {
  a.gh1 = base + s.h[0]; a.gh2 = base + s.h[1]; a.gh3 = base + s.h[2]; a.gh4 = base + s.h[3];
}
template <typename Args, typename P> static void hand_g_bwd(Args& a, P* base, const GBwdWs& w) {
  a.dy1 = base + w.dy[0]; a.dy2 = base + w.dy[1]; a.dy3 = base + w.dy[2]; a.dy4 = base + w.dy[3]; a.dy5 = base + w.dy[4];
}
template <typename Args, typename P> static void hand_d_bwd(Args& a, P* base, const DBwdWs& w) {
  a.xa = base + w.xa; a.h1 = base + w.h[0]; a.h2 = base + w.h[1]; a.h3 = base + w.h[2];
  a.dy1 = base + w.dy[0]; a.dy2 = base + w.dy[1]; a.dy3 = base + w.dy[2]; a.dl = base + w.dy[3];
}

// ---------------------------------------------------------------- launch helpers
static int launch_g_fwd(const GNet& net, const float* code, int64_t ld_code, int code_rep,
                        const float* noise, int64_t ld_noise, int64_t m, float* acts, float* action_hat, hipStream_t st) {
  GFwdArgs a;
  a.net = net;
  a.code = code; a.ld_code = ld_code; a.code_rep = code_rep;
  a.code_vec4 = (ld_code % 4 == 0) && aligned16(code);
  a.noise = noise; a.ld_noise = ld_noise; a.m = m;
  a.h1 = a.h2 = a.h3 = a.h4 = nullptr;
  if (acts) hand_g_acts(a, acts, g_acts(0, pad_rows(m)));
  a.action_hat = action_hat;
  a.noise_out = nullptr; a.noise_seed = 0; a.noise_step = nullptr;
  const int walign = (net.ld1 % 4 == 0) ? 4 : (net.ld1 % 2 == 0 ? 2 : 1);
  KTimer kt("k_g_fwd", st);
  return launch_variant("k_g_fwd", kGFwd, find_variant(kGFwd, walign, net.pf1 != nullptr), (unsigned)(pad_rows(m) / 16), kThreads,
                        -1, st, a);
}

// Every kernel of the step works on 16-row tiles; the 2-pass D step stacks 16 real + 16 fake rows per workgroup.
// Measured (bench.py --batch 192..2048, K = 6 and 32): 16-row tiles win at every size -- their LDS footprint lets 2+
// workgroups share a CU, which hides more latency than the halved weight traffic of 32-row tiles bought.
static int launch_d(DArgs& a, int npass, hipStream_t st) {
  a.ntiles = (int)(a.mpad / 16);
  a.nd.n = 0;
  KTimer kt(a.do_backward ? (npass == 2 ? "k_d[2 pass fwd+bwd]" : "k_d[fwd+bwd]") : "k_d[fwd]", st);
  return launch_variant("k_d", kD, find_variant(kD, npass, a.net.pf1 != nullptr), (unsigned)a.ntiles, kThreads, -1, st, a);
}

static int launch_g_bwd(const GNet& net, int64_t m, const float* acts, const float* d_action, float* ws, const GBwdWs& w, hipStream_t st) {
  GBwdArgs b;
  b.net = net;
  b.m = m;
  hand_g_acts(b, acts, g_acts(0, pad_rows(m)));
  b.d_action = d_action; b.d_action2 = nullptr;
  hand_g_bwd(b, ws, w);
  KTimer kt("k_g_bwd", st);
  return launch_variant("k_g_bwd", kGBwd, find_variant(kGBwd, net.pg2 != nullptr), (unsigned)(pad_rows(m) / 16), kThreads, -1, st, b);
}

// K-deduplicated fc1 code columns: segments per 16-row tile and padded entry count
static int seg_per_tile(int K) { int s = 15 / K + 2; return s < 16 ? s : 16; }
static int64_t seg_entries(int64_t mpad, int K) { return (mpad / 16 * seg_per_tile(K) + 15) / 16 * 16; }

static WgradJob make_job(const float* A, int lda, int a_cols, const float* B, int ldb, int b_cols,
                         int64_t dst_off, int dst_ld, int64_t bias_off, int kind, int nchunks) {
  WgradJob j;
  j.A = A; j.lda = lda; j.a_cols = a_cols;
  j.B = B; j.ldb = ldb; j.b_cols = b_cols;
  j.b_rowmod = 0x7fffffff; j.b_rowdiv = 1; j.b_rowmax = 0x7fffffff;
  j.b_vec = (ldb % 4 == 0) && aligned16(B);
  j.dst_off = (int)dst_off; j.dst_ld = dst_ld; j.bias_off = (int)bias_off; j.kind = kind;
  j.rows = 0; j.seg = 0; j.seg_s = 1; j.seg_k = 1; j.seg_wrap = 0;
  j.nchunks = nchunks;
  return j;
}

// The per-network part of a weight gradient, fc1's columns.  Code: row r reads code row min((r % rowmod) / code_rep,
// (m - 1) / code_rep); with dy1seg (fused step) over seg_rows entries of the phase kernel's per-tile segment sums, those
// from seg_wrap on being plain rows.  Tail: G's noise columns behind the code, D's action columns in front.
struct Fc1Columns {
  const float* code; int64_t ld_code; int code_rep, rowmod;
  const float* dy1seg; int seg_rows, seg_wrap;
  const float* tail; int64_t ld_tail; int tail_cols, tail_rowmax;
};
// The weight-gradient jobs of a network over m rows: 64 x 64 blocks, the bias with the first column block, SKINNY_A for
// outputs narrower than 64, and behind them the WIDE pair for the 256 x 128 layer when the plan has wide chunks.  dy[l]:
// layer l's pre-activation gradient, x[l]: its input (l >= 1).  fc1 and the last layer are light (the reduce's regions).
static void build_jobs(WgradArgs& w, const Mlp& net, bool is_g, const NetPlan& p, const float* const* dy,
                       const float* const* x, const Fc1Columns& f, int64_t m) {
  const MlpLayout L = layout(net);
  const int in1 = net.width[0], out1 = net.width[1], last = net.layers - 1;
  int n = 0, wide_layer = 0;
  for (int jb = 0; jb < out1 / 64; ++jb) {
    for (int kb = 0; kb < CODE / 64; ++kb) {
      WgradJob j = make_job((f.dy1seg ? f.dy1seg : dy[0]) + jb * 64, out1, 64, f.code + kb * 64, (int)f.ld_code, 64,
                            L.w[0] + (int64_t)jb * 64 * in1 + net.code0 + kb * 64, in1, kb == 0 ? L.b[0] + jb * 64 : -1,
                            WG_FULL, p.light);             // the whole fc1 layer is "light" (one slab count per layer)
      j.b_rowmod = f.rowmod; j.b_rowdiv = f.code_rep; j.b_rowmax = (int)((m - 1) / f.code_rep);
      if (f.dy1seg) {
        j.rows = f.seg_rows; j.seg = 1; j.seg_wrap = f.seg_wrap;
        j.seg_s = seg_per_tile(f.code_rep); j.seg_k = f.code_rep;
      }
      w.job[n++] = j;
    }
    WgradJob t = make_job(dy[0] + jb * 64, out1, 64, f.tail, (int)f.ld_tail, f.tail_cols,
                          L.w[0] + (int64_t)jb * 64 * in1 + (net.code0 ? 0 : CODE), in1, -1, WG_SKINNY_B, p.light);
    t.b_rowmax = f.tail_rowmax;
    w.job[n++] = t;
  }
  for (int l = 1; l <= last; ++l) {
    const int out = net.width[l + 1], in = net.width[l];
    if (p.wide && out == 256 && in == 128) { wide_layer = l; continue; }
    const int a_cols = out < 64 ? out : 64;
    for (int jb = 0; jb < (out < 64 ? 1 : out / 64); ++jb)
      for (int kb = 0; kb < in / 64; ++kb)
        w.job[n++] = make_job(dy[l] + jb * 64, out, a_cols, x[l] + kb * 64, in, 64, L.w[l] + (int64_t)jb * 64 * in + kb * 64, in,
                              kb == 0 ? L.b[l] + jb * 64 : -1, out < 64 ? WG_SKINNY_A : WG_FULL, out < 64 ? p.light : p.heavy);
  }
  w.njobs = n; w.net_is_g = is_g;
  w.nchunks = p.heavy;
  w.nwide = 0; w.wide_chunks = 0;
  w.wide_begin = w.wide_end = 0;
  if (wide_layer) {                                      // the 256 x 128 layer as LDS-staged jobs per row chunk (large M)
    const int l = wide_layer;
    w.nwide = 2;
    for (int h = 0; h < 2; ++h)
      w.job[n + h] = make_job(dy[l] + h * 128, 256, 128, x[l], 128, 128, L.w[l] + (int64_t)h * 128 * 128, 128, L.b[l] + h * 128,
                              WG_WIDE, p.wide);
    w.wide_chunks = p.wide;
    w.wide_begin = (int)L.w[l]; w.wide_end = (int)L.b[l] + 256;
  }
  w.nreg = 2;                                            // layers whose jobs are light: fc1 and the last
  w.reg_begin[0] = (int)L.w[0]; w.reg_end[0] = (int)L.b[0] + out1;
  w.reg_begin[1] = (int)L.w[last]; w.reg_end[1] = (int)L.b[last] + net.width[last + 1];
}
// weight-gradient jobs of the Decoder (26): operands dy1..dy5 / code, noise, h1..h4
static void build_g_jobs(WgradArgs& w, int nz, const float* ws, const GBwdWs& g, const float* acts, const GActs& a,
                         const float* code, int64_t ld_code, int code_rep, const float* noise, int64_t ld_noise, int64_t m,
                         const float* dy1seg) {
  const float* dy[5] = {ws + g.dy[0], ws + g.dy[1], ws + g.dy[2], ws + g.dy[3], ws + g.dy[4]};
  const float* x[5] = {nullptr, acts + a.h[0], acts + a.h[1], acts + a.h[2], acts + a.h[3]};
  const Fc1Columns f = {code, ld_code, code_rep, 0x7fffffff, dy1seg, (int)seg_entries(pad_rows(m), code_rep), 0,
                        noise, ld_noise, nz, (int)(m - 1)};
  build_jobs(w, g_mlp(nz), true, g.plan, dy, x, f, m);
}
// weight-gradient jobs of the Discriminator (19) over the rows of `d`
// dy1seg != null (fused step): rows = the rpad distinct real rows followed by the mpad fake rows; fc1's code columns
// run over `dy1seg` = the fake pass' per-tile segment sums followed by the real rows' dY1 (k_phase_a).  Otherwise
// (module backward, repeat D steps) the passes are mpad rows each and every row reads its code row.
static void build_d_jobs(WgradArgs& w, const float* ws, const DBwdWs& d, const float* code, int64_t ld_code, int code_rep,
                         int64_t m, int64_t mpad, const float* dy1seg, int64_t rpad) {
  const float* dy[4] = {ws + d.dy[0], ws + d.dy[1], ws + d.dy[2], ws + d.dy[3]};
  const float* x[4] = {nullptr, ws + d.h[0], ws + d.h[1], ws + d.h[2]};
  const int e = (int)seg_entries(mpad, code_rep);        // entries >= e are real rows: entry e + f pairs with code row f
  const Fc1Columns f = {code, ld_code, code_rep, (int)mpad, dy1seg, e + (int)rpad, e, ws + d.xa, ADIM, ADIM, 0x7fffffff};
  build_jobs(w, d_mlp(), false, d.plan, dy, x, f, m);
}

struct AdamHyper { float lr, beta1, beta2; };

static int launch_wgrad(WgradArgs& w, int64_t rows, const NetPlan& p, float* slabs, int64_t slab_stride, int32_t* bump,
                        const AdamHyper& hp, const NdivArgs* nd, int64_t nd_blocks, hipStream_t st) {
  w.rows = (int)rows;
  w.slabs = slabs; w.slab_stride = slab_stride; w.bump = bump;
  w.lr = hp.lr; w.beta1 = hp.beta1; w.beta2 = hp.beta2;
  if (nd != nullptr && nd_blocks > 0) w.nd = *nd; else { memset(&w.nd, 0, sizeof(w.nd)); nd_blocks = 0; }
  KTimer kt(w.net_is_g ? "k_wgrad[G]" : "k_wgrad[D]", st);
  return launch_variant("k_wgrad", kWgrad, find_variant(kWgrad, w.nwide != 0), wgrad_grid(w.njobs, p, nd_blocks), kThreads, -1, st, w);
}

// + 1: a block without parameters that computes the loss scalars beside the others (P2P: it takes part in the
// hand-shake like any block, every rank launches the same grid)
static unsigned reduce_grid(int64_t n) { return blocks_of(n) + 1; }
static int launch_reduce(ReduceArgs& r, hipStream_t st) {
  KTimer kt("k_reduce_adam", st);
  hipLaunchKernelGGL(r.p2p.world > 1 ? k_reduce_adam<true> : k_reduce_adam<false>, dim3(reduce_grid(r.n)), dim3(kThreads), 0, st, r);
  return check_launch("k_reduce_adam");
}

static int fill_p2p(const char* fn, P2PArgs& x, const ndp_p2p* c, int net, int64_t n);
// the Adam update fused into the reduce, and the packed copies it refreshes
struct FusedAdam { float *params, *exp_avg, *exp_avg_sq; float lr, beta1, beta2, eps; PackSpec pack; };
// Every ReduceArgs: n sums over p.heavy slabs (w: the jobs that wrote them; their light layers sum over p.light slabs, the
// WIDE layer over p.wide), to `grad` and, with `adam`, into the parameters; p2p: the exchange between ranks or null.
static int fill_reduce(const char* fn, ReduceArgs& r, const float* slabs, int64_t slab_stride, int64_t n, const NetPlan& p,
                       const WgradArgs* w, float* grad, const int32_t* step, const FusedAdam* adam, const ndp_p2p* p2p, int net) {
  memset(&r, 0, sizeof(r));
  r.slabs = slabs; r.nchunks = p.heavy; r.slab_stride = slab_stride; r.n = n;
  if (w) {
    r.nregions = p.light != p.heavy ? w->nreg : 0;
    for (int i = 0; i < r.nregions; ++i) { r.reg_begin[i] = w->reg_begin[i]; r.reg_end[i] = w->reg_end[i]; r.reg_slabs[i] = p.light; }
    if (w->nwide) {                                      // the WIDE layer wrote wide_chunks slabs
      const int i = r.nregions++;
      r.reg_begin[i] = w->wide_begin; r.reg_end[i] = w->wide_end; r.reg_slabs[i] = w->wide_chunks;
    }
  }
  r.grad = grad; r.step = step;
  if (adam) {
    r.params = adam->params; r.exp_avg = adam->exp_avg; r.exp_avg_sq = adam->exp_avg_sq;
    r.lr = adam->lr; r.beta1 = adam->beta1; r.beta2 = adam->beta2; r.eps = adam->eps;
    r.pack = adam->pack;
  }
  return fill_p2p(fn, r.p2p, p2p, net, n);
}
static void add_loss(ReduceArgs& r, const float* partials, int64_t count, float scale, int slot) {
  LossTerm& t = r.loss[r.nloss++];
  t.partials = partials; t.count = (int)count; t.scale = scale; t.slot = slot;
}

static int launch_adam(AdamArgs& a, hipStream_t st) {
  KTimer kt("k_adam", st);
  hipLaunchKernelGGL(k_adam, dim3(blocks_of(a.n)), dim3(kThreads), 0, st, a);
  return check_launch("k_adam");
}

static int ndiv_block_threads(int k) { return k <= 64 ? 64 : kThreads; }
static int ndiv_rows_per_block(int k, int threads) { return threads / k; }
static size_t ndiv_lds_bytes(int G, int k, int cx, int cz) { return ((size_t)G * k * (cx + cz + 2) + 8) * 4; }

static NdivArgs ndiv_args(const float* x, int cx, const float* z, int cz, int64_t n, int k, float grad_scale,
                          float* grad, float* partials, int threads) {
  NdivArgs a;
  a.x = x; a.cx = cx; a.z = z; a.cz = cz; a.n = n; a.k = k;
  a.rows_per_block = ndiv_rows_per_block(k, threads);
  a.grad_scale = grad_scale; a.grad = grad; a.partials = partials;
  return a;
}

static int launch_ndiv(const float* x, int cx, const float* z, int cz, int64_t n, int k, float grad_scale,
                       float* grad, float* partials, hipStream_t st) {
  const int threads = ndiv_block_threads(k);
  NdivArgs a = ndiv_args(x, cx, z, cz, n, k, grad_scale, grad, partials, threads);
  const int G = a.rows_per_block;
  KTimer kt("k_ndiv", st);
  return launch_variant("k_ndiv", kNdiv, cx <= 4 && cz <= 2 ? 0 : 1, (unsigned)((n + G - 1) / G), threads,
                        (int64_t)ndiv_lds_bytes(G, k, cx, cz), st, a);
}

// ------------------------------------------------------------------ fused train step
// More workgroups than CUs: several per CU, small weight rings.  Up to 256 workgroups each sits alone on a CU with
// 96-register rings; phase B's then also fetches G's activations at kernel start into LDS of their own (nothing else
// hides the mid-kernel round trip).
static bool several_per_cu(int64_t workgroups) { return workgroups > 256; }

// The K samples of a flat row share its code: a 16-row tile holds 1 distinct code row when K % 16 == 0 and at most 4
// when K >= 6 -- fc1's code columns become that many dot-product rows per tile on the VALU (code_rows_dot in
// ndp_kernels.hip) instead of 16 k-steps on the matrix pipe.  Returns the rows per tile the kernels carry (0: MFMA path).
// It pays only where the matrix pipe is the bound -- several workgroups per CU, the small-ring variants: B = 1024 / K = 6
// 0.529 -> 0.518 ms, B = 128 / K = 32 0.351 -> 0.334 ms.  With one workgroup per CU the MFMA k-loop of fc1 runs while the
// next layers' weights stream in, and the VALU + LDS work that would replace it is longer (measured: config 2 with four
// rows, phase A 27.0 -> 30.4 us; B = 8 / K = 32 with one row, 27.3 -> 28.2 us).
static int step_code_rows(int K, bool several_per_cu) {
  if (!several_per_cu) return 0;
  return K % 16 == 0 ? 1 : (K >= 6 ? 4 : 0);
}
// the phase kernel's variant for a grid: its index in kPhaseA / kPhaseB
template <typename Args, size_t N>
static int phase_variant(const Variant<Args> (&list)[N], int64_t workgroups, int K) {
  const bool small = several_per_cu(workgroups);
  const int nr = step_code_rows(K, small);
  for (size_t i = 0; i < N; ++i)
    if ((list[i].t[0] < 96) == small && list[i].t[1] == nr) return (int)i;
  return -1;
}

// The one predicate of a step configuration, for every step entry point.
static bool step_config_ok(const ndp_step_config* c) {
  return c && c->noise_dim >= 1 && c->noise_dim <= NDP_MAX_NOISE_DIM && c->num_sample >= 1 && c->num_sample <= NDP_MAX_SAMPLES &&
         c->flat >= 1 && c->flat < (1ll << 28) && c->flat * c->num_sample < (1ll << 28);
}
#define NDP_CHECK_STEP_CONFIG(fn, c) \
  NDP_CHECK_ARG(ndp::step_config_ok(c), "%s: null configuration, noise_dim outside 1..16, num_sample outside 1..256, flat < 1 " \
                "or flat * num_sample >= 2^28", fn)

// Everything the host decides about a step, from its configuration and whether the D step is the first of its iteration
// (real pass on the distinct rows, k_phase_a) or a repeat (two full passes, k_d).  No HIP call.
// workspace: [G acts][G bwd ws][D bwd ws][d_action m x 4][ndiv grad m x 4][ndiv partials][packed G][packed D][D seg][G seg]
struct StepPlan {
  int64_t m, mpad, rpad;                 // generated rows, padded; the distinct real rows (FLAT of them, see k_phase_a), padded
  int64_t d_rows;                        // rows of D's weight gradient: rpad + mpad, or 2 mpad on a repeat D step
  int seg_s; int64_t seg_entries;        // K-deduplicated fc1 columns: segments per tile, padded entries
  // NDiv rides in the D-step launch (256-thread blocks) when its shape fits the <4,2>
  // specialisation (noise_dim <= 2); otherwise it is a kernel of its own in phase B.
  bool ndiv_fused; int ndiv_threads; int64_t ndiv_blocks;   // blocks: also its loss partials
  // first D step: one workgroup per fake tile (G + D) and one per tile of distinct real rows; up to 256 of them sit alone
  // on a CU each with deep weight rings, more share CUs (three per CU by LDS) with small ones.  Repeat: one per tile, k_d.
  unsigned d_front_grid; int phase_a;    // phase_a: index in kPhaseA, -1 on a repeat D step
  unsigned phase_b_grid; int phase_b;    // index in kPhaseB
  unsigned wgrad_d_grid, wgrad_g_grid, reduce_d_grid, reduce_g_grid;
  int64_t loss_count_d, loss_count_g;    // workgroups that wrote a BCE partial
  GActs acts; GBwdWs gw; DBwdWs dw;      // dw: this D step's layout of the D scratch (the area holds either)
  int64_t d_action, nd_grad, nd_part, g_packed, d_packed;
  int64_t d_seg, g_seg;                  // segment sums of dY1 for the K-deduplicated fc1 weight gradients
  int64_t floats;
};
static StepPlan step_plan(const ndp_step_config* c, bool first) {
  const int K = c->num_sample;
  StepPlan p;
  p.m = c->flat * K; p.mpad = pad_rows(p.m); p.rpad = pad_rows(c->flat);
  p.d_rows = first ? p.rpad + p.mpad : 2 * p.mpad;
  p.seg_s = seg_per_tile(K); p.seg_entries = seg_entries(p.mpad, K);
  p.ndiv_fused = c->noise_dim <= 2;
  p.ndiv_threads = p.ndiv_fused ? kThreads : ndiv_block_threads(K);
  const int G = ndiv_rows_per_block(K, p.ndiv_threads);
  p.ndiv_blocks = (c->flat + G - 1) / G;
  p.acts = g_acts(0, p.mpad);
  p.gw = g_bwd_ws(p.acts.end, p.mpad, c->noise_dim);
  p.dw = d_bwd_ws(p.gw.end, p.d_rows);   // D scratch: the fused step's layout or two full passes (repeat D steps)
  const int64_t other = d_bwd_ws(p.gw.end, first ? 2 * p.mpad : p.rpad + p.mpad).end;
  p.d_action = p.dw.end > other ? p.dw.end : other;
  p.nd_grad = p.d_action + p.mpad * ADIM;
  p.nd_part = p.nd_grad + p.mpad * ADIM;
  p.g_packed = p.nd_part + pad4(p.ndiv_blocks);
  p.d_packed = p.g_packed + pack_offsets(g_mlp(c->noise_dim)).total;
  p.d_seg = p.d_packed + pack_offsets(d_mlp()).total;   // fc1 operand: fake segment sums + the real rows' dY1 (k_phase_a)
  p.g_seg = p.d_seg + (p.seg_entries + p.rpad) * 64;
  p.floats = p.g_seg + p.seg_entries * 128;
  p.d_front_grid = (unsigned)(first ? p.mpad / 16 + p.rpad / 16 : p.mpad / 16);
  p.phase_a = first ? phase_variant(kPhaseA, p.d_front_grid, K) : -1;
  p.phase_b_grid = (unsigned)(p.mpad / 16);
  p.phase_b = phase_variant(kPhaseB, p.phase_b_grid, K);
  p.wgrad_d_grid = wgrad_grid(job_count(d_mlp(), p.dw.plan.wide), p.dw.plan, p.ndiv_fused ? p.ndiv_blocks : 0);
  p.wgrad_g_grid = wgrad_grid(job_count(g_mlp(c->noise_dim), p.gw.plan.wide), p.gw.plan, 0);
  p.reduce_d_grid = reduce_grid(layout(d_mlp()).total);
  p.reduce_g_grid = reduce_grid(layout(g_mlp(c->noise_dim)).total);
  p.loss_count_d = p.d_front_grid; p.loss_count_g = p.mpad / 16;
  return p;
}

// a network's buffers of a step: which 0 = D, 1 = G
struct NetBuffers { float *params, *grad, *exp_avg, *exp_avg_sq; int32_t* step; };
static NetBuffers net_buffers(const ndp_step_buffers* b, int which) {
  if (which == 1) return NetBuffers{b->g_params, b->g_grad, b->g_exp_avg, b->g_exp_avg_sq, b->g_step};
  return NetBuffers{b->d_params, b->d_grad, b->d_exp_avg, b->d_exp_avg_sq, b->d_step};
}
// the step's reduce of network `which`: its gradient, with fuse_adam its update, the exchange between ranks
static int fill_step_reduce(const char* fn, ReduceArgs& r, const ndp_step_config* c, const ndp_step_buffers* b, const StepPlan& p,
                            int which, const WgradArgs& w) {
  const NetBuffers nb = net_buffers(b, which);
  const Mlp net = which ? g_mlp(c->noise_dim) : d_mlp();
  const FusedAdam adam = {nb.params, nb.exp_avg, nb.exp_avg_sq, c->lr, c->beta1, c->beta2, c->eps,
                          pack_spec(net, b->workspace + (which ? p.g_packed : p.d_packed))};
  int rc = fill_reduce(fn, r, b->workspace + (which ? p.gw.slabs : p.dw.slabs), which ? p.gw.slab_stride : p.dw.slab_stride,
                       layout(net).total, which ? p.gw.plan : p.dw.plan, &w, nb.grad, nb.step, c->fuse_adam ? &adam : nullptr,
                       c->p2p, which);
  r.losses = b->losses; r.loss_sums = b->loss_sums;
  return rc;
}

static int check_step(const char* fn, const ndp_step_config* c, const ndp_step_buffers* b, const float* codes,
                      const float* actions, const float* noise) {
  NDP_CHECK_STEP_CONFIG(fn, c);
  NDP_CHECK_ARG(b && codes && actions && noise, "%s: null pointer", fn);
  NDP_CHECK_ARG(b->g_params && b->d_params && b->losses && b->action_hat && b->workspace && b->g_step && b->d_step,
                "%s: null buffer", fn);
  NDP_CHECK_ARG(c->fuse_adam ? (b->g_exp_avg && b->g_exp_avg_sq && b->d_exp_avg && b->d_exp_avg_sq)
                             : (b->g_grad && b->d_grad), "%s: missing Adam state / gradient buffers", fn);
  NDP_CHECK_ARG(aligned16(b->g_params) && aligned16(b->d_params) && aligned16(b->workspace) && aligned16(b->action_hat) &&
                aligned16(codes) && aligned16(actions), "%s: buffers must be 16-byte aligned", fn);
  return NDP_OK;
}

// ---------------------------------------------------------------- peer-to-peer exchange
static int fill_p2p(const char* fn, P2PArgs& x, const ndp_p2p* c, int net, int64_t n) {
  memset(&x, 0, sizeof(x));
  if (c == nullptr || c->world <= 1) return NDP_OK;
  NDP_CHECK_ARG(c->world <= NDP_P2P_MAX_RANKS && c->rank >= 0 && c->rank < c->world, "%s: p2p world=%d rank=%d", fn, c->world, c->rank);
  NDP_CHECK_ARG(n <= (net == 0 ? kP2PCapD : kP2PCapG), "%s: %lld values exceed the p2p inbox of net %d", fn, (long long)n, net);
  for (int r = 0; r < c->world; ++r) NDP_CHECK_ARG(c->region[r] != nullptr, "%s: p2p region of rank %d is null", fn, r);
  x.world = c->world; x.rank = c->rank; x.net = net;
  x.timeout_ticks = 100000ll * (c->timeout_ms > 0 ? c->timeout_ms : 10000);   // wall_clock64: 100 MHz
  for (int r = 0; r < c->world; ++r) x.region[r] = static_cast<uint32_t*>(c->region[r]);
  return NDP_OK;
}

}  // namespace ndp

// ================================================================== C ABI
using namespace ndp;

extern "C" {

int ndp_version(void) { return NDP_VERSION; }
const char* ndp_last_error(void) { return g_err; }
int64_t ndp_g_param_count(int noise_dim) { return layout(g_mlp(noise_dim)).total; }
int64_t ndp_d_param_count(void) { return layout(d_mlp()).total; }
int64_t ndp_pad_rows(int64_t rows) { return pad_rows(rows); }

int64_t ndp_ndiv_partials(int64_t n, int k) {
  if (k < 1 || k > NDP_MAX_SAMPLES || n < 0) return 0;
  const int G = ndiv_rows_per_block(k, ndiv_block_threads(k));
  return (n + G - 1) / G + 1;
}

int ndp_ndiv_fwd_bwd(const float* x, int cx, const float* z, int cz, int64_t n, int k, float grad_scale,
                     float* loss_out, float* grad_x, float* partials, void* stream) {
  NDP_CHECK_ARG(x && z && loss_out && partials, "ndp_ndiv_fwd_bwd: null pointer");
  NDP_CHECK_ARG(k >= 1 && k <= NDP_MAX_SAMPLES, "ndp_ndiv_fwd_bwd: k=%d outside 1..%d", k, NDP_MAX_SAMPLES);
  NDP_CHECK_ARG(cx >= 1 && cx <= kNdivMaxC && cz >= 1 && cz <= kNdivMaxC, "ndp_ndiv_fwd_bwd: channel count outside 1..16");
  NDP_CHECK_ARG(n >= 1 && n * k < (1ll << 31), "ndp_ndiv_fwd_bwd: bad row count %lld", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_ndiv(x, cx, z, cz, n, k, grad_scale, grad_x, partials, st);
  if (rc) return rc;
  const int G = ndiv_rows_per_block(k, ndiv_block_threads(k));
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kThreads), 0, st, (const float*)partials,
                     (int)((n + G - 1) / G), 1.0f, loss_out);
  return check_launch("k_sum_partials");
}

int64_t ndp_g_acts_floats(int64_t m) { return g_acts(0, pad_rows(m)).end; }

static int check_g_common(const char* fn, const float* g_params, int noise_dim, const float* code,
                          int64_t ld_code, int code_rep, const float* noise, int64_t ld_noise, int64_t m) {
  NDP_CHECK_ARG(g_params && code && noise, "%s: null pointer", fn);
  NDP_CHECK_ARG(aligned16(g_params), "%s: g_params must be 16-byte aligned", fn);
  NDP_CHECK_ARG(noise_dim >= 1 && noise_dim <= NDP_MAX_NOISE_DIM, "%s: noise_dim=%d outside 1..%d", fn, noise_dim, NDP_MAX_NOISE_DIM);
  NDP_CHECK_ARG(m >= 1 && m < (1ll << 30), "%s: bad row count %lld", fn, (long long)m);
  NDP_CHECK_ARG(code_rep >= 1 && ld_code >= NDP_CODE_DIM && ld_noise >= noise_dim, "%s: bad strides", fn);
  return NDP_OK;
}

int ndp_g_forward(const float* g_params, int noise_dim, const float* code, int64_t ld_code, int code_rep,
                  const float* noise, int64_t ld_noise, int64_t m, float* acts, float* action_hat, void* stream) {
  int rc = check_g_common("ndp_g_forward", g_params, noise_dim, code, ld_code, code_rep, noise, ld_noise, m);
  if (rc) return rc;
  NDP_CHECK_ARG(action_hat && aligned16(action_hat), "ndp_g_forward: action_hat null or not 16-byte aligned");
  NDP_CHECK_ARG(!acts || aligned16(acts), "ndp_g_forward: acts not 16-byte aligned");
  return launch_g_fwd(g_net(g_params, noise_dim), code, ld_code, code_rep, noise, ld_noise, m, acts, action_hat,
                      (hipStream_t)stream);
}

int64_t ndp_g_bwd_ws_floats(int64_t m, int noise_dim) { return g_bwd_ws(0, pad_rows(m), noise_dim).end; }

// G's weight-gradient launch from dy1..dy5 in ws (gw) and the saved activations; w: its jobs, for the reduce
static int g_wgrad(int nz, const float* code, int64_t ld_code, int code_rep, const float* noise, int64_t ld_noise,
                          int64_t m, const float* acts, const GActs& a, float* ws, const GBwdWs& gw, WgradArgs& w,
                          int32_t* bump, const AdamHyper& hp, const float* dy1seg, hipStream_t st) {
  build_g_jobs(w, nz, ws, gw, acts, a, code, ld_code, code_rep, noise, ld_noise, m, dy1seg);
  return launch_wgrad(w, pad_rows(m), gw.plan, ws + gw.slabs, gw.slab_stride, bump, hp, nullptr, 0, st);
}

int ndp_g_backward(const float* g_params, int noise_dim, const float* code, int64_t ld_code, int code_rep,
                   const float* noise, int64_t ld_noise, int64_t m, const float* acts, const float* d_action,
                   float* grad, float* ws, void* stream) {
  int rc = check_g_common("ndp_g_backward", g_params, noise_dim, code, ld_code, code_rep, noise, ld_noise, m);
  if (rc) return rc;
  NDP_CHECK_ARG(acts && d_action && grad && ws, "ndp_g_backward: null pointer");
  NDP_CHECK_ARG(aligned16(acts) && aligned16(d_action) && aligned16(ws), "ndp_g_backward: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const GBwdWs gw = g_bwd_ws(0, pad_rows(m), noise_dim);
  rc = launch_g_bwd(g_net(g_params, noise_dim), m, acts, d_action, ws, gw, st);
  if (rc) return rc;
  WgradArgs w;
  rc = g_wgrad(noise_dim, code, ld_code, code_rep, noise, ld_noise, m, acts, g_acts(0, pad_rows(m)), ws, gw, w, nullptr,
                      AdamHyper{0.f, 0.f, 0.f}, nullptr, st);
  if (rc) return rc;
  ReduceArgs red;
  fill_reduce("ndp_g_backward", red, ws + gw.slabs, gw.slab_stride, layout(g_mlp(noise_dim)).total, gw.plan, &w, grad, nullptr,
              nullptr, nullptr, 1);
  return launch_reduce(red, st);
}

int ndp_g_input_grad(const float* g_params, int noise_dim, const float* z, int64_t ld_z, int64_t m, const float* acts,
                     const float* d_action, float* d_z, int64_t ld_dz, float* ws, void* stream) {
  int rc = check_g_common("ndp_g_input_grad", g_params, noise_dim, z, ld_z, 1, z, ld_z, m);
  if (rc) return rc;
  NDP_CHECK_ARG(ld_z >= NDP_CODE_DIM + noise_dim && ld_dz >= NDP_CODE_DIM + noise_dim, "ndp_g_input_grad: bad strides");
  NDP_CHECK_ARG(d_z && ws && aligned16(ws), "ndp_g_input_grad: d_z / ws null or ws not 16-byte aligned");
  NDP_CHECK_ARG(!d_action || (acts && aligned16(acts) && aligned16(d_action)),
                "ndp_g_input_grad: d_action needs the 16-byte aligned activations of ndp_g_forward");
  hipStream_t st = (hipStream_t)stream;
  const int64_t mpad = pad_rows(m);
  const GNet net = g_net(g_params, noise_dim);
  const GBwdWs w = g_bwd_ws(0, mpad, noise_dim);
  if (d_action != nullptr) {          // null: dy1 is what the ndp_g_backward call just before left in ws
    rc = launch_g_bwd(net, m, acts, d_action, ws, w, st);
    if (rc) return rc;
  }
  GInGradArgs g;
  g.w1 = net.w1; g.ld1 = net.ld1; g.nz = noise_dim;
  g.dy1 = ws + w.dy[0]; g.d_z = d_z; g.ld_dz = ld_dz; g.m = m;
  KTimer kt("k_g_in_dgrad", st);
  hipLaunchKernelGGL(k_g_in_dgrad, dim3((unsigned)(mpad / 16)), dim3(kThreads), 0, st, g);
  return check_launch("k_g_in_dgrad");
}

static int check_d_common(const char* fn, const float* d_params, const float* action, int action_rep,
                          const float* code, int64_t ld_code, int code_rep, int64_t m) {
  NDP_CHECK_ARG(d_params && action && code, "%s: null pointer", fn);
  NDP_CHECK_ARG(aligned16(d_params), "%s: d_params must be 16-byte aligned", fn);
  NDP_CHECK_ARG(m >= 1 && m < (1ll << 29), "%s: bad row count %lld", fn, (long long)m);
  NDP_CHECK_ARG(action_rep >= 1 && code_rep >= 1 && ld_code >= NDP_CODE_DIM, "%s: bad strides", fn);
  return NDP_OK;
}

static void d_args_init(DArgs& a, const float* d_params, const float* code, int64_t ld_code, int code_rep, int64_t m) {
  memset(&a, 0, sizeof(a));
  a.net = d_net(d_params);
  a.code = code; a.ld_code = ld_code; a.code_rep = code_rep;
  a.code_vec4 = (ld_code % 4 == 0) && aligned16(code);
  a.m = m; a.mpad = pad_rows(m);
  a.inv_m = 1.f / (float)m;
}

int ndp_d_forward(const float* d_params, const float* action, int action_rep, const float* code, int64_t ld_code,
                  int code_rep, int64_t m, float* logits, void* stream) {
  int rc = check_d_common("ndp_d_forward", d_params, action, action_rep, code, ld_code, code_rep, m);
  if (rc) return rc;
  NDP_CHECK_ARG(logits, "ndp_d_forward: null logits");
  DArgs a;
  d_args_init(a, d_params, code, ld_code, code_rep, m);
  a.pass[0].action = action; a.pass[0].action_rep = action_rep; a.pass[0].target = 0.f;
  a.logits = logits;
  return launch_d(a, 1, (hipStream_t)stream);
}

int64_t ndp_d_bwd_ws_floats(int64_t m) { return d_bwd_ws(0, pad_rows(m)).end; }

static int d_backward_impl(const char* fn, const float* d_params, const float* action, int action_rep, const float* code,
                           int64_t ld_code, int code_rep, int64_t m, const float* d_logits, float* grad, float* d_action,
                           float* d_code, int64_t ld_dcode, float* ws, void* stream) {
  int rc = check_d_common(fn, d_params, action, action_rep, code, ld_code, code_rep, m);
  if (rc) return rc;
  NDP_CHECK_ARG(d_logits, "%s: null d_logits", fn);
  NDP_CHECK_ARG(!grad || (ws && aligned16(ws)), "%s: grad needs a 16-byte aligned workspace", fn);
  NDP_CHECK_ARG(!d_action || action_rep == 1, "%s: d_action needs action_rep == 1", fn);
  NDP_CHECK_ARG(!d_code || (code_rep == 1 && ld_dcode >= NDP_CODE_DIM), "%s: d_code needs code_rep == 1 and ld_dcode >= 256", fn);
  hipStream_t st = (hipStream_t)stream;
  DArgs a;
  d_args_init(a, d_params, code, ld_code, code_rep, m);
  a.pass[0].action = action; a.pass[0].action_rep = action_rep; a.pass[0].target = 0.f;
  a.ext_dlogit = d_logits;
  a.do_backward = 1;
  a.d_action = d_action;
  a.d_code = d_code; a.ld_dcode = ld_dcode;
  const DBwdWs w = d_bwd_ws(0, a.mpad);
  if (grad) hand_d_bwd(a, ws, w);
  rc = launch_d(a, 1, st);
  if (rc || !grad) return rc;
  WgradArgs wa;
  build_d_jobs(wa, ws, w, code, ld_code, code_rep, m, a.mpad, nullptr, 0);
  rc = launch_wgrad(wa, a.mpad, w.plan, ws + w.slabs, w.slab_stride, nullptr, AdamHyper{0.f, 0.f, 0.f}, nullptr, 0, st);
  if (rc) return rc;
  ReduceArgs red;
  fill_reduce(fn, red, ws + w.slabs, w.slab_stride, layout(d_mlp()).total, w.plan, &wa, grad, nullptr, nullptr, nullptr, 0);
  return launch_reduce(red, st);
}

int ndp_d_backward(const float* d_params, const float* action, int action_rep, const float* code, int64_t ld_code,
                   int code_rep, int64_t m, const float* d_logits, float* grad, float* d_action, float* ws,
                   void* stream) {
  return d_backward_impl("ndp_d_backward", d_params, action, action_rep, code, ld_code, code_rep, m, d_logits, grad, d_action,
                         nullptr, 0, ws, stream);
}

int ndp_d_input_grad(const float* d_params, const float* action, int action_rep, const float* code, int64_t ld_code,
                     int code_rep, int64_t m, const float* d_logits, float* grad, float* d_action, float* d_code,
                     int64_t ld_dcode, float* ws, void* stream) {
  NDP_CHECK_ARG(d_code, "ndp_d_input_grad: null d_code (ndp_d_backward is the call without it)");
  return d_backward_impl("ndp_d_input_grad", d_params, action, action_rep, code, ld_code, code_rep, m, d_logits, grad, d_action,
                         d_code, ld_dcode, ws, stream);
}

int ndp_adam_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  int32_t* step_count, float lr, float beta1, float beta2, float eps, void* stream) {
  NDP_CHECK_ARG(params && grad && exp_avg && exp_avg_sq && step_count, "ndp_adam_step: null pointer");
  NDP_CHECK_ARG(n >= 1, "ndp_adam_step: n < 1");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(1), 0, st, step_count, lr, beta1, beta2);
  AdamArgs a;
  a.params = params; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.grad = grad; a.n = n;
  a.step = step_count; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  memset(&a.pack, 0, sizeof(a.pack));
  return launch_adam(a, st);
}

#define NDP_HIP(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
  return ndp::fail(NDP_E_LAUNCH, "%s: %s", what, hipGetErrorString(e_)); } while (0)

int64_t ndp_p2p_region_bytes(void) { return kP2PWords * 4; }

int ndp_p2p_region_alloc(void** region) {
  NDP_CHECK_ARG(region != nullptr, "ndp_p2p_region_alloc: null pointer");
  static_assert(sizeof(hipIpcMemHandle_t) == NDP_P2P_HANDLE_BYTES, "handle size");
  void* p = nullptr;
  NDP_HIP(hipExtMallocWithFlags(&p, (size_t)kP2PWords * 4, hipDeviceMallocUncached), "ndp_p2p_region_alloc");
  hipError_t e = hipMemset(p, 0, (size_t)kP2PWords * 4);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { hipFree(p); return ndp::fail(NDP_E_LAUNCH, "ndp_p2p_region_alloc: %s", hipGetErrorString(e)); }
  *region = p;
  return NDP_OK;
}

int ndp_p2p_region_free(void* region) {
  if (region == nullptr) return NDP_OK;
  NDP_HIP(hipFree(region), "ndp_p2p_region_free");
  return NDP_OK;
}

int ndp_p2p_region_reset(void* region) {
  NDP_CHECK_ARG(region != nullptr, "ndp_p2p_region_reset: null pointer");
  NDP_HIP(hipDeviceSynchronize(), "ndp_p2p_region_reset");
  NDP_HIP(hipMemset(region, 0, (size_t)kP2PInboxD * 4), "ndp_p2p_region_reset");
  NDP_HIP(hipDeviceSynchronize(), "ndp_p2p_region_reset");
  return NDP_OK;
}

int ndp_p2p_export(void* region, void* handle_out) {
  NDP_CHECK_ARG(region && handle_out, "ndp_p2p_export: null pointer");
  hipIpcMemHandle_t h;
  NDP_HIP(hipIpcGetMemHandle(&h, region), "ndp_p2p_export");
  memcpy(handle_out, &h, sizeof(h));
  return NDP_OK;
}

int ndp_p2p_open(const void* handle, void** mapped_out) {
  NDP_CHECK_ARG(handle && mapped_out, "ndp_p2p_open: null pointer");
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof(h));
  void* p = nullptr;
  NDP_HIP(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess), "ndp_p2p_open");
  *mapped_out = p;
  return NDP_OK;
}

int ndp_p2p_close(void* mapped) {
  if (mapped == nullptr) return NDP_OK;
  NDP_HIP(hipIpcCloseMemHandle(mapped), "ndp_p2p_close");
  return NDP_OK;
}

int ndp_p2p_status(const ndp_p2p* c, int32_t* status_out) {
  NDP_CHECK_ARG(c && status_out && c->rank >= 0 && c->rank < NDP_P2P_MAX_RANKS && c->region[c->rank], "ndp_p2p_status: bad arguments");
  NDP_HIP(hipMemcpy(status_out, c->region[c->rank], 4, hipMemcpyDeviceToHost), "ndp_p2p_status");
  return NDP_OK;
}

int ndp_p2p_diagnostics(const ndp_p2p* c, int32_t* words_out) {
  NDP_CHECK_ARG(c && words_out && c->rank >= 0 && c->rank < NDP_P2P_MAX_RANKS && c->region[c->rank], "ndp_p2p_diagnostics: bad arguments");
  NDP_HIP(hipMemcpy(words_out, c->region[c->rank], 4 * NDP_P2P_DIAG_WORDS, hipMemcpyDeviceToHost), "ndp_p2p_diagnostics");
  return NDP_OK;
}

int ndp_p2p_status_async(const ndp_p2p* c, int32_t* pinned_host_out, void* stream) {
  NDP_CHECK_ARG(c && pinned_host_out && c->rank >= 0 && c->rank < NDP_P2P_MAX_RANKS && c->region[c->rank], "ndp_p2p_status_async: bad arguments");
  NDP_HIP(hipMemcpyAsync(pinned_host_out, c->region[c->rank], 4, hipMemcpyDeviceToHost, (hipStream_t)stream), "ndp_p2p_status_async");
  return NDP_OK;
}

int ndp_device_pci_bus_id(char* out, int len) {
  NDP_CHECK_ARG(out && len >= 16, "ndp_device_pci_bus_id: need a buffer of >= 16 bytes");
  int dev = 0;
  NDP_HIP(hipGetDevice(&dev), "ndp_device_pci_bus_id");
  NDP_HIP(hipDeviceGetPCIBusId(out, len, dev), "ndp_device_pci_bus_id");
  return NDP_OK;
}

int ndp_p2p_all_reduce(const ndp_p2p* c, int net, const float* in, float* out, int64_t n, const int32_t* step_word,
                       void* stream) {
  NDP_CHECK_ARG(c && in && out && step_word && n >= 1 && (net == 0 || net == 1), "ndp_p2p_all_reduce: bad arguments");
  ReduceArgs red;
  int rc = fill_reduce("ndp_p2p_all_reduce", red, in, 0, n, NetPlan{1, 1, 0, 1}, nullptr, out, step_word, nullptr, c, net);
  if (rc) return rc;
  return launch_reduce(red, (hipStream_t)stream);
}

int64_t ndp_step_workspace_floats(const ndp_step_config* cfg) {
  return step_config_ok(cfg) ? step_plan(cfg, true).floats : 0;
}

int64_t ndp_step_workspace_offset(const ndp_step_config* cfg, int tensor) {
  if (!step_config_ok(cfg) || tensor < 0 || tensor >= NDP_STEP_TENSORS) return -1;
  // the order of NDP_STEP_TENSORS in ndp.h; D's h1..h3 in both layouts of its scratch: first / repeat D step
  const StepPlan p = step_plan(cfg, true), r = step_plan(cfg, false);
  const int64_t at[NDP_STEP_TENSORS] = {p.acts.h[0], p.acts.h[1], p.acts.h[2], p.acts.h[3], p.nd_grad, p.gw.dy[4],
                                        p.dw.h[0], p.dw.h[1], p.dw.h[2], r.dw.h[0], r.dw.h[1], r.dw.h[2]};
  return at[tensor];
}

int64_t ndp_step_wgrad_blocks(const ndp_step_config* cfg, int which, int first, int32_t* pairs, int64_t capacity,
                              int32_t* table, int64_t* slab_area) {
  if (!step_config_ok(cfg) || which < 0 || which > 1 || !pairs || !table || !slab_area || capacity < 0) return -1;
  const StepPlan p = step_plan(cfg, first != 0);
  // host arithmetic only: the operands are addresses that nothing here reads
  alignas(16) static float origin[4];
  float* ws = origin;
  const int K = cfg->num_sample, nz = cfg->noise_dim;
  WgradArgs w;
  if (which) build_g_jobs(w, nz, ws, p.gw, ws, p.acts, origin, CODE, K, origin, nz, p.m, ws + p.g_seg);
  else build_d_jobs(w, ws, p.dw, origin, CODE, K, p.m, p.mpad, first ? ws + p.d_seg : nullptr, p.rpad);
  const int64_t grid = which ? p.wgrad_g_grid : p.wgrad_d_grid;
  const int slots = w.nwide * w.wide_chunks + 8 * ((w.nchunks + 7) / 8) * w.njobs;   // as wgrad_body
  for (int j = 0; j < kMaxJobs; ++j) table[j] = j < w.njobs + w.nwide ? w.job[j].nchunks : 0;
  table[kMaxJobs] = w.njobs; table[kMaxJobs + 1] = w.nwide; table[kMaxJobs + 2] = w.wide_chunks; table[kMaxJobs + 3] = w.nchunks;
  slab_area[0] = which ? p.gw.slabs : p.dw.slabs;
  slab_area[1] = (which ? p.gw.plan.slabs : p.dw.plan.slabs) * (which ? p.gw.slab_stride : p.dw.slab_stride);
  for (int64_t b = 0; b < grid && b < capacity; ++b) {
    int job = -2, chunk = -2;
    if (b < slots) wgrad_slot(w.njobs, w.nwide, w.wide_chunks, (int)b, job, chunk);   // as wgrad_fetch_args
    pairs[2 * b] = job; pairs[2 * b + 1] = chunk;
  }
  return grid;
}

int ndp_step_d_grads(const ndp_step_config* c, const ndp_step_buffers* b, const float* codes, const float* actions,
                     float* noise, int run_g_forward, void* stream) {
  int rc = check_step("ndp_step_d_grads", c, b, codes, actions, noise);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int K = c->num_sample, nz = c->noise_dim;
  // first D step of an iteration: real pass on the distinct rows (k_phase_a); repeat D steps: two full passes (k_d)
  const StepPlan p = step_plan(c, run_g_forward != 0);
  float* ws = b->workspace;
  NdivArgs nd;
  if (p.ndiv_fused)   // NDiv loss + gradient (train_gan.py:193-199; gradient pre-scaled by pairwise_div_factor)
    nd = ndiv_args(b->action_hat, ADIM, noise, nz, c->flat, K, c->pairwise_div_factor, ws + p.nd_grad, ws + p.nd_part, kThreads);
  if (run_g_forward) {
    // G forward + D(real) + D(fake) + BCE + D's backward data path in one launch
    PhaseAArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.g = g_net(b->g_params, nz, ws + p.g_packed);
    pa.d = d_net(b->d_params, ws + p.d_packed);
    pa.code = codes; pa.code_rep = K;
    pa.noise = c->device_noise ? nullptr : noise;
    pa.noise_out = c->device_noise ? noise : nullptr; pa.noise_seed = c->noise_seed; pa.noise_step = b->g_step;
    pa.actions = actions;
    pa.m = p.m; pa.mpad = p.mpad; pa.flat = c->flat; pa.rpad = p.rpad;
    pa.inv_m = c->inv_m_global; pa.real_scale = (float)K;
    hand_g_acts_phase(pa, ws, p.acts);
    pa.action_hat = b->action_hat;
    hand_d_bwd(pa, ws, p.dw);
    pa.loss_partials = ws + p.dw.lossp;
    pa.dy1seg = ws + p.d_seg; pa.seg_s = p.seg_s; pa.seg_entries = (int)p.seg_entries;
    KTimer kt("k_phase_a", st);
    rc = launch_variant("k_phase_a", kPhaseA, p.phase_a, p.d_front_grid, kThreads, -1, st, pa);
    if (rc) return rc;
  } else {
    // repeat D step of a discrim_steps_per_gen > 1 iteration: action_hat is re-used (train_gan.py:172)
    DArgs a;
    d_args_init(a, b->d_params, codes, CODE, K, p.m);
    a.net = d_net(b->d_params, ws + p.d_packed);
    a.inv_m = c->inv_m_global;
    a.pass[0].action = actions; a.pass[0].action_rep = K; a.pass[0].target = 1.f;        // real (train_gan.py:174-177)
    a.pass[1].action = b->action_hat; a.pass[1].action_rep = 1; a.pass[1].target = 0.f;  // fake (178-181)
    a.do_backward = 1;
    hand_d_bwd(a, ws, p.dw);
    a.loss_partials = ws + p.dw.lossp;
    rc = launch_d(a, 2, st);
    if (rc) return rc;
  }
  WgradArgs wa;
  // the fused kernel also produced fc1's K-deduplicated operand (segment sums of the fake pass + the real rows' dY1)
  build_d_jobs(wa, ws, p.dw, codes, CODE, K, p.m, p.mpad, run_g_forward ? ws + p.d_seg : nullptr, p.rpad);
  // the Adam state word is advanced here in both modes: ndp_step_apply_adam (non-fused) finds it ready
  rc = launch_wgrad(wa, p.d_rows, p.dw.plan, ws + p.dw.slabs, p.dw.slab_stride, b->d_step, AdamHyper{c->lr, c->beta1, c->beta2},
                    p.ndiv_fused ? &nd : nullptr, p.ndiv_blocks, st);
  if (rc) return rc;
  ReduceArgs red;
  rc = fill_step_reduce("ndp_step_d_grads", red, c, b, p, 0, wa);
  if (rc) return rc;
  add_loss(red, ws + p.dw.lossp, p.loss_count_d, c->inv_m_global, 0);
  return launch_reduce(red, st);
}

int ndp_step_g_grads(const ndp_step_config* c, const ndp_step_buffers* b, const float* codes, const float* actions,
                     const float* noise, void* stream) {
  int rc = check_step("ndp_step_g_grads", c, b, codes, actions, noise);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int K = c->num_sample, nz = c->noise_dim;
  const StepPlan p = step_plan(c, true);   // of D's scratch only the loss-partial area is used here
  float* ws = b->workspace;
  if (!p.ndiv_fused) {
    // NDiv loss and gradient (train_gan.py:193-199), gradient pre-scaled by pairwise_div_factor
    rc = launch_ndiv(b->action_hat, ADIM, noise, nz, c->flat, K, c->pairwise_div_factor, ws + p.nd_grad, ws + p.nd_part, st);
    if (rc) return rc;
  }
  // G loss through the updated D (train_gan.py:187-190), dLoss/d action_hat (+ NDiv gradient),
  // G's backward data path: one launch
  PhaseBArgs pb;
  memset(&pb, 0, sizeof(pb));
  pb.g = g_net(b->g_params, nz, ws + p.g_packed);
  pb.d = d_net(b->d_params, ws + p.d_packed);
  pb.code = codes; pb.code_rep = K;
  pb.action_hat = b->action_hat; pb.nd_grad = ws + p.nd_grad;
  pb.m = p.m; pb.inv_m = c->inv_m_global;
  hand_g_acts_phase(pb, ws, p.acts);
  hand_g_bwd(pb, ws, p.gw);
  pb.loss_partials = ws + p.dw.lossp;
  pb.dy1seg = ws + p.g_seg; pb.seg_s = p.seg_s; pb.seg_entries = (int)p.seg_entries;
  {
    KTimer kt("k_phase_b", st);
    rc = launch_variant("k_phase_b", kPhaseB, p.phase_b, p.phase_b_grid, kThreads, -1, st, pb);
  }
  if (rc) return rc;
  WgradArgs w;     // dy1..dy5 were produced by the fused phase B kernel
  rc = g_wgrad(nz, codes, CODE, K, noise, nz, p.m, ws, p.acts, ws, p.gw, w, b->g_step, AdamHyper{c->lr, c->beta1, c->beta2},
                      ws + p.g_seg, st);
  if (rc) return rc;
  ReduceArgs red;
  rc = fill_step_reduce("ndp_step_g_grads", red, c, b, p, 1, w);
  if (rc) return rc;
  add_loss(red, ws + p.dw.lossp, p.loss_count_g, c->inv_m_global, 1);
  add_loss(red, ws + p.nd_part, p.ndiv_blocks, 1.f, 2);
  return launch_reduce(red, st);
}

#ifdef NDP_STAMPS
// diagnostic build only: where the stamps go (device buffer of 32 uint64 per workgroup)
int ndp_debug_set_stamps(void* dev_buffer, int kernel_id) {
  unsigned long long* p = (unsigned long long*)dev_buffer;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_kernel), &kernel_id, sizeof(int)) != hipSuccess) return NDP_E_LAUNCH;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &p, sizeof(p)) == hipSuccess ? 0 : NDP_E_LAUNCH;
}
#endif

int ndp_timing_enable(int on) {
  TimingState& t = g_timing;
  for (int i = 0; i < t.n; ++i) { hipEventDestroy(t.ev[i].t0); hipEventDestroy(t.ev[i].t1); }
  t.n = 0;
  t.on = on != 0;
  return NDP_OK;
}

int ndp_timing_collect(char* names, int names_len, float* total_ms, int32_t* counts, int max_kernels) {
  if (!(names && total_ms && counts && names_len > 0 && max_kernels > 0)) {
    fail(NDP_E_ARG, "ndp_timing_collect: bad arguments");
    return 0;
  }
  TimingState& t = g_timing;
  const char* seen[64];
  int nk = 0;
  names[0] = 0;
  for (int i = 0; i < t.n; ++i) {
    if (hipEventSynchronize(t.ev[i].t1) != hipSuccess) {
      fail(NDP_E_LAUNCH, "ndp_timing_collect: event sync failed");
      return 0;
    }
    float ms = 0.f;
    hipEventElapsedTime(&ms, t.ev[i].t0, t.ev[i].t1);
    int k = 0;
    while (k < nk && strcmp(seen[k], t.ev[i].name) != 0) ++k;
    if (k == nk) {
      if (nk >= max_kernels || nk >= 64) continue;
      seen[nk] = t.ev[i].name; total_ms[nk] = 0.f; counts[nk] = 0; ++nk;
      strncat(names, t.ev[i].name, names_len - strlen(names) - 2);
      strncat(names, ";", names_len - strlen(names) - 1);
    }
    total_ms[k] += ms;
    counts[k] += 1;
    hipEventDestroy(t.ev[i].t0);
    hipEventDestroy(t.ev[i].t1);
  }
  t.n = 0;
  return nk;
}

int ndp_step_pack_params(const ndp_step_config* c, const ndp_step_buffers* b, void* stream) {
  NDP_CHECK_STEP_CONFIG("ndp_step_pack_params", c);
  NDP_CHECK_ARG(b && b->g_params && b->d_params && b->workspace, "ndp_step_pack_params: null pointer");
  const StepPlan p = step_plan(c, true);
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_pack(b->g_params, g_mlp(c->noise_dim), b->workspace + p.g_packed, st);
  if (rc) return rc;
  return launch_pack(b->d_params, d_mlp(), b->workspace + p.d_packed, st);
}

int ndp_step_apply_adam(const ndp_step_config* c, const ndp_step_buffers* b, int which, void* stream) {
  NDP_CHECK_STEP_CONFIG("ndp_step_apply_adam", c);
  NDP_CHECK_ARG(b && b->workspace, "ndp_step_apply_adam: null pointer");
  NDP_CHECK_ARG(which == 0 || which == 1, "ndp_step_apply_adam: which must be 0 (D) or 1 (G)");
  const StepPlan p = step_plan(c, true);
  const NetBuffers nb = net_buffers(b, which);
  NDP_CHECK_ARG(nb.params && nb.grad && nb.exp_avg && nb.exp_avg_sq && nb.step, "ndp_step_apply_adam: null %s buffer", which ? "G" : "D");
  const Mlp net = which ? g_mlp(c->noise_dim) : d_mlp();
  AdamArgs a;
  a.params = nb.params; a.grad = nb.grad; a.exp_avg = nb.exp_avg; a.exp_avg_sq = nb.exp_avg_sq;
  a.n = layout(net).total; a.step = nb.step; a.pack = pack_spec(net, b->workspace + (which ? p.g_packed : p.d_packed));
  a.lr = c->lr; a.beta1 = c->beta1; a.beta2 = c->beta2; a.eps = c->eps;
  // the state word (step count, bias corrections) was advanced by the phase's k_wgrad launch
  return launch_adam(a, (hipStream_t)stream);
}

int ndp_uniform_noise(float* out, int64_t n, uint64_t seed, const int32_t* offset_dev, void* stream) {
  NDP_CHECK_ARG(out && n >= 1, "ndp_uniform_noise: bad arguments");
  hipLaunchKernelGGL(k_philox, dim3(blocks_of(n)), dim3(kThreads), 0, (hipStream_t)stream, out, n, seed, offset_dev);
  return check_launch("k_philox");
}

}  // extern "C"
