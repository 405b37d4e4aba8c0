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

template <typename K>
static void allow_lds(K kernel, int bytes) {
  // dynamic LDS above 64 KiB must be opted into once per kernel
  hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// hipFuncSetAttribute applies to the CURRENT device's copy of the code object: one flag per device (a module on
// cuda:1 must not find the opt-in done "already" by cuda:0)
constexpr int kMaxDevices = 64;
static std::once_flag g_attr_once[kMaxDevices];
static std::once_flag& device_once(std::once_flag (&flags)[kMaxDevices]) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
  return flags[dev];
}
static_assert(phase_a_lds_floats() * 4 * 3 <= 160 * 1024, "phase A: three workgroups per CU at large M");

static void set_attrs() {
  std::call_once(device_once(g_attr_once), [] {
#define NDP_ATTR_GFWD(WA) \
    allow_lds(k_g_fwd<WA, false>, g_fwd_lds_floats() * 4); \
    allow_lds(k_g_fwd<WA, true>, g_fwd_lds_floats() * 4);
    NDP_ATTR_GFWD(1) NDP_ATTR_GFWD(2) NDP_ATTR_GFWD(4)
#undef NDP_ATTR_GFWD
#define NDP_ATTR_D(NP) \
    allow_lds(k_d<NP, false>, (d_lds_floats<NP>() * 4)); \
    allow_lds(k_d<NP, true>, (d_lds_floats<NP>() * 4));
    NDP_ATTR_D(1) NDP_ATTR_D(2)
#undef NDP_ATTR_D
    allow_lds(k_g_bwd<false>, g_bwd_lds_floats() * 4);
    allow_lds(k_g_bwd<true>, g_bwd_lds_floats() * 4);
    allow_lds(k_wgrad, wgrad_lds_floats() * 4);
    allow_lds(k_wgrad_wide, wgrad_wide_launch_lds_floats() * 4);
#define NDP_ALLOW_A(RG, NR) allow_lds((k_phase_a<true, RG, NR>), phase_a_lds_floats() * 4)
#define NDP_ALLOW_B(RG, PRE, NR) allow_lds((k_phase_b<true, RG, PRE, NR>), phase_b_lds_floats(PRE) * 4)
    NDP_ALLOW_A(96, 0);
    NDP_ALLOW_A(kPhaseASmallRing, 0); NDP_ALLOW_A(kPhaseASmallRing, 1); NDP_ALLOW_A(kPhaseASmallRing, 4);
    NDP_ALLOW_B(96, true, 0);
    NDP_ALLOW_B(32, false, 0); NDP_ALLOW_B(32, false, 1); NDP_ALLOW_B(32, false, 4);
#undef NDP_ALLOW_A
#undef NDP_ALLOW_B
    allow_lds(k_ndiv<4, 2>, 64 * 1024);
    allow_lds(k_ndiv<16, 16>, 64 * 1024);
  });
}

// ---------------------------------------------------------------- parameter layouts
struct GLayout { int64_t w1, b1, w2, b2, w3, b3, w4, b4, w5, b5, total; int in1; };
static GLayout g_layout(int nz) {
  GLayout L;
  L.in1 = CODE + nz;
  int64_t o = 0;
  L.w1 = o; o += 128 * (int64_t)L.in1;
  L.b1 = o; o += 128;
  L.w2 = o; o += 64 * 128;
  L.b2 = o; o += 64;
  L.w3 = o; o += 128 * 64;
  L.b3 = o; o += 128;
  L.w4 = o; o += 256 * 128;
  L.b4 = o; o += 256;
  L.w5 = o; o += 4 * 256;
  L.b5 = o; o += 4;
  L.total = o;
  return L;
}
struct DLayout { int64_t w1, b1, w2, b2, w3, b3, w4, b4, total; };
static DLayout d_layout() {
  DLayout L;
  int64_t o = 0;
  L.w1 = o; o += 64 * 260;
  L.b1 = o; o += 64;
  L.w2 = o; o += 128 * 64;
  L.b2 = o; o += 128;
  L.w3 = o; o += 256 * 128;
  L.b3 = o; o += 256;
  L.w4 = o; o += 256;
  L.b4 = o; o += 1;
  L.total = o;
  return L;
}
// packed-copy layout (floats): G: fwd fc1 | fc2 | fc3 | fc4 | dgrad fc2 | fc3 | fc4;  D: fwd fc1 | fc2 | fc3 | dgrad fc2 | fc3
constexpr int kGPackF1 = 0, kGPackF2 = 32768, kGPackF3 = 40960, kGPackF4 = 49152,
              kGPackG2 = 81920, kGPackG3 = 90112, kGPackG4 = 98304, kGPackFloats = 131072;
constexpr int kDPackF1 = 0, kDPackF2 = 16384, kDPackF3 = 24576, kDPackG2 = 57344, kDPackG3 = 65536,
              kDPackFloats = 98304;

static GNet g_net(const float* p, int nz, const float* packed = nullptr) {
  const GLayout L = g_layout(nz);
  GNet n;
  n.w1 = p + L.w1; n.b1 = p + L.b1; n.w2 = p + L.w2; n.b2 = p + L.b2; n.w3 = p + L.w3; n.b3 = p + L.b3;
  n.w4 = p + L.w4; n.b4 = p + L.b4; n.w5 = p + L.w5; n.b5 = p + L.b5;
  n.ld1 = L.in1; n.nz = nz;
  n.pf1 = n.pf2 = n.pf3 = n.pf4 = n.pg2 = n.pg3 = n.pg4 = nullptr;
  if (packed) {
    n.pf1 = packed + kGPackF1; n.pf2 = packed + kGPackF2; n.pf3 = packed + kGPackF3; n.pf4 = packed + kGPackF4;
    n.pg2 = packed + kGPackG2; n.pg3 = packed + kGPackG3; n.pg4 = packed + kGPackG4;
  }
  return n;
}
static DNet d_net(const float* p, const float* packed = nullptr) {
  const DLayout L = d_layout();
  DNet n;
  n.w1 = p + L.w1; n.b1 = p + L.b1; n.w2 = p + L.w2; n.b2 = p + L.b2; n.w3 = p + L.w3; n.b3 = p + L.b3;
  n.w4 = p + L.w4; n.b4 = p + L.b4;
  n.pf1 = n.pf2 = n.pf3 = n.pg2 = n.pg3 = nullptr;
  if (packed) {
    n.pf1 = packed + kDPackF1; n.pf2 = packed + kDPackF2; n.pf3 = packed + kDPackF3;
    n.pg2 = packed + kDPackG2; n.pg3 = packed + kDPackG3;
  }
  return n;
}
static PackLayer pack_layer(int64_t w_off, int ld, int out, int main0, int main_in, int fwd_off, int dg_off) {
  PackLayer l;
  l.w_off = (int)w_off; l.ld = ld; l.out = out; l.main0 = main0; l.main_in = main_in; l.fwd_off = fwd_off; l.dg_off = dg_off;
  return l;
}
static PackSpec g_pack_spec(int nz, float* packed) {
  const GLayout L = g_layout(nz);
  PackSpec ps;
  memset(&ps, 0, sizeof(ps));
  ps.L[0] = pack_layer(L.w1, L.in1, 128, 0, CODE, kGPackF1, -1);
  ps.L[1] = pack_layer(L.w2, 128, 64, 0, 128, kGPackF2, kGPackG2);
  ps.L[2] = pack_layer(L.w3, 64, 128, 0, 64, kGPackF3, kGPackG3);
  ps.L[3] = pack_layer(L.w4, 128, 256, 0, 128, kGPackF4, kGPackG4);
  ps.nl = 4; ps.packed = packed;
  return ps;
}
static PackSpec d_pack_spec(float* packed) {
  const DLayout L = d_layout();
  PackSpec ps;
  memset(&ps, 0, sizeof(ps));
  ps.L[0] = pack_layer(L.w1, 260, 64, ADIM, CODE, kDPackF1, -1);
  ps.L[1] = pack_layer(L.w2, 64, 128, 0, 64, kDPackF2, kDPackG2);
  ps.L[2] = pack_layer(L.w3, 128, 256, 0, 128, kDPackF3, kDPackG3);
  ps.nl = 3; ps.packed = packed;
  return ps;
}
static int launch_pack(const float* params, int64_t n, const PackSpec& ps, hipStream_t st) {
  KTimer kt("k_pack", st);
  PackArgs a;
  a.params = params; a.n = (int)n; a.ps = ps;
  hipLaunchKernelGGL(k_pack, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
  return check_launch("k_pack");
}
static inline int64_t pad4(int64_t n) { return (n + 3) / 4 * 4; }

// ---------------------------------------------------------------- workspaces
// G activations saved by the forward: h1 | h2 | h3 | h4, each [mpad x width]
struct GActs { float *h1, *h2, *h3, *h4; };
static int64_t g_acts_floats(int64_t mpad) { return mpad * (128 + 64 + 128 + 256); }
static GActs g_acts(float* base, int64_t mpad) {
  GActs a;
  a.h1 = base; a.h2 = a.h1 + mpad * 128; a.h3 = a.h2 + mpad * 64; a.h4 = a.h3 + mpad * 128;
  return a;
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
constexpr int kGJobs = 26, kDJobs = 19;
// Chunk counts of a launch: `heavy` for the jobs that run a full 64 x 64 block over every row (fc2..fc4 of G,
// fc2 / fc3 of D), `light` for the K-deduplicated fc1 blocks and the 1..4-wide operands, which finish in half the
// time (stamps): at small M giving the heavy jobs more, shorter chunks and the light ones fewer keeps the launch
// within one resident round (<= 512 workgroups) and shortens its critical path.  heavy >= light; heavy is the slab
// count.  From 16,384 rows, or where the heavy count would leave a chunk fewer than 64 rows, both are wgrad_chunks.
static void wgrad_plan(bool is_g, int64_t rows, int* heavy, int* light) {
  // measured: G 24 at config 2; D (whose real pass is deduplicated: FLAT + M rows) 8 up to 4,096 rows -- 152 workgroups
  // and 8 slabs, 79.0 vs 80.3 us per step at B = 64, 75.2 vs 76.8 at B = 32 -- and 32 above (B = 128, 192)
  // (G's light jobs: 12 chunks, 12,788 vs 12,742 steps/s with 8 at config 2, three alternating runs each)
  const int h = is_g ? 24 : (rows <= 4096 ? 8 : 32), l = is_g ? 12 : 8;
  if (rows >= 16384 || rows / 64 < h) { *heavy = *light = wgrad_chunks(is_g ? kGJobs : kDJobs, rows); return; }
  *heavy = h; *light = l;
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
// slabs a launch may write: the 64 x 64 jobs' chunk count or the WIDE job's, whichever is larger
static int wgrad_slabs(bool is_g, int64_t rows) {
  int h, l;
  wgrad_plan(is_g, rows, &h, &l);
  const int w = wgrad_wide_chunks(rows);
  return h > w ? h : w;
}
// G backward scratch: dy1 | dy2 | dy3 | dy4 | dy5 | slabs
struct GBwdWs { float *dy1, *dy2, *dy3, *dy4, *dy5, *slabs; int nchunks, light; int64_t slab_stride; };
static int64_t g_bwd_floats(int64_t mpad, int nz) {
  return mpad * (128 + 64 + 128 + 256 + 4) + (int64_t)wgrad_slabs(true, mpad) * pad4(g_layout(nz).total);
}
static GBwdWs g_bwd_ws(float* base, int64_t mpad, int nz) {
  GBwdWs w;
  w.dy1 = base; w.dy2 = w.dy1 + mpad * 128; w.dy3 = w.dy2 + mpad * 64; w.dy4 = w.dy3 + mpad * 128;
  w.dy5 = w.dy4 + mpad * 256; w.slabs = w.dy5 + mpad * 4;
  wgrad_plan(true, mpad, &w.nchunks, &w.light);
  w.slab_stride = pad4(g_layout(nz).total);
  return w;
}
// D backward scratch for npass passes: xa | h1 | h2 | h3 | dy1 | dy2 | dy3 | dl | slabs | loss partials
struct DBwdWs { float *xa, *h1, *h2, *h3, *dy1, *dy2, *dy3, *dl, *slabs, *lossp; int nchunks, light; int64_t slab_stride; };
static int64_t d_bwd_floats_rows(int64_t rows) {
  return rows * (4 + 2 * (64 + 128 + 256) + 1) + (int64_t)wgrad_slabs(false, rows) * pad4(d_layout().total) +
         pad4(rows / 16);
}
static int64_t d_bwd_floats(int64_t mpad, int npass) { return d_bwd_floats_rows(mpad * npass); }
// rows: all rows the weight-gradient jobs run over (the passes back to back)
static DBwdWs d_bwd_ws_rows(float* base, int64_t rows) {
  DBwdWs w;
  w.xa = base; w.h1 = w.xa + rows * 4; w.h2 = w.h1 + rows * 64; w.h3 = w.h2 + rows * 128;
  w.dy1 = w.h3 + rows * 256; w.dy2 = w.dy1 + rows * 64; w.dy3 = w.dy2 + rows * 128; w.dl = w.dy3 + rows * 256;
  w.slabs = w.dl + rows;
  wgrad_plan(false, rows, &w.nchunks, &w.light);
  w.slab_stride = pad4(d_layout().total);
  w.lossp = w.slabs + (int64_t)wgrad_slabs(false, rows) * w.slab_stride;
  return w;
}
static DBwdWs d_bwd_ws(float* base, int64_t mpad, int npass) { return d_bwd_ws_rows(base, mpad * npass); }
// The fused step's D pass: the distinct real rows (FLAT of them, see k_phase_a) in front of the M fake rows.
static int64_t step_real_pad(const ndp_step_config* c) { return pad_rows(c->flat); }
static int64_t step_d_rows(const ndp_step_config* c) { return step_real_pad(c) + pad_rows(c->flat * c->num_sample); }

// ---------------------------------------------------------------- launch helpers
struct NoiseGen { float* out; uint64_t seed; const int32_t* step; };

static int launch_g_fwd(const GNet& net, const float* code, int64_t ld_code, int code_rep,
                        const float* noise, int64_t ld_noise, int64_t m, const GActs* acts,
                        float* action_hat, const NoiseGen* gen, hipStream_t st) {
  set_attrs();
  GFwdArgs a;
  a.net = net;
  a.code = code; a.ld_code = ld_code; a.code_rep = code_rep;
  a.code_vec4 = (ld_code % 4 == 0) && aligned16(code);
  a.noise = noise; a.ld_noise = ld_noise; a.m = m;
  a.h1 = acts ? acts->h1 : nullptr; a.h2 = acts ? acts->h2 : nullptr;
  a.h3 = acts ? acts->h3 : nullptr; a.h4 = acts ? acts->h4 : nullptr;
  a.action_hat = action_hat;
  a.noise_out = gen ? gen->out : nullptr; a.noise_seed = gen ? gen->seed : 0; a.noise_step = gen ? gen->step : nullptr;
  const int walign = (net.ld1 % 4 == 0) ? 4 : (net.ld1 % 2 == 0 ? 2 : 1);
  const dim3 grid((unsigned)(pad_rows(m) / 16));
  const bool pk = net.pf1 != nullptr;
#define NDP_LAUNCH_GFWD(WA) \
  do { \
    if (pk) hipLaunchKernelGGL((k_g_fwd<WA, true>), grid, dim3(kThreads), g_fwd_lds_floats() * 4, st, a); \
    else hipLaunchKernelGGL((k_g_fwd<WA, false>), grid, dim3(kThreads), g_fwd_lds_floats() * 4, st, a); \
  } while (0)
  KTimer kt("k_g_fwd", st);
  if (walign == 4) NDP_LAUNCH_GFWD(4); else if (walign == 2) NDP_LAUNCH_GFWD(2); else NDP_LAUNCH_GFWD(1);
#undef NDP_LAUNCH_GFWD
  return check_launch("k_g_fwd");
}

// Every kernel of the step works on 16-row tiles; the 2-pass D step stacks 16 real + 16 fake rows per workgroup.
// Measured (bench.py --batch 192..2048, K = 6 and 32): 16-row tiles win at every size -- their LDS footprint lets 2+
// workgroups share a CU, which hides more latency than the halved weight traffic of 32-row tiles bought.
static int launch_d(DArgs& a, int npass, int nd_blocks, hipStream_t st) {
  set_attrs();
  a.ntiles = (int)(a.mpad / 16);
  if (nd_blocks == 0) a.nd.n = 0;
  const dim3 grid((unsigned)(a.ntiles + nd_blocks));
  KTimer kt(a.do_backward ? (npass == 2 ? "k_d[2 pass fwd+bwd]" : "k_d[fwd+bwd]") : "k_d[fwd]", st);
  const bool pk = a.net.pf1 != nullptr;
#define NDP_LAUNCH_D(NP) \
  do { \
    if (pk) hipLaunchKernelGGL((k_d<NP, true>), grid, dim3(kThreads), (d_lds_floats<NP>() * 4), st, a); \
    else hipLaunchKernelGGL((k_d<NP, false>), grid, dim3(kThreads), (d_lds_floats<NP>() * 4), st, a); \
  } while (0)
  if (npass == 2) NDP_LAUNCH_D(2);
  else NDP_LAUNCH_D(1);
#undef NDP_LAUNCH_D
  return check_launch("k_d");
}

static int launch_g_bwd(GBwdArgs& a, hipStream_t st) {
  set_attrs();
  const dim3 grid((unsigned)(pad_rows(a.m) / 16));
  KTimer kt("k_g_bwd", st);
  if (a.net.pg2 != nullptr) hipLaunchKernelGGL((k_g_bwd<true>), grid, dim3(kThreads), g_bwd_lds_floats() * 4, st, a);
  else hipLaunchKernelGGL((k_g_bwd<false>), grid, dim3(kThreads), g_bwd_lds_floats() * 4, st, a);
  return check_launch("k_g_bwd");
}

static WgradJob make_job(const float* A, int lda, int a_cols, const float* B, int ldb, int b_cols,
                         int64_t dst_off, int dst_ld, int64_t bias_off, int kind) {
  WgradJob j;
  j.A = A; j.lda = lda; j.a_cols = a_cols;
  j.B = B; j.ldb = ldb; j.b_cols = b_cols;
  j.b_rowmod = 0x7fffffff; j.b_rowdiv = 1; j.b_rowmax = 0x7fffffff;
  j.b_vec = (ldb % 4 == 0) && aligned16(B);
  j.dst_off = (int)dst_off; j.dst_ld = dst_ld; j.bias_off = (int)bias_off; j.kind = kind;
  j.rows = 0; j.seg = 0; j.seg_s = 1; j.seg_k = 1; j.seg_wrap = 0;
  j.nchunks = kind == WG_FULL ? 1 : 0;   // 1: heavy, 0: light -- launch_wgrad turns the mark into the chunk count
  return j;
}

// K-deduplicated fc1 code columns: segments per 16-row tile and padded entry count
static int seg_per_tile(int K) { int s = 15 / K + 2; return s < 16 ? s : 16; }
static int64_t seg_entries(int64_t mpad, int K) { return (mpad / 16 * seg_per_tile(K) + 15) / 16 * 16; }

// weight-gradient jobs of the Decoder (26): operands dy1..dy5 / code, noise, h1..h4
static void build_g_jobs(WgradArgs& w, int nz, const GBwdWs& ws, const GActs& acts,
                         const float* code, int64_t ld_code, int code_rep,
                         const float* noise, int64_t ld_noise, int64_t m, const float* dy1seg = nullptr) {
  const GLayout L = g_layout(nz);
  int n = 0;
  const int code_rowmax = (int)((m - 1) / code_rep);
  for (int jb = 0; jb < 2; ++jb) {                       // fc1: [128 x (256+nz)]
    for (int kb = 0; kb < 4; ++kb) {
      WgradJob j = make_job((dy1seg ? dy1seg : ws.dy1) + jb * 64, 128, 64, code + kb * 64, (int)ld_code, 64,
                            L.w1 + (int64_t)jb * 64 * L.in1 + kb * 64, L.in1,
                            kb == 0 ? L.b1 + jb * 64 : -1, WG_FULL);
      j.b_rowdiv = code_rep; j.b_rowmax = code_rowmax;
      if (dy1seg) { j.rows = (int)seg_entries(pad_rows(m), code_rep); j.seg = 1; j.seg_s = seg_per_tile(code_rep); j.seg_k = code_rep; }
      j.nchunks = 0;                                     // the whole fc1 layer is "light" (one slab count per layer)
      w.job[n++] = j;
    }
    WgradJob t = make_job(ws.dy1 + jb * 64, 128, 64, noise, (int)ld_noise, nz,
                          L.w1 + (int64_t)jb * 64 * L.in1 + CODE, L.in1, -1, WG_SKINNY_B);
    t.b_rowmax = (int)(m - 1);
    w.job[n++] = t;
  }
  for (int kb = 0; kb < 2; ++kb)                         // fc2: [64 x 128]
    w.job[n++] = make_job(ws.dy2, 64, 64, acts.h1 + kb * 64, 128, 64, L.w2 + kb * 64, 128,
                          kb == 0 ? L.b2 : -1, WG_FULL);
  for (int jb = 0; jb < 2; ++jb)                         // fc3: [128 x 64]
    w.job[n++] = make_job(ws.dy3 + jb * 64, 128, 64, acts.h2, 64, 64, L.w3 + (int64_t)jb * 64 * 64, 64,
                          L.b3 + jb * 64, WG_FULL);
  const int wide = wgrad_wide_chunks(pad_rows(m));
  if (!wide)
    for (int jb = 0; jb < 4; ++jb)                       // fc4: [256 x 128]
      for (int kb = 0; kb < 2; ++kb)
        w.job[n++] = make_job(ws.dy4 + jb * 64, 256, 64, acts.h3 + kb * 64, 128, 64,
                              L.w4 + (int64_t)jb * 64 * 128 + kb * 64, 128, kb == 0 ? L.b4 + jb * 64 : -1, WG_FULL);
  for (int kb = 0; kb < 4; ++kb)                         // fc5: [4 x 256]
    w.job[n++] = make_job(ws.dy5, 4, 4, acts.h4 + kb * 64, 256, 64, L.w5 + kb * 64, 256,
                          kb == 0 ? L.b5 : -1, WG_SKINNY_A);
  w.njobs = n; w.net_is_g = 1;
  w.nwide = 0; w.wide_chunks = 0;
  w.wide_begin = w.wide_end = 0;
  if (wide) {                                            // fc4 as LDS-staged jobs per row chunk (large M)
    w.nwide = 2;
    for (int h = 0; h < 2; ++h)
      w.job[n + h] = make_job(ws.dy4 + h * 128, 256, 128, acts.h3, 128, 128, L.w4 + (int64_t)h * 128 * 128, 128, L.b4 + h * 128, WG_WIDE);
    w.wide_chunks = wide;
    w.wide_begin = (int)L.w4; w.wide_end = (int)L.b4 + 256;
  }
  w.nreg = 2;                                            // layers whose jobs are light: fc1, fc5
  w.reg_begin[0] = (int)L.w1; w.reg_end[0] = (int)L.b1 + 128;
  w.reg_begin[1] = (int)L.w5; w.reg_end[1] = (int)L.b5 + 4;
}

// weight-gradient jobs of the Discriminator (19) over npass*mpad rows
// dy1seg != null (fused step): rows = the rpad distinct real rows followed by the mpad fake rows; fc1's code columns
// run over `dy1seg` = the fake pass' per-tile segment sums followed by the real rows' dY1 (k_phase_a).  Otherwise
// (module backward, repeat D steps) the passes are mpad rows each and every row reads its code row.
static void build_d_jobs(WgradArgs& w, const DBwdWs& ws, const float* code, int64_t ld_code, int code_rep,
                         int64_t m, int64_t mpad, const float* dy1seg = nullptr, int64_t rpad = 0, int64_t wide_rows = 0) {
  const DLayout L = d_layout();
  int n = 0;
  for (int kb = 0; kb < 4; ++kb) {                       // fc1: [64 x 260], code columns 4..259
    WgradJob j = make_job(dy1seg ? dy1seg : ws.dy1, 64, 64, code + kb * 64, (int)ld_code, 64, L.w1 + ADIM + kb * 64, 260,
                          kb == 0 ? L.b1 : -1, WG_FULL);
    j.b_rowmod = (int)mpad; j.b_rowdiv = code_rep; j.b_rowmax = (int)((m - 1) / code_rep);
    if (dy1seg) {
      const int e = (int)seg_entries(mpad, code_rep);
      j.rows = e + (int)rpad; j.seg = 1; j.seg_wrap = e;  // entries >= e are real rows: entry e + f pairs with code row f
      j.seg_s = seg_per_tile(code_rep); j.seg_k = code_rep;
    }
    j.nchunks = 0;                                       // fc1 is a light layer
    w.job[n++] = j;
  }
  w.job[n++] = make_job(ws.dy1, 64, 64, ws.xa, 4, ADIM, L.w1, 260, -1, WG_SKINNY_B);   // action columns 0..3
  for (int jb = 0; jb < 2; ++jb)                         // fc2: [128 x 64]
    w.job[n++] = make_job(ws.dy2 + jb * 64, 128, 64, ws.h1, 64, 64, L.w2 + (int64_t)jb * 64 * 64, 64,
                          L.b2 + jb * 64, WG_FULL);
  const int wide = wgrad_wide_chunks(wide_rows);
  if (!wide)
    for (int jb = 0; jb < 4; ++jb)                       // fc3: [256 x 128]
      for (int kb = 0; kb < 2; ++kb)
        w.job[n++] = make_job(ws.dy3 + jb * 64, 256, 64, ws.h2 + kb * 64, 128, 64,
                              L.w3 + (int64_t)jb * 64 * 128 + kb * 64, 128, kb == 0 ? L.b3 + jb * 64 : -1, WG_FULL);
  for (int kb = 0; kb < 4; ++kb)                         // fc4: [1 x 256]
    w.job[n++] = make_job(ws.dl, 1, 1, ws.h3 + kb * 64, 256, 64, L.w4 + kb * 64, 256,
                          kb == 0 ? L.b4 : -1, WG_SKINNY_A);
  w.njobs = n; w.net_is_g = 0;
  w.nwide = 0; w.wide_chunks = 0;
  w.wide_begin = w.wide_end = 0;
  if (wide) {                                            // fc3 as LDS-staged jobs per row chunk (large M)
    w.nwide = 2;
    for (int h = 0; h < 2; ++h)
      w.job[n + h] = make_job(ws.dy3 + h * 128, 256, 128, ws.h2, 128, 128, L.w3 + (int64_t)h * 128 * 128, 128, L.b3 + h * 128, WG_WIDE);
    w.wide_chunks = wide;
    w.wide_begin = (int)L.w3; w.wide_end = (int)L.b3 + 256;
  }
  w.nreg = 2;                                            // layers whose jobs are light: fc1, fc4
  w.reg_begin[0] = (int)L.w1; w.reg_end[0] = (int)L.b1 + 64;
  w.reg_begin[1] = (int)L.w4; w.reg_end[1] = (int)L.b4 + 1;
}

struct AdamHyper { float lr, beta1, beta2; };

static int launch_wgrad(WgradArgs& w, int64_t rows, int nchunks, int light, float* slabs, int64_t slab_stride,
                        int32_t* bump, const AdamHyper& hp, const NdivArgs* nd, int nd_blocks, hipStream_t st) {
  set_attrs();
  w.rows = (int)rows;
  for (int i = 0; i < w.njobs; ++i) w.job[i].nchunks = w.job[i].nchunks ? nchunks : light;   // heavy / light mark -> count
  for (int i = 0; i < w.nwide; ++i) w.job[w.njobs + i].nchunks = w.wide_chunks;
  w.slabs = slabs; w.slab_stride = slab_stride; w.bump = bump;
  w.lr = hp.lr; w.beta1 = hp.beta1; w.beta2 = hp.beta2;
  w.nchunks = nchunks;
  if (nd != nullptr && nd_blocks > 0) w.nd = *nd; else { memset(&w.nd, 0, sizeof(w.nd)); nd_blocks = 0; }
  // a chunk may end up empty when rows_per_chunk rounds up; its slab must still be written
  const dim3 grid((unsigned)(w.nwide * w.wide_chunks + 8 * ((nchunks + 7) / 8) * w.njobs + nd_blocks));
  KTimer kt(w.net_is_g ? "k_wgrad[G]" : "k_wgrad[D]", st);
  if (w.nwide) hipLaunchKernelGGL(k_wgrad_wide, grid, dim3(kThreads), wgrad_wide_launch_lds_floats() * 4, st, w);
  else hipLaunchKernelGGL(k_wgrad, grid, dim3(kThreads), wgrad_lds_floats() * 4, st, w);
  return check_launch("k_wgrad");
}

// the light layers' parameters are summed over `light` slabs, the others over red.nchunks
static void set_red_regions(ReduceArgs& r, const WgradArgs& w, int light) {
  r.nregions = light != r.nchunks ? w.nreg : 0;
  for (int i = 0; i < r.nregions; ++i) { r.reg_begin[i] = w.reg_begin[i]; r.reg_end[i] = w.reg_end[i]; r.reg_slabs[i] = light; }
  if (w.nwide) {                                         // the WIDE layer wrote wide_chunks slabs
    const int i = r.nregions++;
    r.reg_begin[i] = w.wide_begin; r.reg_end[i] = w.wide_end; r.reg_slabs[i] = w.wide_chunks;
  }
}

static int launch_reduce(ReduceArgs& r, hipStream_t st) {
  // + 1: a block without parameters that computes the loss scalars beside the others (P2P: it takes part in the
  // hand-shake like any block, every rank launches the same grid)
  const dim3 grid((unsigned)((r.n + kThreads - 1) / kThreads + 1));
  KTimer kt("k_reduce_adam", st);
  if (r.p2p.world > 1)
    hipLaunchKernelGGL(k_reduce_adam<true>, grid, dim3(kThreads), 0, st, r);
  else
    hipLaunchKernelGGL(k_reduce_adam<false>, grid, dim3(kThreads), 0, st, r);
  return check_launch("k_reduce_adam");
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
  set_attrs();
  const int threads = ndiv_block_threads(k);
  NdivArgs a = ndiv_args(x, cx, z, cz, n, k, grad_scale, grad, partials, threads);
  const int G = a.rows_per_block;
  const size_t lds = ndiv_lds_bytes(G, k, cx, cz);
  const dim3 grid((unsigned)((n + G - 1) / G));
  KTimer kt("k_ndiv", st);
  if (cx <= 4 && cz <= 2) hipLaunchKernelGGL((k_ndiv<4, 2>), grid, dim3(threads), lds, st, a);
  else hipLaunchKernelGGL((k_ndiv<16, 16>), grid, dim3(threads), lds, st, a);
  return check_launch("k_ndiv");
}

}  // namespace ndp

// ================================================================== C ABI
using namespace ndp;

extern "C" {

int ndp_version(void) { return NDP_VERSION; }
const char* ndp_last_error(void) { return g_err; }
int64_t ndp_g_param_count(int noise_dim) { return g_layout(noise_dim).total; }
int64_t ndp_d_param_count(void) { return d_layout().total; }
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

int64_t ndp_g_acts_floats(int64_t m) { return g_acts_floats(pad_rows(m)); }

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
  const int64_t mpad = pad_rows(m);
  GActs a;
  if (acts) a = g_acts(acts, mpad);
  return launch_g_fwd(g_net(g_params, noise_dim), code, ld_code, code_rep, noise, ld_noise, m,
                      acts ? &a : nullptr, action_hat, nullptr, (hipStream_t)stream);
}

int64_t ndp_g_bwd_ws_floats(int64_t m, int noise_dim) { return g_bwd_floats(pad_rows(m), noise_dim); }

static int g_backward_impl(const GNet& gnet, int nz, const float* code, int64_t ld_code, int code_rep,
                           const float* noise, int64_t ld_noise, int64_t m, const GActs& acts,
                           const float* d_action, const float* d_action2, float* ws_base,
                           ReduceArgs& red, int32_t* bump, const AdamHyper& hp, hipStream_t st,
                           const float* dy1seg = nullptr) {
  const int64_t mpad = pad_rows(m);
  GBwdWs ws = g_bwd_ws(ws_base, mpad, nz);
  GBwdArgs b;
  b.net = gnet;
  b.m = m;
  b.h1 = acts.h1; b.h2 = acts.h2; b.h3 = acts.h3; b.h4 = acts.h4;
  b.d_action = d_action; b.d_action2 = d_action2;
  b.dy1 = ws.dy1; b.dy2 = ws.dy2; b.dy3 = ws.dy3; b.dy4 = ws.dy4; b.dy5 = ws.dy5;
  int rc = NDP_OK;
  if (d_action != nullptr) {          // null: dy1..dy5 were already produced (fused phase B kernel)
    rc = launch_g_bwd(b, st);
    if (rc) return rc;
  }
  WgradArgs w;
  build_g_jobs(w, nz, ws, acts, code, ld_code, code_rep, noise, ld_noise, m, dy1seg);
  rc = launch_wgrad(w, mpad, ws.nchunks, ws.light, ws.slabs, ws.slab_stride, bump, hp, nullptr, 0, st);
  if (rc) return rc;
  red.slabs = ws.slabs; red.nchunks = ws.nchunks; red.slab_stride = ws.slab_stride;
  set_red_regions(red, w, ws.light);
  red.n = g_layout(nz).total;
  return launch_reduce(red, st);
}

int ndp_g_backward(const float* g_params, int noise_dim, const float* code, int64_t ld_code, int code_rep,
                   const float* noise, int64_t ld_noise, int64_t m, const float* acts, const float* d_action,
                   float* grad, float* ws, void* stream) {
  int rc = check_g_common("ndp_g_backward", g_params, noise_dim, code, ld_code, code_rep, noise, ld_noise, m);
  if (rc) return rc;
  NDP_CHECK_ARG(acts && d_action && grad && ws, "ndp_g_backward: null pointer");
  NDP_CHECK_ARG(aligned16(acts) && aligned16(d_action) && aligned16(ws), "ndp_g_backward: buffers must be 16-byte aligned");
  ReduceArgs red;
  memset(&red, 0, sizeof(red));
  red.grad = grad;
  GActs a = g_acts(const_cast<float*>(acts), pad_rows(m));
  return g_backward_impl(g_net(g_params, noise_dim), noise_dim, code, ld_code, code_rep, noise, ld_noise, m, a, d_action,
                         nullptr, ws, red, nullptr, AdamHyper{0.f, 0.f, 0.f}, (hipStream_t)stream);
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
  const GBwdWs w = g_bwd_ws(ws, mpad, noise_dim);
  if (d_action != nullptr) {          // null: dy1 is what the ndp_g_backward call just before left in ws
    const GActs a = g_acts(const_cast<float*>(acts), mpad);
    GBwdArgs b;
    b.net = net;
    b.m = m;
    b.h1 = a.h1; b.h2 = a.h2; b.h3 = a.h3; b.h4 = a.h4;
    b.d_action = d_action; b.d_action2 = nullptr;
    b.dy1 = w.dy1; b.dy2 = w.dy2; b.dy3 = w.dy3; b.dy4 = w.dy4; b.dy5 = w.dy5;
    rc = launch_g_bwd(b, st);
    if (rc) return rc;
  }
  GInGradArgs g;
  g.w1 = net.w1; g.ld1 = net.ld1; g.nz = noise_dim;
  g.dy1 = w.dy1; g.d_z = d_z; g.ld_dz = ld_dz; g.m = m;
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
  return launch_d(a, 1, 0, (hipStream_t)stream);
}

int64_t ndp_d_bwd_ws_floats(int64_t m) { return d_bwd_floats(pad_rows(m), 1); }

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
  DBwdWs w;
  if (grad) {
    w = d_bwd_ws(ws, a.mpad, 1);
    a.h1 = w.h1; a.h2 = w.h2; a.h3 = w.h3; a.dy1 = w.dy1; a.dy2 = w.dy2; a.dy3 = w.dy3; a.dl = w.dl; a.xa = w.xa;
  }
  rc = launch_d(a, 1, 0, st);
  if (rc || !grad) return rc;
  WgradArgs wa;
  build_d_jobs(wa, w, code, ld_code, code_rep, m, a.mpad, nullptr, 0, a.mpad);
  rc = launch_wgrad(wa, a.mpad, w.nchunks, w.light, w.slabs, w.slab_stride, nullptr, AdamHyper{0.f, 0.f, 0.f}, nullptr, 0, st);
  if (rc) return rc;
  ReduceArgs red;
  memset(&red, 0, sizeof(red));
  red.slabs = w.slabs; red.nchunks = w.nchunks; red.slab_stride = w.slab_stride; red.n = d_layout().total;
  set_red_regions(red, wa, w.light);
  red.grad = grad;
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
  KTimer kt("k_adam", st);
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
  return check_launch("k_adam");
}

// ------------------------------------------------------------------ fused train step
// workspace: [G acts][G bwd ws][D bwd ws (2 passes)][d_action m x 4][ndiv grad m x 4][ndiv partials]
struct StepWs {
  GActs acts; float* gb; float* db; float* d_action; float* nd_grad; float* nd_part; int64_t nd_count;
  float* g_packed; float* d_packed;
  float* d_seg; float* g_seg;    // segment sums of dY1 for the K-deduplicated fc1 weight gradients
};
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

// NDiv rides in the D-step launch (256-thread blocks) when its shape fits the <4,2>
// specialisation (noise_dim <= 2); otherwise it is a kernel of its own in phase B.
static bool step_ndiv_fused(const ndp_step_config* c) { return c->noise_dim <= 2; }
static int step_ndiv_threads(const ndp_step_config* c) {
  return step_ndiv_fused(c) ? kThreads : ndiv_block_threads(c->num_sample);
}

static int64_t step_floats(const ndp_step_config* c, StepWs* out, float* base, int64_t* test_offsets = nullptr) {
  const int64_t m = c->flat * c->num_sample, mpad = pad_rows(m);
  int64_t o = 0;
  const int64_t o_acts = o; o += g_acts_floats(mpad);
  const int64_t o_gb = o; o += g_bwd_floats(mpad, c->noise_dim);
  const int64_t o_db = o;                             // D scratch: the fused step's layout or two full passes (repeat D steps)
  { const int64_t a_ = d_bwd_floats(mpad, 2), b_ = d_bwd_floats_rows(step_d_rows(c)); o += a_ > b_ ? a_ : b_; }
  const int64_t o_da = o; o += mpad * 4;
  const int64_t o_ng = o; o += mpad * 4;
  const int64_t o_np = o;
  const int G = ndiv_rows_per_block(c->num_sample, step_ndiv_threads(c));
  const int64_t npart = (c->flat + G - 1) / G;
  o += pad4(npart);
  const int64_t o_gp = o; o += kGPackFloats;
  const int64_t o_dp = o; o += kDPackFloats;
  const int64_t o_ds = o;                             // fc1 operand: fake segment sums + the real rows' dY1 (k_phase_a)
  o += (seg_entries(mpad, c->num_sample) + step_real_pad(c)) * 64;
  const int64_t o_gs = o; o += seg_entries(mpad, c->num_sample) * 128;
  if (out) {
    out->g_packed = base + o_gp; out->d_packed = base + o_dp;
    out->d_seg = base + o_ds; out->g_seg = base + o_gs;
    out->acts = g_acts(base + o_acts, mpad);
    out->gb = base + o_gb; out->db = base + o_db; out->d_action = base + o_da; out->nd_grad = base + o_ng;
    out->nd_part = base + o_np; out->nd_count = npart;
  }
  if (test_offsets) {                                  // ndp_step_workspace_offset (the order of NDP_STEP_TENSORS in ndp.h)
    test_offsets[0] = o_acts; test_offsets[1] = o_acts + mpad * 128; test_offsets[2] = o_acts + mpad * (128 + 64);
    test_offsets[3] = o_acts + mpad * (128 + 64 + 128); test_offsets[4] = o_ng;
    test_offsets[5] = o_gb + mpad * (128 + 64 + 128 + 256);       // dy5 of g_bwd_ws
    const int64_t rows[2] = {step_d_rows(c), 2 * mpad};           // the layouts of d_bwd_ws_rows: first / repeat D step
    for (int r = 0; r < 2; ++r) {
      test_offsets[6 + 3 * r] = o_db + rows[r] * 4; test_offsets[7 + 3 * r] = o_db + rows[r] * (4 + 64);
      test_offsets[8 + 3 * r] = o_db + rows[r] * (4 + 64 + 128);
    }
  }
  return o;
}

static int check_step(const char* fn, const ndp_step_config* c, const ndp_step_buffers* b, const float* codes,
                      const float* actions, const float* noise) {
  NDP_CHECK_ARG(c && b && codes && actions && noise, "%s: null pointer", fn);
  NDP_CHECK_ARG(c->noise_dim >= 1 && c->noise_dim <= NDP_MAX_NOISE_DIM, "%s: noise_dim=%d outside 1..%d", fn, c->noise_dim, NDP_MAX_NOISE_DIM);
  NDP_CHECK_ARG(c->num_sample >= 1 && c->num_sample <= NDP_MAX_SAMPLES, "%s: num_sample=%d outside 1..%d", fn, c->num_sample, NDP_MAX_SAMPLES);
  NDP_CHECK_ARG(c->flat >= 1 && c->flat * c->num_sample < (1ll << 28), "%s: bad flat=%lld", fn, (long long)c->flat);
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
  memset(&red, 0, sizeof(red));
  int rc = fill_p2p("ndp_p2p_all_reduce", red.p2p, c, net, n);
  if (rc) return rc;
  red.slabs = in; red.nchunks = 1; red.slab_stride = 0; red.n = n;
  red.grad = out; red.step = step_word;
  return launch_reduce(red, (hipStream_t)stream);
}

int64_t ndp_step_workspace_floats(const ndp_step_config* cfg) {
  if (!cfg || cfg->flat < 1 || cfg->num_sample < 1 || cfg->num_sample > NDP_MAX_SAMPLES) return 0;
  return step_floats(cfg, nullptr, nullptr);
}

int64_t ndp_step_workspace_offset(const ndp_step_config* cfg, int tensor) {
  if (!cfg || cfg->flat < 1 || cfg->num_sample < 1 || cfg->num_sample > NDP_MAX_SAMPLES || cfg->noise_dim < 1 ||
      cfg->noise_dim > NDP_MAX_NOISE_DIM || cfg->flat >= (1ll << 28) || cfg->flat * cfg->num_sample >= (1ll << 28) ||
      tensor < 0 || tensor >= NDP_STEP_TENSORS)
    return -1;
  int64_t at[NDP_STEP_TENSORS];
  step_floats(cfg, nullptr, nullptr, at);
  return at[tensor];
}

int ndp_step_d_grads(const ndp_step_config* c, const ndp_step_buffers* b, const float* codes, const float* actions,
                     float* noise, int run_g_forward, void* stream) {
  int rc = check_step("ndp_step_d_grads", c, b, codes, actions, noise);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int K = c->num_sample, nz = c->noise_dim;
  const int64_t m = c->flat * K, mpad = pad_rows(m);
  StepWs ws;
  step_floats(c, &ws, b->workspace);
  // first D step of an iteration: real pass on the distinct rows (k_phase_a); repeat D steps: two full passes (k_d)
  const int64_t rpad = step_real_pad(c);
  DBwdWs dw = run_g_forward ? d_bwd_ws_rows(ws.db, step_d_rows(c)) : d_bwd_ws(ws.db, mpad, 2);
  const bool fused_ndiv = step_ndiv_fused(c);
  NdivArgs nd;
  if (fused_ndiv)   // NDiv loss + gradient (train_gan.py:193-199; gradient pre-scaled by pairwise_div_factor)
    nd = ndiv_args(b->action_hat, ADIM, noise, nz, c->flat, K, c->pairwise_div_factor, ws.nd_grad, ws.nd_part, kThreads);
  int loss_count = (int)(mpad / 16);            // workgroups that wrote a BCE partial
  if (run_g_forward) {
    // G forward + D(real) + D(fake) + BCE + D's backward data path in one launch
    set_attrs();
    PhaseAArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.g = g_net(b->g_params, nz, ws.g_packed);
    pa.d = d_net(b->d_params, ws.d_packed);
    pa.code = codes; pa.code_rep = K;
    pa.noise = c->device_noise ? nullptr : noise;
    pa.noise_out = c->device_noise ? noise : nullptr; pa.noise_seed = c->noise_seed; pa.noise_step = b->g_step;
    pa.actions = actions;
    pa.m = m; pa.mpad = mpad; pa.flat = c->flat; pa.rpad = rpad;
    pa.inv_m = c->inv_m_global; pa.real_scale = (float)K;
    pa.gh1 = ws.acts.h1; pa.gh2 = ws.acts.h2; pa.gh3 = ws.acts.h3; pa.gh4 = ws.acts.h4;
    pa.action_hat = b->action_hat;
    pa.h1 = dw.h1; pa.h2 = dw.h2; pa.h3 = dw.h3; pa.dy1 = dw.dy1; pa.dy2 = dw.dy2; pa.dy3 = dw.dy3; pa.dl = dw.dl; pa.xa = dw.xa;
    pa.loss_partials = dw.lossp;
    pa.dy1seg = ws.d_seg; pa.seg_s = seg_per_tile(K); pa.seg_entries = (int)seg_entries(mpad, K);
    KTimer kt("k_phase_a", st);
    // one workgroup per fake tile (G + D) and one per tile of distinct real rows; up to 256 of them sit alone on a CU
    // each with deep weight rings, more share CUs (three per CU by LDS) with small ones
    loss_count = (int)(mpad / 16 + rpad / 16);
    const bool small = several_per_cu(loss_count);
    const int nr = step_code_rows(K, small);
#define NDP_LAUNCH_A(RG, NR) hipLaunchKernelGGL((k_phase_a<true, RG, NR>), dim3((unsigned)loss_count), dim3(kThreads), phase_a_lds_floats() * 4, st, pa)
    if (small) {
      if (nr == 1) NDP_LAUNCH_A(kPhaseASmallRing, 1);
      else if (nr == 4) NDP_LAUNCH_A(kPhaseASmallRing, 4);
      else NDP_LAUNCH_A(kPhaseASmallRing, 0);
    } else {
      NDP_LAUNCH_A(96, 0);
    }
#undef NDP_LAUNCH_A
    rc = check_launch("k_phase_a");
    if (rc) return rc;
  } else {
    // repeat D step of a discrim_steps_per_gen > 1 iteration: action_hat is re-used (train_gan.py:172)
    DArgs a;
    d_args_init(a, b->d_params, codes, CODE, K, m);
    a.net = d_net(b->d_params, ws.d_packed);
    a.inv_m = c->inv_m_global;
    a.pass[0].action = actions; a.pass[0].action_rep = K; a.pass[0].target = 1.f;        // real (train_gan.py:174-177)
    a.pass[1].action = b->action_hat; a.pass[1].action_rep = 1; a.pass[1].target = 0.f;  // fake (178-181)
    a.do_backward = 1;
    a.h1 = dw.h1; a.h2 = dw.h2; a.h3 = dw.h3; a.dy1 = dw.dy1; a.dy2 = dw.dy2; a.dy3 = dw.dy3; a.dl = dw.dl; a.xa = dw.xa;
    a.loss_partials = dw.lossp;
    rc = launch_d(a, 2, 0, st);
    if (rc) return rc;
  }
  WgradArgs wa;
  // the fused kernel also produced fc1's K-deduplicated operand (segment sums of the fake pass + the real rows' dY1)
  build_d_jobs(wa, dw, codes, CODE, K, m, mpad, run_g_forward ? ws.d_seg : nullptr, rpad, run_g_forward ? step_d_rows(c) : 2 * mpad);
  // the Adam state word is advanced here in both modes: ndp_step_apply_adam (non-fused) finds it ready
  rc = launch_wgrad(wa, run_g_forward ? step_d_rows(c) : 2 * mpad, dw.nchunks, dw.light, dw.slabs, dw.slab_stride, b->d_step,
                    AdamHyper{c->lr, c->beta1, c->beta2}, fused_ndiv ? &nd : nullptr, (int)ws.nd_count, st);
  if (rc) return rc;
  ReduceArgs red;
  memset(&red, 0, sizeof(red));
  red.slabs = dw.slabs; red.nchunks = dw.nchunks; red.slab_stride = dw.slab_stride; red.n = d_layout().total;
  set_red_regions(red, wa, dw.light);
  red.grad = b->d_grad;
  if (c->fuse_adam) {
    red.params = b->d_params; red.exp_avg = b->d_exp_avg; red.exp_avg_sq = b->d_exp_avg_sq; red.step = b->d_step;
    red.lr = c->lr; red.beta1 = c->beta1; red.beta2 = c->beta2; red.eps = c->eps;
    red.pack = d_pack_spec(ws.d_packed);
  }
  red.step = b->d_step;
  rc = fill_p2p("ndp_step_d_grads", red.p2p, c->p2p, 0, red.n);
  if (rc) return rc;
  red.loss[0].partials = dw.lossp; red.loss[0].count = loss_count; red.loss[0].scale = c->inv_m_global;
  red.loss[0].slot = 0;
  red.nloss = 1; red.losses = b->losses; red.loss_sums = b->loss_sums;
  return launch_reduce(red, st);
}

int ndp_step_g_grads(const ndp_step_config* c, const ndp_step_buffers* b, const float* codes, const float* actions,
                     const float* noise, void* stream) {
  int rc = check_step("ndp_step_g_grads", c, b, codes, actions, noise);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int K = c->num_sample, nz = c->noise_dim;
  const int64_t m = c->flat * K, mpad = pad_rows(m);
  StepWs ws;
  step_floats(c, &ws, b->workspace);
  DBwdWs dw = d_bwd_ws_rows(ws.db, step_d_rows(c));   // only its loss-partial area is used here
  if (!step_ndiv_fused(c)) {
    // NDiv loss and gradient (train_gan.py:193-199), gradient pre-scaled by pairwise_div_factor
    rc = launch_ndiv(b->action_hat, ADIM, noise, nz, c->flat, K, c->pairwise_div_factor, ws.nd_grad, ws.nd_part, st);
    if (rc) return rc;
  }
  // G loss through the updated D (train_gan.py:187-190), dLoss/d action_hat (+ NDiv gradient),
  // G's backward data path: one launch
  set_attrs();
  GBwdWs gw = g_bwd_ws(ws.gb, mpad, nz);
  PhaseBArgs pb;
  memset(&pb, 0, sizeof(pb));
  pb.g = g_net(b->g_params, nz, ws.g_packed);
  pb.d = d_net(b->d_params, ws.d_packed);
  pb.code = codes; pb.code_rep = K;
  pb.action_hat = b->action_hat; pb.nd_grad = ws.nd_grad;
  pb.m = m; pb.inv_m = c->inv_m_global;
  pb.gh1 = ws.acts.h1; pb.gh2 = ws.acts.h2; pb.gh3 = ws.acts.h3; pb.gh4 = ws.acts.h4;
  pb.dy1 = gw.dy1; pb.dy2 = gw.dy2; pb.dy3 = gw.dy3; pb.dy4 = gw.dy4; pb.dy5 = gw.dy5;
  pb.loss_partials = dw.lossp;
  pb.dy1seg = ws.g_seg; pb.seg_s = seg_per_tile(K); pb.seg_entries = (int)seg_entries(mpad, K);
  {
    KTimer kt("k_phase_b", st);
    const int nt = (int)(mpad / 16);
    const bool small = several_per_cu(nt);
    const int nr = step_code_rows(K, small);
#define NDP_LAUNCH_B(RG, PRE, NR) hipLaunchKernelGGL((k_phase_b<true, RG, PRE, NR>), dim3((unsigned)nt), dim3(kThreads), phase_b_lds_floats(PRE) * 4, st, pb)
    if (small) {
      if (nr == 1) NDP_LAUNCH_B(32, false, 1);
      else if (nr == 4) NDP_LAUNCH_B(32, false, 4);
      else NDP_LAUNCH_B(32, false, 0);
    } else {
      NDP_LAUNCH_B(96, true, 0);
    }
#undef NDP_LAUNCH_B
  }
  rc = check_launch("k_phase_b");
  if (rc) return rc;
  ReduceArgs red;
  memset(&red, 0, sizeof(red));
  red.grad = b->g_grad;
  if (c->fuse_adam) {
    red.params = b->g_params; red.exp_avg = b->g_exp_avg; red.exp_avg_sq = b->g_exp_avg_sq; red.step = b->g_step;
    red.lr = c->lr; red.beta1 = c->beta1; red.beta2 = c->beta2; red.eps = c->eps;
    red.pack = g_pack_spec(nz, ws.g_packed);
  }
  red.step = b->g_step;
  rc = fill_p2p("ndp_step_g_grads", red.p2p, c->p2p, 1, g_layout(nz).total);
  if (rc) return rc;
  red.loss[0].partials = dw.lossp; red.loss[0].count = (int)(mpad / 16); red.loss[0].scale = c->inv_m_global;
  red.loss[0].slot = 1;
  red.loss[1].partials = ws.nd_part; red.loss[1].count = (int)ws.nd_count; red.loss[1].scale = 1.f;
  red.loss[1].slot = 2;
  red.nloss = 2; red.losses = b->losses; red.loss_sums = b->loss_sums;
  return g_backward_impl(g_net(b->g_params, nz, ws.g_packed), nz, codes, CODE, K, noise, nz, m, ws.acts, nullptr,
                         nullptr, ws.gb, red, b->g_step, AdamHyper{c->lr, c->beta1, c->beta2}, st, ws.g_seg);
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
  NDP_CHECK_ARG(c && b && b->g_params && b->d_params && b->workspace, "ndp_step_pack_params: null pointer");
  NDP_CHECK_ARG(c->noise_dim >= 1 && c->noise_dim <= NDP_MAX_NOISE_DIM && c->flat >= 1 && c->num_sample >= 1 &&
                c->num_sample <= NDP_MAX_SAMPLES, "ndp_step_pack_params: bad configuration");
  StepWs ws;
  step_floats(c, &ws, b->workspace);
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_pack(b->g_params, g_layout(c->noise_dim).total, g_pack_spec(c->noise_dim, ws.g_packed), st);
  if (rc) return rc;
  return launch_pack(b->d_params, d_layout().total, d_pack_spec(ws.d_packed), st);
}

int ndp_step_apply_adam(const ndp_step_config* c, const ndp_step_buffers* b, int which, void* stream) {
  NDP_CHECK_ARG(c && b && b->workspace, "ndp_step_apply_adam: null pointer");
  NDP_CHECK_ARG(which == 0 || which == 1, "ndp_step_apply_adam: which must be 0 (D) or 1 (G)");
  StepWs ws;
  step_floats(c, &ws, b->workspace);
  hipStream_t st = (hipStream_t)stream;
  AdamArgs a;
  if (which == 1) {
    NDP_CHECK_ARG(b->g_params && b->g_grad && b->g_exp_avg && b->g_exp_avg_sq && b->g_step, "ndp_step_apply_adam: null G buffer");
    a.params = b->g_params; a.grad = b->g_grad; a.exp_avg = b->g_exp_avg; a.exp_avg_sq = b->g_exp_avg_sq;
    a.n = g_layout(c->noise_dim).total; a.step = b->g_step; a.pack = g_pack_spec(c->noise_dim, ws.g_packed);
  } else {
    NDP_CHECK_ARG(b->d_params && b->d_grad && b->d_exp_avg && b->d_exp_avg_sq && b->d_step, "ndp_step_apply_adam: null D buffer");
    a.params = b->d_params; a.grad = b->d_grad; a.exp_avg = b->d_exp_avg; a.exp_avg_sq = b->d_exp_avg_sq;
    a.n = d_layout().total; a.step = b->d_step; a.pack = d_pack_spec(ws.d_packed);
  }
  a.lr = c->lr; a.beta1 = c->beta1; a.beta2 = c->beta2; a.eps = c->eps;
  // the state word (step count, bias corrections) was advanced by the phase's k_wgrad launch
  KTimer kt("k_adam", st);
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((a.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
  return check_launch("k_adam");
}

int ndp_uniform_noise(float* out, int64_t n, uint64_t seed, const int32_t* offset_dev, void* stream) {
  NDP_CHECK_ARG(out && n >= 1, "ndp_uniform_noise: bad arguments");
  const int64_t nthreads = n;
  hipLaunchKernelGGL(k_philox, dim3((unsigned)((nthreads + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, out, n, seed, offset_dev);
  return check_launch("k_philox");
}

}  // extern "C"
