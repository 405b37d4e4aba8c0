// ndp_world.inc -- the batched push world (include/ndp.h, "push world"; DESIGN.md section 5q): n environments of a
// gripper, a block and a goal on a table, advanced and drawn on the device.
//   k_world_step_render  one environment step in ONE launch: the physics of every environment and its camera frame
//                        [n][S][S][3] bytes, the layout every frame-reading kernel of this library takes
//   k_world_render       the same pixel path from a given state (after a reset, or a state written from outside)
// Grid (ceil(S*S / 1024), n), 256 threads: a thread owns four neighbouring pixels of a row, 12 bytes, stored as three
// 4-byte words (rows are 4-byte aligned: S % 4 == 0).  Thread 0 of every workgroup advances the environment's state in
// fp64 and quantises the scene to sixteenths of a pixel; both go to the others through LDS.  Meanwhile every thread
// finds its span and the table's colours under it (span_begin: the part that needs no scene).  Workgroup 0 of an
// environment writes state_out, a buffer other than state_in: nobody reads what another workgroup writes.  A span runs
// the 16-sample coverage only for the layers whose bounding box it meets (a layer it does not meet blends with k = 0,
// which is the identity), so most of a frame is the table's two colours.  Integer arithmetic from the quantisation on,
// nothing atomic, nothing spilled: two calls give the same bits.
// The step, the quantisation and the four-pixel span are __host__ __device__ (namespace ndp::world):
// tests/host_drivers/world.inc (a body of main.hip) runs exactly these functions by this schedule on the CPU.  Included
// at the end of ndp_kernels.hip, after ndp_plan.inc.

namespace ndp {
namespace world {

constexpr int kBlock = 256;
constexpr int kSpan = 4;                       // pixels of one thread
constexpr int kQMin = -8192, kQMax = 24576;    // the quantised range: squares of differences stay inside int32

// the scene in sixteenths of a pixel
struct Scene {
  int tx, ty, t_out, t_in;   // goal ring
  int sx, sy, s_r;           // the gripper's shadow
  int ox, oy, o_r;           // object
  int gx, gy, g_r;           // gripper
};

__host__ __device__ inline double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// q(v) of the header: llrint(v * 16 S / SIDE) after saturation to [kQMin, kQMax] (a NaN gives kQMin)
__host__ __device__ inline int quant(double v, int size) {
#pragma clang fp contract(off)
  double s = v * (16.0 * (double)size / NDP_WORLD_SIDE);
  if (!(s >= (double)kQMin)) s = (double)kQMin;
  if (s > (double)kQMax) s = (double)kQMax;
  return (int)rint(s);                         // llrint's value: the saturated range converts exactly
}

// one environment step: state_in[8], action[4] -> state_out[8]
__host__ __device__ inline void step(const float* s_in, const float* act, float* s_out) {
#pragma clang fp contract(off)
  double gx = (double)s_in[0], gy = (double)s_in[1], gz = (double)s_in[2];
  double ox = (double)s_in[3], oy = (double)s_in[4];
  const float a0 = act[0], a1 = act[1], a2 = act[2];
  const double mx = NDP_WORLD_STEP * clampd(a0 != a0 ? 0.0 : (double)a0, -1.0, 1.0) / (double)NDP_WORLD_SUB;
  const double my = NDP_WORLD_STEP * clampd(a1 != a1 ? 0.0 : (double)a1, -1.0, 1.0) / (double)NDP_WORLD_SUB;
  const double mz = NDP_WORLD_STEP * clampd(a2 != a2 ? 0.0 : (double)a2, -1.0, 1.0) / (double)NDP_WORLD_SUB;
  constexpr double kR = NDP_WORLD_R;
  for (int sub = 0; sub < NDP_WORLD_SUB; ++sub) {
    gx = clampd(gx + mx, NDP_WORLD_X0, NDP_WORLD_X0 + NDP_WORLD_SIDE);
    gy = clampd(gy + my, NDP_WORLD_Y0, NDP_WORLD_Y0 + NDP_WORLD_SIDE);
    gz = clampd(gz + mz, NDP_WORLD_Z_MIN, NDP_WORLD_Z_MAX);
    if (gz < NDP_WORLD_Z_CONTACT) {
      const double dx = ox - gx, dy = oy - gy;
      const double r2 = dx * dx + dy * dy;
      if (r2 < kR * kR) {
        if (r2 > 0.0) {
          const double f = kR / sqrt(r2);
          ox = gx + dx * f;
          oy = gy + dy * f;
        } else {
          ox = gx + kR;
          oy = gy;
        }
        ox = clampd(ox, NDP_WORLD_X0 + NDP_WORLD_R_O, NDP_WORLD_X0 + NDP_WORLD_SIDE - NDP_WORLD_R_O);
        oy = clampd(oy, NDP_WORLD_Y0 + NDP_WORLD_R_O, NDP_WORLD_Y0 + NDP_WORLD_SIDE - NDP_WORLD_R_O);
      }
    }
  }
  s_out[0] = (float)gx; s_out[1] = (float)gy; s_out[2] = (float)gz;
  s_out[3] = (float)ox; s_out[4] = (float)oy; s_out[5] = s_in[5];
  s_out[6] = s_in[6]; s_out[7] = s_in[7];
}

__host__ __device__ inline void quantise(const float* s, int size, Scene* sc) {
#pragma clang fp contract(off)
  const double gx = (double)s[0], gy = (double)s[1], gz = (double)s[2];
  const double lift = gz - NDP_WORLD_Z_MIN;
  sc->tx = quant((double)s[6] - NDP_WORLD_X0, size);
  sc->ty = quant((double)s[7] - NDP_WORLD_Y0, size);
  sc->t_out = quant(NDP_WORLD_R_O, size);
  sc->t_in = quant(NDP_WORLD_R_O - NDP_WORLD_RING, size);
  sc->sx = quant(gx + NDP_WORLD_SHADOW * lift - NDP_WORLD_X0, size);
  sc->sy = quant(gy + NDP_WORLD_SHADOW * lift - NDP_WORLD_Y0, size);
  sc->s_r = quant(NDP_WORLD_R_G, size);
  sc->ox = quant((double)s[3] - NDP_WORLD_X0, size);
  sc->oy = quant((double)s[4] - NDP_WORLD_Y0, size);
  sc->o_r = quant(NDP_WORLD_R_O, size);
  sc->gx = quant(gx - NDP_WORLD_X0, size);
  sc->gy = quant(gy - NDP_WORLD_Y0, size);
  sc->g_r = quant(NDP_WORLD_R_G * (1.0 + lift / (NDP_WORLD_Z_MAX - NDP_WORLD_Z_MIN)), size);
}

// how many of pixel (px, py)'s 16 samples lie at a squared distance within [lo2, hi2] of (cx, cy)
__host__ __device__ inline int coverage(int px, int py, int cx, int cy, int lo2, int hi2) {
  int k = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int dy = 16 * py + 2 + 4 * j - cy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int dx = 16 * px + 2 + 4 * i - cx;
      const int d2 = dx * dx + dy * dy;
      k += (d2 >= lo2 && d2 <= hi2) ? 1 : 0;
    }
  }
  return k;
}

__host__ __device__ inline int blend(int c, int fg, int k) { return (c * (16 - k) + fg * k + 8) >> 4; }

// does the box of radius r about (cx, cy) reach a sample of the span px0 .. px0+3 of row py?
__host__ __device__ inline bool meets(int px0, int py, int cx, int cy, int r) {
  return cx - r <= 16 * px0 + 62 && cx + r >= 16 * px0 + 2 && cy - r <= 16 * py + 14 && cy + r >= 16 * py + 2;
}

// one layer over the span's four pixels: colour (r, g, b), or with `shade` the darkened colour under it
__host__ __device__ inline void layer(int (&c)[kSpan][3], int px0, int py, int cx, int cy, int r_in, int r_out, int r, int g,
                                      int b, bool shade) {
  if (!meets(px0, py, cx, cy, r_out)) return;
#pragma unroll
  for (int p = 0; p < kSpan; ++p) {
    const int k = coverage(px0 + p, py, cx, cy, r_in * r_in, r_out * r_out);
    c[p][0] = blend(c[p][0], shade ? (c[p][0] * 10 + 8) >> 4 : r, k);
    c[p][1] = blend(c[p][1], shade ? (c[p][1] * 10 + 8) >> 4 : g, k);
    c[p][2] = blend(c[p][2], shade ? (c[p][2] * 10 + 8) >> 4 : b, k);
  }
}

// Four neighbouring pixels of a row.  What a thread can do before it has seen the scene -- find its span and put the
// table under it -- is span_begin; the layers and the packing are span_finish.  The kernels run the first in front of
// the barrier, beside thread 0's fp64 work, and the second behind it.
struct Span {
  int px0, py;
  int c[kSpan][3];
};

// span `idx` of a frame (row-major, S / 4 spans per row) and the table's colours.  Three unsigned divisions: a span
// of 4 pixels crosses at most one border of the checkerboard's cells, which are S / 8 >= 4 pixels wide.
__host__ __device__ inline void span_begin(int idx, int size, Span* s) {
  const unsigned per_row = (unsigned)size / kSpan, cell = (unsigned)size / 8;
  const unsigned row = (unsigned)idx / per_row, col = kSpan * ((unsigned)idx - row * per_row);
  const unsigned cx = col / cell, rx = col - cx * cell, cy = row / cell;
  s->px0 = (int)col;
  s->py = (int)row;
#pragma unroll
  for (int p = 0; p < kSpan; ++p) {
    const unsigned over = rx + (unsigned)p >= cell ? 1u : 0u;       // (col + p) / cell == cx + over
    const int dark = ((cx + over + cy) & 1u) ? 12 : 0;
    s->c[p][0] = 168 - dark;
    s->c[p][1] = 160 - dark;
    s->c[p][2] = 150 - dark;
  }
}

// the layers over the span, then its three little-endian words: the 12 bytes R G B R G B ...
__host__ __device__ inline void span_finish(const Scene& sc, Span& s, uint32_t (&w)[3]) {
  int (&c)[kSpan][3] = s.c;
  layer(c, s.px0, s.py, sc.tx, sc.ty, sc.t_in, sc.t_out, 40, 200, 60, false);
  layer(c, s.px0, s.py, sc.sx, sc.sy, 0, sc.s_r, 0, 0, 0, true);
  layer(c, s.px0, s.py, sc.ox, sc.oy, 0, sc.o_r, 20, 20, 235, false);
  layer(c, s.px0, s.py, sc.gx, sc.gy, 0, sc.g_r, 250, 245, 10, false);
  w[0] = (uint32_t)c[0][0] | (uint32_t)c[0][1] << 8 | (uint32_t)c[0][2] << 16 | (uint32_t)c[1][0] << 24;
  w[1] = (uint32_t)c[1][1] | (uint32_t)c[1][2] << 8 | (uint32_t)c[2][0] << 16 | (uint32_t)c[2][1] << 24;
  w[2] = (uint32_t)c[2][2] | (uint32_t)c[3][0] << 8 | (uint32_t)c[3][1] << 16 | (uint32_t)c[3][2] << 24;
}

// byte offset of pixel (px, py) of environment env
__host__ __device__ inline int64_t pixel_offset(int64_t env, int size, int px, int py) {
  return ((env * size + py) * size + px) * 3;
}

}  // namespace world

struct WorldArgs {
  const float* state_in; const float* actions;   // [n][8], [n][4] (k_world_render: actions null)
  float* state_out;                              // [n][8] (k_world_render: null)
  uint8_t* frames;                               // [n][S][S][3] or null
  int size;
};

// does this thread own a span of the frame?  (the last workgroup of a frame may be partial)
__device__ __forceinline__ bool world_span(const WorldArgs& a, world::Span* s) {
  using namespace world;
  const int idx = (int)blockIdx.x * kBlock + (int)threadIdx.x;
  if (a.frames == nullptr || idx >= a.size * a.size / kSpan) return false;
  span_begin(idx, a.size, s);
  return true;
}

__device__ __forceinline__ void world_store(const WorldArgs& a, const world::Scene& sc, world::Span& s) {
  using namespace world;
  uint32_t w[3];
  span_finish(sc, s, w);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.frames + pixel_offset((int64_t)blockIdx.y, a.size, s.px0, s.py));
  dst[0] = w[0];
  dst[1] = w[1];
  dst[2] = w[2];
}

__global__ __launch_bounds__(world::kBlock) void k_world_step_render(WorldArgs a) {
  using namespace world;
  __shared__ float state_s[8];
  __shared__ Scene scene_s;
  const int64_t env = blockIdx.y;
  Span span;
  const bool live = world_span(a, &span);
  if (threadIdx.x == 0) {
    step(a.state_in + env * 8, a.actions + env * 4, state_s);
    quantise(state_s, a.size, &scene_s);
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < 8) a.state_out[env * 8 + threadIdx.x] = state_s[threadIdx.x];
  if (!live) return;
  const Scene sc = scene_s;
  world_store(a, sc, span);
}

__global__ __launch_bounds__(world::kBlock) void k_world_render(WorldArgs a) {
  using namespace world;
  __shared__ Scene scene_s;
  Span span;
  const bool live = world_span(a, &span);
  if (threadIdx.x == 0) quantise(a.state_in + (int64_t)blockIdx.y * 8, a.size, &scene_s);
  __syncthreads();
  if (!live) return;
  const Scene sc = scene_s;
  world_store(a, sc, span);
}

inline bool world_size_ok(int size) { return size >= 32 && size <= 1024 && size % 4 == 0; }

}  // namespace ndp

extern "C" {

int ndp_world_step_render(const float* state_in, const float* actions, int64_t n, int size, float* state_out,
                          uint8_t* frames_hwc, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(state_in && actions && state_out, "ndp_world_step_render: null pointer");
  NDP_CHECK_ARG(world_size_ok(size), "ndp_world_step_render: size=%d is not a multiple of 4 in 32..1024", size);
  NDP_CHECK_ARG(n >= 1 && n <= 65535, "ndp_world_step_render: n=%lld outside 1..65535", (long long)n);
  NDP_CHECK_ARG(state_out != state_in, "ndp_world_step_render: state_out aliases state_in");
  NDP_CHECK_ARG(((uintptr_t)frames_hwc & 3) == 0, "ndp_world_step_render: frames_hwc must be 4-byte aligned");
  WorldArgs a{state_in, actions, state_out, frames_hwc, size};
  const unsigned gx = frames_hwc ? (unsigned)((size * size / world::kSpan + world::kBlock - 1) / world::kBlock) : 1u;
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_world_step_render", st);
  hipLaunchKernelGGL(k_world_step_render, dim3(gx, (unsigned)n), dim3(world::kBlock), 0, st, a);
  return check_launch("k_world_step_render");
}

int ndp_world_render(const float* state, int64_t n, int size, uint8_t* frames_hwc, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(state && frames_hwc, "ndp_world_render: null pointer");
  NDP_CHECK_ARG(world_size_ok(size), "ndp_world_render: size=%d is not a multiple of 4 in 32..1024", size);
  NDP_CHECK_ARG(n >= 1 && n <= 65535, "ndp_world_render: n=%lld outside 1..65535", (long long)n);
  NDP_CHECK_ARG(((uintptr_t)frames_hwc & 3) == 0, "ndp_world_render: frames_hwc must be 4-byte aligned");
  WorldArgs a{state, nullptr, nullptr, frames_hwc, size};
  const unsigned gx = (unsigned)((size * size / world::kSpan + world::kBlock - 1) / world::kBlock);
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_world_render", st);
  hipLaunchKernelGGL(k_world_render, dim3(gx, (unsigned)n), dim3(world::kBlock), 0, st, a);
  return check_launch("k_world_render");
}

}  // extern "C"
