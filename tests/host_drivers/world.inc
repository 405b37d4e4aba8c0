// world.inc -- the push world's two kernels (k_world_step_render, k_world_render, csrc/ndp_world.inc) run on the CPU,
// for tests/test_world_host.py.  main.hip includes it behind the library's source (see there); it calls the __host__
// __device__ functions the kernels call
// (ndp::world::step, quantise, span_begin, span_finish, pixel_offset) by the kernels' schedule, workgroup by workgroup
// and thread by thread: every thread below S*S/4 finds its span and the table under it, thread 0 advances the state and
// quantises the scene "in LDS", workgroup 0 of an environment writes state_out, every live thread lays the layers over
// its four pixels and stores its 12 bytes.  What the kernels do outside those
// functions -- the thread's span index, the bound on it, the three word stores -- is restated here and tested as a copy; a
// slip in the device's own form of those is seen only by the GPU tests (tests/test_gpu_push_world.py).  It makes no HIP
// runtime call and needs no GPU.
//
// Usage: host_driver world IN OUT
//   IN   int32 runs, then per run 3 int32 (n, S, with_frames), state_in [n,8], actions [n,4]
//   OUT  per run state_out [n,8], with_frames: the frames of the step [n,S,S,3]; then the frames k_world_render draws of
//        state_in [n,S,S,3]
// Every buffer -- inputs, outputs, each LDS object -- is an allocation of exactly its size (exact.h), so a sanitizer sees
// any access past it.
namespace host::world {

using namespace ndp::world;

// what every thread of workgroup (bx, env) does in front of the barrier (world_span): live[t] and its span
void begin_block(const ndp::WorldArgs& a, int bx, Span* spans, bool* live) {
  for (int t = 0; t < kBlock; ++t) {
    const int idx = bx * kBlock + t;
    live[t] = a.frames != nullptr && idx < a.size * a.size / kSpan;
    if (live[t]) span_begin(idx, a.size, spans + t);
  }
}

// ... and behind it (world_store), scene in "LDS"
void store_block(const ndp::WorldArgs& a, int64_t env, const Scene* scene_s, Span* spans, const bool* live) {
  for (int t = 0; t < kBlock; ++t) {
    if (!live[t]) continue;
    const Scene sc = *scene_s;
    uint32_t w[3];
    span_finish(sc, spans[t], w);
    uint8_t* dst = a.frames + pixel_offset(env, a.size, spans[t].px0, spans[t].py);
    if (((uintptr_t)dst & 3) != 0) abort();                          // the device stores words
    memcpy(dst, w, sizeof(w));
  }
}

// k_world_step_render for workgroup (bx, env)
void step_block(const ndp::WorldArgs& a, int bx, int64_t env) {
  Exact<float> state_s(8);
  Exact<Scene> scene_s(1);
  Exact<Span> spans(kBlock);                                         // the threads' registers
  Exact<bool> live(kBlock);
  begin_block(a, bx, spans.p, live.p);
  step(a.state_in + env * 8, a.actions + env * 4, state_s.p);        // thread 0, up to the barrier
  quantise(state_s.p, a.size, scene_s.p);
  for (int t = 0; t < kBlock; ++t)
    if (bx == 0 && t < 8) a.state_out[env * 8 + t] = state_s.p[t];
  store_block(a, env, scene_s.p, spans.p, live.p);
}

// k_world_render for workgroup (bx, env)
void render_block(const ndp::WorldArgs& a, int bx, int64_t env) {
  Exact<Scene> scene_s(1);
  Exact<Span> spans(kBlock);
  Exact<bool> live(kBlock);
  begin_block(a, bx, spans.p, live.p);
  quantise(a.state_in + env * 8, a.size, scene_s.p);
  store_block(a, env, scene_s.p, spans.p, live.p);
}

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  int32_t runs = 0;
  if (!read_pod(in, &runs) || runs < 0) return kBadInput;
  for (int32_t ri = 0; ri < runs; ++ri) {
    int32_t h[3];
    if (!read_pod(in, &h)) return kBadInput;
    const int n = h[0], size = h[1], with_frames = h[2];
    if (n < 1 || n > 64 || !ndp::world_size_ok(size) || (with_frames != 0 && with_frames != 1)) return kBadInput;
    const size_t bytes = (size_t)n * size * size * 3;
    Exact<float> state_in((size_t)n * 8), actions((size_t)n * 4), state_out((size_t)n * 8);
    if (!state_in.read(in) || !actions.read(in)) return kBadInput;
    Exact<uint8_t, 4> step_frames(with_frames ? bytes : 0), render_frames(bytes);
    state_out.fill(-7.0f);
    step_frames.fill(7);
    render_frames.fill(7);
    const int blocks = (size * size / kSpan + kBlock - 1) / kBlock;
    ndp::WorldArgs a{state_in.p, actions.p, state_out.p, step_frames.p, size};
    for (int64_t env = 0; env < n; ++env)
      for (int bx = 0; bx < (with_frames ? blocks : 1); ++bx) step_block(a, bx, env);
    ndp::WorldArgs r{state_in.p, nullptr, nullptr, render_frames.p, size};
    for (int64_t env = 0; env < n; ++env)
      for (int bx = 0; bx < blocks; ++bx) render_block(r, bx, env);
    if (!state_out.write(out) || !step_frames.write(out) || !render_frames.write(out)) return kBadInput;
  }
  return close_files(in, out);
}

}  // namespace host::world
