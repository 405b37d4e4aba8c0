// fm_rollout.inc -- the rollout link kernels and the gradient sum (k_fm_rollout_begin, k_fm_rollout_advance,
// k_fm_rollout_loss_final, k_fm_rollout_chain, k_fm_grad_sum; csrc/ndp_forward_model.inc) run on the CPU, for
// tests/test_fm_rollout_host.py.  main.hip includes it behind the library's source (see there); it calls the __host__
// __device__ functions the kernels call (ndp::fm_rollout) by the kernels' schedule: workgroups of 256 threads, one
// thread per four neighbouring pixels (begin, advance) or per float4 (chain, gradient sum), the block's fixed tree over
// its threads' fp64 sums "in LDS", then the one workgroup of the final pass.  What the kernels do outside those
// functions -- the grid, the bounds checks, the tree's loop -- is restated here and tested as a copy; a slip in the
// device's own form of those is seen only by the GPU tests (tests/test_gpu_forward_rollout.py).  It makes no HIP runtime
// call and needs no GPU.
//
// Usage: host_driver fm_rollout IN OUT
//   IN   int32 cases, then per case 8 int32 (kind, n, steps, step, target_u8, stride, count, floats) and
//        kind 0 begin         frames ((n - 1) * stride + 49,152 floats or bytes)
//        kind 1 advance       state, resid (n x 49,152 floats each), target (as frames), loss, loss_sum (one float each)
//        kind 2 chain         local, g_next, d_cur (n x 49,152 floats each); g is written in local's place
//        kind 3 gradient sum  grads ((count - 1) * stride + floats floats)
//   OUT  per case  0: state;  1: state_next, local_next, the blocks' sums (n x 16 doubles), step_losses [steps] floats
//        (the sentinel -7 where not written), loss, loss_sum;  2: g;  3: out [floats]
// Every buffer -- inputs, outputs, each LDS array -- is an allocation of exactly its size, so a sanitizer sees any access
// past it.
namespace host::fm_rollout {

using namespace ndp::fm_rollout;
using ndp::kThreads;

template <class T>
using Exact = host::Exact<T, 16>;                                       // (16-byte accesses)

struct Case {
  int32_t kind, n, steps, step, target_u8, stride, count, floats;
};

void fill_lut(float* lut) {
  for (int i = 0; i < 256; ++i) lut[i] = norm_u8(i);
}

// k_fm_rollout_begin
void run_begin(const LinkArgs& a, int64_t n) {
  Exact<float> lut(256);
  fill_lut(lut.p);
  for (int64_t b = 0; b < link_blocks(n); ++b)
    for (int t = 0; t < kThreads; ++t) {
      const int64_t q = b * kThreads + t;
      if (q < a.nquads) begin_thread(a, q, lut.p);
    }
}

// k_fm_rollout_advance, then k_fm_rollout_loss_final
void run_advance(const LinkArgs& a, int64_t n, int step, int steps, float* step_losses, float* loss, float* loss_sum) {
  Exact<float> lut(256);
  fill_lut(lut.p);
  const int64_t blocks = link_blocks(n);
  for (int64_t b = 0; b < blocks; ++b) {
    Exact<double> red(kThreads);
    for (int t = 0; t < kThreads; ++t) {
      const int64_t q = b * kThreads + t;
      red.p[t] = q < a.nquads ? advance_thread(a, q, lut.p) : 0.0;
    }
    for (int w = kThreads / 2; w > 0; w >>= 1)
      for (int t = 0; t < w; ++t) tree_step(red.p, w, t);
    a.partial[b] = red.p[0];
  }
  Exact<double> red(kThreads);
  for (int t = 0; t < kThreads; ++t) red.p[t] = final_share(a.partial, blocks, t);
  final_write(red.p, n * (int64_t)kValues, step, steps, step_losses, loss, loss_sum);
}

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  static_assert(kQuads == 4096 && kBlocksPerImage == 16 && kValues == 49152, "the schedule");
  int32_t cases = 0;
  if (!read_pod(in, &cases) || cases < 0) return kBadInput;
  for (int32_t ci = 0; ci < cases; ++ci) {
    Case c;
    if (!read_pod(in, &c)) return kBadInput;
    if (c.kind < 0 || c.kind > 3 || c.n < 1) return kBadInput;
    const size_t values = (size_t)c.n * kValues;
    if (c.kind == 0 || c.kind == 1) {
      if (c.stride < kValues || c.stride % 4 != 0) return kBadInput;
      const size_t frame_elems = (size_t)(c.n - 1) * c.stride + kValues;
      Exact<float> tf(c.target_u8 ? 0 : frame_elems);
      Exact<unsigned char> t8(c.target_u8 ? frame_elems : 0);
      LinkArgs a;
      memset(&a, 0, sizeof(a));
      a.target_u8 = c.target_u8; a.stride = c.stride; a.nquads = (int64_t)c.n * kQuads;
      a.target = c.target_u8 ? static_cast<const void*>(t8.p) : static_cast<const void*>(tf.p);
      if (c.kind == 0) {
        if (!tf.read(in) || !t8.read(in)) return kBadInput;
        Exact<float> state(values);
        a.state_next = state.p;
        run_begin(a, c.n);
        if (!state.write(out)) return kBadInput;
      } else {
        if (c.steps < 1 || c.step < 0 || c.step >= c.steps) return kBadInput;
        Exact<float> state(values), resid(values), state_next(values), local_next(values), step_losses((size_t)c.steps);
        Exact<float> loss(1), loss_sum(1);
        Exact<double> partial((size_t)link_blocks(c.n));
        if (!state.read(in) || !resid.read(in) || !tf.read(in) || !t8.read(in) || !loss.read(in) || !loss_sum.read(in)) return kBadInput;
        step_losses.fill(-7.0f);
        a.state = state.p; a.resid = resid.p; a.state_next = state_next.p; a.local_next = local_next.p; a.partial = partial.p;
        a.scale = loss_scale(c.n, c.steps);
        run_advance(a, c.n, c.step, c.steps, step_losses.p, loss.p, loss_sum.p);
        if (!state_next.write(out) || !local_next.write(out) || !partial.write(out) || !step_losses.write(out) ||
            !loss.write(out) || !loss_sum.write(out))
          return kBadInput;
      }
    } else if (c.kind == 2) {
      Exact<float> local(values), g_next(values), d_cur(values);
      if (!local.read(in) || !g_next.read(in) || !d_cur.read(in)) return kBadInput;
      const int64_t n4 = (int64_t)values / 4;                           // k_fm_rollout_chain
      for (int64_t b = 0; b < (n4 + kThreads - 1) / kThreads; ++b)
        for (int t = 0; t < kThreads; ++t) {
          const int64_t i = b * kThreads + t;
          if (i < n4) chain_quad(local.p, g_next.p, d_cur.p, local.p, i);
        }
      if (!local.write(out)) return kBadInput;
    } else {
      if (c.count < 1 || c.floats < 1 || c.stride % 4 != 0 || (c.count > 1 && c.stride < c.floats)) return kBadInput;
      Exact<float> grads((size_t)(c.count - 1) * c.stride + c.floats), sum((size_t)c.floats);
      if (!grads.read(in)) return kBadInput;
      const int64_t threads = sum_threads(c.floats);                    // k_fm_grad_sum
      for (int64_t b = 0; b < (threads + kThreads - 1) / kThreads; ++b)
        for (int t = 0; t < kThreads; ++t) {
          const int64_t i = b * kThreads + t;
          if (i < threads) sum_thread(grads.p, c.stride, c.count, c.floats, sum.p, i);
        }
      if (!sum.write(out)) return kBadInput;
    }
  }
  return close_files(in, out);
}

}  // namespace host::fm_rollout
