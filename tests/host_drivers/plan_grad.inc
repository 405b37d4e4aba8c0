// plan_grad.inc -- the three launches of the planner's gradient stage (k_plan_goal_grad, k_plan_grad_gather,
// k_plan_grad_step, csrc/ndp_plan.inc) run on the CPU, for tests/test_plan_grad_host.py.  plan_grad_main.hip includes it
// behind the library's source; it calls the __host__ __device__ functions the kernels call (ndp::plan::goal_elem, sq_acc,
// tree_step, goal_mean, rank_of, gather_pair, step_row, pow_steps) by the kernels' schedules, thread by thread: for the
// goal launch every chunk's loads, stores and LDS writes by thread, then every thread's eight sums behind the barrier, the
// two LDS buffers in turn, the tree in the first of them; for the gather launch the staged errors, every thread's rank,
// src / dst by threads < G, the walk over the (ts, g) pairs; for the step launch every thread of every block, the guard on
// the row count included.  What the kernels do outside those functions -- the loops, the barriers' phases, the guards -- is
// restated here and tested as a copy; a slip in the device's own form of those is seen only by the GPU tests
// (tests/test_gpu_plan_grad.py).  It makes no HIP runtime call and needs no GPU.
//
// Usage: host_driver plan_grad IN OUT     (the program of plan_grad_main.hip)
//   IN   int32 goal cases, then per case 4 int32 (n, n_goal, rows_per_goal, in place), pred [n,V], goal [n_goal,V] with
//        V = 49152; int32 gather cases, then per case 4 int32 (B, R, G, Th), err [B,R], seq [Th,B,R,4]; int32 step cases,
//        then per case 7 int32 (B, R, G, Th, t, optimizer, dst given), 4 floats (lr, beta1, beta2, eps), low[4], high[4],
//        grad, seq_g, m, v [Th,B,G,4], err_g [B,G] and, with dst, dst [B,G] int32 and seq_full [Th,B,R,4]
//   OUT  per goal case err [n], d_pred [n,V]; per gather case src, dst [B,G] int32, seq_g, m, v [Th,B,G,4]; per step case
//        seq_g, m, v [Th,B,G,4], curve [B,G] and, with dst, seq_full [Th,B,R,4]
// Every buffer -- inputs, outputs, each LDS array -- is an allocation of exactly its size (exact.h; the 16-byte operands
// aligned to 16), so a sanitizer sees any access past it.
namespace host::plan_grad {

using namespace ndp::plan;

// k_plan_goal_grad for the workgroup that takes `row`
void goal_block(const float* pred, const float* goal, int rows_per_goal, float c, float* err, float* d_pred, int64_t row) {
  Exact<double> diff0(kGoalChunk), diff1(kGoalChunk), sum(kBlock);
  const float* x = pred + row * kImageValues;
  const float* y = goal + (row / rows_per_goal) * kImageValues;
  float* o = d_pred + row * kImageValues;
  sum.fill(0.0);
  for (int chunk = 0; chunk < kImageValues / kGoalChunk; ++chunk) {
    double* buf = (chunk & 1) ? diff1.p : diff0.p;
    for (int t = 0; t < kBlock; ++t) {                               // up to the barrier
      float p[2][4], g[2][4];
      for (int h = 0; h < 2; ++h) {
        const int at = chunk * kGoalChunk + h * (kGoalChunk / 2) + 4 * t;
        memcpy(p[h], x + at, sizeof(p[h]));
        memcpy(g[h], y + at, sizeof(g[h]));
      }
      for (int h = 0; h < 2; ++h) {
        const int in = h * (kGoalChunk / 2) + 4 * t;
        float d[4];
        for (int j = 0; j < 4; ++j) buf[in + j] = goal_elem(p[h][j], g[h][j], c, &d[j]);
        memcpy(o + chunk * kGoalChunk + in, d, sizeof(d));
      }
    }
    for (int t = 0; t < kBlock; ++t)
      for (int k = 0; k < kGoalSlots; ++k) sum.p[t] = sq_acc(sum.p[t], buf[t + k * kBlock]);
  }
  double* red = diff0.p;
  for (int t = 0; t < kBlock; ++t) red[t] = sum.p[t];
  for (int w = kBlock / 2; w > 0; w >>= 1)
    for (int t = 0; t < kBlock; ++t)
      if (t < w) tree_step(red, t, w);
  err[row] = goal_mean(red[0]);
}

int run_goal(FILE* in, FILE* out) {
  int32_t h[4];
  if (!read_pod(in, &h)) return kBadInput;
  const int n = h[0], n_goal = h[1], rpg = h[2], inplace = h[3];
  if (n < 1 || n > 64 || n_goal < 1 || n_goal > 64 || rpg < 1 || (n - 1) / rpg >= n_goal || (inplace != 0 && inplace != 1))
    return kBadInput;
  Exact<float, 16> pred((size_t)n * kImageValues), goal((size_t)n_goal * kImageValues);
  Exact<float, 16> apart(inplace ? 0 : (size_t)n * kImageValues);
  Exact<float> err(n);
  if (!pred.read(in) || !goal.read(in)) return kBadInput;
  float* d_pred = inplace ? pred.p : apart.p;
  if (!inplace) apart.fill(-7.0f);
  err.fill(-7.0f);
  const float c = (float)(2.0 / (double)kImageValues);               // ndp_plan_goal_grad's
  for (int64_t k = 0; k < goal_grid(n, rpg); ++k) {                   // ndp_plan_goal_grad's grid and the kernel's guard
    const int64_t row = goal_row(k, n, rpg);
    if (row < n) goal_block(pred.p, goal.p, rpg, c, err.p, d_pred, row);
  }
  if (!err.write(out) || fwrite(d_pred, sizeof(float), (size_t)n * kImageValues, out) != (size_t)n * kImageValues)
    return kBadInput;
  return 0;
}

// k_plan_grad_gather for the workgroup of trajectory b
void gather_block(const ndp::PlanGatherArgs& a, int64_t b) {
  const int R = a.rollouts, G = a.rows;
  Exact<float> err_s(R);
  Exact<int> order_s(R);
  for (int t = 0; t < kBlock; ++t)
    if (t < R) err_s.p[t] = a.err[b * R + t];
  for (int t = 0; t < kBlock; ++t)
    if (t < R) order_s.p[rank_of(err_s.p, R, t)] = t;
  for (int t = 0; t < kBlock; ++t) {
    if (t < G) {
      a.src[b * G + t] = order_s.p[t];
      a.dst[b * G + t] = order_s.p[R - G + t];
    }
    for (int i = t; i < a.steps * G; i += kBlock) gather_pair(a, b, i, order_s.p);
  }
}

int run_gather(FILE* in, FILE* out) {
  int32_t h[4];
  if (!read_pod(in, &h)) return kBadInput;
  const int B = h[0], R = h[1], G = h[2], Th = h[3];
  if (B < 1 || B > 65535 || R < 2 || R > NDP_MAX_SAMPLES || G < 1 || G > R / 2 || Th < 1 || Th > kMaxSteps) return kBadInput;
  const size_t small = (size_t)Th * B * G * kActionDim;
  Exact<float> err((size_t)B * R);
  Exact<float, 16> seq((size_t)Th * B * R * kActionDim), seq_g(small), m(small), v(small);
  Exact<int32_t> src((size_t)B * G), dst((size_t)B * G);
  if (!err.read(in) || !seq.read(in)) return kBadInput;
  seq_g.fill(-7.0f);
  m.fill(-7.0f);
  v.fill(-7.0f);
  src.fill(-7);
  dst.fill(-7);
  const ndp::PlanGatherArgs a{err.p, seq.p, B, R, Th, G, src.p, dst.p, seq_g.p, m.p, v.p};
  for (int64_t b = 0; b < B; ++b) gather_block(a, b);
  if (!src.write(out) || !dst.write(out) || !seq_g.write(out) || !m.write(out) || !v.write(out)) return kBadInput;
  return 0;
}

int run_step(FILE* in, FILE* out) {
  int32_t h[7];
  float f[4];
  ndp::PlanStepArgs a{};
  if (!read_pod(in, &h) || !read_pod(in, &f)) return kBadInput;
  if (fread(a.low, sizeof(float), 4, in) != 4 || fread(a.high, sizeof(float), 4, in) != 4) return kBadInput;
  const int B = h[0], R = h[1], G = h[2], Th = h[3], t = h[4], optimizer = h[5], with_dst = h[6];
  if (B < 1 || B > 65535 || G < 1 || G > NDP_MAX_SAMPLES / 2 || R < 2 * G || R > NDP_MAX_SAMPLES || Th < 1 || Th > kMaxSteps ||
      t < 1 || t > 65535 || (optimizer != NDP_PLAN_SGD && optimizer != NDP_PLAN_ADAM) || (with_dst != 0 && with_dst != 1))
    return kBadInput;
  for (int c = 0; c < 4; ++c)
    if (!(a.low[c] <= a.high[c])) return kBadInput;
  if (!(f[0] > 0.f && f[0] < INFINITY) || !(f[1] >= 0.f && f[1] < 1.f) || !(f[2] >= 0.f && f[2] < 1.f) ||
      !(f[3] >= 0.f && f[3] < INFINITY))
    return kBadInput;
  const size_t small = (size_t)Th * B * G * kActionDim, full = with_dst ? (size_t)Th * B * R * kActionDim : 0;
  Exact<float, 16> grad(small), seq_g(small), m(small), v(small), seq_full(full);
  Exact<float> err_g((size_t)B * G), curve((size_t)B * G);
  Exact<int32_t> dst(with_dst ? (size_t)B * G : 0);
  if (!grad.read(in) || !seq_g.read(in) || !m.read(in) || !v.read(in) || !err_g.read(in) || !dst.read(in) ||
      !seq_full.read(in))
    return kBadInput;
  for (size_t i = 0; i < dst.n; ++i)
    if (dst.p[i] < 0 || dst.p[i] >= R) return kBadInput;
  curve.fill(-7.0f);
  const bool adam = optimizer == NDP_PLAN_ADAM;
  a.grad = grad.p; a.seq_g = seq_g.p; a.m = adam ? m.p : nullptr; a.v = adam ? v.p : nullptr; a.err_g = err_g.p;
  a.n_traj = B; a.rows = G; a.steps = Th; a.adam = adam ? 1 : 0;
  a.lr = (double)f[0]; a.beta1 = (double)f[1]; a.beta2 = (double)f[2]; a.eps = (double)f[3];
  a.corr1 = adam ? 1.0 - pow_steps(a.beta1, t) : 1.0;               // ndp_plan_grad_step's
  a.corr2 = adam ? 1.0 - pow_steps(a.beta2, t) : 1.0;
  a.curve_out = curve.p; a.dst = dst.p; a.seq_full = seq_full.p; a.rollouts = R;
  const int64_t n = (int64_t)B * G, blocks = (n + kBlock - 1) / kBlock;      // ndp_plan_grad_step's grid
  for (int64_t blk = 0; blk < blocks; ++blk)
    for (int th = 0; th < kBlock; ++th) {                            // k_plan_grad_step
      const int64_t i = blk * kBlock + th;
      if (i < a.n_traj * a.rows) step_row(a, i);
    }
  if (!seq_g.write(out) || !m.write(out) || !v.write(out) || !curve.write(out) || !seq_full.write(out)) return kBadInput;
  return 0;
}

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  for (int part = 0; part < 3; ++part) {
    int32_t cases = 0;
    if (!read_pod(in, &cases) || cases < 0) return kBadInput;
    for (int32_t ci = 0; ci < cases; ++ci) {
      const int rc = part == 0 ? run_goal(in, out) : part == 1 ? run_gather(in, out) : run_step(in, out);
      if (rc != 0) return rc;
    }
  }
  return close_files(in, out);
}

}  // namespace host::plan_grad
