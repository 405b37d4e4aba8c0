// plan_warm.inc -- the planner's update with its weighting and two flags (k_plan_update) and the warm-start launch
// (k_plan_warm, both csrc/ndp_plan.inc) run on the CPU, for tests/test_plan_warm_host.py.  plan_warm_main.hip includes it
// behind the library's source; it calls the __host__ __device__ functions the kernels call (ndp::plan::rank_of,
// mppi_weight, refit, refit_mppi, sample, best_of, seq_index, warm_row) by the kernels' schedules, thread by thread: the
// errors staged "in
// LDS", every thread's rank, with MPPI the weight of elite k by thread k into its LDS array, the refit of component d by
// thread d, the walk over the (ts, rollout) pairs; and for the warm launch every thread of every block, the guard on the
// row count included.  What the kernels do outside those functions -- the loops, the barriers' phases, the count of the
// non-NaN errors, the guard -- is restated here and tested as a copy; a slip in the device's own form of those is seen only
// by the GPU tests (tests/test_gpu_plan_warm.py).  It makes no HIP runtime call and needs no GPU.
//
// Usage: host_driver plan_warm IN OUT     (the program of plan_warm_main.hip)
//   IN   int32 update cases, then per case 7 int32 (B, R, E, Th, weighting, smooth, first), 3 floats (momentum, min_std,
//        temperature), low[4], high[4], err [B,R], seq_in [Th,B,R,4], normal [Th,B,R,4], mean [B,Th,4], std [B,Th,4],
//        best_err [B]; then int32 warm cases, then per case 4 int32 (B, W, steps_prev, steps), 1 float (warm_std), low[4],
//        high[4], mean_prev [B,steps_prev,4], std_prev [B,steps_prev,4], normal [steps,B,W,4]
//   OUT  per update case mean, std [B,Th,4], seq_out [Th,B,R,4], best_err [B], elite_idx [B,E] int32; per warm case mean,
//        std [B,steps,4], warm [steps,B,W,4]
// Every buffer -- inputs, outputs, each LDS array (the weights' holds E' doubles, what the kernel writes of its 256) -- is
// an allocation of exactly its size (exact.h; the 16-byte operands aligned to 16), so a sanitizer sees any access past it.
namespace host::plan_warm {

using namespace ndp::plan;

// k_plan_update<weighting> for the workgroup of trajectory b
void update_block(const ndp::PlanUpdateArgs& u, int weighting, int64_t b) {
  const ndp::PlanCemArgs& a = u.c;
  const int R = a.rollouts, D = a.steps * kActionDim;
  Exact<float> err_s(R), mean_s(D), std_s(D);
  Exact<int> order_s(R);
  int valid = 0;
  for (int t = 0; t < kBlock; ++t)                                   // up to the counting barrier
    if (t < R) {
      const float e = a.err[b * R + t];
      err_s.p[t] = e;
      valid += e == e;
    }
  for (int t = 0; t < kBlock; ++t)
    if (t < R) order_s.p[rank_of(err_s.p, R, t)] = t;
  const int ne = valid < a.elites ? valid : a.elites;
  const int fresh = !u.smooth;
  Exact<double> w_s(weighting == NDP_PLAN_MPPI ? ne : 0);
  if (weighting == NDP_PLAN_MPPI)
    for (int t = 0; t < kBlock; ++t)                                 // the weights, one per elite
      if (t < ne) w_s.p[t] = mppi_weight(err_s.p[order_s.p[t]], err_s.p[order_s.p[0]], u.temperature);
  for (int t = 0; t < kBlock; ++t) {                                 // the refit
    if (t < D) {
      float m = 0.f, s = 0.f;
      if (u.smooth) { m = a.mean[b * D + t]; s = a.std[b * D + t]; }
      const int ts = t / kActionDim, c = t % kActionDim;
      if (weighting == NDP_PLAN_MPPI)
        refit_mppi(a.seq_in, a.n_traj, R, b, ts, c, order_s.p, w_s.p, ne, fresh, a.momentum, a.min_std, &m, &s);
      else
        refit(a.seq_in, a.n_traj, R, b, ts, c, order_s.p, ne, fresh, a.momentum, a.min_std, &m, &s);
      mean_s.p[t] = m;
      std_s.p[t] = s;
      a.mean[b * D + t] = m;
      a.std[b * D + t] = s;
    }
    if (t == 0) a.best_err[b] = best_of(a.first ? 0.f : a.best_err[b], err_s.p[order_s.p[0]], a.first);
    if (a.elite_idx != nullptr && t < a.elites) a.elite_idx[b * a.elites + t] = t < ne ? order_s.p[t] : -1;
  }
  const int top = order_s.p[0];
  for (int t = 0; t < kBlock; ++t)                                   // the resampling
    for (int i = t; i < a.steps * R; i += kBlock) {
      const int ts = i / R, r = i % R;
      const int64_t at = seq_index(ts, b, r, 0, a.n_traj, R);
      float o[4];
      if (r == 0) {
        memcpy(o, a.seq_in + seq_index(ts, b, top, 0, a.n_traj, R), sizeof(o));
      } else {
        float n[4];
        memcpy(n, a.normal + at, sizeof(n));
        for (int c = 0; c < kActionDim; ++c)
          o[c] = sample(std_s.p[ts * kActionDim + c], n[c], mean_s.p[ts * kActionDim + c], a.low[c], a.high[c]);
      }
      memcpy(a.seq_out + at, o, sizeof(o));
    }
}

bool read_bounds(FILE* in, float* low, float* high) {
  if (fread(low, sizeof(float), 4, in) != 4 || fread(high, sizeof(float), 4, in) != 4) return false;
  for (int c = 0; c < 4; ++c)
    if (!(low[c] <= high[c])) return false;
  return true;
}

int run_update(FILE* in, FILE* out) {
  int32_t h[7];
  float f[3];
  ndp::PlanUpdateArgs u{};
  if (!read_pod(in, &h) || !read_pod(in, &f) || !read_bounds(in, u.c.low, u.c.high)) return kBadInput;
  const int B = h[0], R = h[1], E = h[2], Th = h[3], weighting = h[4], smooth = h[5], first = h[6];
  if (B < 1 || B > 65535 || R < 2 || R > NDP_MAX_SAMPLES || E < 1 || E > R || Th < 1 || Th > kMaxSteps) return kBadInput;
  if ((weighting != NDP_PLAN_ELITES && weighting != NDP_PLAN_MPPI) || (smooth != 0 && smooth != 1) ||
      (first != 0 && first != 1))
    return kBadInput;
  if (!(f[0] >= 0.f && f[0] < 1.f) || !(f[1] >= 0.f)) return kBadInput;
  if (weighting == NDP_PLAN_MPPI && !(f[2] > 0.f && f[2] < INFINITY)) return kBadInput;
  const size_t rows = (size_t)B * R, flat = (size_t)Th * rows * kActionDim, fit = (size_t)B * Th * kActionDim;
  Exact<float> err(rows), mean(fit), std(fit), best(B);
  Exact<float, 16> seq_in(flat), normal(flat), seq_out(flat);
  if (!err.read(in) || !seq_in.read(in) || !normal.read(in) || !mean.read(in) || !std.read(in) || !best.read(in))
    return kBadInput;
  Exact<int32_t> elite_idx((size_t)B * E);
  seq_out.fill(-7.0f);
  elite_idx.fill(-7);
  u.c.err = err.p; u.c.seq_in = seq_in.p; u.c.normal = normal.p;
  u.c.n_traj = B; u.c.rollouts = R; u.c.steps = Th; u.c.elites = E; u.c.first = first;
  u.c.momentum = f[0]; u.c.min_std = f[1];
  u.c.mean = mean.p; u.c.std = std.p; u.c.seq_out = seq_out.p; u.c.best_err = best.p; u.c.elite_idx = elite_idx.p;
  u.smooth = smooth;
  u.temperature = f[2];
  for (int64_t b = 0; b < B; ++b) update_block(u, weighting, b);
  if (!mean.write(out) || !std.write(out) || !seq_out.write(out) || !best.write(out) || !elite_idx.write(out))
    return kBadInput;
  return 0;
}

int run_warm(FILE* in, FILE* out) {
  int32_t h[4];
  float warm_std;
  ndp::PlanWarmArgs a{};
  if (!read_pod(in, &h) || !read_pod(in, &warm_std) || !read_bounds(in, a.low, a.high)) return kBadInput;
  const int B = h[0], W = h[1], Sp = h[2], S = h[3];
  if (B < 1 || B > 65535 || W < 1 || W > NDP_MAX_SAMPLES - 1 || Sp < 1 || Sp > kMaxSteps || S < 1 || S > Sp) return kBadInput;
  if (!(warm_std >= 0.f && warm_std < INFINITY)) return kBadInput;
  const size_t prev = (size_t)B * Sp * kActionDim, fit = (size_t)B * S * kActionDim, flat = (size_t)S * B * W * kActionDim;
  Exact<float, 16> mean_prev(prev), std_prev(prev), normal(flat), mean(fit), std(fit), warm(flat);
  if (!mean_prev.read(in) || !std_prev.read(in) || !normal.read(in)) return kBadInput;
  mean.fill(-7.0f);
  std.fill(-7.0f);
  warm.fill(-7.0f);
  a.mean_prev = mean_prev.p; a.std_prev = std_prev.p; a.normal = normal.p;
  a.n_traj = B; a.rows = W; a.steps_prev = Sp; a.steps = S; a.warm_std = warm_std;
  a.mean = mean.p; a.std = std.p; a.warm = warm.p;
  const int64_t n = (int64_t)S * B * W, blocks = (n + kBlock - 1) / kBlock;   // ndp_plan_warm's grid
  for (int64_t blk = 0; blk < blocks; ++blk)
    for (int t = 0; t < kBlock; ++t) {                               // k_plan_warm
      const int64_t i = blk * kBlock + t;
      if (i < (int64_t)a.steps * a.n_traj * a.rows) warm_row(a, i);
    }
  if (!mean.write(out) || !std.write(out) || !warm.write(out)) return kBadInput;
  return 0;
}

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  for (int part = 0; part < 2; ++part) {
    int32_t cases = 0;
    if (!read_pod(in, &cases) || cases < 0) return kBadInput;
    for (int32_t ci = 0; ci < cases; ++ci) {
      const int rc = part == 0 ? run_update(in, out) : run_warm(in, out);
      if (rc != 0) return rc;
    }
  }
  return close_files(in, out);
}

}  // namespace host::plan_warm
