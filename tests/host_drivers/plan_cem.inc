// plan_cem.inc -- the planner's cross-entropy update (k_plan_cem_update, csrc/ndp_plan.inc) run on the CPU, for
// tests/test_plan_cem_host.py.  main.hip includes it behind the library's source (see there); it calls the __host__
// __device__ functions the kernel calls
// (ndp::plan::rank_of, refit, sample, best_of, seq_index) by the kernel's schedule, thread by thread: the errors staged
// "in LDS", every thread's rank, the refit of component d by thread d, then the walk over the (ts, rollout) pairs.  What
// k_plan_cem_update does outside those functions -- the loops, the barriers' phases, the count of the non-NaN errors --
// is restated here and tested as a copy; a slip in the device's own form of those is seen only by the GPU tests
// (tests/test_gpu_plan_cem.py).  It makes no HIP runtime call and needs no GPU.
//
// Usage: host_driver plan_cem IN OUT
//   IN   int32 cases, then per case 6 int32 (B, R, E, Th, first, elite_idx wanted), 2 floats (momentum, min_std), low[4],
//        high[4], err [B,R], seq_in [Th,B,R,4], normal [Th,B,R,4], mean [B,Th,4], std [B,Th,4], best_err [B]
//   OUT  per case mean, std [B,Th,4], seq_out [Th,B,R,4], best_err [B], elite_idx [B,E] int32 (-7 where not wanted)
// Every buffer -- inputs, outputs, each LDS array -- is an allocation of exactly its size (exact.h; the 16-byte operands
// aligned to 16), so a sanitizer sees any access past it.
namespace host::plan_cem {

using namespace ndp::plan;

// k_plan_cem_update for the workgroup of trajectory b
void update_block(const ndp::PlanCemArgs& a, int64_t b) {
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
  for (int t = 0; t < kBlock; ++t) {                                 // the refit
    if (t < D) {
      float m = 0.f, s = 0.f;
      if (!a.first) { m = a.mean[b * D + t]; s = a.std[b * D + t]; }
      refit(a.seq_in, a.n_traj, R, b, t / kActionDim, t % kActionDim, order_s.p, ne, a.first, a.momentum, a.min_std, &m, &s);
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

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  int32_t cases = 0;
  if (!read_pod(in, &cases) || cases < 0) return kBadInput;
  for (int32_t ci = 0; ci < cases; ++ci) {
    int32_t h[6];
    float f[2], low[4], high[4];
    if (!read_pod(in, &h) || !read_pod(in, &f) || !read_pod(in, &low) || !read_pod(in, &high)) return kBadInput;
    const int B = h[0], R = h[1], E = h[2], Th = h[3], first = h[4];
    if (B < 1 || B > 65535 || R < 2 || R > NDP_MAX_SAMPLES || E < 1 || E > R || Th < 1 || Th > kMaxSteps) return kBadInput;
    if ((first != 0 && first != 1) || !(f[0] >= 0.f && f[0] < 1.f) || !(f[1] >= 0.f)) return kBadInput;
    const size_t rows = (size_t)B * R, flat = (size_t)Th * rows * kActionDim, fit = (size_t)B * Th * kActionDim;
    Exact<float> err(rows), mean(fit), std(fit), best(B);
    Exact<float, 16> seq_in(flat), normal(flat), seq_out(flat);
    if (!err.read(in) || !seq_in.read(in) || !normal.read(in) || !mean.read(in) || !std.read(in) || !best.read(in))
      return kBadInput;
    Exact<int32_t> elite_idx(h[5] ? (size_t)B * E : 0);
    seq_out.fill(-7.0f);
    ndp::PlanCemArgs a{err.p, seq_in.p, normal.p, B, R, Th, E, first, f[0], f[1], {}, {},
                       mean.p, std.p, seq_out.p, best.p, elite_idx.p};
    for (int c = 0; c < 4; ++c) {
      if (!(low[c] <= high[c])) return kBadInput;
      a.low[c] = low[c];
      a.high[c] = high[c];
    }
    for (int64_t b = 0; b < B; ++b) update_block(a, b);
    if (!mean.write(out) || !std.write(out) || !seq_out.write(out) || !best.write(out)) return kBadInput;
    if (elite_idx.p) {
      if (!elite_idx.write(out)) return kBadInput;
    } else {
      Exact<int32_t> s((size_t)B * E);
      s.fill(-7);
      if (!s.write(out)) return kBadInput;
    }
  }
  return close_files(in, out);
}

}  // namespace host::plan_cem
