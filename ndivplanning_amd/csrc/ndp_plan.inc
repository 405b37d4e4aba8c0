// ndp_plan.inc -- the planner's cross-entropy refinement (evaluation.py: mpc_plan / plan_step with `cem`):
//   k_plan_update      one iteration on a scored population of action sequences, seq [Th][B][R][4]: rank the R
//                      rollouts of a trajectory by their goal error, refit a diagonal Gaussian to the E best (equal
//                      weights: the cross-entropy method, ndp_plan_cem_update; or MPPI's exp(-(e - e_best) / temperature),
//                      ndp_plan_update), draw the next population from it (row 0 keeps the best sequence), keep the
//                      running minimum of the error
//   k_plan_warm        the previous planning step's fit shifted by one action: the next step's prior and its injected rows
//   k_normal_noise     standard normal draws, Box-Muller over ndp_uniform_noise's stream
// k_plan_update runs one workgroup of 256 threads per trajectory, in four phases separated by barriers:
//   1  thread r < R stages err[b][r] in LDS;
//   2  thread r < R counts the rollouts that beat it: its rank; order[rank] = r in LDS (a permutation: `beats` is a
//      strict total order).  A NaN error ranks behind every number; among equals and among NaNs the index decides;
//   3  thread d < D = 4 Th refits component d = 4 ts + c from the E' = min(E, non-NaN errors) best rows in rank order
//      (fp64 sums, population variance, fp64 sqrt, smoothing against the previous fit, floor, one rounding to fp32) and
//      leaves mean and std in LDS; thread 0 also updates best_err, threads < E write elite_idx;
//   4  thread i walks the (ts, r) pairs i, i + 256, ...: consecutive rollouts in consecutive lanes, one 16-byte load of
//      the normals and one 16-byte store; row 0 is the rank-0 sequence, copied.
// With MPPI weighting a phase 2b follows the ranking: thread k < E' leaves w_k in LDS once (256 doubles), and after one
// more barrier phase 3 sums with them in rank order; no component thread computes an exponential.
// The gradient stage of the planner (evaluation.py: `grad`, DESIGN.md section 5r) adds three launches:
//   k_plan_goal_grad   err and d err / d pred of every refined row against its goal image, one workgroup per row
//   k_plan_grad_gather the G best rows of a scored population gathered into seq_g [Th][B][G][4], their sources and the G
//                      worst rows' indices (the destinations), zeroed Adam moments
//   k_plan_grad_step   one SGD or Adam update of seq_g from the backward chain's action gradients, one thread per row
// Every sum has a fixed order, nothing is atomic, nothing spills: two calls give the same bits.  The arithmetic is in
// ndp::plan, __host__ __device__: tests/host_drivers/plan_cem.inc (a body of main.hip) and plan_warm.inc (the body of
// plan_warm_main.hip) run exactly these functions by this schedule on the CPU.  Included at the end of ndp_kernels.hip,
// after ndp_store.inc.

namespace ndp {
namespace plan {

constexpr int kBlock = 256;
constexpr int kActionDim = 4;
constexpr int kMaxSteps = 32;
constexpr int kMaxDim = kActionDim * kMaxSteps;

// does rollout i (error ei) come before rollout j (error ej)?  i != j.
__host__ __device__ inline bool beats(float ei, int i, float ej, int j) {
  const bool ni = ei != ei, nj = ej != ej;
  if (ni || nj) return ni == nj ? i < j : nj;
  return ei < ej || (ei == ej && i < j);
}

// the number of rollouts that come before rollout i: 0 is the best
__host__ __device__ inline int rank_of(const float* err, int rollouts, int i) {
  const float ei = err[i];
  int rank = 0;
  for (int j = 0; j < rollouts; ++j)
    if (j != i && beats(err[j], j, ei, i)) ++rank;
  return rank;
}

// element (ts, b, r, c) of a population [Th][B][R][4]
__host__ __device__ inline int64_t seq_index(int ts, int64_t b, int r, int c, int64_t n_traj, int rollouts) {
  return (((int64_t)ts * n_traj + b) * rollouts + r) * kActionDim + c;
}

// the fit (m, s) of one component smoothed against the previous one in *mean / *std (unless `first`), floored and rounded
__host__ __device__ inline void settle(double m, double s, int first, float momentum, float min_std, float* mean,
                                       float* std) {
#pragma clang fp contract(off)
  if (!first) {
    const double mo = (double)momentum, keep = 1.0 - mo;
    m = mo * (double)*mean + keep * m;
    s = mo * (double)*std + keep * s;
  }
  const double least = (double)min_std;
  s = s > least ? s : least;                            // a NaN deviation gives the floor
  *mean = (float)m;
  *std = (float)s;
}

// Component (ts, c) of trajectory b refitted to the rows order[0 .. ne): *mean and *std hold the previous fit on entry
// (unless `first`) and the new one on return.  ne == 0: they stay, or are 0 and min_std with `first`.
__host__ __device__ inline void refit(const float* seq, int64_t n_traj, int rollouts, int64_t b, int ts, int c,
                                      const int* order, int ne, int first, float momentum, float min_std, float* mean,
                                      float* std) {
#pragma clang fp contract(off)
  if (ne == 0) {
    if (first) { *mean = 0.f; *std = min_std; }
    return;
  }
  double sum = 0.0;
  for (int k = 0; k < ne; ++k) sum += (double)seq[seq_index(ts, b, order[k], c, n_traj, rollouts)];
  double m = sum / (double)ne;
  double dev = 0.0;
  for (int k = 0; k < ne; ++k) {
    const double d = (double)seq[seq_index(ts, b, order[k], c, n_traj, rollouts)] - m;
    dev += d * d;
  }
  settle(m, sqrt(dev / (double)ne), first, momentum, min_std, mean, std);
}

// MPPI's weight of the elite with error ek beside the best, e0 <= ek, neither a NaN: equal errors (two infinities too)
// weigh 1, an infinite ek beside a finite e0 weighs 0
__host__ __device__ inline double mppi_weight(float ek, float e0, float temperature) {
#pragma clang fp contract(off)
  if (ek == e0) return 1.0;
  return exp(-((double)ek - (double)e0) / (double)temperature);
}

// refit with the weights w[0 .. ne) of the rows order[0 .. ne), w[0] = 1: m = sum w x / W, s = sqrt(sum w (x - m)^2 / W),
// W = sum w >= 1, all in rank order; `first` and ne == 0 as in refit
__host__ __device__ inline void refit_mppi(const float* seq, int64_t n_traj, int rollouts, int64_t b, int ts, int c,
                                           const int* order, const double* w, int ne, int first, float momentum,
                                           float min_std, float* mean, float* std) {
#pragma clang fp contract(off)
  if (ne == 0) {
    if (first) { *mean = 0.f; *std = min_std; }
    return;
  }
  double total = 0.0, sum = 0.0;
  for (int k = 0; k < ne; ++k) {
    total += w[k];
    sum += w[k] * (double)seq[seq_index(ts, b, order[k], c, n_traj, rollouts)];
  }
  const double m = sum / total;
  double dev = 0.0;
  for (int k = 0; k < ne; ++k) {
    const double d = (double)seq[seq_index(ts, b, order[k], c, n_traj, rollouts)] - m;
    dev += w[k] * (d * d);
  }
  settle(m, sqrt(dev / total), first, momentum, min_std, mean, std);
}

// v clamped to [lo, hi]; a NaN stays NaN
__host__ __device__ inline float clamp_keep_nan(float v, float lo, float hi) {
  return v != v ? v : fminf(fmaxf(v, lo), hi);
}

// one resampled action component: std * n is exact in fp64, so the sum is rounded twice (fp64, then fp32) whether or
// not the two are contracted; clamped to [lo, hi], a NaN stays NaN
__host__ __device__ inline float sample(float std, float n, float mean, float lo, float hi) {
#pragma clang fp contract(off)
  return clamp_keep_nan((float)((double)std * (double)n + (double)mean), lo, hi);
}

// the deviation a planning step carries to the next: floored, a NaN gives the floor
__host__ __device__ inline float carried_std(float std_prev, float warm_std) {
  return std_prev > warm_std ? std_prev : warm_std;
}

// the horizon step of the previous fit that step ts of the next planning step continues
__host__ __device__ inline int warm_source(int ts, int steps_prev) { return ts + 1 < steps_prev ? ts + 1 : steps_prev - 1; }

// the running minimum of the rank-0 error: a NaN never replaces a number
__host__ __device__ inline float best_of(float old, float e, int first) {
  if (first) return e;
  return (e < old || old != old) ? e : old;
}

// ---- the gradient stage -------------------------------------------------------------------------------------------
constexpr int kImageValues = 3 * 128 * 128;               // one image row of ndp_plan_goal_grad
constexpr int kGoalChunk = 2048;                          // floats of a row between two barriers of k_plan_goal_grad
constexpr int kGoalSlots = kGoalChunk / kBlock;           // elements of a chunk that one thread's sum owns

// One element of ndp_plan_goal_grad: *d = (p - g) * c in fp32, two roundings; returns the fp64 difference whose square
// the row's error sums.  A NaN stays NaN.
__host__ __device__ inline double goal_elem(float p, float g, float c, float* d) {
#pragma clang fp contract(off)
  const float diff = p - g;
  *d = diff * c;
  return (double)p - (double)g;
}

// s + d * d with ONE rounding: what k_eval_pair_mse's `s += d * d` compiles to on the device, spelled out so that the
// host and the device agree
__host__ __device__ inline double sq_acc(double s, double d) { return fma(d, d, s); }

// k_eval_pair_mse's tree over the 256 threads' sums, then the mean rounded to fp32
__host__ __device__ inline void tree_step(double* red, int t, int w) { red[t] += red[t + w]; }
__host__ __device__ inline float goal_mean(double sum) { return (float)(sum / (double)kImageValues); }

// Which row workgroup k of k_plan_goal_grad takes.  Workgroups k and k + 8 share an XCD and its L2 (observed, for speed
// only), so the rows_per_goal rows of one goal go to workgroups 8 apart: the first of them brings the goal row into that
// L2 and the others read it there.  Goal j is served on residue j % 8; a k past the last row gives a row >= n_rows.
constexpr int kXcds = 8;
__host__ __device__ inline int64_t goal_group(int64_t n_rows, int rows_per_goal) {
  return rows_per_goal < n_rows ? rows_per_goal : n_rows;            // one goal for every row: one group
}
__host__ __device__ inline int64_t goal_row(int64_t k, int64_t n_rows, int rows_per_goal) {
  const int64_t group = goal_group(n_rows, rows_per_goal), lane = k % kXcds, slot = k / kXcds;
  return (lane + kXcds * (slot / group)) * group + slot % group;
}
// the workgroups that cover n_rows rows: fewer than n_rows + 8 * group
__host__ __device__ inline int64_t goal_grid(int64_t n_rows, int rows_per_goal) {
  const int64_t group = goal_group(n_rows, rows_per_goal), goals = (n_rows + group - 1) / group;
  return (goals + kXcds - 1) / kXcds * kXcds * group;
}

// beta^t by t roundings: the same double on the host, the device and in a restatement (pow need not be)
__host__ __device__ inline double pow_steps(double beta, int t) {
#pragma clang fp contract(off)
  double p = 1.0;
  for (int i = 0; i < t; ++i) p = p * beta;
  return p;
}

}  // namespace plan

struct PlanGatherArgs {
  const float* err; const float* seq;
  int64_t n_traj; int rollouts, steps, rows;
  int32_t* src; int32_t* dst; float* seq_g; float* m; float* v;
};

struct PlanStepArgs {
  const float* grad; float* seq_g; float* m; float* v; const float* err_g;
  int64_t n_traj; int rows, steps, adam;
  double lr, beta1, beta2, eps, corr1, corr2;             // corr = 1 - beta^t
  float low[4], high[4];
  float* curve_out; const int32_t* dst; float* seq_full; int rollouts;
};

namespace plan {

// Pair i = ts * G + g of trajectory b in k_plan_grad_gather: the rank-g row of the population into seq_g, zero moments
__host__ __device__ inline void gather_pair(const PlanGatherArgs& a, int64_t b, int i, const int* order) {
  const int ts = i / a.rows, g = i % a.rows;
  const int64_t to = seq_index(ts, b, g, 0, a.n_traj, a.rows);
  const float4 x = *reinterpret_cast<const float4*>(a.seq + seq_index(ts, b, order[g], 0, a.n_traj, a.rollouts));
  *reinterpret_cast<float4*>(a.seq_g + to) = x;
  const float4 zero = {0.f, 0.f, 0.f, 0.f};
  *reinterpret_cast<float4*>(a.m + to) = zero;
  *reinterpret_cast<float4*>(a.v + to) = zero;
}

__host__ __device__ inline bool finite_f(float x) { return x - x == 0.f; }

// one component of ndp_plan_grad_step, fp64 with every operation rounded on its own; *m and *v in/out (Adam only)
__host__ __device__ inline float step_component(const PlanStepArgs& a, float act, float grad, float* m, float* v, int c) {
#pragma clang fp contract(off)
  const double g = (double)grad;
  double next;
  if (a.adam) {
    const double keep1 = 1.0 - a.beta1, keep2 = 1.0 - a.beta2;
    const double gg = g * g;
    const double mn = a.beta1 * (double)*m + keep1 * g;
    const double vn = a.beta2 * (double)*v + keep2 * gg;
    const double mhat = mn / a.corr1, vhat = vn / a.corr2;
    const double denom = sqrt(vhat) + a.eps;
    const double move = (a.lr * mhat) / denom;
    next = (double)act - move;
    *m = (float)mn;
    *v = (float)vn;
  } else {
    const double move = a.lr * g;
    next = (double)act - move;
  }
  return clamp_keep_nan((float)next, a.low[c], a.high[c]);
}

// Row i = b * G + g of ndp_plan_grad_step: the row moves unless one of its Th * 4 gradient components is not finite
__host__ __device__ inline void step_row(const PlanStepArgs& a, int64_t i) {
  const int64_t b = i / a.rows;
  const int g = (int)(i % a.rows);
  bool ok = true;
  for (int ts = 0; ts < a.steps; ++ts) {
    const float4 d = *reinterpret_cast<const float4*>(a.grad + seq_index(ts, b, g, 0, a.n_traj, a.rows));
    ok = ok && finite_f(d.x) && finite_f(d.y) && finite_f(d.z) && finite_f(d.w);
  }
  if (a.curve_out != nullptr) a.curve_out[i] = a.err_g[i];
  int to = -1;
  if (a.dst != nullptr) {
    to = a.dst[i];
    if (to < 0 || to >= a.rollouts) to = -1;               // nothing is written through an index outside the population
  }
  for (int ts = 0; ts < a.steps; ++ts) {
    const int64_t at = seq_index(ts, b, g, 0, a.n_traj, a.rows);
    float4 x = *reinterpret_cast<const float4*>(a.seq_g + at);
    if (ok) {
      const float4 d = *reinterpret_cast<const float4*>(a.grad + at);
      float4 m = {0.f, 0.f, 0.f, 0.f}, v = m;
      if (a.adam) {
        m = *reinterpret_cast<const float4*>(a.m + at);
        v = *reinterpret_cast<const float4*>(a.v + at);
      }
      x.x = step_component(a, x.x, d.x, &m.x, &v.x, 0);
      x.y = step_component(a, x.y, d.y, &m.y, &v.y, 1);
      x.z = step_component(a, x.z, d.z, &m.z, &v.z, 2);
      x.w = step_component(a, x.w, d.w, &m.w, &v.w, 3);
      *reinterpret_cast<float4*>(a.seq_g + at) = x;
      if (a.adam) {
        *reinterpret_cast<float4*>(a.m + at) = m;
        *reinterpret_cast<float4*>(a.v + at) = v;
      }
    }
    if (to >= 0) *reinterpret_cast<float4*>(a.seq_full + seq_index(ts, b, to, 0, a.n_traj, a.rollouts)) = x;
  }
}

}  // namespace plan

struct PlanCemArgs {
  const float* err; const float* seq_in; const float* normal;
  int64_t n_traj; int rollouts, steps, elites, first;
  float momentum, min_std, low[4], high[4];
  float* mean; float* std; float* seq_out; float* best_err; int32_t* elite_idx;
};

// what ndp_plan_update adds to ndp_plan_cem_update's arguments; c.first: best_err is only written
struct PlanUpdateArgs {
  PlanCemArgs c;
  int smooth;                                             // the refit smooths against the mean / std it is given
  float temperature;                                      // kWeighting == NDP_PLAN_MPPI
};

template <int kWeighting>
__global__ __launch_bounds__(plan::kBlock) void k_plan_update(PlanUpdateArgs u) {
  using namespace plan;
  const PlanCemArgs& a = u.c;
  __shared__ float err_s[NDP_MAX_SAMPLES];
  __shared__ int order_s[NDP_MAX_SAMPLES];
  __shared__ float mean_s[kMaxDim], std_s[kMaxDim];
  __shared__ double w_s[kWeighting == NDP_PLAN_MPPI ? NDP_MAX_SAMPLES : 1];   // the elites' weights; unused without MPPI
  const int t = threadIdx.x, R = a.rollouts, D = a.steps * kActionDim;
  const int64_t b = blockIdx.x;
  float e = 0.f;
  if (t < R) { e = a.err[b * R + t]; err_s[t] = e; }
  const int valid = __syncthreads_count(t < R && e == e);
  if (t < R) order_s[rank_of(err_s, R, t)] = t;
  __syncthreads();
  const int ne = valid < a.elites ? valid : a.elites;
  const int fresh = !u.smooth;
  if constexpr (kWeighting == NDP_PLAN_MPPI) {
    if (t < ne) w_s[t] = mppi_weight(err_s[order_s[t]], err_s[order_s[0]], u.temperature);
    __syncthreads();
  }
  if (t < D) {
    float m = 0.f, s = 0.f;
    if (u.smooth) { m = a.mean[b * D + t]; s = a.std[b * D + t]; }
    const int ts = t / kActionDim, c = t % kActionDim;
    if constexpr (kWeighting == NDP_PLAN_MPPI)
      refit_mppi(a.seq_in, a.n_traj, R, b, ts, c, order_s, w_s, ne, fresh, a.momentum, a.min_std, &m, &s);
    else
      refit(a.seq_in, a.n_traj, R, b, ts, c, order_s, ne, fresh, a.momentum, a.min_std, &m, &s);
    mean_s[t] = m;
    std_s[t] = s;
    a.mean[b * D + t] = m;
    a.std[b * D + t] = s;
  }
  if (t == 0) a.best_err[b] = best_of(a.first ? 0.f : a.best_err[b], err_s[order_s[0]], a.first);
  if (a.elite_idx != nullptr && t < a.elites) a.elite_idx[b * a.elites + t] = t < ne ? order_s[t] : -1;
  __syncthreads();
  const int top = order_s[0];
  for (int i = t; i < a.steps * R; i += kBlock) {
    const int ts = i / R, r = i % R;
    const int64_t at = seq_index(ts, b, r, 0, a.n_traj, R);
    float4 o;
    if (r == 0) {
      o = *reinterpret_cast<const float4*>(a.seq_in + seq_index(ts, b, top, 0, a.n_traj, R));
    } else {
      const float4 n = *reinterpret_cast<const float4*>(a.normal + at);
      const float* mu = mean_s + ts * kActionDim;
      const float* sd = std_s + ts * kActionDim;
      o.x = sample(sd[0], n.x, mu[0], a.low[0], a.high[0]);
      o.y = sample(sd[1], n.y, mu[1], a.low[1], a.high[1]);
      o.z = sample(sd[2], n.z, mu[2], a.low[2], a.high[2]);
      o.w = sample(sd[3], n.w, mu[3], a.low[3], a.high[3]);
    }
    *reinterpret_cast<float4*>(a.seq_out + at) = o;
  }
}

struct PlanWarmArgs {
  const float* mean_prev; const float* std_prev; const float* normal;
  int64_t n_traj; int rows, steps_prev, steps;
  float warm_std, low[4], high[4];
  float* mean; float* std; float* warm;
};

namespace plan {

// Row i = (ts * B + b) * W + w of the warm launch: the fit of step warm_source(ts) of trajectory b, its deviation floored;
// w == 0 stores the carried mean and deviation and writes the clamped mean, every other row a draw around it.
__host__ __device__ inline void warm_row(const PlanWarmArgs& a, int64_t i) {
  const int w = (int)(i % a.rows);
  const int64_t b = i / a.rows % a.n_traj;
  const int ts = (int)(i / a.rows / a.n_traj);
  const int64_t from = (b * a.steps_prev + warm_source(ts, a.steps_prev)) * kActionDim;
  const float4 mu = *reinterpret_cast<const float4*>(a.mean_prev + from);
  float4 sd = *reinterpret_cast<const float4*>(a.std_prev + from);
  sd.x = carried_std(sd.x, a.warm_std);
  sd.y = carried_std(sd.y, a.warm_std);
  sd.z = carried_std(sd.z, a.warm_std);
  sd.w = carried_std(sd.w, a.warm_std);
  float4 o;
  if (w == 0) {
    const int64_t to = (b * a.steps + ts) * kActionDim;
    *reinterpret_cast<float4*>(a.mean + to) = mu;
    *reinterpret_cast<float4*>(a.std + to) = sd;
    o.x = clamp_keep_nan(mu.x, a.low[0], a.high[0]);
    o.y = clamp_keep_nan(mu.y, a.low[1], a.high[1]);
    o.z = clamp_keep_nan(mu.z, a.low[2], a.high[2]);
    o.w = clamp_keep_nan(mu.w, a.low[3], a.high[3]);
  } else {
    const float4 n = *reinterpret_cast<const float4*>(a.normal + i * kActionDim);
    o.x = sample(sd.x, n.x, mu.x, a.low[0], a.high[0]);
    o.y = sample(sd.y, n.y, mu.y, a.low[1], a.high[1]);
    o.z = sample(sd.z, n.z, mu.z, a.low[2], a.high[2]);
    o.w = sample(sd.w, n.w, mu.w, a.low[3], a.high[3]);
  }
  *reinterpret_cast<float4*>(a.warm + i * kActionDim) = o;
}

}  // namespace plan

// one thread per row of warm [Th][B][W][4]: consecutive rows in consecutive lanes, 16-byte loads and stores
__global__ __launch_bounds__(plan::kBlock) void k_plan_warm(PlanWarmArgs a) {
  const int64_t i = (int64_t)blockIdx.x * plan::kBlock + threadIdx.x;
  if (i < (int64_t)a.steps * a.n_traj * a.rows) plan::warm_row(a, i);
}

// One workgroup of 256 threads per row; a row is 24 chunks of 2048 floats.  Per chunk thread t loads pred and goal 16
// bytes at a time at floats 4t and 1024 + 4t, stores d_pred there, and leaves the 8 fp64 differences in LDS; after the
// barrier thread t adds the squares of the chunk's elements t, t + 256, ..., t + 1792 to its sum in that order -- so it
// sums the row's elements t, t + 256, ... as k_eval_pair_mse's thread t does, with the same fused multiply-add -- and the
// tree and the mean are that kernel's.  Two LDS buffers: one barrier per chunk.  Which workgroup takes which row
// (goal_row) keeps the rows of one goal on one XCD; the result does not depend on it.
__global__ __launch_bounds__(plan::kBlock) void k_plan_goal_grad(const float* pred, const float* goal, int64_t n_rows,
                                                                int rows_per_goal, float c, float* err, float* d_pred) {
  using namespace plan;
  __shared__ double diff_s[2][kGoalChunk];
  const int t = threadIdx.x;
  const int64_t row = goal_row(blockIdx.x, n_rows, rows_per_goal);
  if (row >= n_rows) return;                                // the whole workgroup: no barrier is left waiting
  const float* x = pred + row * kImageValues;
  const float* y = goal + (row / rows_per_goal) * kImageValues;
  float* o = d_pred + row * kImageValues;
  double s = 0.0;
  for (int chunk = 0; chunk < kImageValues / kGoalChunk; ++chunk) {
    double* buf = diff_s[chunk & 1];
    float4 p[2], g[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int at = chunk * kGoalChunk + h * (kGoalChunk / 2) + 4 * t;
      p[h] = *reinterpret_cast<const float4*>(x + at);
      g[h] = *reinterpret_cast<const float4*>(y + at);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int in = h * (kGoalChunk / 2) + 4 * t;
      float4 d;
      buf[in + 0] = goal_elem(p[h].x, g[h].x, c, &d.x);
      buf[in + 1] = goal_elem(p[h].y, g[h].y, c, &d.y);
      buf[in + 2] = goal_elem(p[h].z, g[h].z, c, &d.z);
      buf[in + 3] = goal_elem(p[h].w, g[h].w, c, &d.w);
      *reinterpret_cast<float4*>(o + chunk * kGoalChunk + in) = d;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kGoalSlots; ++k) s = sq_acc(s, buf[t + k * kBlock]);
  }
  double* red = diff_s[0];                                  // the last chunk (23) used buffer 1
  red[t] = s;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (t < w) tree_step(red, t, w);
    __syncthreads();
  }
  if (t == 0) err[row] = goal_mean(red[0]);
}

// One workgroup per trajectory: k_plan_update's phases 1 and 2 (errors staged, order[rank] = row), then threads < G write
// src and dst and the (ts, g) pairs are walked 256 at a time.
__global__ __launch_bounds__(plan::kBlock) void k_plan_grad_gather(PlanGatherArgs a) {
  using namespace plan;
  __shared__ float err_s[NDP_MAX_SAMPLES];
  __shared__ int order_s[NDP_MAX_SAMPLES];
  const int t = threadIdx.x, R = a.rollouts, G = a.rows;
  const int64_t b = blockIdx.x;
  if (t < R) err_s[t] = a.err[b * R + t];
  __syncthreads();
  if (t < R) order_s[rank_of(err_s, R, t)] = t;
  __syncthreads();
  if (t < G) {
    a.src[b * G + t] = order_s[t];
    a.dst[b * G + t] = order_s[R - G + t];
  }
  for (int i = t; i < a.steps * G; i += kBlock) gather_pair(a, b, i, order_s);
}

// one thread per row (b, g)
__global__ __launch_bounds__(plan::kBlock) void k_plan_grad_step(PlanStepArgs a) {
  const int64_t i = (int64_t)blockIdx.x * plan::kBlock + threadIdx.x;
  if (i < a.n_traj * a.rows) plan::step_row(a, i);
}

// Box-Muller on one Philox block: thread j owns uniforms 4j .. 4j+3 of the stream (seed, offset), the pairs 2j and
// 2j + 1, and writes out[4j .. 4j+3] (what lies below n of it).
__global__ __launch_bounds__(kThreads) void k_normal_noise(float* out, int64_t n, uint64_t seed, const int32_t* offset_dev,
                                                           int vec4) {
  const int64_t blk = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t at = blk * 4;
  if (at >= n) return;
  const uint32_t off = offset_dev != nullptr ? (uint32_t)*offset_dev : 0u;
  float v[4];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = philox_uniform((uint64_t)(at + 2 * p), seed, off);
    const float u2 = philox_uniform((uint64_t)(at + 2 * p + 1), seed, off);
    const float r = sqrtf(-2.0f * logf(1.0f - u1));
    const float ang = 6.283185307179586f * u2;
    v[2 * p] = r * cosf(ang);
    v[2 * p + 1] = r * sinf(ang);
  }
  if (vec4 && at + 4 <= n) {
    *reinterpret_cast<float4*>(out + at) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < 4 && at + k < n; ++k) out[at + k] = v[k];
  }
}

}  // namespace ndp

extern "C" {

// the checks and the launch behind ndp_plan_cem_update and ndp_plan_update; `who` names the entry point in messages,
// `label` the launch in the timing table
static int plan_update_launch(const char* who, const char* label, const float* err, const float* seq_in,
                              const float* normal, int64_t n_traj, int rollouts, int steps, int elites, int weighting, float temperature,
                              int smooth, int first, float momentum, float min_std, const float* low4, const float* high4,
                              float* mean, float* std, float* seq_out, float* best_err, int32_t* elite_idx, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(err && seq_in && normal && low4 && high4 && mean && std && seq_out && best_err, "%s: null pointer", who);
  NDP_CHECK_ARG(n_traj >= 1 && n_traj <= 65535, "%s: n_traj=%lld outside 1..65535", who, (long long)n_traj);
  NDP_CHECK_ARG(rollouts >= 2 && rollouts <= NDP_MAX_SAMPLES, "%s: rollouts=%d outside 2..%d", who, rollouts,
                NDP_MAX_SAMPLES);
  NDP_CHECK_ARG(elites >= 1 && elites <= rollouts, "%s: elites=%d outside 1..%d", who, elites, rollouts);
  NDP_CHECK_ARG(steps >= 1 && steps <= plan::kMaxSteps, "%s: steps=%d outside 1..%d", who, steps, plan::kMaxSteps);
  NDP_CHECK_ARG(first == 0 || first == 1, "%s: first must be 0 or 1", who);
  NDP_CHECK_ARG(smooth == 0 || smooth == 1, "%s: smooth must be 0 or 1", who);
  NDP_CHECK_ARG(weighting == NDP_PLAN_ELITES || weighting == NDP_PLAN_MPPI, "%s: weighting=%d is neither NDP_PLAN_ELITES "
                "nor NDP_PLAN_MPPI", who, weighting);
  NDP_CHECK_ARG(weighting != NDP_PLAN_MPPI || (temperature > 0.f && temperature < INFINITY),
                "%s: temperature=%g must be finite and > 0", who, (double)temperature);
  NDP_CHECK_ARG(momentum >= 0.f && momentum < 1.f, "%s: momentum=%g outside [0, 1)", who, (double)momentum);
  NDP_CHECK_ARG(min_std >= 0.f, "%s: min_std=%g must be >= 0", who, (double)min_std);
  for (int c = 0; c < 4; ++c)
    NDP_CHECK_ARG(low4[c] <= high4[c], "%s: low[%d]=%g above high[%d]=%g (or NaN)", who, c, (double)low4[c], c,
                  (double)high4[c]);
  NDP_CHECK_ARG(seq_out != seq_in && seq_out != normal, "%s: seq_out aliases seq_in or normal", who);
  NDP_CHECK_ARG(aligned16(seq_in) && aligned16(normal) && aligned16(seq_out),
                "%s: seq_in, normal and seq_out must be 16-byte aligned", who);
  PlanUpdateArgs u{{err, seq_in, normal, n_traj, rollouts, steps, elites, first, momentum, min_std, {}, {},
                    mean, std, seq_out, best_err, elite_idx}, smooth, temperature};
  for (int c = 0; c < 4; ++c) { u.c.low[c] = low4[c]; u.c.high[c] = high4[c]; }
  hipStream_t st = (hipStream_t)stream;
  KTimer kt(label, st);
  if (weighting == NDP_PLAN_MPPI)
    hipLaunchKernelGGL(k_plan_update<NDP_PLAN_MPPI>, dim3((unsigned)n_traj), dim3(plan::kBlock), 0, st, u);
  else
    hipLaunchKernelGGL(k_plan_update<NDP_PLAN_ELITES>, dim3((unsigned)n_traj), dim3(plan::kBlock), 0, st, u);
  return check_launch(label);
}

int ndp_plan_cem_update(const float* err, const float* seq_in, const float* normal, int64_t n_traj, int rollouts, int steps,
                        int elites, int first, float momentum, float min_std, const float* low4, const float* high4,
                        float* mean, float* std, float* seq_out, float* best_err, int32_t* elite_idx, void* stream) {
  return plan_update_launch("ndp_plan_cem_update", "k_plan_cem_update", err, seq_in, normal, n_traj, rollouts, steps,
                            elites, NDP_PLAN_ELITES, 0.f, first == 0, first, momentum, min_std, low4, high4, mean, std, seq_out,
                            best_err, elite_idx, stream);
}

int ndp_plan_update(const float* err, const float* seq_in, const float* normal, int64_t n_traj, int rollouts, int steps,
                    int elites, int weighting, float temperature, int smooth, int first, float momentum, float min_std,
                    const float* low4, const float* high4, float* mean, float* std, float* seq_out, float* best_err,
                    int32_t* elite_idx, void* stream) {
  return plan_update_launch("ndp_plan_update", "k_plan_update", err, seq_in, normal, n_traj, rollouts, steps, elites,
                            weighting, temperature, smooth, first, momentum, min_std, low4, high4, mean, std, seq_out,
                            best_err, elite_idx, stream);
}

int ndp_plan_warm(const float* mean_prev, const float* std_prev, const float* normal, int64_t n_traj, int rows,
                  int steps_prev, int steps, float warm_std, const float* low4, const float* high4, float* mean, float* std,
                  float* warm, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(mean_prev && std_prev && normal && low4 && high4 && mean && std && warm, "ndp_plan_warm: null pointer");
  NDP_CHECK_ARG(n_traj >= 1 && n_traj <= 65535, "ndp_plan_warm: n_traj=%lld outside 1..65535", (long long)n_traj);
  NDP_CHECK_ARG(rows >= 1 && rows <= NDP_MAX_SAMPLES - 1, "ndp_plan_warm: rows=%d outside 1..%d", rows,
                NDP_MAX_SAMPLES - 1);
  NDP_CHECK_ARG(steps_prev >= 1 && steps_prev <= plan::kMaxSteps, "ndp_plan_warm: steps_prev=%d outside 1..%d", steps_prev,
                plan::kMaxSteps);
  NDP_CHECK_ARG(steps >= 1 && steps <= steps_prev, "ndp_plan_warm: steps=%d outside 1..steps_prev=%d", steps, steps_prev);
  NDP_CHECK_ARG(warm_std >= 0.f && warm_std < INFINITY, "ndp_plan_warm: warm_std=%g must be finite and >= 0",
                (double)warm_std);
  for (int c = 0; c < 4; ++c)
    NDP_CHECK_ARG(low4[c] <= high4[c], "ndp_plan_warm: low[%d]=%g above high[%d]=%g (or NaN)", c, (double)low4[c], c,
                  (double)high4[c]);
  const float* in[3] = {mean_prev, std_prev, normal};
  float* out[3] = {mean, std, warm};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      NDP_CHECK_ARG(out[i] != in[j], "ndp_plan_warm: an output aliases an input");
    for (int j = 0; j < i; ++j) NDP_CHECK_ARG(out[i] != out[j], "ndp_plan_warm: two outputs alias");
  }
  NDP_CHECK_ARG(aligned16(mean_prev) && aligned16(std_prev) && aligned16(normal) && aligned16(mean) && aligned16(std) &&
                    aligned16(warm), "ndp_plan_warm: every buffer must be 16-byte aligned");
  PlanWarmArgs a{mean_prev, std_prev, normal, n_traj, rows, steps_prev, steps, warm_std, {}, {}, mean, std, warm};
  for (int c = 0; c < 4; ++c) { a.low[c] = low4[c]; a.high[c] = high4[c]; }
  const int64_t n = (int64_t)steps * n_traj * rows;       // at most 32 * 65535 * 255 rows: under 2^23 blocks
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_plan_warm", st);
  hipLaunchKernelGGL(k_plan_warm, dim3((unsigned)((n + plan::kBlock - 1) / plan::kBlock)), dim3(plan::kBlock), 0, st, a);
  return check_launch("k_plan_warm");
}

// do the n floats at a and the m floats at b share a byte?
static bool plan_overlap(const float* a, int64_t n, const float* b, int64_t m) { return a < b + m && b < a + n; }

int ndp_plan_goal_grad(const float* pred, int64_t n_rows, const float* goal, int64_t n_goal, int rows_per_goal, float* err,
                       float* d_pred, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(pred && goal && err && d_pred, "ndp_plan_goal_grad: null pointer");
  NDP_CHECK_ARG(n_rows >= 1 && n_rows <= kEvalMaxPairs && n_goal >= 1 && rows_per_goal >= 1,
                "ndp_plan_goal_grad: bad sizes (n_rows %lld, n_goal %lld, rows_per_goal %d)", (long long)n_rows,
                (long long)n_goal, rows_per_goal);
  NDP_CHECK_ARG((n_rows - 1) / rows_per_goal < n_goal, "ndp_plan_goal_grad: %lld rows of %d per goal read past the %lld goals",
                (long long)n_rows, rows_per_goal, (long long)n_goal);
  NDP_CHECK_ARG(aligned16(pred) && aligned16(goal) && aligned16(d_pred),
                "ndp_plan_goal_grad: pred, goal and d_pred must be 16-byte aligned");
  const int64_t all = n_rows * plan::kImageValues;
  NDP_CHECK_ARG(d_pred == pred || !plan_overlap(d_pred, all, pred, all),
                "ndp_plan_goal_grad: d_pred must be pred itself or disjoint from it");
  NDP_CHECK_ARG(!plan_overlap(d_pred, all, goal, n_goal * plan::kImageValues) && !plan_overlap(err, n_rows, d_pred, all) &&
                    !plan_overlap(err, n_rows, pred, all) && !plan_overlap(err, n_rows, goal, n_goal * plan::kImageValues),
                "ndp_plan_goal_grad: an output overlaps goal, or err overlaps an image buffer");
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_plan_goal_grad", st);
  // fewer than 9 n_rows workgroups: under 2^31 with the limit above
  hipLaunchKernelGGL(k_plan_goal_grad, dim3((unsigned)plan::goal_grid(n_rows, rows_per_goal)), dim3(plan::kBlock), 0, st, pred,
                     goal, n_rows, rows_per_goal, (float)(2.0 / (double)plan::kImageValues), err, d_pred);
  return check_launch("k_plan_goal_grad");
}

int ndp_plan_grad_gather(const float* err, const float* seq, int64_t n_traj, int rollouts, int steps, int rows, int32_t* src,
                         int32_t* dst, float* seq_g, float* m, float* v, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(err && seq && src && dst && seq_g && m && v, "ndp_plan_grad_gather: null pointer");
  NDP_CHECK_ARG(n_traj >= 1 && n_traj <= 65535, "ndp_plan_grad_gather: n_traj=%lld outside 1..65535", (long long)n_traj);
  NDP_CHECK_ARG(rollouts >= 2 && rollouts <= NDP_MAX_SAMPLES, "ndp_plan_grad_gather: rollouts=%d outside 2..%d", rollouts,
                NDP_MAX_SAMPLES);
  NDP_CHECK_ARG(rows >= 1 && rows <= rollouts / 2, "ndp_plan_grad_gather: rows=%d outside 1..rollouts/2=%d", rows,
                rollouts / 2);
  NDP_CHECK_ARG(steps >= 1 && steps <= plan::kMaxSteps, "ndp_plan_grad_gather: steps=%d outside 1..%d", steps,
                plan::kMaxSteps);
  NDP_CHECK_ARG(aligned16(seq) && aligned16(seq_g) && aligned16(m) && aligned16(v),
                "ndp_plan_grad_gather: seq, seq_g, m and v must be 16-byte aligned");
  const int64_t small = (int64_t)steps * n_traj * rows * 4, full = (int64_t)steps * n_traj * rollouts * 4;
  NDP_CHECK_ARG(!plan_overlap(seq_g, small, m, small) && !plan_overlap(seq_g, small, v, small) &&
                    !plan_overlap(m, small, v, small) && !plan_overlap(seq_g, small, seq, full) &&
                    !plan_overlap(m, small, seq, full) && !plan_overlap(v, small, seq, full) && src != dst,
                "ndp_plan_grad_gather: two outputs overlap, or one overlaps seq");
  PlanGatherArgs a{err, seq, n_traj, rollouts, steps, rows, src, dst, seq_g, m, v};
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_plan_grad_gather", st);
  hipLaunchKernelGGL(k_plan_grad_gather, dim3((unsigned)n_traj), dim3(plan::kBlock), 0, st, a);
  return check_launch("k_plan_grad_gather");
}

int ndp_plan_grad_step(const float* grad, float* seq_g, float* m, float* v, const float* err_g, int64_t n_traj, int rows,
                       int steps, int t, int optimizer, float lr, float beta1, float beta2, float eps, const float* low4,
                       const float* high4, float* curve_out, const int32_t* dst, float* seq_full, int rollouts,
                       void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(grad && seq_g && low4 && high4, "ndp_plan_grad_step: null pointer");
  NDP_CHECK_ARG(optimizer == NDP_PLAN_SGD || optimizer == NDP_PLAN_ADAM, "ndp_plan_grad_step: optimizer=%d is neither "
                "NDP_PLAN_SGD nor NDP_PLAN_ADAM", optimizer);
  const bool adam = optimizer == NDP_PLAN_ADAM;
  NDP_CHECK_ARG(!adam || (m && v), "ndp_plan_grad_step: NDP_PLAN_ADAM needs m and v");
  NDP_CHECK_ARG(curve_out == nullptr || err_g != nullptr, "ndp_plan_grad_step: curve_out needs err_g");
  NDP_CHECK_ARG((dst == nullptr) == (seq_full == nullptr), "ndp_plan_grad_step: dst and seq_full must both be given or both "
                "be NULL");
  NDP_CHECK_ARG(n_traj >= 1 && n_traj <= 65535, "ndp_plan_grad_step: n_traj=%lld outside 1..65535", (long long)n_traj);
  NDP_CHECK_ARG(rows >= 1 && rows <= NDP_MAX_SAMPLES / 2, "ndp_plan_grad_step: rows=%d outside 1..%d", rows,
                NDP_MAX_SAMPLES / 2);
  NDP_CHECK_ARG(seq_full == nullptr || (rollouts >= 2 * rows && rollouts <= NDP_MAX_SAMPLES),
                "ndp_plan_grad_step: rollouts=%d outside 2 rows..%d", rollouts, NDP_MAX_SAMPLES);
  NDP_CHECK_ARG(steps >= 1 && steps <= plan::kMaxSteps, "ndp_plan_grad_step: steps=%d outside 1..%d", steps, plan::kMaxSteps);
  NDP_CHECK_ARG(t >= 1 && t <= 65535, "ndp_plan_grad_step: t=%d outside 1..65535", t);
  NDP_CHECK_ARG(lr > 0.f && lr < INFINITY, "ndp_plan_grad_step: lr=%g must be finite and > 0", (double)lr);
  NDP_CHECK_ARG(!adam || (beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && eps < INFINITY),
                "ndp_plan_grad_step: beta1=%g, beta2=%g outside [0, 1) or eps=%g not finite and >= 0", (double)beta1,
                (double)beta2, (double)eps);
  for (int c = 0; c < 4; ++c)
    NDP_CHECK_ARG(low4[c] <= high4[c], "ndp_plan_grad_step: low[%d]=%g above high[%d]=%g (or NaN)", c, (double)low4[c], c,
                  (double)high4[c]);
  NDP_CHECK_ARG(aligned16(grad) && aligned16(seq_g) && aligned16(m) && aligned16(v) && aligned16(seq_full),
                "ndp_plan_grad_step: grad, seq_g, m, v and seq_full must be 16-byte aligned");
  const int64_t small = (int64_t)steps * n_traj * rows * 4, full = (int64_t)steps * n_traj * rollouts * 4;
  const float* bufs[4] = {grad, seq_g, adam ? m : nullptr, adam ? v : nullptr};
  for (int i = 0; i < 4; ++i) {
    if (bufs[i] == nullptr) continue;
    for (int j = 0; j < i; ++j)
      NDP_CHECK_ARG(bufs[j] == nullptr || !plan_overlap(bufs[i], small, bufs[j], small),
                    "ndp_plan_grad_step: two of grad, seq_g, m and v overlap");
    NDP_CHECK_ARG(seq_full == nullptr || !plan_overlap(bufs[i], small, seq_full, full),
                  "ndp_plan_grad_step: seq_full overlaps grad, seq_g, m or v");
  }
  PlanStepArgs a{grad, seq_g, adam ? m : nullptr, adam ? v : nullptr, err_g, n_traj, rows, steps, adam ? 1 : 0,
                 (double)lr, (double)beta1, (double)beta2, (double)eps, 1.0, 1.0, {}, {}, curve_out, dst, seq_full, rollouts};
  if (adam) {
    a.corr1 = 1.0 - plan::pow_steps(a.beta1, t);
    a.corr2 = 1.0 - plan::pow_steps(a.beta2, t);
  }
  for (int c = 0; c < 4; ++c) { a.low[c] = low4[c]; a.high[c] = high4[c]; }
  const int64_t n = n_traj * rows;
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_plan_grad_step", st);
  hipLaunchKernelGGL(k_plan_grad_step, dim3((unsigned)((n + plan::kBlock - 1) / plan::kBlock)), dim3(plan::kBlock), 0, st, a);
  return check_launch("k_plan_grad_step");
}

int ndp_normal_noise(float* out, int64_t n, uint64_t seed, const int32_t* offset_dev, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(out && n >= 1, "ndp_normal_noise: bad arguments");
  const int64_t nthreads = (n + 3) / 4;
  NDP_CHECK_ARG((nthreads + kThreads - 1) / kThreads < (1ll << 31), "ndp_normal_noise: n=%lld is too large", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_normal_noise", st);
  hipLaunchKernelGGL(k_normal_noise, dim3((unsigned)((nthreads + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, out, n,
                     seed, offset_dev, aligned16(out) ? 1 : 0);
  return check_launch("k_normal_noise");
}

}  // extern "C"
