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
