// ndp_plan.inc -- the planner's cross-entropy refinement (evaluation.py: mpc_plan / plan_step with `cem`):
//   k_plan_cem_update  one CEM iteration on a scored population of action sequences, seq [Th][B][R][4]: rank the R
//                      rollouts of a trajectory by their goal error, refit a diagonal Gaussian to the E best, draw the
//                      next population from it (row 0 keeps the best sequence), keep the running minimum of the error
//   k_normal_noise     standard normal draws, Box-Muller over ndp_uniform_noise's stream
// k_plan_cem_update runs one workgroup of 256 threads per trajectory, in four phases separated by barriers:
//   1  thread r < R stages err[b][r] in LDS;
//   2  thread r < R counts the rollouts that beat it: its rank; order[rank] = r in LDS (a permutation: `beats` is a
//      strict total order).  A NaN error ranks behind every number; among equals and among NaNs the index decides;
//   3  thread d < D = 4 Th refits component d = 4 ts + c from the E' = min(E, non-NaN errors) best rows in rank order
//      (fp64 sums, population variance, fp64 sqrt, smoothing against the previous fit, floor, one rounding to fp32) and
//      leaves mean and std in LDS; thread 0 also updates best_err, threads < E write elite_idx;
//   4  thread i walks the (ts, r) pairs i, i + 256, ...: consecutive rollouts in consecutive lanes, one 16-byte load of
//      the normals and one 16-byte store; row 0 is the rank-0 sequence, copied.
// Every sum has a fixed order, nothing is atomic, nothing spills: two calls give the same bits.  The arithmetic is in
// ndp::plan, __host__ __device__: tests/host_drivers/plan_cem.inc (a body of main.hip) runs exactly these functions by
// this schedule on the CPU.  Included at the end of ndp_kernels.hip, after ndp_store.inc.

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
  double s = sqrt(dev / (double)ne);
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

// one resampled action component: std * n is exact in fp64, so the sum is rounded twice (fp64, then fp32) whether or
// not the two are contracted; clamped to [lo, hi], a NaN stays NaN
__host__ __device__ inline float sample(float std, float n, float mean, float lo, float hi) {
#pragma clang fp contract(off)
  const float v = (float)((double)std * (double)n + (double)mean);
  return v != v ? v : fminf(fmaxf(v, lo), hi);
}

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

__global__ __launch_bounds__(plan::kBlock) void k_plan_cem_update(PlanCemArgs a) {
  using namespace plan;
  __shared__ float err_s[NDP_MAX_SAMPLES];
  __shared__ int order_s[NDP_MAX_SAMPLES];
  __shared__ float mean_s[kMaxDim], std_s[kMaxDim];
  const int t = threadIdx.x, R = a.rollouts, D = a.steps * kActionDim;
  const int64_t b = blockIdx.x;
  float e = 0.f;
  if (t < R) { e = a.err[b * R + t]; err_s[t] = e; }
  const int valid = __syncthreads_count(t < R && e == e);
  if (t < R) order_s[rank_of(err_s, R, t)] = t;
  __syncthreads();
  const int ne = valid < a.elites ? valid : a.elites;
  if (t < D) {
    float m = 0.f, s = 0.f;
    if (!a.first) { m = a.mean[b * D + t]; s = a.std[b * D + t]; }
    refit(a.seq_in, a.n_traj, R, b, t / kActionDim, t % kActionDim, order_s, ne, a.first, a.momentum, a.min_std, &m, &s);
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

int ndp_plan_cem_update(const float* err, const float* seq_in, const float* normal, int64_t n_traj, int rollouts, int steps,
                        int elites, int first, float momentum, float min_std, const float* low4, const float* high4,
                        float* mean, float* std, float* seq_out, float* best_err, int32_t* elite_idx, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(err && seq_in && normal && low4 && high4 && mean && std && seq_out && best_err,
                "ndp_plan_cem_update: null pointer");
  NDP_CHECK_ARG(n_traj >= 1 && n_traj <= 65535, "ndp_plan_cem_update: n_traj=%lld outside 1..65535", (long long)n_traj);
  NDP_CHECK_ARG(rollouts >= 2 && rollouts <= NDP_MAX_SAMPLES, "ndp_plan_cem_update: rollouts=%d outside 2..%d", rollouts,
                NDP_MAX_SAMPLES);
  NDP_CHECK_ARG(elites >= 1 && elites <= rollouts, "ndp_plan_cem_update: elites=%d outside 1..%d", elites, rollouts);
  NDP_CHECK_ARG(steps >= 1 && steps <= plan::kMaxSteps, "ndp_plan_cem_update: steps=%d outside 1..%d", steps,
                plan::kMaxSteps);
  NDP_CHECK_ARG(first == 0 || first == 1, "ndp_plan_cem_update: first must be 0 or 1");
  NDP_CHECK_ARG(momentum >= 0.f && momentum < 1.f, "ndp_plan_cem_update: momentum=%g outside [0, 1)", (double)momentum);
  NDP_CHECK_ARG(min_std >= 0.f, "ndp_plan_cem_update: min_std=%g must be >= 0", (double)min_std);
  for (int c = 0; c < 4; ++c)
    NDP_CHECK_ARG(low4[c] <= high4[c], "ndp_plan_cem_update: low[%d]=%g above high[%d]=%g (or NaN)", c, (double)low4[c], c,
                  (double)high4[c]);
  NDP_CHECK_ARG(seq_out != seq_in && seq_out != normal, "ndp_plan_cem_update: seq_out aliases seq_in or normal");
  NDP_CHECK_ARG(aligned16(seq_in) && aligned16(normal) && aligned16(seq_out),
                "ndp_plan_cem_update: seq_in, normal and seq_out must be 16-byte aligned");
  PlanCemArgs a{err, seq_in, normal, n_traj, rollouts, steps, elites, first, momentum, min_std, {}, {},
                mean, std, seq_out, best_err, elite_idx};
  for (int c = 0; c < 4; ++c) { a.low[c] = low4[c]; a.high[c] = high4[c]; }
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_plan_cem_update", st);
  hipLaunchKernelGGL(k_plan_cem_update, dim3((unsigned)n_traj), dim3(plan::kBlock), 0, st, a);
  return check_launch("k_plan_cem_update");
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
