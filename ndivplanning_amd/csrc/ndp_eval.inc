// ndp_eval.inc -- the evaluation scripts' glue between the three networks (control_evaluation.py, complete_eval.py,
// mpc_eval.py of the reference):
//   k_eval_pair_mse   nn.MSELoss of one predicted image against one target (mpc_eval.py:161, control_evaluation.py:132,
//                     complete_eval.py:141): the 49,152 squared differences summed in fp64 in a fixed order
//   k_eval_group_mse  the mean over a group of pairs (a batch MSE, or the [B,1,...] x [B,...] broadcast of the last
//                     step), rounded to fp32, then `acc += mse` in fp32 (image_error_sum / action_error_sum)
//   k_eval_select     the rollout rule of mpc_eval.py:159-165 per trajectory, the chosen ts = 0 action and prediction
//   k_eval_g_input    cat(state_code, goal_code) with either part broadcast, the generator's 256-wide code input
//   k_eval_frames_u8  byte frames [n,128,128,3] -> [-1,1] NCHW floats with ndp_encoder_forward_u8's table
// All are bandwidth- or launch-bound VALU kernels.  Every reduction has a fixed order (no float atomics): results are
// bit-reproducible.  Included at the end of ndp_kernels.hip, after ndp_autoencoder.inc.

namespace ndp {

constexpr int kEvalThreads = 256;
constexpr int kEvalCopyChunk = 4096;             // floats of the chosen prediction copied per workgroup

struct EvalPairArgs {
  const float* a; int64_t n_a;                   // predictions
  const float* b; int64_t n_b;                   // targets
  const int32_t* a_idx; const int32_t* b_idx;    // NULL: pair p reads a[p], b[p / b_div]
  int64_t b_div, n_pairs, values;
  float* mse;                                    // NULL or [n_pairs]: the pair's MSE rounded to fp32
  double* sums;                                  // NULL or [n_pairs]: the pair's fp64 sum of squares
};

// One workgroup per pair: thread t sums elements t, t + 256, ... in fp64, then a fixed LDS tree.  A pair whose row
// index is out of range yields NaN (nothing is read).
__global__ __launch_bounds__(kEvalThreads) void k_eval_pair_mse(EvalPairArgs p) {
  __shared__ double red[kEvalThreads];
  const int64_t pair = blockIdx.x;
  const int64_t ra = p.a_idx ? (int64_t)p.a_idx[pair] : pair;
  const int64_t rb = p.b_idx ? (int64_t)p.b_idx[pair] : pair / p.b_div;
  const bool ok = ra >= 0 && ra < p.n_a && rb >= 0 && rb < p.n_b;
  double s = 0.0;
  if (ok) {
    const float* x = p.a + ra * p.values;
    const float* y = p.b + rb * p.values;
    for (int64_t i = threadIdx.x; i < p.values; i += kEvalThreads) {
      const double d = (double)x[i] - (double)y[i];
      s += d * d;
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kEvalThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double sum = ok ? red[0] : (double)NAN;
    if (p.mse) p.mse[pair] = (float)(sum / (double)p.values);
    if (p.sums) p.sums[pair] = sum;
  }
}

// One thread per group: the fp64 sums of its pairs in pair order, / (group * values), rounded to fp32; acc[g] += it.
__global__ __launch_bounds__(kEvalThreads) void k_eval_group_mse(const double* sums, int64_t n_groups, int64_t group,
                                                                int64_t values, float* mse, float* acc) {
  const int64_t g = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
  if (g >= n_groups) return;
  double s = 0.0;
  for (int64_t j = 0; j < group; ++j) s += sums[g * group + j];
  const float m = (float)(s / ((double)group * (double)values));
  if (mse) mse[g] = m;
  if (acc) acc[g] = acc[g] + m;                  // fp32 `+=` of fp32 step values, in launch order
}

struct EvalSelectArgs {
  const float* err; int64_t n_traj; int rollouts;
  const int32_t* forced;                         // NULL, or [n_traj]; an index outside 0..R-1 falls back to the rule
  const float* actions0; const float* pred0; int64_t values;
  int32_t* choice; float* action_out; float* pred_out;
};

// The rule of mpc_eval.py:129 and :159-165: min_error = 10000000000 (exact in fp32), strict `<` in rollout order -- the
// first minimum wins, a NaN error is never chosen, and rollout 0 stands when no error is below the sentinel.
__device__ __forceinline__ int eval_choose(const EvalSelectArgs& a, int64_t b) {
  if (a.forced) {
    const int f = a.forced[b];
    if (f >= 0 && f < a.rollouts) return f;
  }
  float best = 10000000000.0f;
  int pick = 0;
  for (int r = 0; r < a.rollouts; ++r) {
    const float e = a.err[b * a.rollouts + r];
    if (e < best) { best = e; pick = r; }
  }
  return pick;
}

// grid (n_traj, copy chunks): every workgroup re-derives its trajectory's choice (R reads), chunk 0 also writes the
// index and the action, each workgroup copies its slice of the chosen ts = 0 prediction.
__global__ __launch_bounds__(kEvalThreads) void k_eval_select(EvalSelectArgs a) {
  __shared__ int pick_s;
  const int64_t b = blockIdx.x;
  if (threadIdx.x == 0) pick_s = eval_choose(a, b);
  __syncthreads();
  const int pick = pick_s;
  const int64_t row = b * a.rollouts + pick;
  if (blockIdx.y == 0) {
    if (threadIdx.x == 0) a.choice[b] = pick;
    if (threadIdx.x < 4) a.action_out[b * 4 + threadIdx.x] = a.actions0[row * 4 + threadIdx.x];
  }
  if (a.pred_out) {
    const int64_t lo = (int64_t)blockIdx.y * kEvalCopyChunk;
    const int64_t hi = lo + kEvalCopyChunk < a.values ? lo + kEvalCopyChunk : a.values;
    const float* src = a.pred0 + row * a.values;
    float* dst = a.pred_out + b * a.values;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kEvalThreads) dst[i] = src[i];
  }
}

// out[r] = cat(state_code[r / state_rep], goal_code[r / goal_rep]): one workgroup of 256 threads per row.
__global__ __launch_bounds__(kEvalThreads) void k_eval_g_input(const float* state_code, int state_rep,
                                                              const float* goal_code, int goal_rep, int64_t rows,
                                                              float* out) {
  const int64_t r = blockIdx.x;
  if (r >= rows) return;
  const int c = threadIdx.x;
  const float v = c < 128 ? state_code[(r / state_rep) * 128 + c] : goal_code[(r / goal_rep) * 128 + (c - 128)];
  out[r * 256 + c] = v;
}

// One workgroup per image row: thread x reads the 3 bytes of pixel (y, x) and writes them to the three planes.
__global__ __launch_bounds__(128) void k_eval_frames_u8(const unsigned char* frames, int64_t n, float* out) {
  __shared__ float lut[256];
  u8_norm_table(lut);
  __syncthreads();
  const int64_t img = blockIdx.x / 128;
  const int y = blockIdx.x % 128;
  if (img >= n) return;
  const int x = threadIdx.x;
  const unsigned char* px = frames + ((img * 128 + y) * 128 + x) * 3;
  float* o = out + img * 3 * 128 * 128 + y * 128 + x;
  for (int c = 0; c < 3; ++c) o[c * 128 * 128] = lut[px[c]];
}

static int eval_pair_launch(const EvalPairArgs& p, hipStream_t st) {
  KTimer kt("k_eval_pair_mse", st);
  hipLaunchKernelGGL(k_eval_pair_mse, dim3((unsigned)p.n_pairs), dim3(kEvalThreads), 0, st, p);
  return check_launch("k_eval_pair_mse");
}

constexpr int64_t kEvalMaxPairs = 1ll << 24;
constexpr int64_t kEvalMaxValues = 1ll << 26;

}  // namespace ndp

extern "C" {

int ndp_eval_score_select(const float* pred, int64_t n_traj, int rollouts, const float* target, int64_t n_target,
                          const int32_t* target_idx, int64_t values, const float* actions0, const float* pred0,
                          const int32_t* forced, float* err, int32_t* choice, float* action_out, float* pred_out,
                          void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(pred && target && actions0 && err && choice && action_out, "ndp_eval_score_select: null pointer");
  NDP_CHECK_ARG((pred0 == nullptr) == (pred_out == nullptr),
                "ndp_eval_score_select: pred0 and pred_out must both be given or both be NULL");
  NDP_CHECK_ARG(n_traj >= 1 && rollouts >= 1 && n_target >= 1 && values >= 1,
                "ndp_eval_score_select: sizes must be >= 1 (n_traj %lld, rollouts %d, n_target %lld, values %lld)",
                (long long)n_traj, rollouts, (long long)n_target, (long long)values);
  NDP_CHECK_ARG(n_traj * rollouts <= kEvalMaxPairs && n_traj <= 65535 && values <= kEvalMaxValues,
                "ndp_eval_score_select: too large (n_traj %lld, rollouts %d, values %lld)", (long long)n_traj, rollouts,
                (long long)values);
  hipStream_t st = (hipStream_t)stream;
  EvalPairArgs p{pred, n_traj * rollouts, target, n_target, nullptr, target_idx, rollouts, n_traj * rollouts, values,
                 err, nullptr};
  int rc = eval_pair_launch(p, st);
  if (rc) return rc;
  EvalSelectArgs a{err, n_traj, rollouts, forced, actions0, pred0, values, choice, action_out, pred_out};
  const unsigned chunks = pred_out ? (unsigned)((values + kEvalCopyChunk - 1) / kEvalCopyChunk) : 1u;
  KTimer kt("k_eval_select", st);
  hipLaunchKernelGGL(k_eval_select, dim3((unsigned)n_traj, chunks), dim3(kEvalThreads), 0, st, a);
  return check_launch("k_eval_select");
}

int64_t ndp_eval_mse_ws_floats(int64_t n_pairs) {
  return n_pairs < 1 || n_pairs > ndp::kEvalMaxPairs ? 0 : 2 * n_pairs;
}

int ndp_eval_mse(const float* a, int64_t n_a, const float* b, int64_t n_b, const int32_t* a_idx, const int32_t* b_idx,
                 int64_t n_pairs, int64_t values, int64_t group, float* mse, float* acc, float* ws, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(a && b && ws && (mse || acc), "ndp_eval_mse: null pointer");
  NDP_CHECK_ARG(n_a >= 1 && n_b >= 1 && n_pairs >= 1 && values >= 1 && group >= 1,
                "ndp_eval_mse: sizes must be >= 1 (n_a %lld, n_b %lld, n_pairs %lld, values %lld, group %lld)",
                (long long)n_a, (long long)n_b, (long long)n_pairs, (long long)values, (long long)group);
  NDP_CHECK_ARG(n_pairs <= kEvalMaxPairs && values <= kEvalMaxValues, "ndp_eval_mse: too large");
  NDP_CHECK_ARG(n_pairs % group == 0, "ndp_eval_mse: n_pairs %lld is not a multiple of group %lld", (long long)n_pairs,
                (long long)group);
  NDP_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "ndp_eval_mse: ws must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* sums = reinterpret_cast<double*>(ws);
  EvalPairArgs p{a, n_a, b, n_b, a_idx, b_idx, 1, n_pairs, values, nullptr, sums};
  int rc = eval_pair_launch(p, st);
  if (rc) return rc;
  const int64_t n_groups = n_pairs / group;
  KTimer kt("k_eval_group_mse", st);
  hipLaunchKernelGGL(k_eval_group_mse, dim3((unsigned)((n_groups + kEvalThreads - 1) / kEvalThreads)), dim3(kEvalThreads),
                     0, st, (const double*)sums, n_groups, group, values, mse, acc);
  return check_launch("k_eval_group_mse");
}

int ndp_eval_g_input(const float* state_code, int64_t n_state, int state_rep, const float* goal_code, int64_t n_goal,
                     int goal_rep, int64_t rows, float* out, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(state_code && goal_code && out, "ndp_eval_g_input: null pointer");
  NDP_CHECK_ARG(n_state >= 1 && n_goal >= 1 && state_rep >= 1 && goal_rep >= 1 && rows >= 1 && rows <= kEvalMaxPairs,
                "ndp_eval_g_input: bad sizes (n_state %lld, state_rep %d, n_goal %lld, goal_rep %d, rows %lld)",
                (long long)n_state, state_rep, (long long)n_goal, goal_rep, (long long)rows);
  NDP_CHECK_ARG((rows - 1) / state_rep < n_state && (rows - 1) / goal_rep < n_goal,
                "ndp_eval_g_input: %lld rows read past the codes", (long long)rows);
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_eval_g_input", st);
  hipLaunchKernelGGL(k_eval_g_input, dim3((unsigned)rows), dim3(kEvalThreads), 0, st, state_code, state_rep, goal_code,
                     goal_rep, rows, out);
  return check_launch("k_eval_g_input");
}

int ndp_eval_frames_u8(const uint8_t* frames_hwc, int64_t n_images, float* images, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(frames_hwc && images, "ndp_eval_frames_u8: null pointer");
  // one workgroup per image row: n_images * 128 workgroups must fit the grid's x dimension
  NDP_CHECK_ARG(n_images >= 1 && n_images <= ((1ll << 31) - 1) / 128, "ndp_eval_frames_u8: bad image count %lld",
                (long long)n_images);
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_eval_frames_u8", st);
  hipLaunchKernelGGL(k_eval_frames_u8, dim3((unsigned)(n_images * 128)), dim3(128), 0, st, frames_hwc, n_images, images);
  return check_launch("k_eval_frames_u8");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ forward-model scoring
// k_fm_score: what an evaluation of the forward model does with every prediction (forward_model_eval.py), in one launch:
// the MSE of the prediction against its target frame, the MSE of a base frame against the same target ("the frame does
// not change": the persistence baseline) and the reference's display bytes, denorm(...).astype(np.uint8) of
// train_forward_model.py:116-145.  Targets and base frames are floats NCHW or byte frames HWC (normalised through
// u8_norm_table: the floats of the same bytes, bit for bit) and are addressed through index maps: no gathered copy.
// One workgroup of 768 threads per prediction.  The image is walked in 16 tiles of 1,024 pixels: thread t owns, in every
// tile, the four consecutive pixels 4 (t % 256) .. + 3 of plane t / 256 -- one 16-byte load per float operand -- while
// the 3,072 bytes of a tile's HWC byte frames (in and out) are contiguous: they pass through LDS as 768 dwords, one per
// thread, so that the byte loads and stores are coalesced and the NCHW <-> HWC transposition happens in LDS (byte address
// 12 (t % 256) + 3 e + plane: a wave's stride is 3 dwords, conflict-free).  The difference is taken in fp32, its square
// accumulated in fp64: by the thread over its tiles in order, then over the workgroup by a fixed tree (768 -> 512 ->
// 256 .. 1).  No atomics, no scratch memory: two calls give the same bits.
namespace ndp {
namespace fm_score {

constexpr int kScoreThreads = 768;                    // 3 planes x 256 pixel quads
constexpr int kPlane = 128 * 128;
constexpr int kValues = 3 * kPlane;              // 49,152 per image
constexpr int kTilePixels = 1024;
constexpr int kTiles = kPlane / kTilePixels;     // 16
constexpr int kTileBytes = 3 * kTilePixels;      // of an HWC byte frame: kScoreThreads dwords

// u8_norm_table's entry (utils/hdf5_load.py:9-11)
__host__ __device__ inline float norm_u8(int b) { return ((float)b / 255.0f - 0.5f) * 2.0f; }

// trunc(((y + 1) / 2) * 255) as ndp_ae_decode writes it, saturated: the forward model's state + residual can leave
// [-1, 1] (numpy's cast wraps there; a display wants the nearest end).  NaN -> 0.
__host__ __device__ inline unsigned char to_byte(float y) {
  const float v = ((y + 1.0f) / 2.0f) * 255.0f;
  return !(v > 0.0f) ? (unsigned char)0 : v >= 255.0f ? (unsigned char)255 : (unsigned char)(int)v;
}

__host__ __device__ inline double sq_diff(float a, float b) {
  const float d = a - b;
  return (double)d * (double)d;
}

// the row image i addresses (idx NULL: i itself), -1 where it is outside 0 .. rows - 1
__host__ __device__ inline int64_t row_of(const int32_t* idx, int64_t i, int64_t rows) {
  const int64_t r = idx ? (int64_t)idx[i] : i;
  return r >= 0 && r < rows ? r : -1;
}

// thread t in tile `tile`: its plane, its first pixel in the tile, the float offset of that pixel in an NCHW image
__host__ __device__ inline void thread_elems(int t, int tile, int* plane, int* lp0, int* off) {
  *plane = t >> 8;
  *lp0 = 4 * (t & 255);
  *off = *plane * kPlane + tile * kTilePixels + *lp0;
}

// the byte of (pixel lp of the tile, plane) in the tile's HWC bytes
__host__ __device__ inline int tile_byte(int lp, int plane) { return lp * 3 + plane; }

}  // namespace fm_score

struct FmScoreArgs {
  const float* pred;
  const float* tgt_f32; const unsigned char* tgt_u8; int64_t n_target; const int32_t* target_idx;
  const float* base_f32; const unsigned char* base_u8; int64_t n_base; const int32_t* base_idx;
  float* pred_err; float* base_err; unsigned char* pred_u8;
};

// the workgroup's sum of `v` in a fixed order; every thread calls it (uniform)
__device__ __forceinline__ double fm_score_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  if (t < 256) red[t] += red[t + 512];
  __syncthreads();
  for (int w = 256; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

// TGT / BASE: 1 floats NCHW, 2 byte frames HWC; BASE 0: no base frame
template <int TGT, int BASE>
__global__ __launch_bounds__(fm_score::kScoreThreads) void k_fm_score(FmScoreArgs a) {
  using namespace fm_score;
  __shared__ float lut[(TGT == 2 || BASE == 2) ? 256 : 1];
  __shared__ unsigned int tin[TGT == 2 ? kScoreThreads : 1];
  __shared__ unsigned int bin[BASE == 2 ? kScoreThreads : 1];
  __shared__ unsigned int tout[kScoreThreads];
  __shared__ double red[kScoreThreads];
  const int t = threadIdx.x;
  const int64_t img = blockIdx.x;
  if (TGT == 2 || BASE == 2) u8_norm_table(lut);                       // (visible behind the first barrier below)
  const int64_t tr = row_of(a.target_idx, img, a.n_target);
  const int64_t br = BASE != 0 ? row_of(a.base_idx, img, a.n_base) : -1;
  const bool do_pred = a.pred_err != nullptr && tr >= 0;              // (all four: uniform over the workgroup)
  const bool do_base = BASE != 0 && tr >= 0 && br >= 0;
  const bool do_tgt = do_pred || do_base;
  const bool do_bytes = a.pred_u8 != nullptr;
  const float* pred = a.pred + img * kValues;
  double sp = 0.0, sb = 0.0;
  for (int tile = 0; tile < kTiles; ++tile) {
    int plane, lp0, off;
    thread_elems(t, tile, &plane, &lp0, &off);
    if (TGT == 2 && do_tgt)
      tin[t] = reinterpret_cast<const unsigned int*>(a.tgt_u8 + tr * kValues + (int64_t)tile * kTileBytes)[t];
    if (BASE == 2 && do_base)
      bin[t] = reinterpret_cast<const unsigned int*>(a.base_u8 + br * kValues + (int64_t)tile * kTileBytes)[t];
    f32x4 y = {0.f, 0.f, 0.f, 0.f}, x = y, b = y;
    if (do_pred || do_bytes) y = *reinterpret_cast<const f32x4*>(pred + off);
    if (TGT == 1 && do_tgt) x = *reinterpret_cast<const f32x4*>(a.tgt_f32 + tr * kValues + off);
    if (BASE == 1 && do_base) b = *reinterpret_cast<const f32x4*>(a.base_f32 + br * kValues + off);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int byte = tile_byte(lp0 + e, plane);
      if (TGT == 2 && do_tgt) x[e] = lut[reinterpret_cast<const unsigned char*>(tin)[byte]];
      if (BASE == 2 && do_base) b[e] = lut[reinterpret_cast<const unsigned char*>(bin)[byte]];
      if (do_pred) sp += sq_diff(y[e], x[e]);
      if (do_base) sb += sq_diff(b[e], x[e]);
      if (do_bytes) reinterpret_cast<unsigned char*>(tout)[byte] = to_byte(y[e]);
    }
    __syncthreads();
    if (do_bytes)
      reinterpret_cast<unsigned int*>(a.pred_u8 + img * kValues + (int64_t)tile * kTileBytes)[t] = tout[t];
  }
  if (a.pred_err != nullptr) {
    const double s = fm_score_block_sum(sp, red);
    if (t == 0) a.pred_err[img] = do_pred ? (float)(s / (double)kValues) : NAN;
  }
  if (BASE != 0) {
    const double s = fm_score_block_sum(sb, red);
    if (t == 0) a.base_err[img] = do_base ? (float)(s / (double)kValues) : NAN;
  }
}

template <int TGT>
static void fm_score_launch(int base, unsigned grid, hipStream_t st, const FmScoreArgs& a) {
  const dim3 g(grid), b(fm_score::kScoreThreads);
  if (base == 0) hipLaunchKernelGGL((k_fm_score<TGT, 0>), g, b, 0, st, a);
  else if (base == 1) hipLaunchKernelGGL((k_fm_score<TGT, 1>), g, b, 0, st, a);
  else hipLaunchKernelGGL((k_fm_score<TGT, 2>), g, b, 0, st, a);
}

}  // namespace ndp

extern "C" {

int ndp_fm_score(const float* pred, int64_t n_images, const float* target_f32, const uint8_t* target_u8, int64_t n_target,
                 const int32_t* target_idx, const float* base_f32, const uint8_t* base_u8, int64_t n_base,
                 const int32_t* base_idx, float* pred_err, float* base_err, uint8_t* pred_u8, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(pred != nullptr, "ndp_fm_score: null pointer (pred)");
  NDP_CHECK_ARG(n_images >= 1 && n_images <= kEvalMaxPairs, "ndp_fm_score: bad image count %lld", (long long)n_images);
  NDP_CHECK_ARG(!(target_f32 && target_u8), "ndp_fm_score: two targets given (float and byte frames)");
  NDP_CHECK_ARG(target_f32 || target_u8, "ndp_fm_score: no target given");
  NDP_CHECK_ARG(n_target >= 1, "ndp_fm_score: n_target %lld must be >= 1", (long long)n_target);
  NDP_CHECK_ARG(!(base_f32 && base_u8), "ndp_fm_score: two base frames given (float and byte frames)");
  const bool has_base = base_f32 || base_u8;
  NDP_CHECK_ARG(!has_base || base_err, "ndp_fm_score: a base frame is given without base_err");
  NDP_CHECK_ARG(has_base || (!base_err && !base_idx), "ndp_fm_score: base_err / base_idx without a base frame");
  NDP_CHECK_ARG(!has_base || n_base >= 1, "ndp_fm_score: n_base %lld must be >= 1", (long long)n_base);
  NDP_CHECK_ARG(pred_err || base_err || pred_u8, "ndp_fm_score: no output requested");
  NDP_CHECK_ARG(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target_f32) |
                  reinterpret_cast<uintptr_t>(base_f32)) & 15) == 0, "ndp_fm_score: float images must be 16-byte aligned");
  NDP_CHECK_ARG(((reinterpret_cast<uintptr_t>(target_u8) | reinterpret_cast<uintptr_t>(base_u8) |
                  reinterpret_cast<uintptr_t>(pred_u8)) & 3) == 0, "ndp_fm_score: byte frames must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  FmScoreArgs a{pred, target_f32, target_u8, n_target, target_idx, base_f32, base_u8, has_base ? n_base : 0, base_idx,
                pred_err, base_err, pred_u8};
  const int base = base_f32 ? 1 : base_u8 ? 2 : 0;
  KTimer kt("k_fm_score", st);
  if (target_f32) fm_score_launch<1>(base, (unsigned)n_images, st, a);
  else fm_score_launch<2>(base, (unsigned)n_images, st, a);
  return check_launch("k_fm_score");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ generator scoring
// k_gan_score: what an evaluation of the action generator does with the K samples of every conditioning row
// (gan_eval.py), in one launch: each sample's error against the true action, their mean, the best of the K (and the
// running best of the first k + 1: the whole best-of-k curve from one evaluation at K), how far apart the samples are,
// the row's share of the Normalized-Diversification loss and what the discriminator makes of the samples.
// k_ndiv's layout: one thread per (row, sample); K <= 64: 64 threads, a wave holds 64 / K rows, else 256 threads and
// 256 / K rows.  The rows' samples, noise and logits sit in LDS.  Pass 1: thread i computes e_i, the row sums s_i =
// sum_j d_ij of x and z in fp32 in j order (ndiv_block's arithmetic) and sum_j dx_ij in fp64; pass 2: its K hinge terms,
// summed in fp64 in j order.  Then the row's thread 0 walks the K per-sample values in index order: the fp64 sums over
// i, the arg-min / arg-max and the running minimum are serial loops of K steps -- a fixed order by construction.  No
// atomics, no scratch buffer: two calls give the same bits.  The per-element arithmetic is in ndp::gan_score, __host__
// __device__: tests/gan_score_host_driver.hip runs exactly these functions by this schedule on the CPU.
namespace ndp {
namespace gan_score {

constexpr int kActionDim = 4;
constexpr int kMaxNoise = 16;

__host__ __device__ inline int block_threads(int k) { return k <= 64 ? 64 : 256; }
__host__ __device__ inline int rows_per_block(int k) { return block_threads(k) / k; }

// the LDS of a block of `slots` = rows_per_block * k (row, sample) slots: two fp64 arrays, then the fp32 ones
__host__ __device__ inline size_t lds_bytes(int slots, int nz) {
  return (size_t)slots * (2 * sizeof(double) + (kActionDim + nz + 4) * sizeof(float));
}

// e_k: the mean of the 4 squares of the fp32 differences, summed in fp64 in index order, rounded to fp32
__host__ __device__ inline float sample_error(const float* x, const float* a) {
  double s = 0.0;
  for (int d = 0; d < kActionDim; ++d) {
    const float e = x[d] - a[d];
    s += (double)e * (double)e;
  }
  return (float)(s / (double)kActionDim);
}

// one more sample's 4 squares onto the row's fp64 sum, in (k, component) order
__host__ __device__ inline double add_squares(double s, const float* x, const float* a) {
  for (int d = 0; d < kActionDim; ++d) {
    const float e = x[d] - a[d];
    s += (double)e * (double)e;
  }
  return s;
}

// ||a - b||_2 over c channels as ndiv_block takes it: an fmaf chain from 0 in channel order, then sqrtf
__host__ __device__ inline float distance(const float* a, const float* b, int c) {
  float d2 = 0.f;
  for (int d = 0; d < c; ++d) {
    const float e = a[d] - b[d];
    d2 = fmaf(e, e, d2);
  }
  return sqrtf(d2);
}

// relu(0.8 * dz / sz - dx / sx), two roundings for the product and the difference (never contracted), NaN kept
__host__ __device__ inline float hinge(float dz, float sz, float dx, float sx) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float h = __fsub_rn(__fmul_rn(dz / sz, 0.8f), dx / sx);
#else
  volatile float m = (dz / sz) * 0.8f;
  const float h = m - dx / sx;
#endif
  return (h > 0.f || h != h) ? h : 0.f;
}

// the repository's BCE kernels' sigmoid (k_d: 1 / (1 + expf(-x)))
__host__ __device__ inline float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// does `v` replace the running minimum `best`?  The first minimum wins; NaN is never chosen while a non-NaN exists.
__host__ __device__ inline bool better_min(float v, float best) { return v == v && (best != best || v < best); }
__host__ __device__ inline bool better_max(float v, float best) { return v == v && (best != best || v > best); }

}  // namespace gan_score

struct GanScoreArgs {
  const float* x; const float* action; const float* z; const float* logits;
  int64_t n; int k; int nz; int rows_per_block;
  float* sample_err; float* mean_err; float* best_err; int32_t* best_k; float* best_curve;
  float* spread; float* ndiv; float* d_fake_prob; int32_t* d_pick_k; float* d_pick_err;
};

__global__ __launch_bounds__(256) void k_gan_score(GanScoreArgs a) {
  using namespace gan_score;
  extern __shared__ __attribute__((aligned(16))) double gs_smem[];
  const int k = a.k, nz = a.nz, G = a.rows_per_block, slots = G * k;
  double* hs = gs_smem;                                  // [slots] sum_j hinge_ij
  double* ds = hs + slots;                               // [slots] sum_j dx_ij
  float* xs = reinterpret_cast<float*>(ds + slots);      // [slots,4]
  float* zs = xs + slots * kActionDim;                   // [slots,nz]
  float* sx = zs + slots * nz;                           // [slots]
  float* sz = sx + slots;                                // [slots]
  float* es = sz + slots;                                // [slots] e_k
  float* ls = es + slots;                                // [slots] logits
  const int nthreads = blockDim.x, t = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * G;
  const int nrows = (int)((a.n - n0) < G ? (a.n - n0) : G);
  const int nact = nrows * k;
  const bool pairs = a.spread != nullptr || a.ndiv != nullptr;
  for (int idx = t; idx < nact * kActionDim; idx += nthreads) xs[idx] = a.x[n0 * k * kActionDim + idx];
  if (a.ndiv != nullptr)
    for (int idx = t; idx < nact * nz; idx += nthreads) zs[idx] = a.z[n0 * k * nz + idx];
  if (a.logits != nullptr)
    for (int idx = t; idx < nact; idx += nthreads) ls[idx] = a.logits[n0 * k + idx];
  __syncthreads();
  const bool on = t < nact;
  const int g = on ? t / k : 0;
  const int64_t row = n0 + g;
  if (on) {
    if (a.action != nullptr) {
      const float e = sample_error(xs + t * kActionDim, a.action + row * kActionDim);
      es[t] = e;
      if (a.sample_err != nullptr) a.sample_err[n0 * k + t] = e;
    }
    if (pairs) {
      float ssx = 0.f, ssz = 0.f;
      double dsum = 0.0;
      for (int j = 0; j < k; ++j) {
        const float dx = distance(xs + t * kActionDim, xs + (g * k + j) * kActionDim, kActionDim);
        ssx += dx;
        dsum += (double)dx;
        if (a.ndiv != nullptr) ssz += distance(zs + t * nz, zs + (g * k + j) * nz, nz);
      }
      sx[t] = ssx;
      sz[t] = ssz;
      ds[t] = dsum;
    }
  }
  __syncthreads();
  if (on && a.ndiv != nullptr) {
    const float sxi = sx[t], szi = sz[t];
    double h = 0.0;
    for (int j = 0; j < k; ++j) {
      const float dx = distance(xs + t * kActionDim, xs + (g * k + j) * kActionDim, kActionDim);
      const float dz = distance(zs + t * nz, zs + (g * k + j) * nz, nz);
      h += (double)hinge(dz, szi, dx, sxi);
    }
    hs[t] = h;
  }
  __syncthreads();
  if (!on || t != g * k) return;                         // the row's thread 0 walks its K samples in index order
  const int s0 = g * k;
  if (a.action != nullptr) {
    double sum = 0.0;
    float best = es[s0];
    int bk = 0;
    for (int i = 0; i < k; ++i) {
      if (a.mean_err != nullptr) sum = add_squares(sum, xs + (s0 + i) * kActionDim, a.action + row * kActionDim);
      if (better_min(es[s0 + i], best)) { best = es[s0 + i]; bk = i; }
      if (a.best_curve != nullptr) a.best_curve[row * k + i] = best;
    }
    if (a.mean_err != nullptr) a.mean_err[row] = (float)(sum / (double)(k * kActionDim));
    if (a.best_err != nullptr) a.best_err[row] = best;
    if (a.best_k != nullptr) a.best_k[row] = bk;
  }
  if (a.spread != nullptr) {
    double sum = 0.0;
    for (int i = 0; i < k; ++i) sum += ds[s0 + i];
    a.spread[row] = (float)(sum / ((double)k * (double)(k - 1)));
  }
  if (a.ndiv != nullptr) {
    double sum = 0.0;
    for (int i = 0; i < k; ++i) sum += hs[s0 + i];
    a.ndiv[row] = (float)sum;
  }
  if (a.logits != nullptr) {
    double sum = 0.0;
    float top = ls[s0];
    int pk = 0;
    for (int i = 0; i < k; ++i) {
      if (a.d_fake_prob != nullptr) sum += (double)sigmoid(ls[s0 + i]);
      if (better_max(ls[s0 + i], top)) { top = ls[s0 + i]; pk = i; }
    }
    if (a.d_fake_prob != nullptr) a.d_fake_prob[row] = (float)(sum / (double)k);
    if (a.d_pick_k != nullptr) a.d_pick_k[row] = pk;
    if (a.d_pick_err != nullptr) a.d_pick_err[row] = es[s0 + pk];
  }
}

}  // namespace ndp

extern "C" {

int ndp_gan_score(const float* action_hat, int64_t n, int k, const float* action, const float* noise, int nz,
                  const float* fake_logits, float* sample_err, float* mean_err, float* best_err, int32_t* best_k,
                  float* best_curve, float* spread, float* ndiv, float* d_fake_prob, int32_t* d_pick_k, float* d_pick_err,
                  void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(action_hat != nullptr, "ndp_gan_score: null pointer (action_hat)");
  NDP_CHECK_ARG(k >= 1 && k <= NDP_MAX_SAMPLES, "ndp_gan_score: k=%d outside 1..%d", k, NDP_MAX_SAMPLES);
  NDP_CHECK_ARG(n >= 1 && n * k < (1ll << 31), "ndp_gan_score: bad row count %lld", (long long)n);
  NDP_CHECK_ARG(sample_err || mean_err || best_err || best_k || best_curve || spread || ndiv || d_fake_prob || d_pick_k ||
                d_pick_err, "ndp_gan_score: no output requested");
  NDP_CHECK_ARG(action || !(sample_err || mean_err || best_err || best_k || best_curve || d_pick_err),
                "ndp_gan_score: sample_err / mean_err / best_err / best_k / best_curve / d_pick_err need the true actions");
  NDP_CHECK_ARG(noise || !ndiv, "ndp_gan_score: ndiv needs the noise");
  NDP_CHECK_ARG(!noise || (nz >= 1 && nz <= gan_score::kMaxNoise), "ndp_gan_score: nz=%d outside 1..%d", nz,
                gan_score::kMaxNoise);
  NDP_CHECK_ARG(fake_logits || !(d_fake_prob || d_pick_k || d_pick_err),
                "ndp_gan_score: d_fake_prob / d_pick_k / d_pick_err need fake_logits");
  hipStream_t st = (hipStream_t)stream;
  const int threads = gan_score::block_threads(k), G = gan_score::rows_per_block(k);
  GanScoreArgs a{action_hat, action, ndiv ? noise : nullptr, fake_logits, n, k, ndiv ? nz : 0, G,
                 sample_err, mean_err, best_err, best_k, best_curve, spread, ndiv, d_fake_prob, d_pick_k, d_pick_err};
  const size_t lds = gan_score::lds_bytes(G * k, a.nz);
  KTimer kt("k_gan_score", st);
  hipLaunchKernelGGL(k_gan_score, dim3((unsigned)((n + G - 1) / G)), dim3(threads), lds, st, a);
  return check_launch("k_gan_score");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ image quality
// k_image_quality: SSIM and PSNR of image pairs, 3 x 128 x 128 each, floats NCHW in [-1, 1] or byte frames HWC.  The
// definition (DESIGN 5l): u = clamp((x + 1) / 2, 0, 1) in fp32 with NaN kept (bytes through u8_norm_table: the bits of the
// floats of the same bytes); PSNR = 10 log10(1 / mse) of the fp32 differences of u, squares summed in fp64; SSIM in the
// form scikit-image computes with gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=1: an 11-tap
// separable Gaussian over the windows wholly inside the image (118 x 118 positions per channel), filtering and S in fp32,
// the 41,772 values of S summed in fp64.
// One workgroup per (pair, channel, band of ROWS = 16 or 32 output rows): ROWS + 10 rows of both operands are scaled into LDS, the
// five maps x, y, xx, yy, xy are filtered along the rows into LDS, then 16 consecutive lanes own one output row: lane j
// filters columns j, j + 16, ... down the 11 rows, evaluates S and adds it to its fp64 sum in column order; the 16 sums
// are folded by a fixed butterfly.  The squared differences of the band's own input rows are summed by the same lane
// schedule.  What leaves a workgroup is one fp64 sum per output row and per input row, in the workspace: which workgroup
// computed a row does not show in it, so the result does not depend on ROWS.  k_image_quality_finish, one workgroup per
// pair, adds the 354 and 384 row sums by a fixed tree and writes the two floats.  No atomics, no host synchronisation:
// two calls give the same bits.  The arithmetic and the schedule are in ndp::image_quality, __host__ __device__:
// tests/image_quality_host_driver.hip runs exactly these functions on the CPU.
namespace ndp {
namespace image_quality {

constexpr int kSide = 128, kPlane = kSide * kSide, kValues = 3 * kPlane;
constexpr int kTaps = 11, kHalo = kTaps - 1;
constexpr int kOut = kSide - kHalo;               // 118 window positions per axis
constexpr int kSsimValues = 3 * kOut * kOut;      // 41,772
constexpr int kRowLanes = 16;                     // lanes that share one row's sum
constexpr int kSsimRows = 3 * kOut, kPsnrRows = 3 * kSide;
constexpr int kRowSums = kSsimRows + kPsnrRows;   // doubles per pair in the workspace: [3][118] then [3][128]
constexpr int kFinishThreads = 256;               // folds up to 512 row sums

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, computed in double and rounded to fp32 once (the host driver recomputes it)
__host__ __device__ inline float tap(int i) {
  constexpr float g[6] = {0x1.10656p-2f, 0x1.b43c4p-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
  return g[i < 5 ? 5 - i : i - 5];
}

// [-1, 1] -> [0, 1], clamped; -Inf -> 0, +Inf -> 1, NaN stays NaN (both comparisons are false)
__host__ __device__ inline float unit(float x) {
  const float u = (x + 1.0f) * 0.5f;
  return u < 0.0f ? 0.0f : u > 1.0f ? 1.0f : u;
}

// one rounding: the products that are filtered, never contracted into the filter's first fmaf
__host__ __device__ inline float product(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// the filter: an fmaf chain from 0 in tap order over v[0], v[stride], ..
__host__ __device__ inline float filter(const float* v, int stride) {
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < kTaps; ++k) acc = fmaf(tap(k), v[k * stride], acc);
  return acc;
}

// S at one position from the five filtered moments.  Every operation is rounded on its own (no contraction), in an
// order that makes numerator and denominator the same bits when the operands are: 2ab = ab + ab, 2v = v + v.
__host__ __device__ inline float ssim_at(float ux, float uy, float uxx, float uyy, float uxy) {
#pragma clang fp contract(off)
  constexpr float c1 = (float)(0.01 * 0.01), c2 = (float)(0.03 * 0.03);
  const float mxx = ux * ux, myy = uy * uy, mxy = ux * uy;
  const float vx = uxx - mxx, vy = uyy - myy, vxy = uxy - mxy;
  const float num = (2.0f * mxy + c1) * (2.0f * vxy + c2);
  const float den = ((mxx + myy) + c1) * ((vx + vy) + c2);
  return num / den;
}

__host__ __device__ inline double sq_diff(float a, float b) {
#pragma clang fp contract(off)
  const float d = a - b;
  return (double)d * (double)d;
}

// ---- the band schedule
__host__ __device__ inline int bands(int rows) { return (kOut + rows - 1) / rows; }
__host__ __device__ inline int block_threads(int rows) { return rows * kRowLanes; }

// band `band` of `rows` output rows: its first row (output and input), how many output rows it computes, how many input
// rows it stages and how many of those it owns for PSNR (the last band also owns the 10 rows below its windows)
__host__ __device__ inline void band_rows(int band, int rows, int* r0, int* out_rows, int* in_rows, int* own_rows) {
  *r0 = band * rows;
  *out_rows = kOut - *r0 < rows ? kOut - *r0 : rows;
  *in_rows = *out_rows + kHalo;
  *own_rows = band == bands(rows) - 1 ? *in_rows : *out_rows;
}

// horizontal pass, item i of in_rows * 118: its staged row and its first column
__host__ __device__ inline void h_item(int i, int* row, int* col) {
  *row = i / kOut;
  *col = i - *row * kOut;
}

// where pair p, channel c keeps its row sums
__host__ __device__ inline int64_t ssim_slot(int64_t pair, int c, int row) { return pair * kRowSums + c * kOut + row; }
__host__ __device__ inline int64_t psnr_slot(int64_t pair, int c, int row) {
  return pair * kRowSums + kSsimRows + c * kSide + row;
}

// the results from the two folded sums
__host__ __device__ inline float ssim_of(double sum) { return (float)(sum / (double)kSsimValues); }
__host__ __device__ inline float psnr_of(double sum) {
  const double mse = sum / (double)kValues;
  return mse == 0.0 ? INFINITY : (float)(10.0 * log10(1.0 / mse));
}

}  // namespace image_quality

struct ImageQualityArgs {
  const float* a_f32; const unsigned char* a_u8; int64_t n_a; const int32_t* a_idx;
  const float* b_f32; const unsigned char* b_u8; int64_t n_b; const int32_t* b_idx;
  int64_t n_pairs;
  double* sums;                                      // [n_pairs][kRowSums]
  float* ssim; float* psnr;
};

// rows [r0, r0 + in_rows) of channel c of one image, scaled, into dst[in_rows][128]
__device__ __forceinline__ void iq_stage(const float* f32, const unsigned char* u8, int64_t row, int c, int r0, int in_rows,
                                         const float* lut, float* dst) {
  using namespace image_quality;
  const int t = threadIdx.x, nt = blockDim.x;
  if (f32) {
    const f32x4* src = reinterpret_cast<const f32x4*>(f32 + row * kValues + c * kPlane + r0 * kSide);
    for (int i = t; i < in_rows * (kSide / 4); i += nt) {
      const f32x4 v = src[i];
      *reinterpret_cast<f32x4*>(dst + 4 * i) = f32x4{unit(v[0]), unit(v[1]), unit(v[2]), unit(v[3])};
    }
  } else {
    const unsigned char* src = u8 + row * kValues + (int64_t)r0 * kSide * 3 + c;
    for (int i = t; i < in_rows * kSide; i += nt) dst[i] = unit(lut[src[3 * i]]);
  }
}

// the sum over the 16 lanes of a row, the same bits in each: v[j] += v[j + w], w = 8, 4, 2, 1
__device__ __forceinline__ double iq_row_fold(double v) {
#pragma unroll
  for (int w = image_quality::kRowLanes / 2; w > 0; w >>= 1) v += __shfl_xor(v, w, image_quality::kRowLanes);
  return v;
}

template <int ROWS>
__global__ __launch_bounds__(ROWS * image_quality::kRowLanes) void k_image_quality(ImageQualityArgs a) {
  using namespace image_quality;
  constexpr int kIn = ROWS + kHalo;
  __shared__ __attribute__((aligned(16))) float xs[kIn * kSide];
  __shared__ __attribute__((aligned(16))) float ys[kIn * kSide];
  __shared__ float hs[5][kIn * kOut];                 // x, y, xx, yy, xy filtered along the rows
  __shared__ float lut[256];
  const int t = threadIdx.x, nt = ROWS * kRowLanes;
  const int nb = bands(ROWS);
  const int band = blockIdx.x % nb, c = (blockIdx.x / nb) % 3;
  const int64_t pair = blockIdx.x / (3 * nb);
  const int64_t ra = fm_score::row_of(a.a_idx, pair, a.n_a), rb = fm_score::row_of(a.b_idx, pair, a.n_b);
  if (ra < 0 || rb < 0) return;                       // (uniform) the finish kernel writes NaN and reads no sum
  int r0, out_rows, in_rows, own_rows;
  band_rows(band, ROWS, &r0, &out_rows, &in_rows, &own_rows);
  if (a.a_u8 || a.b_u8) {
    u8_norm_table(lut);
    __syncthreads();
  }
  iq_stage(a.a_f32, a.a_u8, ra, c, r0, in_rows, lut, xs);
  iq_stage(a.b_f32, a.b_u8, rb, c, r0, in_rows, lut, ys);
  __syncthreads();
  const int lane = t % kRowLanes, group = t / kRowLanes;
  if (a.psnr) {                                       // own_rows <= ROWS + 10 <= 2 ROWS: at most two rounds
    for (int r = group; r < own_rows; r += ROWS) {
      double s = 0.0;
      for (int col = lane; col < kSide; col += kRowLanes) s += sq_diff(xs[r * kSide + col], ys[r * kSide + col]);
      s = iq_row_fold(s);
      if (lane == 0) a.sums[psnr_slot(pair, c, r0 + r)] = s;
    }
  }
  if (!a.ssim) return;
  for (int i = t; i < in_rows * kOut; i += nt) {
    int row, col;
    h_item(i, &row, &col);
    float x[kTaps], y[kTaps], xx[kTaps], yy[kTaps], xy[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      x[k] = xs[row * kSide + col + k];
      y[k] = ys[row * kSide + col + k];
      xx[k] = product(x[k], x[k]);
      yy[k] = product(y[k], y[k]);
      xy[k] = product(x[k], y[k]);
    }
    hs[0][i] = filter(x, 1);
    hs[1][i] = filter(y, 1);
    hs[2][i] = filter(xx, 1);
    hs[3][i] = filter(yy, 1);
    hs[4][i] = filter(xy, 1);
  }
  __syncthreads();
  if (group < out_rows) {                             // (uniform over each 16 lanes)
    double s = 0.0;
    for (int col = lane; col < kOut; col += kRowLanes) {
      const int at = group * kOut + col;
      s += (double)ssim_at(filter(hs[0] + at, kOut), filter(hs[1] + at, kOut), filter(hs[2] + at, kOut),
                           filter(hs[3] + at, kOut), filter(hs[4] + at, kOut));
    }
    s = iq_row_fold(s);
    if (lane == 0) a.sums[ssim_slot(pair, c, r0 + group)] = s;
  }
}

// the sum of v[0 .. n), n <= 512, by a fixed tree over 512 slots (the empty ones hold 0); every thread calls it
__device__ __forceinline__ double iq_finish_sum(const double* v, int n, double* red) {
  constexpr int T = image_quality::kFinishThreads;
  const int t = threadIdx.x;
  red[t] = (t < n ? v[t] : 0.0) + (t + T < n ? v[t + T] : 0.0);
  __syncthreads();
  for (int w = T / 2; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(image_quality::kFinishThreads) void k_image_quality_finish(ImageQualityArgs a) {
  using namespace image_quality;
  __shared__ double red[kFinishThreads];
  const int64_t pair = blockIdx.x;
  const bool ok = fm_score::row_of(a.a_idx, pair, a.n_a) >= 0 && fm_score::row_of(a.b_idx, pair, a.n_b) >= 0;
  if (!ok) {                                          // (uniform) nothing was written for this pair, nothing is read
    if (threadIdx.x == 0) {
      if (a.ssim) a.ssim[pair] = NAN;
      if (a.psnr) a.psnr[pair] = NAN;
    }
    return;
  }
  if (a.ssim) {
    const double s = iq_finish_sum(a.sums + ssim_slot(pair, 0, 0), kSsimRows, red);
    if (threadIdx.x == 0) a.ssim[pair] = ssim_of(s);
  }
  if (a.psnr) {
    const double s = iq_finish_sum(a.sums + psnr_slot(pair, 0, 0), kPsnrRows, red);
    if (threadIdx.x == 0) a.psnr[pair] = psnr_of(s);
  }
}

// 16-row bands (24 workgroups of 256 threads per pair) while each of them still gets a CU of its own (24 n <= 256), 32-row
// bands (12 of 512 threads: two waves per SIMD, and 42 rows filtered for 32 instead of 26 for 16) beyond that.  Measured
// on an MI355X (DESIGN 5l): 16 rows win by 5 % at 1 .. 10 pairs, 32 rows by 20 to 35 % at 16 .. 224.
__host__ __device__ inline int image_quality_band_rows(int64_t n_pairs) { return n_pairs <= 10 ? 16 : 32; }

}  // namespace ndp

extern "C" {

int64_t ndp_image_quality_ws_bytes(int64_t n_pairs) {
  return n_pairs < 1 || n_pairs > ndp::kEvalMaxPairs ? 0
                                                     : n_pairs * ndp::image_quality::kRowSums * (int64_t)sizeof(double);
}

int ndp_image_quality(const float* a_f32, const uint8_t* a_u8, int64_t n_a, const int32_t* a_idx, const float* b_f32,
                      const uint8_t* b_u8, int64_t n_b, const int32_t* b_idx, int64_t n_pairs, float* ssim, float* psnr,
                      void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG((a_f32 != nullptr) != (a_u8 != nullptr),
                "ndp_image_quality: exactly one of a_f32 and a_u8 must be given");
  NDP_CHECK_ARG((b_f32 != nullptr) != (b_u8 != nullptr),
                "ndp_image_quality: exactly one of b_f32 and b_u8 must be given");
  NDP_CHECK_ARG(ssim || psnr, "ndp_image_quality: no output requested (null pointer ssim and psnr)");
  NDP_CHECK_ARG(n_pairs >= 1 && n_a >= 1 && n_b >= 1 && n_pairs <= kEvalMaxPairs,
                "ndp_image_quality: bad sizes (n_pairs %lld, n_a %lld, n_b %lld)", (long long)n_pairs, (long long)n_a,
                (long long)n_b);
  NDP_CHECK_ARG(workspace && workspace_bytes >= ndp_image_quality_ws_bytes(n_pairs),
                "ndp_image_quality: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)ndp_image_quality_ws_bytes(n_pairs));
  NDP_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "ndp_image_quality: workspace must be 8-byte aligned");
  NDP_CHECK_ARG(((reinterpret_cast<uintptr_t>(a_f32) | reinterpret_cast<uintptr_t>(b_f32)) & 15) == 0,
                "ndp_image_quality: float images must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ImageQualityArgs a{a_f32, a_u8, n_a, a_idx, b_f32, b_u8, n_b, b_idx, n_pairs, reinterpret_cast<double*>(workspace),
                     ssim, psnr};
  const int rows = image_quality_band_rows(n_pairs);
  const unsigned grid = (unsigned)(n_pairs * 3 * image_quality::bands(rows));
  {
    KTimer kt("k_image_quality", st);
    if (rows == 16) hipLaunchKernelGGL(k_image_quality<16>, dim3(grid), dim3(image_quality::block_threads(16)), 0, st, a);
    else hipLaunchKernelGGL(k_image_quality<32>, dim3(grid), dim3(image_quality::block_threads(32)), 0, st, a);
    const int rc = check_launch("k_image_quality");
    if (rc) return rc;
  }
  KTimer kt("k_image_quality_finish", st);
  hipLaunchKernelGGL(k_image_quality_finish, dim3((unsigned)n_pairs), dim3(image_quality::kFinishThreads), 0, st, a);
  return check_launch("k_image_quality_finish");
}

}  // extern "C"
