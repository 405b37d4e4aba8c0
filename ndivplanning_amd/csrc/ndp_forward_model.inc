// ndp_forward_model.inc -- one training iteration (and the inference pass) of the reference's action-conditioned
// next-frame model, SURVEY.md section 8 row f4:
//   models/forward_encoder.py:20-57    Encoder: conv1..5 (3x3 s2 p1, 3 -> 64 -> 128 -> 256 -> 512 -> 1024), BatchNorm after
//                                      conv1..3 only, ReLU; conv6 (4x4 on the 4x4 map) -> 128-d code; returns the 5 maps
//   :60-97    Decoder: deconv1 (132 -> 1024, 4x4 on the 1x1 map), deconv2..6 (ConvTranspose2d(2c, c/2, 4, 2, 1) on
//             cat([up, skip])), each + BatchNorm + ReLU; conv_refine_1 (32 -> 16) + BN + ReLU; conv_refine_2 (16 -> 3) + tanh
//   :99-114   ForwardAutoencoder.forward: training mode returns the residual, eval mode state_cur + residual
//   train_forward_model.py:98-112      loss = mse(model(cur, action), fut - cur); zero_grad; backward; Adam step
// Included at the end of ndp_kernels.hip, after ndp_encoder.inc.
//
// Everything that multiplies is one of two kernels on the fp32 matrix pipe:
//   k_fm_gemm   out[pixel m][n] = sum over taps, channels  src[pixel(m) + tap][ci] . w[n][tap][ci]
//               -- every forward layer and every data gradient: a convolution gathers its taps from the source map
//               (implicit GEMM, as k_conv_gemm); a stride-2 transposed convolution is four stride-1 2x2 convolutions, one
//               per output parity class; the data gradient of a stride-2 3x3 convolution is four parity classes with
//               1 / 2 / 2 / 4 taps; the 4x4 <-> 1x1 layers are sixteen one-tap classes;
//   k_fm_wgrad  dW[j][tap][k] = sum over pixels m  dense[m][j] . gathered[pixel(m) + tap][k]
//               -- every weight gradient (rows = the reduction, both operands read along channels, as k_wgrad).
// (The eval-mode pass can run its nine stride-2 layers with bf16 operands instead -- the FmBf16 instantiations of k_fm_gemm and
// k_fm_deconv32, ndp_fm_forward_lp with NDP_FM_BF16 -- which changes nothing of what follows: every stored map stays fp32.)
// Activations are NHWC with an explicit pixel stride, so that cat([up, skip]) is never copied: the decoder's BatchNorm
// + ReLU writes the lower channels of the next layer's input map, the encoder's writes the upper ones; their gradients
// come back the same way (the encoder's data gradients accumulate onto the skip halves).  Channel counts that are not
// multiples of 32 are zero-padded (image 3 -> 32, code + action 132 -> 160, refine 16 -> 32, output 3 -> 4 of 32).
// Weights live in the layout the weight-gradient kernel produces ("P1": convolution [co][kh][kw][ci], transposed
// convolution [ci][kh][kw][co]); Adam runs on it; the second operand order some layers need ("P2") is rebuilt from it
// after every update.  BatchNorm (training mode: batch statistics, biased variance; running statistics with momentum
// 0.1 and the unbiased variance) is a column-statistics pass + an elementwise pass in each direction.
// Reductions are fixed-order (split-K partial sums, row-chunk slabs, per-block column partials): a step is
// bit-reproducible.

#include <atomic>
#include <unordered_map>

namespace ndp {

// ------------------------------------------------------------------------------------------ network tables
// A network of this family is an FmNet: its layers, how many of the BatchNorms below it uses, and its gradient buckets.
// Every size, offset and pack / optimizer segment on the host side is derived from that table (the helpers below,
// fm_pack, fm_adam_pack, fm_layout, fm_bucket_range), and so is the geometry of every layer launch (fm_geom; fm_layer_fwd,
// fm_layer_dgrad, fm_layer_wgrad); the instances are kFmNet here, kAeNet and kAeDecNet in ndp_autoencoder.inc.
// A further network adds its table with its launch labels, its workspace tensors, where its maps live in them (an FmMaps)
// and its launch sequences: one line per launch that names the layer -- no size, stride or tensor offset is written there.
enum { FM_CONV = 0, FM_DECONV = 1 };
// p2: how the layer's second weight order is made from P1 -- a k_fm_pack kind (see there), or none (the layer reads P1 only)
enum { FM_P2_NONE = -1, FM_P2_CONV_S2 = 0, FM_P2_REFINE = 1, FM_P2_CONV6 = 2, FM_P2_DECONV_S2 = 3, FM_P2_DECONV1 = 4, FM_P2_COLUMNS = 5 };
struct FmLayer { int kind, cin, cout, hin, hout, ksz, stride, pad, cin_pad, cout_pad, p2; };
// kernel-timer labels of a layer's launches: forward, data gradient, weight gradient (static strings: benchmarks and tests
// filter on them)
enum { FM_FWD = 0, FM_DGRAD = 1, FM_WGRAD = 2 };
struct FmLabels { const char* of[3]; };
#define FM_LABELS(name) {{"k_fm_gemm[" name "]", "k_fm_dgrad[" name "]", "k_fm_wgrad[" name "]"}}
struct FmNet {
  const FmLayer* layer; int layers;
  int bns;                                              // it uses the first `bns` of kFmBnC / kFmBnLayer
  const int* bucket_first; const int* bucket_end; int buckets;   // layer ranges [first, end); first -1: the BatchNorm parameters
  const FmLabels* label;
};
constexpr int kFmLayers = 14;
static const FmLayer kFm[kFmLayers] = {
    {FM_CONV, 3, 64, 128, 64, 3, 2, 1, 32, 64, FM_P2_COLUMNS},          // 0  encoder.conv1
    {FM_CONV, 64, 128, 64, 32, 3, 2, 1, 64, 128, FM_P2_CONV_S2},        // 1  encoder.conv2
    {FM_CONV, 128, 256, 32, 16, 3, 2, 1, 128, 256, FM_P2_CONV_S2},      // 2  encoder.conv3
    {FM_CONV, 256, 512, 16, 8, 3, 2, 1, 256, 512, FM_P2_CONV_S2},       // 3  encoder.conv4
    {FM_CONV, 512, 1024, 8, 4, 3, 2, 1, 512, 1024, FM_P2_CONV_S2},      // 4  encoder.conv5
    {FM_CONV, 1024, 128, 4, 1, 4, 1, 0, 1024, 128, FM_P2_CONV6},        // 5  encoder.conv6
    {FM_DECONV, 132, 1024, 1, 4, 4, 1, 0, 160, 1024, FM_P2_DECONV1},    // 6  decoder.deconv1
    {FM_DECONV, 2048, 512, 4, 8, 4, 2, 1, 2048, 512, FM_P2_DECONV_S2},  // 7  decoder.deconv2
    {FM_DECONV, 1024, 256, 8, 16, 4, 2, 1, 1024, 256, FM_P2_DECONV_S2}, // 8  decoder.deconv3
    {FM_DECONV, 512, 128, 16, 32, 4, 2, 1, 512, 128, FM_P2_DECONV_S2},  // 9  decoder.deconv4
    {FM_DECONV, 256, 64, 32, 64, 4, 2, 1, 256, 64, FM_P2_DECONV_S2},    // 10 decoder.deconv5
    {FM_DECONV, 128, 32, 64, 128, 4, 2, 1, 128, 32, FM_P2_DECONV_S2},   // 11 decoder.deconv6
    {FM_CONV, 32, 16, 128, 128, 3, 1, 1, 32, 16, FM_P2_REFINE},         // 12 decoder.conv_refine_1
    {FM_CONV, 16, 3, 128, 128, 3, 1, 1, 32, 4, FM_P2_REFINE},           // 13 decoder.conv_refine_2
};
static const FmLabels kFmLabels[kFmLayers] = {
    FM_LABELS("conv1"), FM_LABELS("conv2"), FM_LABELS("conv3"), FM_LABELS("conv4"), FM_LABELS("conv5"), FM_LABELS("conv6"),
    FM_LABELS("deconv1"), FM_LABELS("deconv2"), FM_LABELS("deconv3"), FM_LABELS("deconv4"), FM_LABELS("deconv5"),
    FM_LABELS("deconv6"), FM_LABELS("refine1"), FM_LABELS("refine2")};
#define FM_LP_LABEL(name) "k_fm_gemm_bf16[" name "]"
static const char* const kFmLpLabel[kFmLayers] = {                      // forward launches with bf16 operands (fm_lp_layer)
    nullptr, FM_LP_LABEL("conv2"), FM_LP_LABEL("conv3"), FM_LP_LABEL("conv4"), FM_LP_LABEL("conv5"), nullptr, nullptr,
    FM_LP_LABEL("deconv2"), FM_LP_LABEL("deconv3"), FM_LP_LABEL("deconv4"), FM_LP_LABEL("deconv5"), FM_LP_LABEL("deconv6"),
    nullptr, nullptr};
// Gradient buckets for a data-parallel driver (SURVEY.md section 8e / 8f-4: "RCCL all-reduce ... overlapped with backward"):
// ranges of the flat gradient in the order in which the backward pass completes them.  The weight gradients are produced
// last layer first, so the range of layers 9..13 is final while the data-gradient chain is still at deconv3; one event per
// bucket is recorded on the stream that wrote its last byte, and ndp_fm_bucket_wait makes the caller's communication
// stream wait for it: the all-reduce of a bucket runs beside the rest of the backward pass.
//   bucket 0  layers 9..13 (deconv4..6, refinement)      4  layer 4 (conv5)
//          1  layer 8 (deconv3)                          5  layers 0..3 (conv1..4)
//          2  layer 7 (deconv2: half of all parameters)  6  the BatchNorm weights and biases
//          3  layers 5, 6 (conv6, deconv1)
constexpr int kFmBuckets = 7;
static const int kFmBucketFirst[kFmBuckets] = {9, 8, 7, 5, 4, 0, -1};
static const int kFmBucketEnd[kFmBuckets] = {14, 9, 8, 7, 5, 4, -1};
// BatchNorms in use (conv4_bn / conv5_bn are constructed by the reference and never applied: forward_encoder.py:51-54)
constexpr int kFmBns = 10;
constexpr int kFmBnC[kFmBns] = {64, 128, 256, 1024, 512, 256, 128, 64, 32, 16};   // conv1..3, deconv1..6, conv_refine_1
static const int kFmBnLayer[kFmBns] = {0, 1, 2, 6, 7, 8, 9, 10, 11, 12};
constexpr float kFmBnEps = 1e-5f, kFmBnMomentum = 0.1f;
static const FmNet kFmNet = {kFm, kFmLayers, kFmBns, kFmBucketFirst, kFmBucketEnd, kFmBuckets, kFmLabels};
// the BatchNorm behind layer l of `net`, or -1
static int fm_bn_of(const FmNet& net, int l) {
  for (int b = 0; b < net.bns; ++b)
    if (kFmBnLayer[b] == l) return b;
  return -1;
}
// channels of the BatchNorms before b: where b's batch mean / invstd / mean residual start in their scratch vectors
constexpr int fm_bn_stat_index(int b) {
  int o = 0;
  for (int i = 0; i < b; ++i) o += kFmBnC[i];
  return o;
}
constexpr int kFmBnChannels = fm_bn_stat_index(kFmBns);    // 2,480: the length of each scratch vector, in every network's workspace

// P1 weight floats of layer l: rows x taps x columns
static int64_t fm_w_rows(const FmNet& net, int l) { return net.layer[l].kind == FM_CONV ? net.layer[l].cout_pad : net.layer[l].cin_pad; }
static int64_t fm_w_cols(const FmNet& net, int l) { return net.layer[l].kind == FM_CONV ? net.layer[l].cin_pad : net.layer[l].cout_pad; }
static int64_t fm_w_floats(const FmNet& net, int l) { return fm_w_rows(net, l) * net.layer[l].ksz * net.layer[l].ksz * fm_w_cols(net, l); }
// flat parameter buffer: per layer [W (P1)][bias (cout_pad)], then per BatchNorm [weight][bias]
static int64_t fm_param_offset(const FmNet& net, int l, bool bias) {
  int64_t o = 0;
  for (int i = 0; i < l; ++i) o += fm_w_floats(net, i) + net.layer[i].cout_pad;
  return o + (bias ? fm_w_floats(net, l) : 0);
}
static int64_t fm_bn_offset(const FmNet& net, int b, bool bias) {
  int64_t o = fm_param_offset(net, net.layers, false);
  for (int i = 0; i < b; ++i) o += 2 * kFmBnC[i];
  return o + (bias ? kFmBnC[b] : 0);
}
static int64_t fm_param_floats(const FmNet& net) { return fm_bn_offset(net, net.bns, false); }
// running statistics: per BatchNorm [running_mean][running_var] (the same for every network: each uses the first ones)
static int64_t fm_stat_offset(int b, bool var) {
  int64_t o = 0;
  for (int i = 0; i < b; ++i) o += 2 * kFmBnC[i];
  return o + (var ? kFmBnC[b] : 0);
}
// P2 (second operand order): its size follows from the layer's kind
static int64_t fm_p2_floats(const FmNet& net, int l) {
  const FmLayer& L = net.layer[l];
  if (L.p2 == FM_P2_NONE) return 0;
  if (L.p2 == FM_P2_COLUMNS) return (int64_t)64 * 32;                     // conv1: [co][k = tap * 3 + ci, 27 -> 32] for the column form
  if (L.p2 == FM_P2_REFINE) return (int64_t)L.cin * 9 * 32;               // [ci (unpadded: 32 / 16)][tap][co -> 32]
  return fm_w_floats(net, l);
}
static int64_t fm_p2_offset(const FmNet& net, int l) {
  int64_t o = 0;
  for (int i = 0; i < l; ++i) o += fm_p2_floats(net, i);
  return o;
}
// The layers that precision NDP_FM_BF16 runs with bf16 operands: the stride-2 3x3 convolutions behind the first and the
// stride-2 4x4 transposed convolutions (kFm: 1..4 and 7..11, 99 % of the multiplications).  The bf16 weight buffer holds,
// layer after layer, the weight order each one's forward launch reads (a convolution P1, a transposed convolution P2),
// element for element: fm_w_floats values of 2 bytes each.
static bool fm_lp_layer(const FmNet& net, int l) { return net.layer[l].p2 == FM_P2_CONV_S2 || net.layer[l].p2 == FM_P2_DECONV_S2; }
static int64_t fm_lp_offset(const FmNet& net, int l) {
  int64_t o = 0;
  for (int i = 0; i < l; ++i) o += fm_lp_layer(net, i) ? fm_w_floats(net, i) : 0;
  return o;
}


// ------------------------------------------------------------------------------------------ epilogue statistics
// Per-channel sums over the pixels of a map come out of the kernel that PRODUCES the map (k_fm_gemm, k_fm_splitk_reduce,
// k_fm_r2_dgrad) instead of a pass of their own, and the kernel that CONSUMES them (the elementwise BatchNorm kernels)
// turns them into mean / invstd / gradients in its prologue: two dependent launches fewer per BatchNorm and direction, and
// one read of the map less.
//   mode 1  (sum v, sum v^2) of the raw output v                                   BatchNorm forward
//   mode 2  g = d * (y > 0), xhat = (x - mean) * invstd:  (sum g, sum g * xhat)      BatchNorm backward (= d beta, d gamma)
//   mode 3  the output becomes g = d * (y > 0);  (sum g, -)                          ReLU backward + bias gradient
//   mode 4  (sum d, -)                                                               bias gradient
// over output columns [0, cols).  Every workgroup sums its tile's columns in fp32 in a fixed order, as the statistics
// kernels of the earlier design summed their blocks of rows; what crosses workgroups is ORDER-FREE: each partial sum is
// added to its channel's accumulator as a fixed-point number of two 64-bit integers (hi: units of 2^-12, lo: the rest in
// units of 2^-52; exact to 2^-53 per partial sum, range 2^50) with integer atomics -- integer addition is associative, so
// the total does not depend on which workgroup arrives when: bit-reproducible with no ordered pass, no flag, no fence.
// `replicas` accumulators per channel (workgroup index modulo) spread the contention of the big maps' thousand tiles.
// The accumulators are zeroed by one memset at the start of the forward and of the backward pass.
struct FmStatEp {
  int mode, cols, replicas;           // replicas: power of two
  long long* acc;                     // [replica][2 sums][cols][2 words]
  const float* x; const float* y; const float* mean; const float* invstd; int x_ld, y_ld;
};
constexpr double kFmFixHi = 4096.0, kFmFixLo = 4503599627370496.0;     // 2^12, 2^52
__device__ __forceinline__ void fm_fix_add(long long* acc, float v) {
  const double d = (double)v;
  const long long hi = __double2ll_rn(d * kFmFixHi);
  const long long lo = __double2ll_rn((d - (double)hi * (1.0 / kFmFixHi)) * kFmFixLo);   // the difference is exact
  __hip_atomic_fetch_add(acc, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(acc + 1, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the total of channel ch, sum s, over the replicas (the integers add exactly, in any order)
__device__ __forceinline__ double fm_fix_read(const long long* acc, int replicas, int cols, int s, int ch) {
  typedef long long ll2 __attribute__((ext_vector_type(2)));
  ll2 v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {                                        // replicas is 1 or 8: every load in flight at once
    v[r] = ll2{0, 0};
    if (r < replicas) v[r] = *reinterpret_cast<const ll2*>(acc + (((size_t)r * 2 + s) * cols + ch) * 2);
  }
  long long hi = 0, lo = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) { hi += v[r][0]; lo += v[r][1]; }
  return (double)hi * (1.0 / kFmFixHi) + (double)lo * (1.0 / kFmFixLo);
}
// A workgroup's column sums are in LDS, sums[2][ncols] for output columns col_base .. col_base + ncols - 1 (those below
// a.cols count): add them to the accumulators of replica `row` mod replicas.  (mode 3 and 4 have one sum.)
__device__ __forceinline__ void fm_stat_publish(const FmStatEp& a, int row, int col_base, int ncols, const float* sums) {
  const int nc = col_base + ncols <= a.cols ? ncols : a.cols - col_base;
  const int nsums = a.mode <= 2 ? 2 : 1;
  const int rep = row & (a.replicas - 1);
  for (int i = threadIdx.x; i < nsums * nc; i += kThreads) {
    const int s = i / nc, j = i - s * nc;
    fm_fix_add(a.acc + (((size_t)rep * 2 + s) * a.cols + col_base + j) * 2, sums[s * ncols + j]);
  }
}

// ------------------------------------------------------------------------------------------ k_fm_gemm
// mode 0  one class: KH x KW taps, source pixel (y*ss - pad + kh, x*ss - pad + kw), output pixel (y, x)
// mode 1  4 classes (py, px) of a stride-2 4x4 transposed convolution: 2x2 taps, source pixel (y + py - 1 + kh, ..),
//         output pixel (2y + py, 2x + px)
// mode 2  4 classes (py, px) of the data gradient of a stride-2 3x3 convolution: (1 + py) x (1 + px) taps, source pixel
//         (y + kh, x + kw), output pixel (2y + py, 2x + px)
// mode 3  16 classes = the pixels of a 4x4 map, one tap at the source's single pixel, output pixel (cls / 4, cls % 4)
//
// Operand paths (ndp_device.h): FmF32, and FmBf16 for precision NDP_FM_BF16 of the eval-mode pass (the definition is in
// include/ndp.h): out = act(bias + sum bf16(x) . bf16(w)) -- `w` is then the layer's bf16 weights, rounded once by k_pack_lp,
// the gathered fp32 activations are rounded where they are staged.
constexpr int kFmBM = 128, kFmBK = 32;
constexpr int kFmLD = 40;      // LDS row stride (floats): 36 costs 8 LDS cycles per ds_read_b128 of an MFMA operand, 40 the ideal 4
using FmF32 = PathF32<kFmLD>;
using FmBf16 = PathFmBf16;

struct FmGemmArgs {
  const float* src; const void* w; const float* bias; float* out; float* part;    // w: P::B::elem of the launched path P
  int src_ld, SH, SW, ss;
  int out_ld, OH, OW;
  int GH, GW, M, C, N;                // rows m = (image*GH + y)*GW + x; C gathered channels (multiple of 32); N columns
  int mode, KH, KW, pad;
  int act, accumulate;                // act 0 none, 1 ReLU, 2 tanh; accumulate: out += result
  int zero_to;                        // columns N .. zero_to-1 of the output pixel are written as zeros (channel padding that
                                      // a later gather meets with zero weights: it must be finite); never with a K split
  int nsplit, steps_per_split;        // K split over blockIdx.y: partial sums [cls][split][M][N] in `part`
  int cls_units;                      // mode 2, > 0: blockIdx.y = one of 9 * cls_units equal K units (see fm_unit)
  int mtiles, ntiles;
  int rows_per_block;                 // k_fm_splitk_reduce: global rows (cls, m) per workgroup
  FmStatEp ep;                        // epilogue statistics (mode 0: none); with a K split they come out of k_fm_splitk_reduce
};
struct FmClass { int KH, KW, pad_y, pad_x, py, px, os; int64_t w_off; };
__device__ __forceinline__ FmClass fm_class(const FmGemmArgs& a, int cls) {
  FmClass c;
  if (a.mode == 0) {
    c.KH = a.KH; c.KW = a.KW; c.pad_y = c.pad_x = a.pad; c.py = c.px = 0; c.os = 1; c.w_off = 0;
  } else if (a.mode == 1) {
    c.py = cls >> 1; c.px = cls & 1; c.KH = c.KW = 2; c.pad_y = 1 - c.py; c.pad_x = 1 - c.px; c.os = 2;
    c.w_off = (int64_t)cls * a.N * 4 * a.C;
  } else if (a.mode == 2) {
    c.py = cls >> 1; c.px = cls & 1; c.KH = 1 + c.py; c.KW = 1 + c.px; c.pad_y = c.pad_x = 0; c.os = 2;
    const int before = cls == 0 ? 0 : (cls == 1 ? 1 : (cls == 2 ? 3 : 5));
    c.w_off = (int64_t)before * a.N * a.C;
  } else {
    c.py = cls >> 2; c.px = cls & 3; c.KH = c.KW = 1; c.pad_y = c.pad_x = 0; c.os = 1;
    c.w_off = (int64_t)cls * a.N * a.C;
  }
  return c;
}
// Mode 2 has 1 / 2 / 2 / 4 taps per parity class: a grid of (tile, class) workgroups is as slow as its 4-tap class while
// the 1-tap class idles (conv3's data gradient at 32 images: 256 workgroups, 56 % of their slots busy).  With cls_units = s
// the K loops are cut into 9 s units of C / 32 / s steps -- every (class, tap) pair s units -- so that all workgroups are
// equal; unit u belongs to class 0 below s, class 1 below 3 s, class 2 below 5 s, else class 3, and is that class's
// split u - first.  Partial sums [unit][M][N]; k_fm_splitk_reduce adds a class's units in unit order.
__device__ __forceinline__ int fm_unit_first(int cls, int s) { return s * (cls == 0 ? 0 : (cls == 1 ? 1 : (cls == 2 ? 3 : 5))); }
__device__ __forceinline__ int fm_unit_count(int cls, int s) { return s * (cls == 0 ? 1 : (cls == 3 ? 4 : 2)); }
__device__ __forceinline__ float fm_act(float v, int act) {
  return act == 1 ? fmaxf(v, 0.f) : (act == 2 ? tanhf(v) : v);
}
// row m -> index of its output pixel, and its offset (floats) in the output map
__device__ __forceinline__ size_t fm_out_pixel_index(const FmGemmArgs& a, const FmClass& k, int m) {
  const int img = m / (a.GH * a.GW), rem = m - img * (a.GH * a.GW);
  const int y = rem / a.GW, x = rem - y * a.GW;
  return ((size_t)img * a.OH + y * k.os + k.py) * a.OW + x * k.os + k.px;
}
__device__ __forceinline__ size_t fm_out_pixel(const FmGemmArgs& a, const FmClass& k, int m) {
  return fm_out_pixel_index(a, k, m) * a.out_ld;
}
// statistics terms of 4 adjacent output values v; y, x: the 4 values of the post-ReLU map / the raw BatchNorm input at the
// same place (modes 2, 3), mu / is: the channels' batch mean and invstd (mode 2); mode 3 replaces v by the masked gradient
__device__ __forceinline__ void fm_stat_terms(int mode, f32x4& v, const f32x4& y, const f32x4& x, const f32x4& mu, const f32x4& is,
                                              f32x4& s1, f32x4& s2) {
  if (mode == 1) {
    s1 += v;
    s2 += v * v;
  } else if (mode == 4) {
    s1 += v;
  } else {
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = y[e] > 0.f ? v[e] : 0.f;
    s1 += g;
    if (mode == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) s2[e] += g[e] * ((x[e] - mu[e]) * is[e]);
    } else {
      v = g;
    }
  }
}
// ... with the operands fetched here (callers that cannot prefetch)
__device__ __forceinline__ void fm_stat_terms(const FmStatEp& ep, size_t pix, int col, f32x4& v, f32x4& s1, f32x4& s2) {
  f32x4 y = {0.f, 0.f, 0.f, 0.f}, x = y, mu = y, is = y;
  if (ep.mode == 2 || ep.mode == 3) y = *reinterpret_cast<const f32x4*>(ep.y + pix * ep.y_ld + col);
  if (ep.mode == 2) {
    x = *reinterpret_cast<const f32x4*>(ep.x + pix * ep.x_ld + col);
    mu = *reinterpret_cast<const f32x4*>(ep.mean + col);
    is = *reinterpret_cast<const f32x4*>(ep.invstd + col);
  }
  fm_stat_terms(ep.mode, v, y, x, mu, is, s1, s2);
}

// The bf16 instantiation differs from the fp32 ones outside the operand path, deliberately, in this: it has no statistics
// epilogue (FmStatEp: the eval-mode pass never asks for one) and neither cls_units nor the mode-2 class order (modes 0
// and 1 only) -- left out at compile time; fm_gemm refuses such a launch.
template <int BN, class P = FmF32>
__global__ __launch_bounds__(kThreads, 2) void k_fm_gemm(FmGemmArgs a) {
  using SA = typename P::A; using SB = typename P::B; using Mma = typename P::Mma;
  extern __shared__ __attribute__((aligned(16))) float smem[];       // the statistics' scratch (the tiles: Mma::tiles())
  constexpr bool LP = P::kLp;
  constexpr int BM = kFmBM, BK = kFmBK, LD = Mma::LD, V = P::V;
  constexpr int TI = BN == 128 ? 4 : 2, TJ = BN == 128 ? 4 : 2;     // 16 x 16 tiles per wave: rows x columns
  // 8 or more row tiles: the column tiles of one row tile share an XCD (k_conv_gemm).  Fewer (the deep layers at small
  // batches): plain order -- the padded scheme would leave every workgroup that has work on XCD 0 (measured: deconv2 at 8
  // images 326 us on one XCD)
  int n_tile, m_tile;
  if (a.mtiles >= 8) {
    const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
    n_tile = jb % a.ntiles;
    m_tile = (jb / a.ntiles) * 8 + xcd;
    if (m_tile >= a.mtiles) return;
  } else {
    n_tile = blockIdx.x % a.ntiles;
    m_tile = blockIdx.x / a.ntiles;
  }
  // mode 2 (data gradient of a stride-2 3x3 convolution): the parity classes have 1 / 2 / 2 / 4 taps -- the grid is
  // dispatched z-major, so the 4-tap class goes first and the 1-tap class fills the tail
  int split = blockIdx.y, cls = blockIdx.z;
  if constexpr (!LP) {
    if (a.mode == 2) cls = 3 - (int)blockIdx.z;
    if (a.cls_units > 0) {
      const int u = blockIdx.y, s = a.cls_units;
      cls = u < s ? 0 : (u < 3 * s ? 1 : (u < 5 * s ? 2 : 3));
      split = u - fm_unit_first(cls, s);
    }
  }
  const FmClass kc = fm_class(a, cls);
  const int ksteps = kc.KH * kc.KW * a.C / BK;
  const int sbeg = split * a.steps_per_split;
  const int send = sbeg + a.steps_per_split < ksteps ? sbeg + a.steps_per_split : ksteps;
  const int K = kc.KH * kc.KW * a.C;
  const typename SB::elem* wcls = static_cast<const typename SB::elem*>(a.w) + kc.w_off;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int row0 = BN == 128 ? (wave >> 1) * 64 : wave * 32, col0 = BN == 128 ? (wave & 1) * 64 : 0;

  constexpr int QPR = BK / V, RPP = kThreads / QPR, NUA = BM / RPP, NUB = BN / RPP;
  const int r0 = t / QPR, kq = t % QPR;
  const typename SA::elem* a_img[NUA];
  int a_y0[NUA], a_x0[NUA];
#pragma unroll
  for (int u = 0; u < NUA; ++u) {
    int m = m_tile * BM + r0 + RPP * u;
    const bool valid = m < a.M;
    m = valid ? m : a.M - 1;
    const int img = m / (a.GH * a.GW), rem = m - img * (a.GH * a.GW);
    const int y = rem / a.GW, x = rem - y * a.GW;
    a_img[u] = a.src + (size_t)img * a.SH * a.SW * a.src_ld + V * kq;
    a_y0[u] = valid ? y * a.ss - kc.pad_y : -(1 << 20);             // rows past M: every tap out of bounds -> zeros
    a_x0[u] = x * a.ss - kc.pad_x;
  }
  const typename SB::elem* b_row[NUB];
  bool b_ok[NUB];
#pragma unroll
  for (int u = 0; u < NUB; ++u) {
    const int n = n_tile * BN + r0 + RPP * u;
    b_ok[u] = n < a.N;
    b_row[u] = wcls + (size_t)(b_ok[u] ? n : a.N - 1) * K + V * kq;
  }
  typename SA::reg ra[NUA];
  typename SB::reg rb[NUB];
  bool ra_ok[NUA];
  auto fetch = [&](int step) {
    const int k0 = step * BK;
    const int tap = k0 / a.C, ci0 = k0 - tap * a.C;                  // uniform: one tap, 32 consecutive channels
    const int kh = tap / kc.KW, kw = tap - kh * kc.KW;
#pragma unroll
    for (int u = 0; u < NUA; ++u) {
      const int yy = a_y0[u] + kh, xx = a_x0[u] + kw;
      const bool ok = (unsigned)yy < (unsigned)a.SH && (unsigned)xx < (unsigned)a.SW;
      ra[u] = SA::load(a_img[u] + (ok ? (size_t)(yy * a.SW + xx) * a.src_ld + ci0 : 0));
      ra_ok[u] = ok;
    }
#pragma unroll
    for (int u = 0; u < NUB; ++u) rb[u] = SB::load(b_row[u] + k0);
    pin_vmem();
  };
  auto stage = [&](int buf) {
    typename P::lds* As = Mma::tiles() + buf * (BM + BN) * LD;
    typename P::lds* Bs = As + BM * LD;
#pragma unroll
    for (int u = 0; u < NUA; ++u) *reinterpret_cast<typename SA::quad*>(As + (r0 + RPP * u) * LD + V * kq) = SA::staged(ra[u], ra_ok[u]);
#pragma unroll
    for (int u = 0; u < NUB; ++u) *reinterpret_cast<typename SB::quad*>(Bs + (r0 + RPP * u) * LD + V * kq) = SB::staged(rb[u], b_ok[u]);
  };

  f32x4 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int jn = 0; jn < TJ; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (sbeg < send) {
    fetch(sbeg);
    stage(0);
  }
  __syncthreads();
  int buf = 0;
  for (int step = sbeg; step < send; ++step) {
    const bool more = step + 1 < send;
    if (more) fetch(step + 1);
    const typename P::lds* As = Mma::tiles() + buf * (BM + BN) * LD + (row0 + c) * LD + Mma::KQ * q;
    const typename P::lds* Bs = Mma::tiles() + buf * (BM + BN) * LD + BM * LD + (col0 + c) * LD + Mma::KQ * q;
    typename Mma::frag af[TI], bf[TJ];
#pragma unroll
    for (int h = 0; h < Mma::PARTS; ++h) {
#pragma unroll
      for (int i = 0; i < TI; ++i) Mma::read(af[i], As + i * 16 * LD, h);
#pragma unroll
      for (int jn = 0; jn < TJ; ++jn) Mma::read(bf[jn], Bs + jn * 16 * LD, h);
    }
#pragma unroll
    for (int ks = 0; ks < Mma::KSUB; ++ks)
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int jn = 0; jn < TJ; ++jn) acc[i][jn] = Mma::mma(bf[jn], af[i], acc[i][jn], ks);   // transposed tiles
    pin_vmem();
    if (more) stage(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // a lane holds output row (pixel) c and the 4 consecutive columns 4q .. 4q+3 of each tile
  const bool fin = a.nsplit == 1;
  const bool stat = !LP && fin && a.ep.mode != 0 && n_tile * BN < a.ep.cols;
  const bool need_y = stat && (a.ep.mode == 2 || a.ep.mode == 3), need_x = stat && a.ep.mode == 2;
  f32x4 cs1[TJ], cs2[TJ], bias4[TJ], mu4[TJ], is4[TJ];
  int colj[TJ];
#pragma unroll
  for (int jn = 0; jn < TJ; ++jn) {
    cs1[jn] = cs2[jn] = bias4[jn] = mu4[jn] = is4[jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    colj[jn] = n_tile * BN + col0 + jn * 16 + 4 * q;
    if (fin && a.bias != nullptr && colj[jn] < a.N) bias4[jn] = *reinterpret_cast<const f32x4*>(a.bias + colj[jn]);
    if (need_x && colj[jn] < a.ep.cols) {
      mu4[jn] = *reinterpret_cast<const f32x4*>(a.ep.mean + colj[jn]);
      is4[jn] = *reinterpret_cast<const f32x4*>(a.ep.invstd + colj[jn]);
    }
  }
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int m = m_tile * BM + row0 + i * 16 + c;
    if (m >= a.M) continue;
    const size_t pix = fm_out_pixel_index(a, kc, m);
    float* orow = fin ? a.out + pix * a.out_ld
                      : a.part + ((size_t)(!LP && a.cls_units > 0 ? (int)blockIdx.y : cls * a.nsplit + split) * a.M + m) * a.N;
    // every load of this row tile before its first store (the compiler cannot move a load above a store that may alias it:
    // issued one by one between the stores, each would expose its own latency)
    f32x4 prev[TJ], yv[TJ], xv[TJ];
#pragma unroll
    for (int jn = 0; jn < TJ; ++jn) {
      prev[jn] = yv[jn] = xv[jn] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int col = colj[jn];
      if (fin && a.accumulate && col < a.N) prev[jn] = *reinterpret_cast<const f32x4*>(orow + col);
      if (need_y && col < a.ep.cols) yv[jn] = *reinterpret_cast<const f32x4*>(a.ep.y + pix * a.ep.y_ld + col);
      if (need_x && col < a.ep.cols) xv[jn] = *reinterpret_cast<const f32x4*>(a.ep.x + pix * a.ep.x_ld + col);
    }
#pragma unroll
    for (int jn = 0; jn < TJ; ++jn) {
      const int col = colj[jn];
      if (col >= a.N) {                                              // N is a multiple of 4
        if (fin && col < a.zero_to) *reinterpret_cast<f32x4*>(orow + col) = f32x4{0.f, 0.f, 0.f, 0.f};
        continue;
      }
      f32x4 v = acc[i][jn];
      if (fin) {
        v += bias4[jn];
        v = f32x4{fm_act(v[0], a.act), fm_act(v[1], a.act), fm_act(v[2], a.act), fm_act(v[3], a.act)};
        v += prev[jn];
        if (stat && col < a.ep.cols) fm_stat_terms(a.ep.mode, v, yv[jn], xv[jn], mu4[jn], is4[jn], cs1[jn], cs2[jn]);
      }
      *reinterpret_cast<f32x4*>(orow + col) = v;
    }
  }
  if (!stat) return;
  // column sums of the workgroup's tile: over the 16 lanes that hold the rows of a tile (lane = 16 q + c: xor 1, 2, 4, 8
  // stays inside the 16), then over the waves that share columns, through LDS, in wave order
  float* red = smem;                                                  // [wave][2][WC]; the main loop ended with a barrier
  constexpr int WC = TJ * 16;                                         // columns per wave
#pragma unroll
  for (int jn = 0; jn < TJ; ++jn)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v1 = cs1[jn][e], v2 = cs2[jn][e];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        v1 += __shfl_xor(v1, off, 64);
        v2 += __shfl_xor(v2, off, 64);
      }
      if (c == 0) {
        red[(wave * 2 + 0) * WC + jn * 16 + 4 * q + e] = v1;
        red[(wave * 2 + 1) * WC + jn * 16 + 4 * q + e] = v2;
      }
    }
  __syncthreads();
  float* sums = smem + kWaves * 2 * WC;                               // [2][BN]
  for (int i = t; i < 2 * BN; i += kThreads) {
    const int sidx = i / BN, col = i - sidx * BN;
    float v;
    if (BN == 128) {                                                  // waves (w & 1) == col / 64 hold the column: w = col/64, then + 2
      const int w0 = col >> 6, cc = col & 63;
      v = red[(w0 * 2 + sidx) * WC + cc] + red[((w0 + 2) * 2 + sidx) * WC + cc];
    } else {
      v = red[(0 * 2 + sidx) * WC + col];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v += red[(w * 2 + sidx) * WC + col];
    }
    sums[sidx * BN + col] = v;
  }
  __syncthreads();
  fm_stat_publish(a.ep, cls * a.mtiles + m_tile, n_tile * BN, BN, sums);
}

// deconv6 (128 -> 32 channels at 128 x 128; deconv5, 64 channels, as two halves when it has the tiles): the FOUR parity
// classes of a row tile in one workgroup.  As four mode-1
// launches' worth of 128 x 32 tiles the layer staged every source pixel once per (class, tap) pair -- 16 operand tiles per
// 32 channels -- with a barrier per 32 MFMAs of a wave; the classes share their source pixels (a 3 x 3 neighbourhood, each
// class a 2 x 2 corner of it), so this kernel walks the NINE taps, stages the source tile once per tap and the weights of
// the classes that use that tap (1, 2 or 4), and every wave -- 32 rows x all 128 = 4 x 32 columns -- runs the MFMAs of
// those classes: 9 operand tiles and 9 barriers per 32 channels for the same MFMAs, a quarter of the workgroups.
// Weights: the mode-1 order [cls][co][kh'][kw'][ci]; class (py, px) meets tap (dy, dx) in {-1, 0, 1}^2 at kh' = dy - py + 1,
// kw' = dx - px + 1 when both are 0 or 1.  Statistics (mode 1) over the 32 output channels, all classes together.
// RELU: the stored output is max(v, 0) (the eval-mode decoder of ndp_autoencoder.inc, BatchNorm folded into w and bias: no
// statistics there); the training paths' instantiation, RELU = false, is the kernel as it was.
// The bf16 instantiation (precision NDP_FM_BF16: deconv6, and deconv5 where fm_geom chooses this form; measured against
// mode 1 of k_fm_gemm's, 16 operand tiles per 32 channels instead of 9: DESIGN.md 5s) differs outside the operand path,
// deliberately, in this: bias only -- no ReLU and no statistics, which the eval-mode pass never asks of these layers;
// fm_deconv32 refuses such a launch.
struct FmDcArgs {
  const float* src; const void* w; const float* bias; float* out;      // w: P::B::elem of the launched path P
  int src_ld, SH, SW, out_ld, M, C, N, mtiles;        // N output channels: blockIdx.y = which 32 of them
  FmStatEp ep;
};
template <bool RELU, class P = FmF32>
__global__ __launch_bounds__(kThreads, 2) void k_fm_deconv32(FmDcArgs a) {
  using SA = typename P::A; using SB = typename P::B; using Mma = typename P::Mma;
  static_assert(!(P::kLp && RELU), "k_fm_deconv32: the bf16 instantiation has no ReLU");
  extern __shared__ __attribute__((aligned(16))) float smem[];       // the statistics' scratch (the tiles: Mma::tiles())
  constexpr int BM = kFmBM, BK = kFmBK, LD = Mma::LD, V = P::V, NB = 128;   // NB: 4 classes x 32 output channels
  int m_tile;
  if (a.mtiles >= 8) {
    const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
    m_tile = jb * 8 + xcd;
    if (m_tile >= a.mtiles) return;
  } else {
    m_tile = blockIdx.x;
  }
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int row0 = wave * 32;
  constexpr int QPR = BK / V, RPP = kThreads / QPR, NUA = BM / RPP;      // 8 quads per row, 32 rows per pass, 4 passes
  static_assert(RPP == 32, "k_fm_deconv32: a pass of B rows is one class's 32 output channels");
  const int r0 = t / QPR, kq = t % QPR;
  const typename SA::elem* a_img[NUA];
  int a_y[NUA], a_x[NUA];
#pragma unroll
  for (int u = 0; u < NUA; ++u) {
    int m = m_tile * BM + r0 + RPP * u;
    const bool valid = m < a.M;
    m = valid ? m : a.M - 1;
    const int img = m / (a.SH * a.SW), rem = m - img * (a.SH * a.SW);
    const int y = rem / a.SW, x = rem - y * a.SW;
    a_img[u] = a.src + (size_t)img * a.SH * a.SW * a.src_ld + V * kq;
    a_y[u] = valid ? y : -(1 << 20);
    a_x[u] = x;
  }
  // B rows: pass u = class u, row r0 = output channel
  const typename SB::elem* b_cls[4];
  const int co0 = blockIdx.y * 32;
#pragma unroll
  for (int u = 0; u < 4; ++u) b_cls[u] = static_cast<const typename SB::elem*>(a.w) + ((size_t)u * a.N + co0 + r0) * 4 * a.C + V * kq;
  const int chunks = a.C / BK, nsteps = 9 * chunks;
  typename SA::reg ra[NUA];
  typename SB::reg rb[4];
  bool ra_ok[NUA];
  auto fetch = [&](int step) {
    const int tap = step / chunks, ci0 = (step - tap * chunks) * BK;
    const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
#pragma unroll
    for (int u = 0; u < NUA; ++u) {
      const int yy = a_y[u] + dy, xx = a_x[u] + dx;
      const bool ok = (unsigned)yy < (unsigned)a.SH && (unsigned)xx < (unsigned)a.SW;
      ra[u] = SA::load(a_img[u] + (ok ? (size_t)(yy * a.SW + xx) * a.src_ld + ci0 : 0));
      ra_ok[u] = ok;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int khp = dy - (u >> 1) + 1, kwp = dx - (u & 1) + 1;
      if ((unsigned)khp < 2u && (unsigned)kwp < 2u) rb[u] = SB::load(b_cls[u] + (size_t)(khp * 2 + kwp) * a.C + ci0);   // (uniform)
    }
    pin_vmem();
  };
  auto stage = [&](int buf, int step) {
    const int tap = step / chunks;
    const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
    typename P::lds* As = Mma::tiles() + buf * (BM + NB) * LD;
    typename P::lds* Bs = As + BM * LD;
#pragma unroll
    for (int u = 0; u < NUA; ++u) *reinterpret_cast<typename SA::quad*>(As + (r0 + RPP * u) * LD + V * kq) = SA::staged(ra[u], ra_ok[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int khp = dy - (u >> 1) + 1, kwp = dx - (u & 1) + 1;
      if ((unsigned)khp < 2u && (unsigned)kwp < 2u) *reinterpret_cast<typename SB::quad*>(Bs + (u * 32 + r0) * LD + V * kq) = SB::staged(rb[u]);
    }
  };
  f32x4 acc[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 8; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  stage(0, 0);
  __syncthreads();
  int buf = 0;
  for (int step = 0; step < nsteps; ++step) {
    const bool more = step + 1 < nsteps;
    if (more) fetch(step + 1);
    const int tap = step / chunks;
    const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
    const typename P::lds* As = Mma::tiles() + buf * (BM + NB) * LD + (row0 + c) * LD + Mma::KQ * q;
    const typename P::lds* Bs = Mma::tiles() + buf * (BM + NB) * LD + BM * LD + c * LD + Mma::KQ * q;
    typename Mma::frag af[2];
#pragma unroll
    for (int h = 0; h < Mma::PARTS; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i) Mma::read(af[i], As + i * 16 * LD, h);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int khp = dy - (u >> 1) + 1, kwp = dx - (u & 1) + 1;
      if ((unsigned)khp >= 2u || (unsigned)kwp >= 2u) continue;       // (uniform: this tap is not one of class u's)
      typename Mma::frag bf[2];
#pragma unroll
      for (int h = 0; h < Mma::PARTS; ++h)
#pragma unroll
        for (int jn = 0; jn < 2; ++jn) Mma::read(bf[jn], Bs + (u * 32 + jn * 16) * LD, h);
#pragma unroll
      for (int ks = 0; ks < Mma::KSUB; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int jn = 0; jn < 2; ++jn) acc[i][u * 2 + jn] = Mma::mma(bf[jn], af[i], acc[i][u * 2 + jn], ks);
    }
    pin_vmem();
    if (more) stage(buf ^ 1, step + 1);
    __syncthreads();
    buf ^= 1;
  }

  // a lane holds row (grid position) c of a tile and output channels 4q .. 4q + 3 of each 16-column tile
  const bool stat = !P::kLp && a.ep.mode != 0;
  f32x4 cs1[2], cs2[2], bias4[2];
#pragma unroll
  for (int jn = 0; jn < 2; ++jn) {
    cs1[jn] = cs2[jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    bias4[jn] = *reinterpret_cast<const f32x4*>(a.bias + co0 + jn * 16 + 4 * q);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m_tile * BM + row0 + i * 16 + c;
    if (m >= a.M) continue;
    const int img = m / (a.SH * a.SW), rem = m - img * (a.SH * a.SW);
    const int y = rem / a.SW, x = rem - y * a.SW;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t pix = ((size_t)img * 2 * a.SH + 2 * y + (u >> 1)) * 2 * a.SW + 2 * x + (u & 1);
      float* orow = a.out + pix * a.out_ld + co0;
#pragma unroll
      for (int jn = 0; jn < 2; ++jn) {
        f32x4 v = acc[i][u * 2 + jn] + bias4[jn];
        if constexpr (RELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        *reinterpret_cast<f32x4*>(orow + jn * 16 + 4 * q) = v;
        cs1[jn] += v;
        cs2[jn] += v * v;
      }
    }
  }
  if (!stat) return;
  float* red = smem;                                                  // [wave][2][32]; the main loop ended with a barrier
#pragma unroll
  for (int jn = 0; jn < 2; ++jn)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v1 = cs1[jn][e], v2 = cs2[jn][e];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        v1 += __shfl_xor(v1, off, 64);
        v2 += __shfl_xor(v2, off, 64);
      }
      if (c == 0) {
        red[(wave * 2 + 0) * 32 + jn * 16 + 4 * q + e] = v1;
        red[(wave * 2 + 1) * 32 + jn * 16 + 4 * q + e] = v2;
      }
    }
  __syncthreads();
  float* sums = smem + kWaves * 2 * 32;                               // [2][32]
  if (t < 64) {
    const int sidx = t >> 5, col = t & 31;
    float v = red[(0 * 2 + sidx) * 32 + col];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += red[(w * 2 + sidx) * 32 + col];
    sums[sidx * 32 + col] = v;
  }
  __syncthreads();
  fm_stat_publish(a.ep, m_tile, co0, 32, sums);
}

// The 4x4 <-> 1x1 layers (deconv1 forward, conv6's data gradient: mode 3, sixteen one-tap classes) at a handful of rows:
// the rows are the IMAGES, so at 8 images a 128-row tile is 94 % padding, and each of the 128 (class, column tile)
// workgroups staged 80 KB of weights through LDS for five K steps: 24-25 us for 2 M MACs per image.  Here a WAVE owns one
// (class, 16 columns) tile: its weights (16 rows x C <= 160, 640 contiguous bytes per row) go straight into MFMA operands,
// the 16-row tiles of images are looped with the weights kept in registers; no LDS, no barrier.  Epilogue as k_fm_gemm's
// (bias, activation, accumulate, statistics modes 1 / 3 / 4); a wave adds its 16 columns' sums to the accumulators itself.
constexpr int kFmRowsMaxC = 160;
__global__ __launch_bounds__(kThreads) void k_fm_rows_cls(FmGemmArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int ntile_count = a.N / 16;
  const int tile = blockIdx.x * kWaves + wave;                         // (class, column tile)
  if (tile >= 16 * ntile_count) return;
  const int cls = tile / ntile_count, n0 = (tile - cls * ntile_count) * 16;
  const FmClass kc = fm_class(a, cls);
  const int nk = a.C / 16;                                             // k groups of 16 (C is a multiple of 32)
  f32x4 wf[kFmRowsMaxC / 16];
  const float* wrow = static_cast<const float*>(a.w) + kc.w_off + (size_t)(n0 + c) * a.C + 4 * q;
#pragma unroll
  for (int t = 0; t < kFmRowsMaxC / 16; ++t) wf[t] = t < nk ? *reinterpret_cast<const f32x4*>(wrow + 16 * t) : f32x4{0.f, 0.f, 0.f, 0.f};
  const int col = n0 + 4 * q;
  const bool stat = a.ep.mode != 0 && n0 < a.ep.cols;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (a.bias != nullptr) bias4 = *reinterpret_cast<const f32x4*>(a.bias + col);
  f32x4 cs1 = {0.f, 0.f, 0.f, 0.f}, cs2 = {0.f, 0.f, 0.f, 0.f};
  for (int m0 = 0; m0 < a.M; m0 += 16) {
    const int m = m0 + c;
    const bool live = m < a.M;
    const float* arow = a.src + (size_t)(live ? m : a.M - 1) * a.SH * a.SW * a.src_ld + 4 * q;   // (SH = SW = 1: the image's one pixel)
    // the epilogue's operands go out with the row operands: one memory round trip per row tile instead of two
    const size_t pix = fm_out_pixel_index(a, kc, live ? m : a.M - 1);
    float* o = a.out + pix * a.out_ld + col;
    const bool st_on = stat && col < a.ep.cols;
    f32x4 prev = {0.f, 0.f, 0.f, 0.f}, yv = prev, xv = prev, mu = prev, is = prev;
    if (a.accumulate) prev = *reinterpret_cast<const f32x4*>(o);
    if (st_on && (a.ep.mode == 2 || a.ep.mode == 3)) yv = *reinterpret_cast<const f32x4*>(a.ep.y + pix * a.ep.y_ld + col);
    if (st_on && a.ep.mode == 2) {
      xv = *reinterpret_cast<const f32x4*>(a.ep.x + pix * a.ep.x_ld + col);
      mu = *reinterpret_cast<const f32x4*>(a.ep.mean + col);
      is = *reinterpret_cast<const f32x4*>(a.ep.invstd + col);
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < kFmRowsMaxC / 16; ++t) {
      if (t >= nk) break;
      const f32x4 av = *reinterpret_cast<const f32x4*>(arow + 16 * t);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = mfma16(wf[t][e], live ? av[e] : 0.f, acc);
    }
    if (!live) continue;
    f32x4 v = acc + bias4;
    v = f32x4{fm_act(v[0], a.act), fm_act(v[1], a.act), fm_act(v[2], a.act), fm_act(v[3], a.act)};
    v += prev;
    if (st_on) fm_stat_terms(a.ep.mode, v, yv, xv, mu, is, cs1, cs2);
    *reinterpret_cast<f32x4*>(o) = v;
  }
  if (!stat) return;
  const int nsums = a.ep.mode <= 2 ? 2 : 1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v1 = cs1[e], v2 = cs2[e];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {                           // over the 16 lanes that hold the tile's rows
      v1 += __shfl_xor(v1, off, 64);
      v2 += __shfl_xor(v2, off, 64);
    }
    if (c == 0 && col + e < a.ep.cols) {
      const int rep = tile & (a.ep.replicas - 1);
      fm_fix_add(a.ep.acc + (((size_t)rep * 2 + 0) * a.ep.cols + col + e) * 2, v1);
      if (nsums == 2) fm_fix_add(a.ep.acc + (((size_t)rep * 2 + 1) * a.ep.cols + col + e) * 2, v2);
    }
  }
}

// split-K epilogue: out = act(bias + sum of the partial sums in split order) [+ out], and the epilogue statistics of the
// finished values.  Workgroup = (slab of 64 output columns, blockIdx.x) x (chunk of `rows_per_block` global rows r = cls *
// M + m, blockIdx.y); threads = 16 float4 column groups x 16 row lanes: a statistics accumulator receives one add per row
// chunk (adds to ONE address serialise at ~66 ns each: measured 25 us for 256 workgroups adding to the same 2,048 words).
constexpr int kFmRedSlab = 64;
__global__ __launch_bounds__(kThreads) void k_fm_splitk_reduce(FmGemmArgs a, int ncls) {
  __shared__ __attribute__((aligned(16))) float lane_sums[2 * kThreads * 4];
  __shared__ __attribute__((aligned(16))) float sums[2 * kFmRedSlab];
  const int t = threadIdx.x;
  const int cg = t & 15, lane = t >> 4;
  const int col = blockIdx.x * kFmRedSlab + 4 * cg;
  const bool col_on = col < a.N;                                        // N is a multiple of 4, not always of 64 (160)
  const int64_t R = (int64_t)ncls * a.M;
  const int64_t r0 = (int64_t)blockIdx.y * a.rows_per_block;
  const int64_t r1 = r0 + a.rows_per_block < R ? r0 + a.rows_per_block : R;
  const bool stat = a.ep.mode != 0 && (int)blockIdx.x * kFmRedSlab < a.ep.cols;
  const bool col_stat = stat && col < a.ep.cols;
  const size_t stride = (size_t)a.M * a.N;
  f32x4 cs1 = {0.f, 0.f, 0.f, 0.f}, cs2 = {0.f, 0.f, 0.f, 0.f};
  if (col_on) {
    const f32x4 bias = a.bias != nullptr ? *reinterpret_cast<const f32x4*>(a.bias + col) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t r = r0 + lane; r < r1; r += 16) {
      const int m = (int)(r % a.M), cls = (int)(r / a.M);
      const FmClass kc = fm_class(a, cls);
      const size_t pix = fm_out_pixel_index(a, kc, m);
      f32x4 s = bias;
      const int first = a.cls_units > 0 ? fm_unit_first(cls, a.cls_units) : cls * a.nsplit;
      const int count = a.cls_units > 0 ? fm_unit_count(cls, a.cls_units) : a.nsplit;
      const float* p = a.part + ((size_t)first * a.M + m) * a.N + col;
      int sp = 0;
      for (; sp + 8 <= count; sp += 8) {                               // 8 loads in flight, added in split order
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4*>(p + (size_t)(sp + u) * stride);
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
      }
      for (; sp < count; ++sp) s += *reinterpret_cast<const f32x4*>(p + (size_t)sp * stride);
      s = f32x4{fm_act(s[0], a.act), fm_act(s[1], a.act), fm_act(s[2], a.act), fm_act(s[3], a.act)};
      float* o = a.out + pix * a.out_ld + col;
      if (a.accumulate) s += *reinterpret_cast<const f32x4*>(o);
      if (col_stat) fm_stat_terms(a.ep, pix, col, s, cs1, cs2);
      *reinterpret_cast<f32x4*>(o) = s;
    }
  }
  if (!stat) return;
  // the 16 row lanes' sums, in lane order
  *reinterpret_cast<f32x4*>(lane_sums + (lane * 2 + 0) * kFmRedSlab + 4 * cg) = cs1;
  *reinterpret_cast<f32x4*>(lane_sums + (lane * 2 + 1) * kFmRedSlab + 4 * cg) = cs2;
  __syncthreads();
  if (t < 2 * kFmRedSlab) {
    const int sidx = t / kFmRedSlab, c = t - sidx * kFmRedSlab;
    float v = lane_sums[sidx * kFmRedSlab + c];
#pragma unroll
    for (int l = 1; l < 16; ++l) v += lane_sums[(l * 2 + sidx) * kFmRedSlab + c];
    sums[sidx * kFmRedSlab + c] = v;
  }
  __syncthreads();
  fm_stat_publish(a.ep, (int)blockIdx.y, blockIdx.x * kFmRedSlab, kFmRedSlab, sums);
}

// ------------------------------------------------------------------------------------------ k_fm_wgrad
// Workgroup = (64 rows j of dW) x (KT columns of one tap) x (one chunk of pixels).  The 4 waves take interleaved 4-pixel
// steps of the chunk (one MFMA k = 4 pixels), accumulate in registers and add their results through LDS (k_wgrad).
// Lane (c, q) of a step reads pixel q's dense channels 4c..4c+3 and gathered channels NV c .. NV c + NV-1: MFMA tile (u, v)
// holds dW rows {4c + u} x columns {NV c + v}.
struct FmWgradArgs {
  const float* dense; const float* gath; float* slabs;
  int dense_ld, hw_shift, dw_shift;   // pixels m = (image*DH + y)*DW + x (DH, DW powers of two: log2(DH*DW), log2(DW)), J channels
  int gath_ld, SH, SW, ss, KH, KW, pad;
  int J, C, M;
  int rows_per_chunk;                 // multiple of 16
  int jtiles, ktiles_per_tap;
  int64_t slab_floats;                // J * KH*KW * C
};
constexpr int kFmWgPF = 6;
// JT = 16: the refinement layers (16 and 3 output channels): one 16-row tile of dW instead of a 64-row tile that is 75 %
// padding; lane (c, q) then reads the ONE dense channel c of pixel q.
template <int KT, int JT> constexpr int fm_wgrad_lds_floats() { return kWaves * JT * KT; }

// (A variant in which every WAVE owns a tile over all the pixels and stores it from registers -- no LDS sum, no barrier --
// was measured for the deep layers, few pixels and thousands of tiles: -0.7 % of the batch-8 step, +24 % at batch 32.)
template <int KT, int JT>
__global__ __launch_bounds__(kThreads) void k_fm_wgrad(FmWgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NV = KT / 16, NU = JT / 16;
  typedef float gvec __attribute__((ext_vector_type(NV)));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int jt = blockIdx.x % a.jtiles, kt = blockIdx.x / a.jtiles;
  const int tap = kt / a.ktiles_per_tap, k0 = (kt - tap * a.ktiles_per_tap) * KT;
  const int kh = tap / a.KW, kw = tap - kh * a.KW;
  const int j0 = jt * JT;
  const int rbeg = blockIdx.y * a.rows_per_chunk;
  const int rend = rbeg + a.rows_per_chunk < a.M ? rbeg + a.rows_per_chunk : a.M;
  const int nsteps = (rend - rbeg + 15) >> 4;
  const bool j_on = j0 + NU * c < a.J;                               // NU = 4: J is a multiple of 4, a float4 is all in or all out
  const int jc = j_on ? j0 + NU * c : 0;
  const int kcx = k0 + NV * c < a.C ? k0 + NV * c : 0;
  const bool k_on = k0 + NV * c < a.C;

  f32x4 acc[NU][NV];
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[u][v] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int PF = kFmWgPF;
  f32x4 rd[PF];
  gvec rg[PF];
  bool okd[PF], okg[PF];
  auto load = [&](int step, int p) {
    int m = rbeg + 16 * step + 4 * wave + q;
    const bool live = m < rend;
    m = live ? m : rend - 1;
    const int img = m >> a.hw_shift, rem = m - (img << a.hw_shift);
    const int y = rem >> a.dw_shift, x = rem - (y << a.dw_shift);
    const int yy = y * a.ss - a.pad + kh, xx = x * a.ss - a.pad + kw;
    const bool in = (unsigned)yy < (unsigned)a.SH && (unsigned)xx < (unsigned)a.SW;
    if (NU == 4) rd[p] = ldg4<4>(a.dense + (size_t)m * a.dense_ld + jc);
    else rd[p] = f32x4{a.dense[(size_t)m * a.dense_ld + jc], 0.f, 0.f, 0.f};
    const float* gp = a.gath + ((size_t)img * a.SH * a.SW + (in ? yy * a.SW + xx : 0)) * a.gath_ld + kcx;
    rg[p] = *reinterpret_cast<const gvec*>(gp);
    okd[p] = live && j_on;
    okg[p] = live && in && k_on;
  };
  auto mma = [&](int p) {
    const f32x4 vd = okd[p] ? rd[p] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float g = okg[p] ? rg[p][v] : 0.f;
#pragma unroll
      for (int u = 0; u < NU; ++u) acc[u][v] = mfma16(vd[u], g, acc[u][v]);
    }
  };
#pragma unroll
  for (int p = 0; p < PF; ++p) load(p < nsteps ? p : 0, p);
  pin_vmem();
  int step = 0;
  for (; step + PF <= nsteps; step += PF) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const f32x4 vd = okd[p] ? rd[p] : f32x4{0.f, 0.f, 0.f, 0.f};
      float g[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) g[v] = okg[p] ? rg[p][v] : 0.f;
      const int nxt = step + p + PF;
      load(nxt < nsteps ? nxt : nsteps - 1, p);
      pin_vmem();
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int u = 0; u < NU; ++u) acc[u][v] = mfma16(vd[u], g[v], acc[u][v]);
    }
  }
  const int rem_steps = nsteps - step;
#pragma unroll
  for (int p = 0; p < PF; ++p)
    if (p < rem_steps) mma(p);

  float* slab = a.slabs + (size_t)blockIdx.y * a.slab_floats;
  const int ktot = a.KH * a.KW * a.C;
  // cross-wave sum through LDS: image [JT j][KT k] per wave; C tile (u, v): lane holds row 4q + i -> j = NU (4q + i) + u,
  // column c -> k = NV c + v
  float* mine = smem + wave * (JT * KT);
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gvec tv;
#pragma unroll
      for (int v = 0; v < NV; ++v) tv[v] = acc[u][v][i];
      *reinterpret_cast<gvec*>(mine + (NU * (4 * q + i) + u) * KT + NV * c) = tv;
    }
  __syncthreads();
  for (int e = threadIdx.x; e < JT * KT / 4; e += kThreads) {
    const int j = e / (KT / 4), k = 4 * (e % (KT / 4));
    f32x4 s = *reinterpret_cast<const f32x4*>(smem + j * KT + k);
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += *reinterpret_cast<const f32x4*>(smem + w * (JT * KT) + j * KT + k);
    if (j0 + j < a.J && k0 + k < a.C)
      *reinterpret_cast<f32x4*>(slab + (size_t)(j0 + j) * ktot + tap * a.C + k0 + k) = s;
  }
}

// conv_refine_1 (32 -> 16 channels, 3x3): ONE workgroup per pixel chunk takes all nine taps.  As nine k_fm_wgrad<32, 16>
// tiles the layer read its 16-channel gradient map nine times and issued a load per MFMA (169 us at 32 images, the
// matrix pipe 17 % busy); here a step reads the pixel's gradient once and its nine neighbours' 32 channels (L1 hits of
// each other) for 18 MFMAs.  Same lane mapping as k_fm_wgrad<32, 16>: lane (c, q) holds dense channel c of pixel q and
// gathered channels 2c, 2c + 1; tile (tap, v): dW rows j = 4q + i, columns k = 2c + v.
constexpr int kFmWgTapsPF = 4;
__global__ __launch_bounds__(kThreads) void k_fm_wgrad_taps9(FmWgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int KT = 32, JT = 16, NV = 2, TAPS = 9, PF = kFmWgTapsPF;
  typedef float gvec __attribute__((ext_vector_type(NV)));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int rbeg = blockIdx.y * a.rows_per_chunk;
  const int rend = rbeg + a.rows_per_chunk < a.M ? rbeg + a.rows_per_chunk : a.M;
  const int nsteps = (rend - rbeg + 15) >> 4;
  const bool j_on = c < a.J;
  const int jc = j_on ? c : 0;

  f32x4 acc[TAPS][NV];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[t][v] = f32x4{0.f, 0.f, 0.f, 0.f};
  float rd[PF];
  gvec rg[PF][TAPS];
  bool okd[PF];
  unsigned okg[PF];                                                   // bit t: tap t is inside the map
  auto load = [&](int step, int p) {
    int m = rbeg + 16 * step + 4 * wave + q;
    const bool live = m < rend;
    m = live ? m : rend - 1;
    const int img = m >> a.hw_shift, rem = m - (img << a.hw_shift);
    const int y = rem >> a.dw_shift, x = rem - (y << a.dw_shift);
    rd[p] = a.dense[(size_t)m * a.dense_ld + jc];
    okd[p] = live && j_on;
    const float* gbase = a.gath + (size_t)img * a.SH * a.SW * a.gath_ld + NV * c;
    unsigned bits = 0u;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      const int yy = y - 1 + t / 3, xx = x - 1 + t % 3;               // stride 1, pad 1
      const bool in = (unsigned)yy < (unsigned)a.SH && (unsigned)xx < (unsigned)a.SW;
      rg[p][t] = *reinterpret_cast<const gvec*>(gbase + (size_t)(in ? yy * a.SW + xx : 0) * a.gath_ld);
      bits |= (live && in) ? (1u << t) : 0u;
    }
    okg[p] = bits;
  };
  auto mma = [&](int p) {
    const float vd = okd[p] ? rd[p] : 0.f;
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[t][v] = mfma16(vd, (okg[p] >> t) & 1u ? rg[p][t][v] : 0.f, acc[t][v]);
  };
#pragma unroll
  for (int p = 0; p < PF; ++p) load(p < nsteps ? p : 0, p);
  pin_vmem();
  int step = 0;
  for (; step + PF <= nsteps; step += PF) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const float vd = okd[p] ? rd[p] : 0.f;
      float g[TAPS][NV];
#pragma unroll
      for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int v = 0; v < NV; ++v) g[t][v] = (okg[p] >> t) & 1u ? rg[p][t][v] : 0.f;
      const int nxt = step + p + PF;
      load(nxt < nsteps ? nxt : nsteps - 1, p);
      pin_vmem();
#pragma unroll
      for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[t][v] = mfma16(vd, g[t][v], acc[t][v]);
    }
  }
  const int rem_steps = nsteps - step;
#pragma unroll
  for (int p = 0; p < PF; ++p)
    if (p < rem_steps) mma(p);

  // cross-wave sums through LDS, [wave][tap][JT j][KT k]; then slab[j][tap][k], wave order
  float* slab = a.slabs + (size_t)blockIdx.y * a.slab_floats;
  float* mine = smem + wave * (TAPS * JT * KT);
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<gvec*>(mine + (t * JT + 4 * q + i) * KT + NV * c) = gvec{acc[t][0][i], acc[t][1][i]};
  __syncthreads();
  for (int e = threadIdx.x; e < TAPS * JT * KT / 4; e += kThreads) {
    const int k = 4 * (e % (KT / 4)), j = (e / (KT / 4)) % JT, t = e / (JT * KT / 4);
    f32x4 sum = *reinterpret_cast<const f32x4*>(smem + (t * JT + j) * KT + k);
#pragma unroll
    for (int w = 1; w < kWaves; ++w) sum += *reinterpret_cast<const f32x4*>(smem + w * (TAPS * JT * KT) + (t * JT + j) * KT + k);
    if (j < a.J && k < a.C) *reinterpret_cast<f32x4*>(slab + (size_t)j * (TAPS * a.C) + t * a.C + k) = sum;
  }
}
constexpr int fm_wgrad_taps9_lds_floats() { return kWaves * 9 * 16 * 32; }

// grad[i] = sum over chunks of slab[chunk][i], in chunk order -- for every layer whose weight gradient was computed
// in row chunks, in ONE launch at the end of the backward pass: workgroup -> segment by its block range.
constexpr int kFmMaxSeg = 16;
struct FmSlabSumArgs {
  int nseg;
  int remap_seg;                     // -1, or the segment that holds conv1's gradient in the column form [64][32]: its sums go
                                     // to the parameters' [64][9][32] (n4 of that segment = the 4,608 float4 of the destination)
  int block_begin[kFmMaxSeg + 1];
  const float* slabs[kFmMaxSeg]; float* grad[kFmMaxSeg]; int nchunks[kFmMaxSeg]; int64_t n4[kFmMaxSeg];
};
__global__ __launch_bounds__(kThreads) void k_fm_slab_sum(FmSlabSumArgs a) {
  int seg = 0;
  while (seg + 1 < a.nseg && (int)blockIdx.x >= a.block_begin[seg + 1]) ++seg;
  const int64_t i = (int64_t)((int)blockIdx.x - a.block_begin[seg]) * kThreads + threadIdx.x;
  const int64_t n4 = a.n4[seg];
  if (i >= n4) return;
  const int nchunks = a.nchunks[seg];
  if (seg == a.remap_seg) {                                            // destination float4 (co, tap, c4): ci = 4 c4 .. + 3
    const int c4 = (int)(i % 8), tp = (int)((i / 8) % 9), co = (int)(i / 72);
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    if (c4 == 0) {
      const float* sl = a.slabs[seg] + co * 32 + tp * 3;
      int ch = 0;
      for (; ch + 8 <= nchunks; ch += 8) {                             // 8 chunks in flight, added in chunk order
        float v[8][3];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float* q = sl + (size_t)(ch + u) * 2048;
          v[u][0] = q[0]; v[u][1] = q[1]; v[u][2] = q[2];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { sum[0] += v[u][0]; sum[1] += v[u][1]; sum[2] += v[u][2]; }
      }
      for (; ch < nchunks; ++ch) {
        const float* q = sl + (size_t)ch * 2048;
        sum[0] += q[0]; sum[1] += q[1]; sum[2] += q[2];
      }
    }
    reinterpret_cast<f32x4*>(a.grad[seg])[i] = sum;
    return;
  }
  const f32x4* sl = reinterpret_cast<const f32x4*>(a.slabs[seg]);
  f32x4 sum = sl[i];
  int ch = 1;
  for (; ch + 8 <= nchunks; ch += 8) {                                // 8 loads in flight, added in chunk order
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = sl[(size_t)(ch + u) * n4 + i];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u];
  }
  for (; ch < nchunks; ++ch) sum += sl[(size_t)ch * n4 + i];
  reinterpret_cast<f32x4*>(a.grad[seg])[i] = sum;
}

// ------------------------------------------------------------------------------------------ BatchNorm helpers
// eval mode: mean / invstd from the running statistics
__global__ __launch_bounds__(kThreads) void k_fm_bn_eval_stats(const float* running_mean, const float* running_var, int C,
                                                              float eps, float* mean, float* invstd) {
  const int ch = blockIdx.x * kThreads + threadIdx.x;
  if (ch >= C) return;
  mean[ch] = running_mean[ch];
  invstd[ch] = 1.0f / sqrtf(running_var[ch] + eps);
}

// ------------------------------------------------------------------------------------------ elementwise passes
// What the consumer of a statistics accumulator makes of it, per channel, in its prologue (every workgroup for itself;
// workgroup 0 also writes the results the later kernels and the caller read):
//   what 0  BatchNorm forward: mean, invstd (biased variance), the rounding residual of the mean (see what 2) and, when
//           running != null, the running statistics (momentum, unbiased variance; torch.nn.functional.batch_norm)
//   what 1  out1 = sum 1 (bias gradients: k_fm_bias_finish)
//   what 2  BatchNorm backward: out1 = d beta = sum 1, out2 = d gamma = sum 2, out3 = the gradient of the bias of the
//           convolution in front: the column sum of dx = gamma invstd (g - sum1 / P - xhat sum2 / P), which is
//           -gamma invstd sum2 / P * sum(xhat), and sum(xhat) = P invstd (mean - fl(mean)): zero but for the rounding of
//           the stored mean (the reference's value is rounding noise of its own); no further pass over the map.
struct FmStatFin {
  const long long* acc; int replicas, what, P;       // acc == null: nothing to do (eval mode: mean / invstd are given)
  const long long* acc_local;                        // cross-rank statistics (ndp_fm_stat_sync_fn): acc holds the sums over ALL
                                                     // ranks (P counts their pixels), acc_local this rank's -- what 2 writes
                                                     // d beta / d gamma / the bias gradient from the LOCAL sums (the gradient
                                                     // all-reduce adds the ranks' up), dx uses the global ones; null: acc
  float* out1; float* out2; float* out3; float* running_mean; float* running_var; float* meanres; const float* gamma;
  const float* invstd; float eps, momentum;
};
// the two per-channel values the consumer's elementwise pass uses: (mean, invstd) for what 0, (sum 1, sum 2) for what 2
__device__ __forceinline__ void fm_stat_finish(const FmStatFin& a, int cols, int ch, bool write, float& r1, float& r2) {
  const double t1 = fm_fix_read(a.acc, a.replicas, cols, 0, ch);
  const double t2 = a.what == 1 ? 0.0 : fm_fix_read(a.acc, a.replicas, cols, 1, ch);
  if (a.what == 0) {
    const double mean = t1 / a.P;
    double var = t2 / a.P - mean * mean;
    var = var > 0.0 ? var : 0.0;
    r1 = (float)mean;
    r2 = (float)(1.0 / sqrt(var + (double)a.eps));
    if (write) {
      a.out1[ch] = r1;
      a.out2[ch] = r2;
      a.meanres[ch] = (float)(mean - (double)(float)mean);
      if (a.running_mean != nullptr) {
        const double unbiased = a.P > 1 ? var * ((double)a.P / (double)(a.P - 1)) : var;
        a.running_mean[ch] = (float)((1.0 - a.momentum) * (double)a.running_mean[ch] + a.momentum * mean);
        a.running_var[ch] = (float)((1.0 - a.momentum) * (double)a.running_var[ch] + a.momentum * unbiased);
      }
    }
  } else {
    r1 = (float)t1;
    r2 = (float)t2;
    if (write) {
      double l1 = t1, l2 = t2;
      if (a.acc_local != nullptr) {
        l1 = fm_fix_read(a.acc_local, a.replicas, cols, 0, ch);
        l2 = a.what == 1 ? 0.0 : fm_fix_read(a.acc_local, a.replicas, cols, 1, ch);
      }
      a.out1[ch] = (float)l1;
      if (a.out2 != nullptr) a.out2[ch] = (float)l2;
      if (a.what == 2) {
        const double is = (double)a.invstd[ch];
        a.out3[ch] = (float)(-(double)a.gamma[ch] * is * is * l2 * (double)a.meanres[ch]);
      }
    }
  }
}

struct FmEltArgs {
  const float* x; const float* y; const float* dy; float* out;
  const float* mean; const float* invstd; const float* gamma; const float* beta; const float* sum1; const float* sum2;
  int x_ld, y_ld, dy_ld, out_ld, C, P;
  int zero_to;                        // k_fm_bn_apply: output channels C .. zero_to-1 are written as zeros (see FmGemmArgs)
  int iters;                          // batches of kFmEltPerThread float4 per thread (the statistics prologue is paid once per workgroup)
  FmStatFin fin;
};
constexpr int kFmMaxBnC = 1024;
constexpr int kFmEltPerThread = 4;
// y = relu(gamma * (x - mean) * invstd + beta); training mode: mean / invstd from the accumulators the producer of x filled
__global__ __launch_bounds__(kThreads) void k_fm_bn_apply(FmEltArgs a) {
  __shared__ __attribute__((aligned(16))) float sh1[kFmMaxBnC], sh2[kFmMaxBnC];
  for (int ch = threadIdx.x; ch < a.C; ch += kThreads) {
    if (a.fin.acc != nullptr) fm_stat_finish(a.fin, a.C, ch, blockIdx.x == 0, sh1[ch], sh2[ch]);
    else { sh1[ch] = a.mean[ch]; sh2[ch] = a.invstd[ch]; }
  }
  __syncthreads();
  const int c4 = (a.zero_to > a.C ? a.zero_to : a.C) / 4;
  const int64_t total = (int64_t)a.P * c4;
  // kFmEltPerThread float4 per thread (the prologue above is paid once per 4 KB instead of once per 1 KB), loads first
  for (int it = 0; it < a.iters; ++it) {
    f32x4 xv[kFmEltPerThread];
    int cgv[kFmEltPerThread];
    int64_t pv[kFmEltPerThread];
#pragma unroll
    for (int k = 0; k < kFmEltPerThread; ++k) {
      const int64_t i = (((int64_t)blockIdx.x * a.iters + it) * kFmEltPerThread + k) * kThreads + threadIdx.x;
      cgv[k] = (int)(i % c4);
      pv[k] = i < total ? i / c4 : -1;
      xv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (pv[k] >= 0 && 4 * cgv[k] < a.C) xv[k] = *reinterpret_cast<const f32x4*>(a.x + pv[k] * a.x_ld + 4 * cgv[k]);
    }
#pragma unroll
    for (int k = 0; k < kFmEltPerThread; ++k) {
      if (pv[k] < 0) continue;
      const int cg = cgv[k];
      f32x4 y = {0.f, 0.f, 0.f, 0.f};
      if (4 * cg < a.C) {
        const f32x4 mu = *reinterpret_cast<const f32x4*>(sh1 + 4 * cg), is = *reinterpret_cast<const f32x4*>(sh2 + 4 * cg);
        const f32x4 ga = *reinterpret_cast<const f32x4*>(a.gamma + 4 * cg), be = *reinterpret_cast<const f32x4*>(a.beta + 4 * cg);
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = fmaxf((xv[k][e] - mu[e]) * is[e] * ga[e] + be[e], 0.f);
      }
      *reinterpret_cast<f32x4*>(a.out + pv[k] * a.out_ld + 4 * cg) = y;
    }
  }
}
// BatchNorm + ReLU backward: g = dy * (y > 0); dx = gamma * invstd * (g - sum1 / P - xhat * sum2 / P), written over x;
// sum1 = d beta, sum2 = d gamma from the accumulators the producer of dy filled
__global__ __launch_bounds__(kThreads) void k_fm_bn_bwd_apply(FmEltArgs a) {
  __shared__ __attribute__((aligned(16))) float sh1[kFmMaxBnC], sh2[kFmMaxBnC];
  for (int ch = threadIdx.x; ch < a.C; ch += kThreads) {
    if (a.fin.acc != nullptr) fm_stat_finish(a.fin, a.C, ch, blockIdx.x == 0, sh1[ch], sh2[ch]);
    else { sh1[ch] = a.sum1[ch]; sh2[ch] = a.sum2[ch]; }
  }
  __syncthreads();
  const int c4 = a.C / 4;
  const int64_t total = (int64_t)a.P * c4;
  const float invp = 1.0f / (float)(a.fin.acc != nullptr ? a.fin.P : a.P);   // (cross-rank statistics: all ranks' pixels)
  for (int it = 0; it < a.iters; ++it) {
    f32x4 xv[kFmEltPerThread], yv[kFmEltPerThread], dv[kFmEltPerThread];
    int cgv[kFmEltPerThread];
    int64_t pv[kFmEltPerThread];
#pragma unroll
    for (int k = 0; k < kFmEltPerThread; ++k) {
      const int64_t i = (((int64_t)blockIdx.x * a.iters + it) * kFmEltPerThread + k) * kThreads + threadIdx.x;
      cgv[k] = (int)(i % c4);
      pv[k] = i < total ? i / c4 : -1;
      xv[k] = yv[k] = dv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (pv[k] >= 0) {
        xv[k] = *reinterpret_cast<const f32x4*>(a.x + pv[k] * a.x_ld + 4 * cgv[k]);
        yv[k] = *reinterpret_cast<const f32x4*>(a.y + pv[k] * a.y_ld + 4 * cgv[k]);
        dv[k] = *reinterpret_cast<const f32x4*>(a.dy + pv[k] * a.dy_ld + 4 * cgv[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < kFmEltPerThread; ++k) {
      if (pv[k] < 0) continue;
      const int cg = cgv[k];
      const f32x4 mu = *reinterpret_cast<const f32x4*>(a.mean + 4 * cg), is = *reinterpret_cast<const f32x4*>(a.invstd + 4 * cg);
      const f32x4 ga = *reinterpret_cast<const f32x4*>(a.gamma + 4 * cg);
      const f32x4 s1 = *reinterpret_cast<const f32x4*>(sh1 + 4 * cg), s2 = *reinterpret_cast<const f32x4*>(sh2 + 4 * cg);
      f32x4 dx;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float g = yv[k][e] > 0.f ? dv[k][e] : 0.f;
        const float xhat = (xv[k][e] - mu[e]) * is[e];
        dx[e] = ga[e] * is[e] * (g - s1[e] * invp - xhat * (s2[e] * invp));
      }
      *reinterpret_cast<f32x4*>(a.out + pv[k] * a.out_ld + 4 * cg) = dx;
    }
  }
}
// BatchNorm + ReLU backward for RUNNING statistics (eval mode: mean and invstd are constants of the input, so no batch sum
// enters): dx = [y > 0] * dy * gamma * invstd, written over x; invstd as k_fm_bn_eval_stats left it.
__global__ __launch_bounds__(kThreads) void k_fm_bn_eval_bwd_apply(FmEltArgs a) {
  const int c4 = a.C / 4;
  const int64_t total = (int64_t)a.P * c4;
  for (int it = 0; it < a.iters; ++it) {
    f32x4 yv[kFmEltPerThread], dv[kFmEltPerThread];
    int cgv[kFmEltPerThread];
    int64_t pv[kFmEltPerThread];
#pragma unroll
    for (int k = 0; k < kFmEltPerThread; ++k) {
      const int64_t i = (((int64_t)blockIdx.x * a.iters + it) * kFmEltPerThread + k) * kThreads + threadIdx.x;
      cgv[k] = (int)(i % c4);
      pv[k] = i < total ? i / c4 : -1;
      yv[k] = dv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (pv[k] >= 0) {
        yv[k] = *reinterpret_cast<const f32x4*>(a.y + pv[k] * a.y_ld + 4 * cgv[k]);
        dv[k] = *reinterpret_cast<const f32x4*>(a.dy + pv[k] * a.dy_ld + 4 * cgv[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < kFmEltPerThread; ++k) {
      if (pv[k] < 0) continue;
      const int cg = cgv[k];
      const f32x4 is = *reinterpret_cast<const f32x4*>(a.invstd + 4 * cg), ga = *reinterpret_cast<const f32x4*>(a.gamma + 4 * cg);
      f32x4 dx;
#pragma unroll
      for (int e = 0; e < 4; ++e) dx[e] = yv[k][e] > 0.f ? dv[k][e] * (ga[e] * is[e]) : 0.f;
      *reinterpret_cast<f32x4*>(a.out + pv[k] * a.out_ld + 4 * cg) = dx;
    }
  }
}

// Data gradient of conv1 (3 -> 64, 3x3, stride 2, pad 1) in gather form, plus the identity of the eval-mode output
// (out = state_cur + residual):  d_cur[n][ci][ih][iw] = d_out[n][ci][ih][iw] + sum over the taps (kh, kw) with
// ih + 1 - kh = 2 oh, iw + 1 - kw = 2 ow -- at most 2 x 2 output positions -- and the 64 channels of
// draw1[(n, oh, ow)][co] * W[co][kh][kw][ci].  Every sum is taken in one fixed order by one thread: no float atomics.
// One workgroup per (image, oh): output rows oh and oh + 1 of draw1 (2 x 64 pixels x 64 channels, the 1 MB per image that
// bounds the kernel, read as whole 256-byte rows) are staged in LDS and feed input rows 2 oh (needs oh) and 2 oh + 1
// (needs oh and oh + 1), one thread per input pixel.  Row stride 68 floats (lds_ld): the ds_read_b128 of a wave's
// neighbouring pixels spread over the banks.  The blocks behind the images' copy d_actions out of dz's action columns
// (128..131, where k_fm_image_cols put the actions in z); nimg_rows == 0: only those.
// IDENT = false: the training-mode output is the residual alone (ndp_fm_backward_inputs): no d_out term, d_out is not read.
struct FmC1DgArgs {
  const float* draw1; const float* w; const float* d_out; float* d_cur; int64_t nimg_rows;   // nimg_rows = n * 64, or 0
  const float* dz; float* d_actions; int64_t nimg;                                           // d_actions null: no copy
};
constexpr int kFmC1LD = 68;
template <bool IDENT>
__global__ __launch_bounds__(kThreads) void k_fm_conv1_dgrad(FmC1DgArgs a) {
  __shared__ __attribute__((aligned(16))) float D[2 * 64 * kFmC1LD];
  __shared__ __attribute__((aligned(16))) float Ws[27 * 64];               // [k = (kh * 3 + kw) * 3 + ci][co]
  if ((int64_t)blockIdx.x >= a.nimg_rows) {
    const int64_t i = ((int64_t)blockIdx.x - a.nimg_rows) * kThreads + threadIdx.x;
    if (a.d_actions != nullptr && i < a.nimg * 4) a.d_actions[i] = a.dz[(i >> 2) * 160 + 128 + (i & 3)];
    return;
  }
  const int64_t n = (int64_t)blockIdx.x >> 6;
  const int oh = (int)blockIdx.x & 63;
  for (int i = threadIdx.x; i < 27 * 64; i += kThreads) {
    const int co = i & 63, k = i >> 6;                                   // P1 of conv1: [co][tap][ci -> 32]
    Ws[i] = a.w[(size_t)co * 9 * 32 + (k / 3) * 32 + (k % 3)];
  }
  for (int i = threadIdx.x; i < 2 * 64 * 16; i += kThreads) {
    const int c4 = i & 15, px = (i >> 4) & 63, r = i >> 10;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (oh + r < 64) v = *reinterpret_cast<const f32x4*>(a.draw1 + ((n * 64 + oh + r) * 64 + px) * 64 + 4 * c4);
    *reinterpret_cast<f32x4*>(D + (r * 64 + px) * kFmC1LD + 4 * c4) = v;
  }
  __syncthreads();
  const int iw = threadIdx.x & 127, ir = threadIdx.x >> 7;                 // input row 2 oh + ir
  // rows: ir == 0 -> (kh 1, staged row 0); ir == 1 -> (kh 2, row 0), (kh 0, row 1).  Columns alike from iw's parity.
  const int nrow = ir + 1, ncol = (iw & 1) + 1;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int u = 0; u < nrow; ++u) {
    const int kh = ir == 0 ? 1 : (u == 0 ? 2 : 0), r = u;
    for (int v = 0; v < ncol; ++v) {
      const int kw = (iw & 1) == 0 ? 1 : (v == 0 ? 2 : 0);
      const int ow = (iw + 1 - kw) >> 1;
      if (ow >= 64) continue;                                             // (iw = 127, kw = 0: past the map; row oh + 1 = 64 is staged as zeros)
      const float* d = D + (r * 64 + ow) * kFmC1LD;
      const float* w = Ws + (kh * 3 + kw) * 3 * 64;
#pragma unroll 4
      for (int c4 = 0; c4 < 16; ++c4) {
        const f32x4 dv = *reinterpret_cast<const f32x4*>(d + 4 * c4);
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(w + ci * 64 + 4 * c4);
          acc[ci] = fmaf(dv[0], wv[0], acc[ci]); acc[ci] = fmaf(dv[1], wv[1], acc[ci]);
          acc[ci] = fmaf(dv[2], wv[2], acc[ci]); acc[ci] = fmaf(dv[3], wv[3], acc[ci]);
        }
      }
    }
  }
  const int64_t base = n * 3 * 16384 + (int64_t)(2 * oh + ir) * 128 + iw;
#pragma unroll
  for (int ci = 0; ci < 3; ++ci) a.d_cur[base + ci * 16384] = IDENT ? a.d_out[base + ci * 16384] + acc[ci] : acc[ci];
}

// a bias gradient that is a plain column sum (conv4, conv5, conv6): accumulator -> grad, one workgroup
struct FmBiasFinishArgs { FmStatFin fin; int cols; };
__global__ __launch_bounds__(kThreads) void k_fm_bias_finish(FmBiasFinishArgs a) {
  float r1, r2;
  for (int ch = threadIdx.x; ch < a.cols; ch += kThreads) fm_stat_finish(a.fin, a.cols, ch, true, r1, r2);
}

// NCHW image [n][3][128][128] -> NHWC, 32 channels per pixel (3 + zeros).  U8: byte frames [n][128][128][3] instead, turned
// into the reference's [-1, 1] floats on the way (u8_norm_table, ndp_encoder.inc).
// The blocks behind the image's write the code + action row of the decoder: z[n][128..131] = action, [132..159] = 0 (the
// code columns are conv6's output).
template <bool U8>
__global__ __launch_bounds__(kThreads) void k_fm_image_cols(const void* img, int64_t npix, float* out, const float* actions,
                                                            int64_t nimg, float* z, long long* zero, int64_t zero_words) {
  // conv1 (3 -> 64 channels, 3x3, stride 2, pad 1) reads its input as COLUMNS: per output pixel the 27 values of its window,
  // k = (kh * 3 + kw) * 3 + ci, zero-padded to 32 -- one K step of k_fm_gemm per output tile and of k_fm_wgrad per pixel
  // block, where the image as a 32-channel NHWC map (round 2) cost nine, 29 of whose 32 channels were padding.
  // npix = output pixels (4,096 per image).
  __shared__ float lut[256];
  const int64_t image_blocks = (npix + kThreads - 1) / kThreads;
  const int64_t action_blocks = (nimg * 32 + kThreads - 1) / kThreads;
  if ((int64_t)blockIdx.x >= image_blocks + action_blocks) {
    // the first launch of a training pass also zeroes the statistics accumulators (a memset launch of its own before)
    const int64_t i = (((int64_t)blockIdx.x - image_blocks - action_blocks) * kThreads + threadIdx.x) * 2;   // an even count of words
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    if (i < zero_words) *reinterpret_cast<ll2*>(zero + i) = ll2{0, 0};
    return;
  }
  if ((int64_t)blockIdx.x >= image_blocks) {
    const int64_t i = ((int64_t)blockIdx.x - image_blocks) * kThreads + threadIdx.x;
    if (i >= nimg * 32) return;
    const int64_t r = i / 32;
    const int cidx = (int)(i % 32);
    z[r * 160 + 128 + cidx] = cidx < 4 ? actions[r * 4 + cidx] : 0.f;
    return;
  }
  if (U8) {
    u8_norm_table(lut);
    __syncthreads();
  }
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= npix) return;
  const int64_t n = p >> 12;
  const int oh = (int)(p >> 6) & 63, ow = (int)p & 63;
  float v[32];
#pragma unroll
  for (int k = 27; k < 32; ++k) v[k] = 0.f;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = 2 * oh - 1 + kh;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int iw = 2 * ow - 1 + kw;
      const bool ok = (unsigned)ih < 128u && (unsigned)iw < 128u;
      const int64_t pix = ok ? (int64_t)ih * 128 + iw : 0;
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        float x;
        if (U8) x = lut[static_cast<const unsigned char*>(img)[(n * 16384 + pix) * 3 + ci]];
        else x = static_cast<const float*>(img)[(n * 3 + ci) * 16384 + pix];
        v[(kh * 3 + kw) * 3 + ci] = ok ? x : 0.f;
      }
    }
  }
  float* o = out + p * 32;
#pragma unroll
  for (int e = 0; e < 8; ++e) *reinterpret_cast<f32x4*>(o + 4 * e) = f32x4{v[4 * e], v[4 * e + 1], v[4 * e + 2], v[4 * e + 3]};
}
// ------------------------------------------------------------------------------------------ conv_refine_2 (16 -> 3, 3x3)
// 7 M MAC per image and three output channels: as a 128 x 32 GEMM tile it is eight parts padding and moves a 32-wide
// output map; as three small VALU kernels over y2 [pixel][4] (3 channels + a zero) it moves what it needs.
//   forward   y2[p][co] = tanh(b[co] + sum over taps, ci<16  r1[p + tap][ci] * W[co][tap][ci])       one thread per pixel
//   dgrad     dr1[p][ci] = sum over taps, co<3  dy2[p - tap][co] * W[co][tap][ci]                    one thread per pixel
//   wgrad     dW[co][tap][ci] = sum over pixels  dy2[p][co] * r1[p + tap][ci]     thread = (pixel lane, tap, 4 ci); a block's
//             432 sums go to its slab, k_fm_slab_sum adds the blocks in order
// W: the layer's P1 weights [4][9][32] (ci >= 16 and co = 3 are zero padding), staged in LDS.  r1 / dr1: [pixel][16]
// (kFmR1LD: the 16-channel maps of the refinement stage are stored without padding -- with a stride of 32 every pass
// over them moved twice their bytes, HBM lines being 128 bytes).
constexpr int kFmR1LD = 16;
struct FmR2Args { const float* r1; float* y2; const float* w; const float* bias; float* dr1; float* slabs; int64_t npix; int rows_per_block;
                  FmStatEp ep; };   // k_fm_r2_dgrad: the BatchNorm-backward sums of conv_refine_1_bn (mode 2; x, y: [pixel][32] maps)
__device__ __forceinline__ void fm_r2_stage_weights(float* Ws, const float* __restrict__ w) {
  for (int i = threadIdx.x; i < 3 * 9 * 16; i += kThreads) {
    const int ci = i & 15, r = i >> 4;                     // r = co * 9 + tap
    Ws[i] = w[r * 32 + ci];
  }
  __syncthreads();
}
__global__ __launch_bounds__(kThreads) void k_fm_r2_fwd(FmR2Args a) {
  __shared__ __attribute__((aligned(16))) float Ws[3 * 9 * 16];
  fm_r2_stage_weights(Ws, a.w);
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= a.npix) return;
  const int x = (int)(p & 127), y = (int)((p >> 7) & 127);
  float acc[3] = {a.bias[0], a.bias[1], a.bias[2]};
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int yy = y + kh - 1, xx = x + kw - 1;
      if ((unsigned)yy >= 128u || (unsigned)xx >= 128u) continue;
      const float* src = a.r1 + (p + (kh - 1) * 128 + (kw - 1)) * kFmR1LD;
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * c4);
#pragma unroll
        for (int co = 0; co < 3; ++co) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(Ws + (co * 9 + kh * 3 + kw) * 16 + 4 * c4);
          acc[co] = fmaf(v[0], wv[0], acc[co]); acc[co] = fmaf(v[1], wv[1], acc[co]);
          acc[co] = fmaf(v[2], wv[2], acc[co]); acc[co] = fmaf(v[3], wv[3], acc[co]);
        }
      }
    }
  *reinterpret_cast<f32x4*>(a.y2 + p * 4) = f32x4{tanhf(acc[0]), tanhf(acc[1]), tanhf(acc[2]), 0.f};
}
__global__ __launch_bounds__(kThreads) void k_fm_r2_dgrad(FmR2Args a) {
  __shared__ __attribute__((aligned(16))) float Ws[3 * 9 * 16];
  __shared__ __attribute__((aligned(16))) float red[kWaves * 32 + 32];
  fm_r2_stage_weights(Ws, a.w);
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = p < a.npix;
  const int x = (int)(p & 127), y = (int)((p >> 7) & 127);
  f32x4 acc[4], xv[4], yv[4];
#pragma unroll
  for (int c4 = 0; c4 < 4; ++c4) {
    acc[c4] = xv[c4] = yv[c4] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live && a.ep.mode != 0) {                            // operands of the statistics: in flight during the convolution
      xv[c4] = *reinterpret_cast<const f32x4*>(a.ep.x + p * a.ep.x_ld + 4 * c4);
      yv[c4] = *reinterpret_cast<const f32x4*>(a.ep.y + p * a.ep.y_ld + 4 * c4);
    }
  }
  if (live) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int yy = y - (kh - 1), xx = x - (kw - 1);      // the output pixel this input pixel fed through tap (kh, kw)
        if ((unsigned)yy >= 128u || (unsigned)xx >= 128u) continue;
        const f32x4 d = *reinterpret_cast<const f32x4*>(a.y2 + (p - (kh - 1) * 128 - (kw - 1)) * 4);
#pragma unroll
        for (int co = 0; co < 3; ++co)
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(Ws + (co * 9 + kh * 3 + kw) * 16 + 4 * c4);
            acc[c4] += wv * d[co];
          }
      }
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) *reinterpret_cast<f32x4*>(a.dr1 + p * kFmR1LD + 4 * c4) = acc[c4];
  }
  if (a.ep.mode == 0) return;
  // BatchNorm backward sums over this workgroup's 256 pixels: lanes of a wave by shuffles, the 4 waves through LDS in order
  f32x4 s1[4], s2[4];
#pragma unroll
  for (int c4 = 0; c4 < 4; ++c4) {
    s1[c4] = s2[c4] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) {
      const f32x4 mu = *reinterpret_cast<const f32x4*>(a.ep.mean + 4 * c4), is = *reinterpret_cast<const f32x4*>(a.ep.invstd + 4 * c4);
      fm_stat_terms(a.ep.mode, acc[c4], yv[c4], xv[c4], mu, is, s1[c4], s2[c4]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c4 = 0; c4 < 4; ++c4)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v1 = s1[c4][e], v2 = s2[c4][e];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        v1 += __shfl_xor(v1, off, 64);
        v2 += __shfl_xor(v2, off, 64);
      }
      if (lane == 0) {
        red[wave * 32 + 4 * c4 + e] = v1;
        red[wave * 32 + 16 + 4 * c4 + e] = v2;
      }
    }
  __syncthreads();
  float* sums = red + kWaves * 32;
  if (threadIdx.x < 32) sums[threadIdx.x] = ((red[threadIdx.x] + red[32 + threadIdx.x]) + red[64 + threadIdx.x]) + red[96 + threadIdx.x];
  __syncthreads();
  fm_stat_publish(a.ep, (int)blockIdx.x, 0, 16, sums);
}
constexpr int kFmR2Groups = 36;                              // (tap, 4 ci) groups; 7 pixel lanes of 36 threads = 252 of 256
__global__ __launch_bounds__(kThreads) void k_fm_r2_wgrad(FmR2Args a) {
  __shared__ __attribute__((aligned(16))) float sh[7 * 36 * 12];
  const int grp = threadIdx.x % kFmR2Groups, lane = threadIdx.x / kFmR2Groups;      // lane 7: the 4 spare threads idle
  const int tap = grp >> 2, c4 = grp & 3;
  const int kh = tap / 3, kw = tap - 3 * kh;
  const int64_t p0 = (int64_t)blockIdx.x * a.rows_per_block;
  const int64_t p1 = p0 + a.rows_per_block < a.npix ? p0 + a.rows_per_block : a.npix;
  f32x4 acc[3];
#pragma unroll
  for (int co = 0; co < 3; ++co) acc[co] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (lane < 7) {
    // 4 pixels in flight per thread (unconditional loads from a clamped address, zeroed by a select: a branch around a
    // load would serialise them), added in pixel order
    for (int64_t pb = p0 + lane; pb < p1; pb += 28) {
      f32x4 d[4], v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t p = pb + 7 * u;
        const int x = (int)(p & 127), y = (int)((p >> 7) & 127);
        const int yy = y + kh - 1, xx = x + kw - 1;
        const bool ok = p < p1 && (unsigned)yy < 128u && (unsigned)xx < 128u;
        const int64_t ps = ok ? p : p0;
        d[u] = *reinterpret_cast<const f32x4*>(a.y2 + ps * 4);
        v[u] = *reinterpret_cast<const f32x4*>(a.r1 + (ok ? p + (kh - 1) * 128 + (kw - 1) : p0) * kFmR1LD + 4 * c4);
        if (!ok) d[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int co = 0; co < 3; ++co) acc[co] += v[u] * d[u][co];
    }
#pragma unroll
    for (int co = 0; co < 3; ++co) *reinterpret_cast<f32x4*>(sh + ((lane * 36 + grp) * 3 + co) * 4) = acc[co];
  }
  __syncthreads();
  // slab [4][9][32] of this block: element (co, tap, ci) = the 7 lanes' sums in lane order; the padding stays zero
  float* slab = a.slabs + (size_t)blockIdx.x * (4 * 9 * 32);
  for (int i = threadIdx.x; i < 4 * 9 * 32; i += kThreads) {
    const int ci = i & 31, r = i >> 5, co = r / 9, tp = r - 9 * co;
    float sum = 0.f;
    if (co < 3 && ci < 16) {
#pragma unroll
      for (int l = 0; l < 7; ++l) sum += sh[((l * 36 + tp * 4 + (ci >> 2)) * 3 + co) * 4 + (ci & 3)];
    }
    slab[i] = sum;
  }
}

// Output of conv_refine_2 y2 [pixel][4] (channels 0..2 = tanh output).  training = 1: MSE against fut - cur
// (train_forward_model.py:106-107): per-block sums of squared differences, and in place of y the gradient with respect to
// the pre-tanh output, 2 (y - t) / (3 P) * (1 - y^2); resid_out (NCHW, optional) = y.  training = 0 (eval mode):
// resid_out = cur + y.  training = 2: resid_out = y, nothing else.  training = 3: `cur` holds d loss / d residual
// (NCHW, any loss the caller differentiated): y := cur * (1 - y^2), the gradient at the pre-tanh output.
struct FmLossArgs {
  float* y2; const void* cur; const void* fut; float* resid_out; float* partial; int64_t npix; int training;
  int u8;                             // cur / fut are byte frames [n][128][128][3] (training 0, 1) instead of float NCHW
};
// partial[block][4] = (sum of squared differences, column sums of the gradient g: the bias gradient of conv_refine_2)
__global__ __launch_bounds__(kThreads) void k_fm_loss(FmLossArgs a) {
  __shared__ float red[4];
  __shared__ float lut[256];
  if (a.u8) {
    u8_norm_table(lut);
    __syncthreads();
  }
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  float sq = 0.f;
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  if (p < a.npix) {
    const int64_t n = p >> 14, r = p & 16383;
    f32x4 y = *reinterpret_cast<const f32x4*>(a.y2 + p * 4);
    const int64_t base = n * 3 * 16384 + r;
    const float* curf = static_cast<const float*>(a.cur);
    const float* futf = static_cast<const float*>(a.fut);
    const unsigned char* cur8 = static_cast<const unsigned char*>(a.cur) + p * 3;
    const unsigned char* fut8 = static_cast<const unsigned char*>(a.fut) + p * 3;
    if (a.training == 3) {
#pragma unroll
      for (int e = 0; e < 3; ++e) g[e] = curf[base + e * 16384] * (1.f - y[e] * y[e]);
      *reinterpret_cast<f32x4*>(a.y2 + p * 4) = g;
    } else if (a.training == 1) {
      const float scale = 2.0f / (3.0f * (float)a.npix);
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const float tgt = a.u8 ? lut[fut8[e]] - lut[cur8[e]] : futf[base + e * 16384] - curf[base + e * 16384];
        const float d = y[e] - tgt;
        sq += d * d;
        g[e] = scale * d * (1.f - y[e] * y[e]);
        if (a.resid_out != nullptr) a.resid_out[base + e * 16384] = y[e];
      }
      *reinterpret_cast<f32x4*>(a.y2 + p * 4) = g;
    } else {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const float c0 = a.training != 0 ? 0.f : (a.u8 ? lut[cur8[e]] : curf[base + e * 16384]);
        a.resid_out[base + e * 16384] = c0 + y[e];
      }
    }
  }
  if (a.training == 1 || a.training == 3) {
    sq = block_sum(sq, red);
    const float g0 = block_sum(g[0], red), g1 = block_sum(g[1], red), g2 = block_sum(g[2], red);
    if (threadIdx.x == 0) *reinterpret_cast<f32x4*>(a.partial + 4 * (size_t)blockIdx.x) = f32x4{sq, g0, g1, g2};
  }
}
// conv_refine_2's forward pass and the MSE step of a training iteration in one launch (ndp_fm_train_grads): the thread that
// finishes a pixel's three outputs goes on to its squared error and its gradient, which is what y2 then holds -- the
// outputs themselves are never written and read back (k_fm_r2_fwd + k_fm_loss with training == 1, same arithmetic).
__global__ __launch_bounds__(kThreads) void k_fm_r2_fwd_loss(FmR2Args a, FmLossArgs l) {
  __shared__ __attribute__((aligned(16))) float Ws[3 * 9 * 16];
  __shared__ float red[4];
  __shared__ float lut[256];
  if (l.u8) u8_norm_table(lut);
  fm_r2_stage_weights(Ws, a.w);                                       // (ends with a barrier: the table is visible too)
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  float sq = 0.f;
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  if (p < a.npix) {
    const int x = (int)(p & 127), y = (int)((p >> 7) & 127);
    float acc[3] = {a.bias[0], a.bias[1], a.bias[2]};
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int yy = y + kh - 1, xx = x + kw - 1;
        if ((unsigned)yy >= 128u || (unsigned)xx >= 128u) continue;
        const float* src = a.r1 + (p + (kh - 1) * 128 + (kw - 1)) * kFmR1LD;
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * c4);
#pragma unroll
          for (int co = 0; co < 3; ++co) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(Ws + (co * 9 + kh * 3 + kw) * 16 + 4 * c4);
            acc[co] = fmaf(v[0], wv[0], acc[co]); acc[co] = fmaf(v[1], wv[1], acc[co]);
            acc[co] = fmaf(v[2], wv[2], acc[co]); acc[co] = fmaf(v[3], wv[3], acc[co]);
          }
        }
      }
    const float yv[3] = {tanhf(acc[0]), tanhf(acc[1]), tanhf(acc[2])};
    const int64_t n = p >> 14, r = p & 16383;
    const int64_t base = n * 3 * 16384 + r;
    const float* curf = static_cast<const float*>(l.cur);
    const float* futf = static_cast<const float*>(l.fut);
    const unsigned char* cur8 = static_cast<const unsigned char*>(l.cur) + p * 3;
    const unsigned char* fut8 = static_cast<const unsigned char*>(l.fut) + p * 3;
    const float scale = 2.0f / (3.0f * (float)l.npix);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float tgt = l.u8 ? lut[fut8[e]] - lut[cur8[e]] : futf[base + e * 16384] - curf[base + e * 16384];
      const float d = yv[e] - tgt;
      sq += d * d;
      g[e] = scale * d * (1.f - yv[e] * yv[e]);
      if (l.resid_out != nullptr) l.resid_out[base + e * 16384] = yv[e];
    }
    *reinterpret_cast<f32x4*>(a.y2 + p * 4) = g;
  }
  sq = block_sum(sq, red);
  const float g0 = block_sum(g[0], red), g1 = block_sum(g[1], red), g2 = block_sum(g[2], red);
  if (threadIdx.x == 0) *reinterpret_cast<f32x4*>(l.partial + 4 * (size_t)blockIdx.x) = f32x4{sq, g0, g1, g2};
}
// loss = scale * sum of the blocks' squared errors (loss == null: a caller-supplied loss gradient, no loss here);
// bias_grad[0..2] = the column sums, [3] = 0 (the padded output channel)
__global__ __launch_bounds__(kThreads) void k_fm_loss_final(const float* partial, int count, double scale, float* loss,
                                                            float* loss_sum, float* bias_grad) {
  __shared__ double red[4][kThreads];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < count; i += kThreads) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(partial + 4 * (size_t)i);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += (double)v[e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[e][threadIdx.x] = s[e];
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0.0;
    for (int i = 0; i < kThreads; ++i) t += red[threadIdx.x][i];
    if (threadIdx.x == 0) {
      if (loss != nullptr) *loss = (float)(t * scale);
      if (loss_sum != nullptr) *loss_sum += (float)(t * scale);
      bias_grad[3] = 0.f;
    } else {
      bias_grad[threadIdx.x - 1] = (float)t;
    }
  }
}

// ------------------------------------------------------------------------------------------ rollout links
// Training on a window of H + 1 frames (DESIGN 5n): pass k runs the network on the state s_k the passes before it
// predicted, s_{k+1} = s_k + r_k is not detached, and the loss is the mean over the H steps of mean((s_{k+1} - x_{k+1})^2).
// Between the passes -- ndp_fm_forward (training) and ndp_fm_backward_inputs, one workspace per pass -- run four small
// elementwise kernels over the n x 3 x 128 x 128 values of a state, float NCHW, 16 bytes per access:
//   begin    s_0 = x_0, gathered from the window (image stride `stride`: floats NCHW, or byte frames HWC normalised as
//            u8_norm_table does -- the floats the loader would have uploaded, bit for bit)
//   advance  s_{k+1} = s_k + r_k;  d = s_{k+1} - x_{k+1};  local_{k+1} = (2 / (H N)) d;  the block's sum of d^2
//   final    loss_k = (sum of the blocks' sums) / N;  L = (k == 0 ? 0 : L) + loss_k / H;  after the last step loss_sum += L
//   chain    G_k = (local_k + G_{k+1}) + dcur_k        -- what pass k - 1 receives as d loss / d residual
// and, over the flat gradient, the sum of the passes' gradients in pass order:  grad = ((g_0 + g_1) + ...) + g_{H-1}.
// Squares are taken and added in fp64 (the product of two floats is exact there: contraction cannot change a bit), a
// thread's twelve in the order channel, pixel; a block's 256 in a fixed tree; the blocks' in a fixed order by one
// workgroup.  No float atomics anywhere: two runs give the same bits.
// A thread owns four neighbouring pixels of one image in all three channels: three 16-byte accesses per float array,
// and the 12 bytes (one load) that hold exactly those pixels of a byte frame.
// The arithmetic and the schedule are in ndp::fm_rollout, __host__ __device__: tests/fm_rollout_host_driver.hip runs
// them on the CPU by the kernels' schedule under the sanitizers.
namespace fm_rollout {
constexpr int kPlane = 128 * 128, kValues = 3 * kPlane;
constexpr int kQuads = kPlane / 4;                                        // pixel quads (threads) per image
constexpr int kBlocksPerImage = kQuads / kThreads;                        // 16
static_assert(kQuads % kThreads == 0, "a block never spans two images");

struct LinkArgs {
  const float* state; const float* resid;                                 // s_k, r_k: contiguous [n][3][128][128]
  const void* target; int target_u8; int64_t stride;                      // x_{k+1} (begin: x_0): image i at target + i * stride elements
  float* state_next; float* local_next;                                   // s_{k+1} (begin: s_0), local_{k+1}
  double* partial; int64_t nquads; float scale;                           // [blocks]; n * kQuads; 2 / (H N) in fp32
};

// u8_norm_table's entry (utils/hdf5_load.py:9-11)
__host__ __device__ inline float norm_u8(int b) { return ((float)b / 255.0f - 0.5f) * 2.0f; }
__host__ __device__ inline int64_t link_blocks(int64_t n) { return n * kBlocksPerImage; }
__host__ __device__ inline float loss_scale(int64_t n, int steps) { return (float)(2.0 / ((double)steps * (double)(n * kValues))); }

// the 12 bytes that hold pixels pix .. pix + 3 of image img of a byte frame, loaded once per thread (4-byte aligned: pix % 4 == 0)
struct QuadBytes { uint32_t w[3]; };
__host__ __device__ inline QuadBytes target_bytes(const LinkArgs& a, int64_t img, int pix) {
  QuadBytes q = {{0u, 0u, 0u}};
  if (a.target_u8) {
    typedef uint32_t word __attribute__((may_alias));
    const word* pw = reinterpret_cast<const word*>(static_cast<const unsigned char*>(a.target) + img * a.stride + (int64_t)pix * 3);
    q.w[0] = pw[0]; q.w[1] = pw[1]; q.w[2] = pw[2];
  }
  return q;
}
// the four target values of channel c at pixels pix .. pix + 3 of image img; lut: the 256 floats of norm_u8
__host__ __device__ inline f32x4 target_quad(const LinkArgs& a, const QuadBytes& q, int64_t img, int pix, int c, const float* lut) {
  if (!a.target_u8)
    return *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.target) + img * a.stride + (int64_t)c * kPlane + pix);
  f32x4 x;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int b = e * 3 + c;                                               // byte of (pixel e, channel c)
    x[e] = lut[(q.w[b >> 2] >> (8 * (b & 3))) & 255u];
  }
  return x;
}
// begin: thread q of the launch
__host__ __device__ inline void begin_thread(const LinkArgs& a, int64_t q, const float* lut) {
  const int64_t img = q / kQuads;
  const int pix = (int)(q % kQuads) * 4;
  const QuadBytes by = target_bytes(a, img, pix);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    *reinterpret_cast<f32x4*>(a.state_next + img * kValues + (int64_t)c * kPlane + pix) = target_quad(a, by, img, pix, c, lut);
}
// advance: thread q of the launch; returns its sum of squared errors
__host__ __device__ inline double advance_thread(const LinkArgs& a, int64_t q, const float* lut) {
  const int64_t img = q / kQuads;
  const int pix = (int)(q % kQuads) * 4;
  const QuadBytes by = target_bytes(a, img, pix);
  double sq = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t at = img * kValues + (int64_t)c * kPlane + pix;
    const f32x4 s = *reinterpret_cast<const f32x4*>(a.state + at);
    const f32x4 r = *reinterpret_cast<const f32x4*>(a.resid + at);
    const f32x4 x = target_quad(a, by, img, pix, c, lut);
    const f32x4 sn = s + r;
    const f32x4 d = sn - x;
    *reinterpret_cast<f32x4*>(a.state_next + at) = sn;
    *reinterpret_cast<f32x4*>(a.local_next + at) = a.scale * d;
#pragma unroll
    for (int e = 0; e < 4; ++e) sq += (double)d[e] * (double)d[e];
  }
  return sq;
}
// the block's tree over its threads' sums in red[kThreads]: step `w` (128, 64 .. 1) for thread t < w
__host__ __device__ inline void tree_step(double* red, int w, int t) { red[t] += red[t + w]; }
// final: thread t's share of the blocks' sums, then thread 0's sum of the shares
__host__ __device__ inline double final_share(const double* partial, int64_t count, int t) {
  double s = 0.0;
  for (int64_t i = t; i < count; i += kThreads) s += partial[i];
  return s;
}
__host__ __device__ inline void final_write(const double* red, int64_t values, int step, int steps, float* step_losses,
                                            float* loss, float* loss_sum) {
  double t = 0.0;
  for (int i = 0; i < kThreads; ++i) t += red[i];
  const double lk = t / (double)values;
  step_losses[step] = (float)lk;
  const float l = (step == 0 ? 0.f : *loss) + (float)(lk / (double)steps);
  *loss = l;
  if (step == steps - 1 && loss_sum != nullptr) *loss_sum += l;
}
// chain: float4 i
__host__ __device__ inline void chain_quad(const float* local, const float* g_next, const float* d_cur, float* g, int64_t i) {
  const f32x4 l = reinterpret_cast<const f32x4*>(local)[i];
  const f32x4 u = reinterpret_cast<const f32x4*>(g_next)[i];
  const f32x4 d = reinterpret_cast<const f32x4*>(d_cur)[i];
  reinterpret_cast<f32x4*>(g)[i] = (l + u) + d;
}
// gradient sum: thread i of the launch -- float4 i of the vector, or (behind the float4s) one of the up to 3 last floats
__host__ __device__ inline int64_t sum_threads(int64_t floats) { return floats / 4 + floats % 4; }
__host__ __device__ inline void sum_thread(const float* grads, int64_t stride, int count, int64_t floats, float* out, int64_t i) {
  const int64_t n4 = floats / 4;
  if (i < n4) {
    f32x4 s = reinterpret_cast<const f32x4*>(grads)[i];
    for (int h = 1; h < count; ++h) s += reinterpret_cast<const f32x4*>(grads + (int64_t)h * stride)[i];
    reinterpret_cast<f32x4*>(out)[i] = s;
  } else {
    const int64_t j = 4 * n4 + (i - n4);
    float s = grads[j];
    for (int h = 1; h < count; ++h) s += grads[(int64_t)h * stride + j];
    out[j] = s;
  }
}
}  // namespace fm_rollout

__global__ __launch_bounds__(kThreads) void k_fm_rollout_begin(fm_rollout::LinkArgs a) {
  __shared__ float lut[256];
  if (a.target_u8) {
    u8_norm_table(lut);
    __syncthreads();
  }
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q < a.nquads) fm_rollout::begin_thread(a, q, lut);
}
__global__ __launch_bounds__(kThreads) void k_fm_rollout_advance(fm_rollout::LinkArgs a) {
  __shared__ float lut[256];
  __shared__ double red[kThreads];
  if (a.target_u8) {
    u8_norm_table(lut);
    __syncthreads();
  }
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  red[threadIdx.x] = q < a.nquads ? fm_rollout::advance_thread(a, q, lut) : 0.0;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) fm_rollout::tree_step(red, w, threadIdx.x);
    __syncthreads();
  }
  if (threadIdx.x == 0) a.partial[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(kThreads) void k_fm_rollout_loss_final(const double* partial, int64_t count, int64_t values, int step,
                                                                    int steps, float* step_losses, float* loss, float* loss_sum) {
  __shared__ double red[kThreads];
  red[threadIdx.x] = fm_rollout::final_share(partial, count, threadIdx.x);
  __syncthreads();
  if (threadIdx.x == 0) fm_rollout::final_write(red, values, step, steps, step_losses, loss, loss_sum);
}
__global__ __launch_bounds__(kThreads) void k_fm_rollout_chain(const float* local, const float* g_next, const float* d_cur, float* g,
                                                               int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n4) fm_rollout::chain_quad(local, g_next, d_cur, g, i);
}
__global__ __launch_bounds__(kThreads) void k_fm_grad_sum(const float* grads, int64_t stride, int count, int64_t floats, float* out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < fm_rollout::sum_threads(floats)) fm_rollout::sum_thread(grads, stride, count, floats, out, i);
}

// ------------------------------------------------------------------------------------------ P1 -> P2
// For one tap, P2 is the transpose of P1's [rows][columns] slice: a workgroup moves one 32 x 32 tile through LDS, 16-byte
// loads along P1's columns, 16-byte stores along P2's.  One launch for all layers: workgroup -> layer by its block range,
// then -> (tap, row tile, column tile).
//   kind 0  stride-2 3x3 convolution  P1 [co][ky*3+kx][ci]  ->  mode-2 classes (py, px), class offset {0,1,3,5} cin cout:
//           [ci][kh'][kw'][co], ky = py ? 2 - 2 kh' : 1
//   kind 2  conv6                     P1 [co][tap][ci]      ->  mode 3 [tap][ci][co]
//   kind 3  stride-2 transposed conv  P1 [ci][ky*4+kx][co]  ->  mode-1 classes [cls][co][kh'][kw'][ci], ky = 3 - 2 kh' - py
//   kind 4  deconv1                   P1 [ci][tap][co]      ->  mode 3 [tap][co][ci]
//   kind 1  stride-1 3x3 convolution (refinement, a few K floats): elementwise, [ci][8 - tap][co padded to 32]
struct FmPackArgs {
  const float* params; float* p2_base;
  int nseg;
  int block_begin[kFmMaxSeg + 1];
  int64_t p1_off[kFmMaxSeg], p2_off[kFmMaxSeg], count[kFmMaxSeg];
  int kind[kFmMaxSeg], cin_[kFmMaxSeg], cout_[kFmMaxSeg], cin_pad_[kFmMaxSeg], cout_pad_[kFmMaxSeg];
};
// the 32 x 32 tile a workgroup of a transposing segment owns: where it starts in P1 and where its transpose goes in P2
struct FmPackTile { int64_t src_off, src_rs, dst_off, dst_rs; };
__device__ __forceinline__ FmPackTile fm_pack_tile(const FmPackArgs& t, int seg, int blk) {
  const int kind = t.kind[seg], cin = t.cin_[seg], cout = t.cout_[seg], cin_pad = t.cin_pad_[seg];
  // rows x columns of P1's per-tap slice, their strides, and where the transposed tile goes
  const bool conv = kind == 0 || kind == 2;
  const int R = conv ? cout : cin_pad, C = conv ? cin : cout;          // (cin == cin_pad, cout == cout_pad but for deconv1's rows)
  const int ntaps = kind == 0 ? 9 : 16;
  const int tiles_c = C / 32, tiles_r = R / 32;
  const int tap = blk / (tiles_r * tiles_c), rem = blk - tap * (tiles_r * tiles_c);
  const int r0 = (rem / tiles_c) * 32, c0 = (rem % tiles_c) * 32;
  FmPackTile o;
  o.src_rs = (int64_t)ntaps * C;                                       // P1 row stride
  o.src_off = (int64_t)tap * C + (int64_t)r0 * o.src_rs + c0;
  int64_t dst_off;                                                     // P2: element (column c, row r) at dst_off + c * dst_rs + r
  if (kind == 0) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    const int py = ky == 1 ? 0 : 1, px = kx == 1 ? 0 : 1;
    const int khp = py ? (2 - ky) / 2 : 0, kwp = px ? (2 - kx) / 2 : 0;
    const int cls = 2 * py + px, nt = (1 + py) * (1 + px), tt = khp * (1 + px) + kwp;
    const int before = cls == 0 ? 0 : (cls == 1 ? 1 : (cls == 2 ? 3 : 5));
    dst_off = (int64_t)before * cin * cout + (int64_t)tt * cout;       // [ci][t][co]: column ci, row co
    o.dst_rs = (int64_t)nt * cout;
  } else if (kind == 2) {
    dst_off = (int64_t)tap * cin * cout;                               // [tap][ci][co]
    o.dst_rs = cout;
  } else if (kind == 3) {
    const int ky = tap >> 2, kx = tap & 3;
    const int py = (ky + 1) & 1, px = (kx + 1) & 1;
    const int khp = (3 - ky - py) >> 1, kwp = (3 - kx - px) >> 1;
    const int cls = 2 * py + px, tt = 2 * khp + kwp;
    dst_off = ((int64_t)cls * cout * 4 + tt) * cin;                    // [cls][co][t][ci]: column co, row ci
    o.dst_rs = (int64_t)4 * cin;
  } else {
    dst_off = (int64_t)tap * cout * cin_pad;                           // [tap][co][ci]
    o.dst_rs = cin_pad;
  }
  o.dst_off = dst_off + (int64_t)c0 * o.dst_rs + r0;
  return o;
}
// transposes the tile whose row `row`, columns 4 q4 .. 4 q4 + 3 this thread holds in v
__device__ __forceinline__ void fm_pack_tile_store(float (*tile)[33], const f32x4& v, float* p2, const FmPackTile& o) {
  const int row = threadIdx.x >> 3, q4 = threadIdx.x & 7;
  tile[row][4 * q4 + 0] = v[0];
  tile[row][4 * q4 + 1] = v[1];
  tile[row][4 * q4 + 2] = v[2];
  tile[row][4 * q4 + 3] = v[3];
  __syncthreads();
  const f32x4 t4 = {tile[4 * q4 + 0][row], tile[4 * q4 + 1][row], tile[4 * q4 + 2][row], tile[4 * q4 + 3][row]};
  *reinterpret_cast<f32x4*>(p2 + o.dst_off + (int64_t)row * o.dst_rs + 4 * q4) = t4;
}

__global__ __launch_bounds__(kThreads) void k_fm_pack(FmPackArgs t) {
  __shared__ float tile[32][33];
  int seg = 0;
  while (seg + 1 < t.nseg && (int)blockIdx.x >= t.block_begin[seg + 1]) ++seg;
  const float* p1 = t.params + t.p1_off[seg];
  float* p2 = t.p2_base + t.p2_off[seg];
  const int blk = (int)blockIdx.x - t.block_begin[seg];
  if (t.kind[seg] == 5) {                                               // conv1: [co][tap][ci 3 of 32] -> [co][tap * 3 + ci, 27 of 32]
    for (int e = 0; e < 4; ++e) {
      const int64_t i = (int64_t)blk * 1024 + e * kThreads + threadIdx.x;
      if (i >= t.count[seg]) return;
      const int k = (int)(i % 32), co = (int)(i / 32);
      p2[i] = k < 27 ? p1[(int64_t)co * 288 + (k / 3) * 32 + k % 3] : 0.f;
    }
    return;
  }
  if (t.kind[seg] == 1) {
    const int cin_pad = t.cin_pad_[seg], cout_pad = t.cout_pad_[seg];
    for (int e = 0; e < 4; ++e) {
      const int64_t i = (int64_t)blk * 1024 + e * kThreads + threadIdx.x;
      if (i >= t.count[seg]) return;
      const int co = (int)(i % 32);
      const int64_t r = i / 32;
      const int tp = (int)(r % 9), ci = (int)(r / 9);
      p2[i] = co < cout_pad ? p1[((int64_t)co * 9 + (8 - tp)) * cin_pad + ci] : 0.f;
    }
    return;
  }
  const FmPackTile o = fm_pack_tile(t, seg, blk);
  const int row = threadIdx.x >> 3, q4 = threadIdx.x & 7;
  const f32x4 v = *reinterpret_cast<const f32x4*>(p1 + o.src_off + (int64_t)row * o.src_rs + 4 * q4);
  fm_pack_tile_store(tile, v, p2, o);
}

// The optimizer step and the repack in one pass (round 2: k_adam over the flat buffer, then k_fm_pack reading the new
// weights again: 133 MB of reads and a launch more).  Workgroups [0, tile_blocks): one 32 x 32 tile of a transposing
// segment each -- Adam on the tile (a float4 of parameter, gradient and both moments per thread), the new values to P1
// and, through LDS, transposed to P2.  The rest: the parameters no tile covers (conv1, the refinement layers, biases,
// BatchNorm), 1,024 per workgroup; an element of a refinement layer's weights also stores its own P2 position (a few K
// floats; P2's zero padding was written by ndp_fm_pack_params and never changes).
struct FmAdamPackArgs {
  FmPackArgs pk;                                                       // the transposing segments (kinds 0, 2, 3, 4)
  float *params, *exp_avg, *exp_avg_sq; const float* grad;
  const int32_t* step; float beta1, beta2, eps;
  int tile_blocks, nplain;
  int plain_begin[kFmMaxSeg + 1];
  int64_t plain_off[kFmMaxSeg], plain_count[kFmMaxSeg];
  int64_t r_off[2], r_count[2], r_p2[2];                               // conv_refine_1 / 2: P1 range of the weights, P2 offset
  int r_cin_pad[2], r_cin[2];
  int64_t c1_count, c1_p2;                                             // conv1 (P1 offset 0): its weights' count, P2 offset
};
__global__ __launch_bounds__(kThreads) void k_fm_adam_pack(FmAdamPackArgs a) {
  __shared__ float tile[32][33];
  const float step_size = reinterpret_cast<const float*>(a.step)[1];
  const float bc2_sqrt = reinterpret_cast<const float*>(a.step)[2];
  if ((int)blockIdx.x < a.tile_blocks) {
    int seg = 0;
    while (seg + 1 < a.pk.nseg && (int)blockIdx.x >= a.pk.block_begin[seg + 1]) ++seg;
    const FmPackTile o = fm_pack_tile(a.pk, seg, (int)blockIdx.x - a.pk.block_begin[seg]);
    const int row = threadIdx.x >> 3, q4 = threadIdx.x & 7;
    const int64_t i = a.pk.p1_off[seg] + o.src_off + (int64_t)row * o.src_rs + 4 * q4;
    f32x4 pv = *reinterpret_cast<const f32x4*>(a.params + i);
    const f32x4 g = *reinterpret_cast<const f32x4*>(a.grad + i);
    f32x4 m = *reinterpret_cast<const f32x4*>(a.exp_avg + i);
    f32x4 v = *reinterpret_cast<const f32x4*>(a.exp_avg_sq + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = pv[e], me = m[e], ve = v[e];
      adam_update(pe, g[e], me, ve, step_size, bc2_sqrt, a.beta1, a.beta2, a.eps);
      pv[e] = pe; m[e] = me; v[e] = ve;
    }
    *reinterpret_cast<f32x4*>(a.params + i) = pv;
    *reinterpret_cast<f32x4*>(a.exp_avg + i) = m;
    *reinterpret_cast<f32x4*>(a.exp_avg_sq + i) = v;
    fm_pack_tile_store(tile, pv, a.pk.p2_base + a.pk.p2_off[seg], o);
    return;
  }
  const int pb = (int)blockIdx.x - a.tile_blocks;
  int seg = 0;
  while (seg + 1 < a.nplain && pb >= a.plain_begin[seg + 1]) ++seg;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t i = (int64_t)(pb - a.plain_begin[seg]) * 1024 + e * kThreads + threadIdx.x;
    if (i >= a.plain_count[seg]) return;
    const int64_t p = a.plain_off[seg] + i;
    float pv = a.params[p], m = a.exp_avg[p], v = a.exp_avg_sq[p];
    adam_update(pv, a.grad[p], m, v, step_size, bc2_sqrt, a.beta1, a.beta2, a.eps);
    a.params[p] = pv;
    a.exp_avg[p] = m;
    a.exp_avg_sq[p] = v;
    if (p < a.c1_count) {                                              // conv1 [co][tap][ci of 32] -> [co][tap * 3 + ci]
      const int ci = (int)(p % 32), tp = (int)((p / 32) % 9), co = (int)(p / 288);
      if (ci < 3) a.pk.p2_base[a.c1_p2 + co * 32 + tp * 3 + ci] = pv;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int64_t j = p - a.r_off[r];
      if (j < 0 || j >= a.r_count[r]) continue;
      const int ci = (int)(j % a.r_cin_pad[r]);                        // P1 [co][tap][ci]
      const int64_t ct = j / a.r_cin_pad[r];
      const int tp = (int)(ct % 9), co = (int)(ct / 9);
      if (ci < a.r_cin[r]) a.pk.p2_base[a.r_p2[r] + ((int64_t)ci * 9 + (8 - tp)) * 32 + co] = pv;   // [ci][8 - tap][co -> 32]
    }
  }
}

// ------------------------------------------------------------------------------------------ conv_refine_1 (32 -> 16, 3x3)
// The layer's forward pass and data gradient as direct convolutions on the matrix pipe, without the GEMM's LDS tiles:
// a wave owns 32 consecutive pixels of an image row (two 16-pixel MFMA tiles), reads every tap's operand straight from
// the map -- the 16 lanes of a tile read 16 neighbouring pixels, 64 contiguous bytes each; the nine taps are L1 hits of
// each other -- and the weights from LDS (18 KB, staged once per workgroup).  As k_fm_gemm<32> tiles the forward pass
// spent half its MFMAs on 16 columns of padding and a barrier per 32 channels of one tap (132 us at 32 images, 0.33 of
// the pipe), the data gradient half its K steps on the 16 padded channels of its source (146 us).
//   forward   raw[p][co]  = bias[co] + sum_tap sum_ci up[p + tap - 1][ci] * W[co][tap][ci]              (P1 [16][9][32])
//   dgrad     dup[p][ci]  = sum_tap sum_co draw[p + tap - 1][co] * W2[ci][tap][co]                      (P2 [32][9][32], taps flipped)
// A workgroup takes `rows_per_block` image rows; its statistics (FmStatEp: forward mode 1 over 16 columns, data gradient
// mode 2 over 32) are summed over the workgroup's pixels in a fixed order and published once.
struct FmR1Args {
  const float* src; const float* w; const float* bias; float* out;    // the 32-channel map [pixel][32], the 16-channel one [pixel][kFmR1LD]
  int64_t nrows; int rows_per_block;                                   // nrows = images * 128
  FmStatEp ep;
};
constexpr int kFmR1FwdLD = 292, kFmR1DgLD = 148;                       // LDS row strides: conflict-free ds_read_b128 of the weights
__device__ __forceinline__ void fm_r1_publish(const FmStatEp& ep, float* red, float* sums, const f32x4* cs1, const f32x4* cs2,
                                              int ntiles, int ncols) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
  for (int jn = 0; jn < ntiles; ++jn)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v1 = cs1[jn][e], v2 = cs2[jn][e];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        v1 += __shfl_xor(v1, off, 64);
        v2 += __shfl_xor(v2, off, 64);
      }
      if (c == 0) {
        red[(wave * 2 + 0) * 32 + jn * 16 + 4 * q + e] = v1;
        red[(wave * 2 + 1) * 32 + jn * 16 + 4 * q + e] = v2;
      }
    }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * ncols; i += kThreads) {
    const int sidx = i / ncols, col = i - sidx * ncols;
    float v = red[(0 * 2 + sidx) * 32 + col];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += red[(w * 2 + sidx) * 32 + col];
    sums[sidx * ncols + col] = v;
  }
  __syncthreads();
  fm_stat_publish(ep, (int)blockIdx.x, 0, ncols, sums);
}
__global__ __launch_bounds__(kThreads) void k_fm_r1_fwd(FmR1Args a) {
  __shared__ __attribute__((aligned(16))) float Ws[16 * kFmR1FwdLD];
  __shared__ float red[kWaves * 2 * 32];
  __shared__ float sums[2 * 32];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, c = lane & 15, q = lane >> 4;
  for (int i = t; i < 16 * 72; i += kThreads) {
    const int co = i / 72, k4 = i - 72 * co;
    *reinterpret_cast<f32x4*>(Ws + co * kFmR1FwdLD + 4 * k4) = *reinterpret_cast<const f32x4*>(a.w + co * 288 + 4 * k4);
  }
  const f32x4 bias4 = *reinterpret_cast<const f32x4*>(a.bias + 4 * q);
  const bool stat = a.ep.mode != 0;
  f32x4 cs1[1] = {f32x4{0.f, 0.f, 0.f, 0.f}}, cs2[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
  __syncthreads();
  const int x0 = wave * 32 + c;
  const float* wl = Ws + c * kFmR1FwdLD + 4 * q;
  for (int r = 0; r < a.rows_per_block; ++r) {
    const int64_t row = (int64_t)blockIdx.x * a.rows_per_block + r;
    if (row >= a.nrows) break;
    const int y = (int)(row & 127);
    const float* img = a.src + (row - y) * 128 * 32 + 4 * q;           // the image's first pixel, this lane's 4 channels
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int yy = y + kh - 1;
      if ((unsigned)yy >= 128u) continue;                              // (uniform: a workgroup's row)
      f32x4 av[3][2][2];
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int xx = x0 + 16 * i + kw - 1;
          const bool ok = (unsigned)xx < 128u;
          const float* px = img + (size_t)(yy * 128 + (ok ? xx : 0)) * 32;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(px + 16 * h);
            av[kw][i][h] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + (kh * 3 + kw) * 32 + 16 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = mfma16(wv[e], av[kw][i][h][e], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x4 v = acc[i] + bias4;
      *reinterpret_cast<f32x4*>(a.out + ((size_t)row * 128 + x0 + 16 * i) * kFmR1LD + 4 * q) = v;
      cs1[0] += v;
      cs2[0] += v * v;
    }
  }
  if (stat) fm_r1_publish(a.ep, red, sums, cs1, cs2, 1, 16);
}
__global__ __launch_bounds__(kThreads) void k_fm_r1_dgrad(FmR1Args a) {
  __shared__ __attribute__((aligned(16))) float Ws[32 * kFmR1DgLD];
  __shared__ float red[kWaves * 2 * 32];
  __shared__ float sums[2 * 32];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, c = lane & 15, q = lane >> 4;
  for (int i = t; i < 32 * 9 * 4; i += kThreads) {                     // P2 [ci][tap][co 16 of 32] -> Ws[ci][tap * 16 + co]
    const int co4 = i & 3, r = i >> 2;                                 // r = ci * 9 + tap
    const int ci = r / 9, tp = r - 9 * ci;
    *reinterpret_cast<f32x4*>(Ws + ci * kFmR1DgLD + tp * 16 + 4 * co4) = *reinterpret_cast<const f32x4*>(a.w + r * 32 + 4 * co4);
  }
  const bool stat = a.ep.mode != 0;
  f32x4 cs1[2], cs2[2], mu4[2], is4[2];
#pragma unroll
  for (int jn = 0; jn < 2; ++jn) {
    cs1[jn] = cs2[jn] = mu4[jn] = is4[jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (stat && a.ep.mode == 2) {
      mu4[jn] = *reinterpret_cast<const f32x4*>(a.ep.mean + 16 * jn + 4 * q);
      is4[jn] = *reinterpret_cast<const f32x4*>(a.ep.invstd + 16 * jn + 4 * q);
    }
  }
  __syncthreads();
  const int x0 = wave * 32 + c;
  for (int r = 0; r < a.rows_per_block; ++r) {
    const int64_t row = (int64_t)blockIdx.x * a.rows_per_block + r;
    if (row >= a.nrows) break;
    const int y = (int)(row & 127);
    const float* img = a.src + (row - y) * 128 * kFmR1LD + 4 * q;      // this lane's 4 of the 16 gradient channels
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jn = 0; jn < 2; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 av[9][2];
#pragma unroll
    for (int tp = 0; tp < 9; ++tp) {
      const int yy = y + tp / 3 - 1;
      const bool yok = (unsigned)yy < 128u;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int xx = x0 + 16 * i + tp % 3 - 1;
        const bool ok = yok && (unsigned)xx < 128u;
        const f32x4 v = *reinterpret_cast<const f32x4*>(img + (size_t)(ok ? yy * 128 + xx : 0) * kFmR1LD);
        av[tp][i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    // the statistics' operands of this row, before its stores (k_fm_gemm's epilogue)
    f32x4 yv[2][2], xv[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jn = 0; jn < 2; ++jn) {
        yv[i][jn] = xv[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
        const size_t pix = (size_t)row * 128 + x0 + 16 * i;
        if (stat && (a.ep.mode == 2 || a.ep.mode == 3)) yv[i][jn] = *reinterpret_cast<const f32x4*>(a.ep.y + pix * a.ep.y_ld + 16 * jn + 4 * q);
        if (stat && a.ep.mode == 2) xv[i][jn] = *reinterpret_cast<const f32x4*>(a.ep.x + pix * a.ep.x_ld + 16 * jn + 4 * q);
      }
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
      for (int jn = 0; jn < 2; ++jn) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(Ws + (16 * jn + c) * kFmR1DgLD + tp * 16 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[i][jn] = mfma16(wv[e], av[tp][i][e], acc[i][jn]);
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jn = 0; jn < 2; ++jn) {
        f32x4 v = acc[i][jn];
        if (stat) fm_stat_terms(a.ep.mode, v, yv[i][jn], xv[i][jn], mu4[jn], is4[jn], cs1[jn], cs2[jn]);
        *reinterpret_cast<f32x4*>(a.out + ((size_t)row * 128 + x0 + 16 * i) * 32 + 16 * jn + 4 * q) = v;
      }
  }
  if (stat) fm_r1_publish(a.ep, red, sums, cs1, cs2, 2, 32);
}

// ------------------------------------------------------------------------------------------ host side
// Workspace (floats): [P2 weights][statistics scratch][per-image maps x n][loss partial sums][level-1 statistics partial
// sums][split-K partial sums][weight-gradient slabs]
// the launch sequences (here and in ndp_autoencoder.inc): a step that fails ends the sequence with its code, in `int rc`
#define FM_TRY(x) do { rc = (x); if (rc) return rc; } while (0)
constexpr int64_t kFmPartCap = (int64_t)12 << 20;      // split-K partial sums (floats)
constexpr int64_t kFmSlabCap = (int64_t)32 << 20;      // row-chunk slabs of the weight gradients (floats)
enum FmTensor {
  FMT_COLS = 0, FMT_CAT6, FMT_CAT5, FMT_CAT4, FMT_CAT3, FMT_CAT2, FMT_Z, FMT_RAW1, FMT_RAW2, FMT_RAW3,
  FMT_RAWU1, FMT_RAWU2, FMT_RAWU3, FMT_RAWU4, FMT_RAWU5, FMT_RAWU6, FMT_UP6, FMT_RAWR1, FMT_R1, FMT_Y2,
  FMT_DCAT6, FMT_DCAT5, FMT_DCAT4, FMT_DCAT3, FMT_DCAT2, FMT_DZ, FMT_DUP6, FMT_DR1, FMT_COUNT
};
static const int64_t kFmTensorFloats[FMT_COUNT] = {          // per image
    4096 * 32, 4096 * 128, 1024 * 256, 256 * 512, 64 * 1024, 16 * 2048, 160, 4096 * 64, 1024 * 128, 256 * 256,
    16 * 1024, 64 * 512, 256 * 256, 1024 * 128, 4096 * 64, 16384 * 32, 16384 * 32, 16384 * 32, 16384 * 32, 16384 * 32,
    4096 * 128, 1024 * 256, 256 * 512, 64 * 1024, 16 * 2048, 160, 16384 * 32, 16384 * 32};
static int64_t fm_round4(int64_t v) { return (v + 3) & ~(int64_t)3; }
// Statistics accumulators (FmStatEp): slot 0..9 = the forward sums of BatchNorm b, 10..19 = its backward sums, 20..22 = the
// bias gradients of conv6, conv5, conv4.  Per slot [replicas][2 sums][cols][2 words] 64-bit integers.
constexpr int kFmStatSlots = 23;
static int fm_stat_cols(int slot) { return slot < 20 ? kFmBnC[slot % 10] : (slot == 20 ? 128 : (slot == 21 ? 1024 : 512)); }
// the maps with few channels are the big ones (a thousand tiles and more): 8 accumulators per channel there
static int fm_stat_replicas(int cols) { return cols <= 128 ? 8 : 1; }
static int64_t fm_stat_words(int slot) { return (int64_t)fm_stat_replicas(fm_stat_cols(slot)) * 2 * fm_stat_cols(slot) * 2; }
static int64_t fm_stat_offset_words(int slot) {
  int64_t o = 0;
  for (int i = 0; i < slot; ++i) o += fm_stat_words(i);
  return o;
}
static int64_t fm_fixed_floats() {
  return fm_p2_offset(kFmNet, kFmLayers)               // P2
         + 3 * kFmBnChannels                           // BatchNorm batch mean / invstd / mean residual
         + 4 * fm_stat_offset_words(kFmStatSlots);     // statistics accumulators (64-bit words) + their per-rank copies
}
static int64_t fm_tensor_offset(int64_t n, int t) {
  int64_t o = fm_fixed_floats();
  for (int i = 0; i < t; ++i) o += fm_round4(n * kFmTensorFloats[i]);
  return o;
}
static int64_t fm_ws_floats(int64_t n) {
  return fm_tensor_offset(n, FMT_COUNT) + fm_round4(n * 256) /* loss partial sums */ + kFmPartCap + kFmSlabCap;
}
struct FmWs {
  float* p2; float* bn_mean; float* bn_invstd; float* bn_meanres; long long* stat_acc; long long* stat_acc_local;
  float* t[FMT_COUNT];
  float* loss_partial; float* part; float* slabs;
};
// the start of every network's workspace: [P2][batch mean][invstd][mean residual][statistics accumulators]
static void fm_ws_head(FmWs& w, float* ws, const FmNet& net) {
  w.p2 = ws;
  w.bn_mean = ws + fm_p2_offset(net, net.layers);
  w.bn_invstd = w.bn_mean + kFmBnChannels;
  w.bn_meanres = w.bn_invstd + kFmBnChannels;
  w.stat_acc = reinterpret_cast<long long*>(w.bn_meanres + kFmBnChannels);   // 16-byte aligned: every size before it is a multiple of 4 floats
}
static FmWs fm_ws(float* ws, int64_t n) {
  FmWs w;
  fm_ws_head(w, ws, kFmNet);
  w.stat_acc_local = w.stat_acc + fm_stat_offset_words(kFmStatSlots);
  for (int i = 0; i < FMT_COUNT; ++i) w.t[i] = ws + fm_tensor_offset(n, i);
  w.loss_partial = ws + fm_tensor_offset(n, FMT_COUNT);
  w.part = w.loss_partial + fm_round4(n * 256);
  w.slabs = w.part + kFmPartCap;
  return w;
}
// zero the accumulators of slots [first, last)
static int fm_stat_clear(hipStream_t st, const FmWs& ws, int first, int last) {
  KTimer kt("memset[statistics]", st);
  if (hipMemsetAsync(ws.stat_acc + fm_stat_offset_words(first), 0,
                     sizeof(long long) * (size_t)(fm_stat_offset_words(last) - fm_stat_offset_words(first)), st) != hipSuccess)
    return fail(NDP_E_LAUNCH, "forward model: hipMemsetAsync failed");
  return NDP_OK;
}

struct FmView { float* p; int ld; };
static std::once_flag g_fm_attr_once[kMaxDevices];
static void fm_attrs() {
  std::call_once(device_once(g_fm_attr_once), [] {
    allow_lds((k_fm_gemm<128, FmF32>), FmF32::lds_bytes(kFmBM + 128));
    allow_lds((k_fm_gemm<32, FmF32>), FmF32::lds_bytes(kFmBM + 32));
    allow_lds((k_fm_gemm<128, FmBf16>), FmBf16::lds_bytes(kFmBM + 128));
    allow_lds((k_fm_gemm<32, FmBf16>), FmBf16::lds_bytes(kFmBM + 32));
    allow_lds((k_fm_deconv32<false, FmF32>), FmF32::lds_bytes(kFmBM + 128));
    allow_lds((k_fm_deconv32<true, FmF32>), FmF32::lds_bytes(kFmBM + 128));      // (the eval-mode decoder of ndp_autoencoder.inc)
    allow_lds((k_fm_deconv32<false, FmBf16>), FmBf16::lds_bytes(kFmBM + 128));
    allow_lds((k_fm_wgrad<64, 64>), (fm_wgrad_lds_floats<64, 64>() * 4));
    allow_lds((k_fm_wgrad<32, 64>), (fm_wgrad_lds_floats<32, 64>() * 4));
    allow_lds((k_fm_wgrad<32, 16>), (fm_wgrad_lds_floats<32, 16>() * 4));
    allow_lds(k_fm_wgrad_taps9, fm_wgrad_taps9_lds_floats() * 4);
  });
}
static int fm_log2(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }

// What a launch is to add up over its output's columns on the way out (FmStatEp): built by the callers below.
struct FmEpReq { int mode, slot; FmView x, y; const float* mean; const float* invstd; };
static FmEpReq fm_ep_none() { FmEpReq r; memset(&r, 0, sizeof(r)); return r; }
static void fm_ep_fill(FmStatEp& ep, const FmEpReq& rq, const FmWs& ws) {
  memset(&ep, 0, sizeof(ep));
  if (rq.mode == 0) return;
  ep.mode = rq.mode; ep.cols = fm_stat_cols(rq.slot); ep.replicas = fm_stat_replicas(ep.cols);
  ep.acc = ws.stat_acc + fm_stat_offset_words(rq.slot);
  ep.x = rq.x.p; ep.x_ld = rq.x.ld; ep.y = rq.y.p; ep.y_ld = rq.y.ld; ep.mean = rq.mean; ep.invstd = rq.invstd;
}
// Cross-rank BatchNorm statistics (ndp_fm_stat_sync_fn): between the launch that fills a BatchNorm's accumulator and the
// launch that consumes it, the caller's function sums the accumulator over the ranks on the launch stream -- 64-bit
// integers, so the sum is exact and the same on every rank in any order: W ranks with B / W images each then normalise
// exactly as one process with B images does (SyncBatchNorm's semantics; the reference trains on one device).  The
// backward sums are copied first: d beta / d gamma are written from this rank's own sums (the gradient all-reduce adds
// the ranks' up), dx is computed with the global ones.
// The descriptor travels with the call (FmBnAt::sync): ndp_fm_train_grads_dp and ndp_ae_train_grads_dp build one on
// their stack from their arguments, every other entry point passes null: this rank's sums only.
struct FmStatSync { ndp_fm_stat_sync_fn fn; void* ctx; int world; };
static bool fm_sync_on(const FmStatSync* s) { return s != nullptr && s->fn != nullptr && s->world > 1; }
static int fm_stat_sync(hipStream_t st, const FmWs& ws, int slot, const FmStatSync* sync) {
  if (!fm_sync_on(sync)) return NDP_OK;
  long long* acc = ws.stat_acc + fm_stat_offset_words(slot);
  const int64_t words = fm_stat_words(slot);
  if (slot >= 10 && hipMemcpyAsync(ws.stat_acc_local + fm_stat_offset_words(slot), acc, sizeof(long long) * (size_t)words,
                                   hipMemcpyDeviceToDevice, st) != hipSuccess)
    return fail(NDP_E_LAUNCH, "forward model: hipMemcpyAsync of the statistics failed");
  sync->fn(acc, words, (void*)st, sync->ctx);
  return NDP_OK;
}
// ... and what the consumer makes of the accumulator of `slot` (FmStatFin); P = this rank's pixels summed over
static FmStatFin fm_fin(int slot, int what, int64_t P, const FmWs& ws, const FmStatSync* sync = nullptr) {
  FmStatFin f;
  memset(&f, 0, sizeof(f));
  f.acc = ws.stat_acc + fm_stat_offset_words(slot); f.replicas = fm_stat_replicas(fm_stat_cols(slot));
  f.what = what; f.P = (int)P; f.eps = kFmBnEps; f.momentum = kFmBnMomentum;
  if (fm_sync_on(sync) && slot < 20) {
    f.P = (int)(P * sync->world);
    if (slot >= 10) f.acc_local = ws.stat_acc_local + fm_stat_offset_words(slot);
  }
  return f;
}

// Workgroups a K-split launch aims for: one per CU (a target of 512 -- two per CU -- measured 2 % slower at batch 8 and
// 32: the partial sums cost more than the second workgroup hides).
constexpr int kFmSplitTarget = 256;

// out = act(bias + gather-GEMM) [+ out]; see k_fm_gemm for the modes.  GH = grid of rows per image (square maps).
// rq: statistics of the finished output, from this launch's epilogue or -- with a K split -- from the split sums'.
// lp: `w` is the address of the layer's bf16 weights and the launch is k_fm_gemm's bf16 instantiation (modes 0 and 1, no
// statistics); otherwise `w` is fp32.
static int fm_gemm(hipStream_t st, const char* label, int mode, FmView src, int SH, int ss, const void* w, const float* bias,
                   FmView out, int OH, int GH, int64_t n, int C, int N, int KH, int pad, int act, int accumulate,
                   const FmWs& ws, const FmEpReq* rq = nullptr, bool lp = false) {
  if (lp && (mode > 1 || (rq != nullptr && rq->mode != 0)))
    return fail(NDP_E_UNSUPPORTED, "forward model: %s has no bf16 launch of this kind", label);
  FmGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src.p; a.w = w; a.bias = bias; a.out = out.p; a.part = ws.part;
  a.src_ld = src.ld; a.SH = a.SW = SH; a.ss = ss;
  a.out_ld = out.ld; a.OH = a.OW = OH;
  a.GH = a.GW = GH; a.M = (int)(n * GH * GH); a.C = C; a.N = N;
  a.mode = mode; a.KH = a.KW = KH; a.pad = pad; a.act = act; a.accumulate = accumulate;
  if (mode == 3 && a.M <= 64 && C <= kFmRowsMaxC && C % 32 == 0 && N % 16 == 0) {
    // a few images: one wave per (class, 16 columns), weights straight into MFMA operands (k_fm_rows_cls)
    const FmEpReq none0 = fm_ep_none();
    fm_ep_fill(a.ep, rq ? *rq : none0, ws);
    a.nsplit = 1;
    const unsigned blocks = (unsigned)((16 * (N / 16) + kWaves - 1) / kWaves);
    KTimer kt(label, st);
    hipLaunchKernelGGL(k_fm_rows_cls, dim3(blocks), dim3(kThreads), 0, st, a);
    return check_launch("k_fm_rows_cls");
  }
  const int ncls = mode == 0 ? 1 : (mode == 3 ? 16 : 4);
  const int maxtaps = mode == 0 ? KH * KH : (mode == 3 ? 1 : 4);
  const int ksteps = maxtaps * C / kFmBK;
  const int bn = N >= 128 ? 128 : 32;
  a.mtiles = (a.M + kFmBM - 1) / kFmBM; a.ntiles = (N + bn - 1) / bn;
  const int64_t gx = a.mtiles >= 8 ? (int64_t)8 * ((a.mtiles + 7) / 8) * a.ntiles : (int64_t)a.mtiles * a.ntiles;
  // K split: the deep layers have few output tiles at small batches (deconv2 at 8 images: 16): one workgroup per CU
  // (kFmSplitTarget), each with at least 8 K steps
  const int64_t tiles = (int64_t)a.mtiles * a.ntiles * ncls;
  int nsplit = 1;
  while (tiles * nsplit < kFmSplitTarget && nsplit * 8 <= ksteps && nsplit < 128 &&
         (int64_t)ncls * nsplit * 2 * a.M * N <= kFmPartCap) nsplit *= 2;
  a.steps_per_split = (ksteps + nsplit - 1) / nsplit;
  a.nsplit = (ksteps + a.steps_per_split - 1) / a.steps_per_split;
  // mode 2 where the K loop is split anyway: nine equal K units per tile instead of four unequal classes (fm_unit_first).
  // (Measured at 32 images: conv4 / conv5 85 -> 80 us each; conv3, unsplit before, 100 -> 70 us + 16 us of reduce launch
  // + 38 MB of partial sums: step unchanged, so a layer that needs no split keeps its one launch.)
  const int tap_steps = C / kFmBK;
  if (mode == 2 && a.nsplit > 1 && tap_steps >= 8 && tiles <= kFmSplitTarget && (int64_t)9 * a.M * N <= kFmPartCap) {
    int s = 1;
    while ((int64_t)a.mtiles * a.ntiles * 9 * s < kFmSplitTarget && tap_steps / (2 * s) >= 8 && tap_steps % (2 * s) == 0 &&
           (int64_t)9 * 2 * s * a.M * N <= kFmPartCap) s *= 2;
    a.cls_units = s;
    a.steps_per_split = tap_steps / s;
    a.nsplit = 9 * s;
  }
  const FmEpReq none = fm_ep_none();
  const FmEpReq& want = rq ? *rq : none;
  const int64_t P = (int64_t)ncls * a.M;                             // pixels of the output map
  int rc;
  fm_ep_fill(a.ep, a.nsplit == 1 ? want : none, ws);
  const dim3 grid((unsigned)gx, (unsigned)a.nsplit, (unsigned)(a.cls_units > 0 ? 1 : ncls));
  {
    KTimer kt(label, st);
    auto launch = [&](auto path) {
      using P = decltype(path);
      if (bn == 128) hipLaunchKernelGGL((k_fm_gemm<128, P>), grid, dim3(kThreads), P::lds_bytes(kFmBM + 128), st, a);
      else hipLaunchKernelGGL((k_fm_gemm<32, P>), grid, dim3(kThreads), P::lds_bytes(kFmBM + 32), st, a);
    };
    if (lp) launch(FmBf16{});
    else launch(FmF32{});
  }
  rc = check_launch("k_fm_gemm");
  if (rc || a.nsplit == 1) return rc;
  // the split sums: 64-column slabs x row chunks, about 512 workgroups, at least 16 rows (one per row lane) per chunk
  const int slabs = (N + kFmRedSlab - 1) / kFmRedSlab;
  int64_t chunks = (512 + slabs - 1) / slabs;
  if (chunks > (P + 15) / 16) chunks = (P + 15) / 16;
  if (chunks < 1) chunks = 1;
  a.rows_per_block = (int)(((P + chunks - 1) / chunks + 15) / 16 * 16);
  const int nchunks = (int)((P + a.rows_per_block - 1) / a.rows_per_block);
  fm_ep_fill(a.ep, want, ws);
  KTimer kt("k_fm_splitk_reduce", st);
  hipLaunchKernelGGL(k_fm_splitk_reduce, dim3((unsigned)slabs, (unsigned)nchunks), dim3(kThreads), 0, st, a, ncls);
  return check_launch("k_fm_splitk_reduce");
}

// grad[J][KH*KH][C] = sum over the n * DH * DH pixels of dense[pixel][j] * gath[pixel * ss - pad + tap][k]
// Layers whose weight gradient is computed in row chunks leave their slabs in the workspace; fm_slab_sums adds them all
// in one launch at the end of the backward pass.
struct FmSlabPlan { FmSlabSumArgs a; int64_t used; int blocks; };
// no segment planned (a new plan; a bucket's slabs summed -- slab memory is not reused: plan.used keeps growing)
static void fm_plan_reset(FmSlabPlan& plan) { plan.a.nseg = 0; plan.a.remap_seg = -1; plan.a.block_begin[0] = 0; plan.blocks = 0; }
static FmSlabPlan fm_plan_new() {
  FmSlabPlan plan;
  memset(&plan, 0, sizeof(plan));
  fm_plan_reset(plan);
  return plan;
}
// the next segment: `nchunks` slabs of chunk_floats floats at ws.slabs + plan.used, their first n4 float4 summed into grad
static float* fm_plan_append(FmSlabPlan& plan, const FmWs& ws, float* grad, int64_t nchunks, int64_t chunk_floats, int64_t n4) {
  FmSlabSumArgs& p = plan.a;
  float* slabs = ws.slabs + plan.used;
  p.slabs[p.nseg] = slabs; p.grad[p.nseg] = grad; p.nchunks[p.nseg] = (int)nchunks; p.n4[p.nseg] = n4;
  p.block_begin[p.nseg] = plan.blocks;
  plan.blocks += (int)((n4 + kThreads - 1) / kThreads);
  p.block_begin[++p.nseg] = plan.blocks;
  plan.used += nchunks * chunk_floats;
  return slabs;
}
static int fm_wgrad(hipStream_t st, const char* label, FmView dense, int DH, int J, FmView gath, int SH, int ss, int KH,
                    int pad, int C, int64_t n, float* grad, const FmWs& ws, FmSlabPlan& plan, bool conv1_columns = false) {
  FmWgradArgs a;
  a.dense = dense.p; a.gath = gath.p;
  a.dense_ld = dense.ld; a.hw_shift = fm_log2(DH * DH); a.dw_shift = fm_log2(DH);
  a.gath_ld = gath.ld; a.SH = a.SW = SH; a.ss = ss; a.KH = a.KW = KH; a.pad = pad;
  a.J = J; a.C = C; a.M = (int)(n * DH * DH);
  const int kt_w = C >= 64 ? 64 : 32;
  const int jt_w = (J <= 16 && kt_w == 32) ? 16 : 64;
  a.jtiles = (J + jt_w - 1) / jt_w; a.ktiles_per_tap = C / kt_w;
  a.slab_floats = (int64_t)J * KH * KH * C;
  // conv_refine_1: all nine taps in one workgroup (k_fm_wgrad_taps9)
  const bool taps9 = jt_w == 16 && kt_w == 32 && KH == 3 && ss == 1 && pad == 1 && C == 32 && J <= 16;
  const int64_t tiles = taps9 ? 1 : (int64_t)a.jtiles * KH * KH * a.ktiles_per_tap;
  int64_t nch = taps9 ? 256 : 1024 / tiles;
  if (conv1_columns && nch > 256) nch = 256;                           // (one tile: a workgroup per CU; the remapping sum walks the chunks)
  if (nch > (a.M + 63) / 64) nch = (a.M + 63) / 64;
  if (nch > (kFmSlabCap - plan.used) / a.slab_floats) nch = (kFmSlabCap - plan.used) / a.slab_floats;
  if (nch < 1 || plan.a.nseg >= kFmMaxSeg) nch = 1;
  a.rows_per_chunk = (int)(((a.M + nch - 1) / nch + 15) / 16 * 16);
  const int nchunks = (a.M + a.rows_per_chunk - 1) / a.rows_per_chunk;
  if (conv1_columns && (plan.a.nseg >= kFmMaxSeg || (int64_t)nchunks * a.slab_floats > kFmSlabCap - plan.used))
    return fail(NDP_E_UNSUPPORTED, "fm_wgrad: no slab space for conv1's column gradient");
  a.slabs = grad;
  if (nchunks > 1 || conv1_columns) {
    if (conv1_columns) plan.a.remap_seg = plan.a.nseg;
    a.slabs = fm_plan_append(plan, ws, grad, nchunks, a.slab_floats, conv1_columns ? 64 * 9 * 8 : a.slab_floats / 4);
  }
  const dim3 grid((unsigned)tiles, (unsigned)nchunks);
  KTimer kt(label, st);
  if (taps9) hipLaunchKernelGGL(k_fm_wgrad_taps9, grid, dim3(kThreads), fm_wgrad_taps9_lds_floats() * 4, st, a);
  else if (kt_w == 64) hipLaunchKernelGGL((k_fm_wgrad<64, 64>), grid, dim3(kThreads), (fm_wgrad_lds_floats<64, 64>() * 4), st, a);
  else if (jt_w == 64) hipLaunchKernelGGL((k_fm_wgrad<32, 64>), grid, dim3(kThreads), (fm_wgrad_lds_floats<32, 64>() * 4), st, a);
  else hipLaunchKernelGGL((k_fm_wgrad<32, 16>), grid, dim3(kThreads), (fm_wgrad_lds_floats<32, 16>() * 4), st, a);
  return check_launch("k_fm_wgrad");
}
static int fm_slab_sums(hipStream_t st, const FmSlabPlan& plan) {
  if (plan.a.nseg == 0) return NDP_OK;
  KTimer kt("k_fm_slab_sum", st);
  hipLaunchKernelGGL(k_fm_slab_sum, dim3((unsigned)plan.blocks), dim3(kThreads), 0, st, plan.a);
  return check_launch("k_fm_slab_sum");
}

// elementwise BatchNorm launches: `iters` batches per thread so that a launch has about 1,024 workgroups at most
static int fm_elt_iters(int64_t P, int C) {
  const int64_t per = (int64_t)kThreads * kFmEltPerThread;
  int64_t it = ((P * (C / 4) + per - 1) / per + 1023) / 1024;
  return (int)(it < 1 ? 1 : (it > 16 ? 16 : it));
}
static dim3 fm_elt_grid(int64_t P, int C) {
  const int64_t per = (int64_t)kThreads * kFmEltPerThread * fm_elt_iters(P, C);
  return dim3((unsigned)((P * (C / 4) + per - 1) / per));
}

// Statistics request for the launch that produces the raw input of BatchNorm b (training-mode forward) ...
static FmEpReq fm_ep_bn_fwd(int b) {
  FmEpReq r = fm_ep_none();
  r.mode = 1; r.slot = b;
  return r;
}
// ... for the launch that produces d loss / d (output of BatchNorm b + ReLU): the sums that are d beta and d gamma ...
static FmEpReq fm_ep_bn_bwd(int b, FmView raw, FmView y, const FmWs& ws) {
  FmEpReq r = fm_ep_none();
  r.mode = 2; r.slot = 10 + b;
  r.x = raw; r.y = y; r.mean = ws.bn_mean + fm_bn_stat_index(b); r.invstd = ws.bn_invstd + fm_bn_stat_index(b);
  return r;
}
// ... and for a layer without BatchNorm: mode 3 = ReLU backward applied to the output (y: the layer's post-ReLU map) +
// bias gradient; mode 4 = bias gradient (column sums) only
static FmEpReq fm_ep_bias(int mode, int slot, FmView y) {
  FmEpReq r = fm_ep_none();
  r.mode = mode; r.slot = slot; r.y = y;
  return r;
}

// Where BatchNorm b's tensors live in a network's flat vectors.  sync: where the statistics are summed over the ranks
// (fm_stat_sync; null: this rank's own) -- the function a *_train_grads_dp call was given.
struct FmBnAt {
  const float* gamma; const float* beta; float* running_mean; float* running_var;
  float* d_gamma; float* d_beta; float* d_conv_bias;     // backward outputs (d_conv_bias: the bias of the layer in front)
  const FmStatSync* sync;
};
static FmBnAt fm_bn_at(const FmNet& net, int b, const float* params, float* running, float* grad, const FmStatSync* sync) {
  FmBnAt at;
  at.gamma = params + fm_bn_offset(net, b, false); at.beta = params + fm_bn_offset(net, b, true);
  at.running_mean = running ? running + fm_stat_offset(b, false) : nullptr;
  at.running_var = running ? running + fm_stat_offset(b, true) : nullptr;
  at.d_gamma = grad ? grad + fm_bn_offset(net, b, false) : nullptr;
  at.d_beta = grad ? grad + fm_bn_offset(net, b, true) : nullptr;
  at.d_conv_bias = grad ? grad + fm_param_offset(net, kFmBnLayer[b], true) : nullptr;
  at.sync = sync;
  return at;
}

// BatchNorm b (+ ReLU) forward: raw [P][C] -> dest.  Training mode: batch statistics from the sums the launch that produced
// `raw` accumulated (mean / invstd / running statistics are written for the backward pass and the caller); eval mode: from
// the running statistics.
static int fm_bn_fwd_at(hipStream_t st, int b, FmView raw, int64_t P, FmView dest, const FmBnAt& at, int training,
                        const FmWs& ws) {
  const int C = kFmBnC[b];
  float* mean = ws.bn_mean + fm_bn_stat_index(b);
  float* invstd = ws.bn_invstd + fm_bn_stat_index(b);
  int rc;
  FmEltArgs e;
  memset(&e, 0, sizeof(e));
  if (training) {
    rc = fm_stat_sync(st, ws, b, at.sync);
    if (rc) return rc;
    e.fin = fm_fin(b, 0, P, ws, at.sync);
    e.fin.out1 = mean; e.fin.out2 = invstd; e.fin.meanres = ws.bn_meanres + fm_bn_stat_index(b);
    e.fin.running_mean = at.running_mean;
    e.fin.running_var = at.running_var;
  } else {
    hipLaunchKernelGGL(k_fm_bn_eval_stats, dim3((unsigned)((C + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       (const float*)at.running_mean, (const float*)at.running_var, C, kFmBnEps, mean, invstd);
    rc = check_launch("k_fm_bn_eval_stats");
    if (rc) return rc;
  }
  e.x = raw.p; e.x_ld = raw.ld; e.out = dest.p; e.out_ld = dest.ld; e.mean = mean; e.invstd = invstd;
  e.gamma = at.gamma; e.beta = at.beta; e.C = C; e.P = (int)P;
  e.zero_to = 0;                                                     // (no padded map is left: conv_refine_1's 16 channels are stored as 16, kFmR1LD)
  e.iters = fm_elt_iters(P, e.zero_to > C ? e.zero_to : C);
  KTimer kt("k_fm_bn_apply", st);
  hipLaunchKernelGGL(k_fm_bn_apply, fm_elt_grid(P, e.zero_to > C ? e.zero_to : C), dim3(kThreads), 0, st, e);
  return check_launch("k_fm_bn_apply");
}
// BatchNorm b + ReLU backward: raw (x) := d loss / d x, from the sums the launch that produced dy accumulated; writes the
// BatchNorm weight / bias gradients and the gradient of the convolution bias in front of it (layer l: the column sum of
// dx -- zero but for rounding, as in the reference)
static int fm_bn_bwd_at(hipStream_t st, int b, FmView raw, FmView y, FmView dy, int64_t P, const FmBnAt& at, const FmWs& ws) {
  const int C = kFmBnC[b];
  FmEltArgs e;
  memset(&e, 0, sizeof(e));
  e.x = raw.p; e.x_ld = raw.ld; e.y = y.p; e.y_ld = y.ld; e.dy = dy.p; e.dy_ld = dy.ld; e.out = raw.p; e.out_ld = raw.ld;
  e.mean = ws.bn_mean + fm_bn_stat_index(b); e.invstd = ws.bn_invstd + fm_bn_stat_index(b);
  e.gamma = at.gamma;
  e.C = C; e.P = (int)P;
  const int rc = fm_stat_sync(st, ws, 10 + b, at.sync);
  if (rc) return rc;
  e.fin = fm_fin(10 + b, 2, P, ws, at.sync);
  e.fin.out1 = at.d_beta; e.fin.out2 = at.d_gamma;
  e.fin.out3 = at.d_conv_bias;
  e.fin.meanres = ws.bn_meanres + fm_bn_stat_index(b); e.fin.gamma = e.gamma; e.fin.invstd = e.invstd;
  e.iters = fm_elt_iters(P, C);
  {
    KTimer kt("k_fm_bn_bwd_apply", st);
    hipLaunchKernelGGL(k_fm_bn_bwd_apply, fm_elt_grid(P, C), dim3(kThreads), 0, st, e);
  }
  return check_launch("k_fm_bn_bwd_apply");
}

// deconv6's forward pass, the four parity classes per workgroup (k_fm_deconv32)
static int fm_deconv32(hipStream_t st, const char* label, FmView src, int SH, const void* w, const float* bias, FmView out,
                       int64_t n, int C, int N, const FmEpReq& rq, const FmWs& ws, bool relu = false, bool lp = false) {
  if (lp && (relu || rq.mode != 0)) return fail(NDP_E_UNSUPPORTED, "forward model: %s has no bf16 launch of this kind", label);
  FmDcArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src.p; a.src_ld = src.ld; a.SH = a.SW = SH; a.w = w; a.bias = bias; a.out = out.p; a.out_ld = out.ld;
  a.M = (int)(n * SH * SH); a.C = C; a.N = N;
  a.mtiles = (a.M + kFmBM - 1) / kFmBM;
  fm_ep_fill(a.ep, rq, ws);
  const unsigned gx = a.mtiles >= 8 ? 8u * (unsigned)((a.mtiles + 7) / 8) : (unsigned)a.mtiles;
  KTimer kt(label, st);
  const dim3 grid(gx, (unsigned)(N / 32));
  if (lp) hipLaunchKernelGGL((k_fm_deconv32<false, FmBf16>), grid, dim3(kThreads), FmBf16::lds_bytes(kFmBM + 128), st, a);
  else if (relu) hipLaunchKernelGGL((k_fm_deconv32<true, FmF32>), grid, dim3(kThreads), FmF32::lds_bytes(kFmBM + 128), st, a);
  else hipLaunchKernelGGL((k_fm_deconv32<false, FmF32>), grid, dim3(kThreads), FmF32::lds_bytes(kFmBM + 128), st, a);
  return check_launch(label);
}

// conv_refine_1 as a direct convolution (k_fm_r1_fwd / k_fm_r1_dgrad): about 512 workgroups of whole image rows
static int fm_r1(hipStream_t st, const char* label, bool dgrad, const float* src, const float* w, const float* bias, float* out,
                 int64_t n, const FmEpReq& rq, const FmWs& ws) {
  FmR1Args a;
  memset(&a, 0, sizeof(a));
  a.src = src; a.w = w; a.bias = bias; a.out = out; a.nrows = n * 128;
  a.rows_per_block = (int)((a.nrows + 511) / 512);                  // (256 / 512 / 1,024 / 2,048 workgroups measured: 512)
  fm_ep_fill(a.ep, rq, ws);
  const unsigned blocks = (unsigned)((a.nrows + a.rows_per_block - 1) / a.rows_per_block);
  KTimer kt(label, st);
  if (dgrad) hipLaunchKernelGGL(k_fm_r1_dgrad, dim3(blocks), dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL(k_fm_r1_fwd, dim3(blocks), dim3(kThreads), 0, st, a);
  return check_launch(label);
}

// ------------------------------------------------------------------------------------------ layer launches
// What a launch of layer l needs beyond its tensors follows from the layer's table row: fm_geom, a pure function (the
// CPU test tests/test_fm_geometry_host.py compares it with the recorded argument lists for every layer of every network).
//   forward          conv1 as a one-tap GEMM over its columns (FM_P2_COLUMNS); a convolution gathers its taps (mode 0, P1);
//                    deconv1 is sixteen one-tap classes (mode 3, P2); a stride-2 transposed convolution four 2x2 classes
//                    (mode 1, P2) or, all four classes per workgroup, k_fm_deconv32 (see fm_geom)
//   data gradient    of a transposed convolution: the convolution of d(raw output) with P1 (mode 0); of conv6: sixteen
//                    one-tap classes (mode 3, P2); of a stride-2 convolution: four parity classes (mode 2, P2)
//   weight gradient  dense = d(raw output) of a convolution / the input of a transposed one (DH x DH pixels, J channels),
//                    gathered = the other one (SH x SH pixels, C channels)
// mode < 0: the layer has no launch of that kind here (the refinement stage and the autoencoder's output layer have their
// own kernels; conv1's data gradient is k_fm_conv1_dgrad).
struct FmGeom {
  int mode, SH, ss, OH, GH, C, N, KH, pad;   // fm_gemm's arguments (weight gradient: SH, ss, C, KH, pad of the gathered map)
  int p2;                                    // the launch reads the second weight order
  int deconv32;                              // forward: k_fm_deconv32 instead of mode 1
  int DH, J, columns;                        // weight gradient: the dense map; conv1's column form
};
static FmGeom fm_geom(const FmNet& net, int l, int dir, int64_t n) {
  const FmLayer& L = net.layer[l];
  const bool conv = L.kind == FM_CONV, columns = L.p2 == FM_P2_COLUMNS;
  FmGeom g;
  memset(&g, 0, sizeof(g));
  g.mode = -1;
  if (L.p2 == FM_P2_NONE || (L.p2 == FM_P2_REFINE && dir != FM_WGRAD) || (columns && dir == FM_DGRAD)) return g;
  g.ss = L.stride; g.KH = L.ksz; g.pad = L.pad;
  if (dir == FM_WGRAD) {
    g.mode = 0;
    g.DH = conv ? L.hout : L.hin; g.J = conv ? L.cout_pad : L.cin_pad;
    g.SH = conv ? L.hin : L.hout; g.C = conv ? L.cin_pad : L.cout_pad;
    g.columns = columns;
  } else if (dir == FM_FWD) {
    g.SH = L.hin; g.OH = L.hout; g.GH = conv ? L.hout : L.hin; g.C = L.cin_pad; g.N = L.cout_pad;
    g.mode = conv ? 0 : (L.p2 == FM_P2_DECONV1 ? 3 : 1);
    g.p2 = !conv || columns;
    // k_fm_deconv32: 32 output channels always; 64 as two halves where those make enough tiles (deconv5: from 16 images)
    g.deconv32 = g.mode == 1 && (L.cout_pad == 32 || (L.cout_pad == 64 && n * L.hin * L.hin / kFmBM * 2 >= 256));
  } else {
    g.SH = L.hout; g.OH = L.hin; g.GH = conv ? L.hout : L.hin; g.C = L.cout_pad; g.N = L.cin_pad;
    g.mode = !conv ? 0 : (L.p2 == FM_P2_CONV6 ? 3 : 2);
    g.p2 = conv;
  }
  if (columns) { g.SH = L.hout; g.ss = 1; g.KH = 1; g.pad = 0; }            // (the taps are in the columns)
  if (g.mode == 1 || g.mode == 2) { g.ss = 1; g.KH = 2; g.pad = 0; }        // (per class; k_fm_gemm's fm_class has the rest)
  if (g.mode == 3) { g.ss = 1; g.KH = 1; g.pad = 0; }
  return g;
}

// Where a network's maps live: for layer l its input map, its raw (pre-BatchNorm) output and the gradient of its input
// map.  in[l + 1] is the activated output of layer l; a layer without BatchNorm writes it directly (fm_maps_close sets
// raw[l] = in[l + 1]), and the gradient of its raw output is din[l + 1]; a BatchNorm's backward pass overwrites raw[l]
// with the gradient of the raw output (fm_draw).
constexpr int kFmMaxLayers = 14;
struct FmMaps { FmView in[kFmMaxLayers + 1], raw[kFmMaxLayers], din[kFmMaxLayers + 1]; };
static void fm_maps_close(FmMaps& m, const FmNet& net) {
  for (int l = 0; l < net.layers; ++l)
    if (fm_bn_of(net, l) < 0) m.raw[l] = m.in[l + 1];
}
static FmView fm_draw(const FmNet& net, const FmMaps& m, int l) { return fm_bn_of(net, l) >= 0 ? m.raw[l] : m.din[l + 1]; }
// the two maps of a launch of layer l: forward in[l] -> raw[l]; data gradient d(raw) -> din[l]; weight gradient the dense
// and the gathered map (fm_geom)
static void fm_layer_views(const FmNet& net, const FmMaps& m, int l, int dir, FmView* a, FmView* b) {
  const bool conv = net.layer[l].kind == FM_CONV;
  if (dir == FM_FWD) { *a = m.in[l]; *b = m.raw[l]; }
  else if (dir == FM_DGRAD) { *a = fm_draw(net, m, l); *b = m.din[l]; }
  else { *a = conv ? fm_draw(net, m, l) : m.in[l]; *b = conv ? m.in[l] : fm_draw(net, m, l); }
}
// The forward model: cat([up, skip]) is one map of twice the channels, the decoder's half in front (`lo`), the encoder's
// behind it (`hi`); the gradient maps DCAT* the same way.  This is the only place that says so.
static FmMaps fm_maps(const FmWs& ws) {
  float* const* t = ws.t;
  auto lo = [&](int tensor, int ld) { return FmView{t[tensor], ld}; };
  auto hi = [&](int tensor, int ld) { return FmView{t[tensor] + ld / 2, ld}; };
  FmMaps m;
  memset(&m, 0, sizeof(m));
  m.in[0] = lo(FMT_COLS, 32);    m.raw[0] = lo(FMT_RAW1, 64);                                          // conv1
  m.in[1] = hi(FMT_CAT6, 128);   m.raw[1] = lo(FMT_RAW2, 128);    m.din[1] = hi(FMT_DCAT6, 128);       // conv2
  m.in[2] = hi(FMT_CAT5, 256);   m.raw[2] = lo(FMT_RAW3, 256);    m.din[2] = hi(FMT_DCAT5, 256);       // conv3
  m.in[3] = hi(FMT_CAT4, 512);                                    m.din[3] = hi(FMT_DCAT4, 512);       // conv4
  m.in[4] = hi(FMT_CAT3, 1024);                                   m.din[4] = hi(FMT_DCAT3, 1024);      // conv5
  m.in[5] = hi(FMT_CAT2, 2048);                                   m.din[5] = hi(FMT_DCAT2, 2048);      // conv6
  m.in[6] = lo(FMT_Z, 160);      m.raw[6] = lo(FMT_RAWU1, 1024);  m.din[6] = lo(FMT_DZ, 160);          // deconv1
  m.in[7] = lo(FMT_CAT2, 2048);  m.raw[7] = lo(FMT_RAWU2, 512);   m.din[7] = lo(FMT_DCAT2, 2048);      // deconv2
  m.in[8] = lo(FMT_CAT3, 1024);  m.raw[8] = lo(FMT_RAWU3, 256);   m.din[8] = lo(FMT_DCAT3, 1024);      // deconv3
  m.in[9] = lo(FMT_CAT4, 512);   m.raw[9] = lo(FMT_RAWU4, 128);   m.din[9] = lo(FMT_DCAT4, 512);       // deconv4
  m.in[10] = lo(FMT_CAT5, 256);  m.raw[10] = lo(FMT_RAWU5, 64);   m.din[10] = lo(FMT_DCAT5, 256);      // deconv5
  m.in[11] = lo(FMT_CAT6, 128);  m.raw[11] = lo(FMT_RAWU6, 32);   m.din[11] = lo(FMT_DCAT6, 128);      // deconv6
  m.in[12] = lo(FMT_UP6, 32);    m.raw[12] = lo(FMT_RAWR1, kFmR1LD); m.din[12] = lo(FMT_DUP6, 32);     // conv_refine_1
  m.in[13] = lo(FMT_R1, kFmR1LD);                                 m.din[13] = lo(FMT_DR1, kFmR1LD);    // conv_refine_2
  m.in[14] = lo(FMT_Y2, 4);                                                                            // (the pre-tanh output, then its gradient)
  fm_maps_close(m, kFmNet);
  return m;
}

// One pass over a network: what every layer launch of it shares.  running / grad / sync as fm_bn_at takes them.
struct FmRun {
  hipStream_t st; const FmNet& net; const FmMaps& m; const FmWs& ws; int64_t n;
  const float* params; float* running; float* grad; const FmStatSync* sync;
  const uint16_t* lp;                        // the bf16 weights (fm_lp_offset), or null: every layer in fp32
};
static const float* fm_w1(const FmRun& r, int l) { return r.params + fm_param_offset(r.net, l, false); }
static const float* fm_w2(const FmRun& r, int l) { return r.ws.p2 + fm_p2_offset(r.net, l); }
static const float* fm_bias(const FmRun& r, int l) { return r.params + fm_param_offset(r.net, l, true); }
static int64_t fm_out_pixels(const FmRun& r, int l) { return r.n * r.net.layer[l].hout * r.net.layer[l].hout; }
static int fm_no_launch(const FmRun& r, int l, int dir) {
  return fail(NDP_E_UNSUPPORTED, "forward model: layer %d has no %s launch", l, r.net.label[l].of[dir]);
}

// forward of layer l: m.raw[l] = act(bias + layer(m.in[l])); act 0 none, 1 ReLU (k_fm_deconv32: those two only)
static int fm_layer_fwd(const FmRun& r, int l, int act, const FmEpReq& rq) {
  const FmGeom g = fm_geom(r.net, l, FM_FWD, r.n);
  if (g.mode < 0) return fm_no_launch(r, l, FM_FWD);
  if (r.lp != nullptr && fm_lp_layer(r.net, l)) {
    // bf16 operands: the same geometry and kernel choice, the bf16 copy of the weight order the launch reads
    FmView lsrc, lout;
    fm_layer_views(r.net, r.m, l, FM_FWD, &lsrc, &lout);
    const uint16_t* lw = r.lp + fm_lp_offset(r.net, l);
    if (g.deconv32 && act == 0)
      return fm_deconv32(r.st, kFmLpLabel[l], lsrc, g.SH, lw, fm_bias(r, l), lout, r.n, g.C, g.N, rq, r.ws, false, true);
    return fm_gemm(r.st, kFmLpLabel[l], g.mode, lsrc, g.SH, g.ss, lw, fm_bias(r, l), lout, g.OH, g.GH, r.n, g.C, g.N, g.KH, g.pad,
                   act, 0, r.ws, &rq, true);
  }
  const float* w = g.p2 ? fm_w2(r, l) : fm_w1(r, l);
  const char* label = r.net.label[l].of[FM_FWD];
  FmView src, out;
  fm_layer_views(r.net, r.m, l, FM_FWD, &src, &out);
  if (g.deconv32 && act <= 1) return fm_deconv32(r.st, label, src, g.SH, w, fm_bias(r, l), out, r.n, g.C, g.N, rq, r.ws, act == 1);
  return fm_gemm(r.st, label, g.mode, src, g.SH, g.ss, w, fm_bias(r, l), out, g.OH, g.GH, r.n, g.C, g.N, g.KH, g.pad, act, 0, r.ws, &rq);
}
// data gradient of layer l: m.din[l] (+)= the gradient of its input from the gradient of its raw output; rq: the sums the
// backward pass of the layer below needs (fm_ep_bn_bwd_of, fm_ep_bias)
static int fm_layer_dgrad(const FmRun& r, int l, int accumulate, const FmEpReq& rq) {
  const FmGeom g = fm_geom(r.net, l, FM_DGRAD, r.n);
  if (g.mode < 0) return fm_no_launch(r, l, FM_DGRAD);
  FmView src, out;
  fm_layer_views(r.net, r.m, l, FM_DGRAD, &src, &out);
  return fm_gemm(r.st, r.net.label[l].of[FM_DGRAD], g.mode, src, g.SH, g.ss, g.p2 ? fm_w2(r, l) : fm_w1(r, l), nullptr, out, g.OH,
                 g.GH, r.n, g.C, g.N, g.KH, g.pad, 0, accumulate, r.ws, &rq);
}
// weight gradient of layer l into r.grad, on stream sw
static int fm_layer_wgrad(const FmRun& r, hipStream_t sw, int l, FmSlabPlan& plan) {
  const FmGeom g = fm_geom(r.net, l, FM_WGRAD, r.n);
  if (g.mode < 0) return fm_no_launch(r, l, FM_WGRAD);
  FmView dense, gath;
  fm_layer_views(r.net, r.m, l, FM_WGRAD, &dense, &gath);
  return fm_wgrad(sw, r.net.label[l].of[FM_WGRAD], dense, g.DH, g.J, gath, g.SH, g.ss, g.KH, g.pad, g.C, r.n,
                  r.grad + fm_param_offset(r.net, l, false), r.ws, plan, g.columns != 0);
}
// the BatchNorm (+ ReLU) behind layer l: m.raw[l] -> m.in[l + 1]; backward: m.raw[l] := d loss / d raw from m.din[l + 1]
static int fm_layer_bn_fwd(const FmRun& r, int l, int training) {
  const int b = fm_bn_of(r.net, l);
  return fm_bn_fwd_at(r.st, b, r.m.raw[l], fm_out_pixels(r, l), r.m.in[l + 1], fm_bn_at(r.net, b, r.params, r.running, nullptr, r.sync),
                      training, r.ws);
}
static int fm_layer_bn_bwd(const FmRun& r, int l) {
  const int b = fm_bn_of(r.net, l);
  return fm_bn_bwd_at(r.st, b, r.m.raw[l], r.m.in[l + 1], r.m.din[l + 1], fm_out_pixels(r, l),
                      fm_bn_at(r.net, b, r.params, nullptr, r.grad, r.sync), r.ws);
}
// the statistics request of the launch that produces m.din[l + 1]: the backward sums of the BatchNorm behind layer l
static FmEpReq fm_ep_bn_bwd_of(const FmRun& r, int l) { return fm_ep_bn_bwd(fm_bn_of(r.net, l), r.m.raw[l], r.m.in[l + 1], r.ws); }

// bias gradient of conv6 / conv5 / conv4 (i = 0, 1, 2; statistics slot 20 + i): column sums from the accumulator its
// producer filled
static int fm_bias_finish(const FmRun& r, hipStream_t st, int i) {
  FmBiasFinishArgs bf;
  memset(&bf, 0, sizeof(bf));
  bf.fin = fm_fin(20 + i, 1, 1, r.ws);
  bf.fin.out1 = r.grad + fm_param_offset(r.net, 5 - i, true);
  bf.cols = fm_stat_cols(20 + i);
  KTimer kt("k_fm_bias_finish", st);
  hipLaunchKernelGGL(k_fm_bias_finish, dim3(1), dim3(kThreads), 0, st, bf);
  return check_launch("k_fm_bias_finish");
}

// layer l of `net` becomes the next segment of a k_fm_pack / k_fm_adam_pack launch: a 32 x 32 tile (or 1,024 elements) per workgroup
static void fm_pack_segment(FmPackArgs& a, const FmNet& net, int l) {
  const FmLayer& L = net.layer[l];
  const int i = a.nseg++;
  a.p1_off[i] = fm_param_offset(net, l, false); a.p2_off[i] = fm_p2_offset(net, l); a.count[i] = fm_p2_floats(net, l);
  a.cin_[i] = L.cin; a.cout_[i] = L.cout; a.cin_pad_[i] = L.cin_pad; a.cout_pad_[i] = L.cout_pad;
  a.kind[i] = L.p2;
  a.block_begin[i + 1] = a.block_begin[i] + (int)((a.count[i] + 1023) / 1024);
}
static bool fm_p2_transposes(int p2) {
  return p2 == FM_P2_CONV_S2 || p2 == FM_P2_CONV6 || p2 == FM_P2_DECONV_S2 || p2 == FM_P2_DECONV1;
}

// P1 -> P2 of every layer that has a P2, one launch (k_fm_pack)
static int fm_pack(hipStream_t st, const FmNet& net, const float* params, const FmWs& ws) {
  FmPackArgs a;
  memset(&a, 0, sizeof(a));
  a.params = params; a.p2_base = ws.p2;
  for (int l = 0; l < net.layers; ++l)
    if (net.layer[l].p2 != FM_P2_NONE) fm_pack_segment(a, net, l);
  KTimer kt("k_fm_pack", st);
  hipLaunchKernelGGL(k_fm_pack, dim3((unsigned)a.block_begin[a.nseg]), dim3(kThreads), 0, st, a);
  return check_launch("k_fm_pack");
}

// the bf16 weights of the fm_lp_layer layers from P1 (params) / P2 (the workspace head, packed before), one launch
static int fm_pack_lp(hipStream_t st, const FmNet& net, const float* params, const FmWs& ws, uint16_t* lp) {
  PackLpArgs a;
  memset(&a, 0, sizeof(a));
  a.dst = lp;
  for (int l = 0; l < net.layers; ++l) {
    if (!fm_lp_layer(net, l)) continue;
    if (a.nseg == kPackLpMaxSegs) return fail(NDP_E_UNSUPPORTED, "forward model: more than %d bf16 layers", kPackLpMaxSegs);
    const int i = a.nseg++;
    a.src[i] = net.layer[l].kind == FM_CONV ? params + fm_param_offset(net, l, false) : ws.p2 + fm_p2_offset(net, l);
    a.dst_off[i] = fm_lp_offset(net, l); a.count[i] = fm_w_floats(net, l);
    a.block_begin[i + 1] = a.block_begin[i] + (int)((a.count[i] + 4095) / 4096);
  }
  KTimer kt("k_fm_pack_lp", st);
  hipLaunchKernelGGL(k_pack_lp, dim3((unsigned)a.block_begin[a.nseg]), dim3(kThreads), 0, st, a);
  return check_launch("k_fm_pack_lp");
}

// Adam over the flat parameter buffer + the P2 rebuild, one launch (k_fm_adam_pack); `step` was advanced by the caller.
// Tiles: the transposing layers.  Plain elements: everything between and after their weights -- among them the refinement
// layers' weights (FM_P2_REFINE: at most the kernel's two) and conv1's (FM_P2_COLUMNS), which store their P2 position too.
static int fm_adam_pack(hipStream_t st, const FmNet& net, float* params, const float* grad, float* exp_avg, float* exp_avg_sq,
                        const int32_t* step, float beta1, float beta2, float eps, const FmWs& ws) {
  FmAdamPackArgs a;
  memset(&a, 0, sizeof(a));
  a.params = params; a.grad = grad; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.step = step;
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  a.pk.params = params; a.pk.p2_base = ws.p2;
  a.r_cin_pad[0] = a.r_cin_pad[1] = 1;                                 // (an unused refinement slot: count 0, divisor 1)
  int64_t covered = 0;                                                 // end of the parameters handled so far
  auto plain = [&](int64_t off, int64_t count) {
    if (count <= 0) return;
    const int i = a.nplain;
    a.plain_off[i] = off; a.plain_count[i] = count;
    a.plain_begin[i + 1] = a.plain_begin[i] + (int)((count + 1023) / 1024);
    ++a.nplain;
  };
  int r = 0;
  for (int l = 0; l < net.layers; ++l) {
    const FmLayer& L = net.layer[l];
    if (fm_p2_transposes(L.p2)) {                                      // (whole tiles: its P2 is its P1 size, a multiple of 1,024)
      fm_pack_segment(a.pk, net, l);
      plain(covered, fm_param_offset(net, l, false) - covered);        // what lies before this layer's weights
      covered = fm_param_offset(net, l, true);
    } else if (L.p2 == FM_P2_REFINE) {
      a.r_off[r] = fm_param_offset(net, l, false); a.r_count[r] = fm_w_floats(net, l); a.r_p2[r] = fm_p2_offset(net, l);
      a.r_cin_pad[r] = L.cin_pad; a.r_cin[r] = L.cin;
      ++r;
    } else if (L.p2 == FM_P2_COLUMNS) {                                // (conv1, layer 0: the kernel takes its P1 offset as 0)
      a.c1_count = fm_w_floats(net, l); a.c1_p2 = fm_p2_offset(net, l);
    }
  }
  plain(covered, fm_param_floats(net) - covered);                      // the last bias, the layers without tiles, BatchNorm
  a.tile_blocks = a.pk.block_begin[a.pk.nseg];
  KTimer kt("k_fm_adam_pack", st);
  hipLaunchKernelGGL(k_fm_adam_pack, dim3((unsigned)(a.tile_blocks + a.plain_begin[a.nplain])), dim3(kThreads), 0, st, a);
  return check_launch("k_fm_adam_pack");
}

// forward pass up to the tanh output y2 (workspace); training: batch statistics (+ running update when running != null)
static int fm_forward(hipStream_t st, const float* params, float* running, const void* cur, bool u8, const float* actions,
                      int64_t n, int training, const FmWs& ws, const FmStatSync* sync, bool clear_backward_too = false,
                      const FmLossArgs* with_loss = nullptr, const uint16_t* lp = nullptr) {
  fm_attrs();
  const FmMaps m = fm_maps(ws);
  const FmRun r = {st, kFmNet, m, ws, n, params, running, nullptr, sync, lp};
  const int64_t npix = n * 16384;
  // (the refinement stage's 16-channel maps are stored unpadded, kFmR1LD, and y2 as 3 + 1 channels written by k_fm_r2_fwd)
  {
    KTimer kt("k_fm_image_cols", st);
    const int64_t opix = n * 4096;
    // (training: the statistics accumulators of this pass -- and of the backward pass when it follows at once -- are zeroed here)
    const int last_slot = clear_backward_too ? kFmStatSlots : 10;
    const int64_t zero_words = training ? fm_stat_offset_words(last_slot) - fm_stat_offset_words(0) : 0;
    const unsigned blocks = (unsigned)((opix + kThreads - 1) / kThreads + (n * 32 + kThreads - 1) / kThreads +
                                       (zero_words / 2 + kThreads - 1) / kThreads);
    if (u8) hipLaunchKernelGGL(k_fm_image_cols<true>, dim3(blocks), dim3(kThreads), 0, st, cur, opix, m.in[0].p, actions, n, m.in[6].p,
                               ws.stat_acc + fm_stat_offset_words(0), zero_words);
    else hipLaunchKernelGGL(k_fm_image_cols<false>, dim3(blocks), dim3(kThreads), 0, st, cur, opix, m.in[0].p, actions, n, m.in[6].p,
                            ws.stat_acc + fm_stat_offset_words(0), zero_words);
  }
  int rc = check_launch("k_fm_image_cols");
  if (rc) return rc;
  // the batch statistics of every BatchNorm come out of the launch that produces its input (training mode)
  const FmEpReq none = fm_ep_none();
  auto EP = [&](int l) { return training ? fm_ep_bn_fwd(fm_bn_of(kFmNet, l)) : none; };
  // ---- encoder (forward_encoder.py:41-57): conv1 (its columns: one tap) .. conv3 + BatchNorm, conv4 / conv5 + ReLU, conv6
  for (int l = 0; l < 3; ++l) {
    FM_TRY(fm_layer_fwd(r, l, 0, EP(l)));
    FM_TRY(fm_layer_bn_fwd(r, l, training));
  }
  FM_TRY(fm_layer_fwd(r, 3, 1, none));
  FM_TRY(fm_layer_fwd(r, 4, 1, none));
  FM_TRY(fm_layer_fwd(r, 5, 0, none));
  // ---- decoder (forward_encoder.py:86-97): deconv1 .. deconv6 + BatchNorm, the refinement stage
  for (int l = 6; l < 12; ++l) {
    FM_TRY(fm_layer_fwd(r, l, 0, EP(l)));
    FM_TRY(fm_layer_bn_fwd(r, l, training));
  }
  FM_TRY(fm_r1(st, kFmLabels[12].of[FM_FWD], false, m.in[12].p, fm_w1(r, 12), fm_bias(r, 12), m.raw[12].p, n, EP(12), ws));
  FM_TRY(fm_layer_bn_fwd(r, 12, training));
  {
    FmR2Args r2;
    memset(&r2, 0, sizeof(r2));
    r2.r1 = m.in[13].p; r2.y2 = m.raw[13].p; r2.w = fm_w1(r, 13); r2.bias = fm_bias(r, 13); r2.npix = npix;
    KTimer kt("k_fm_r2_fwd", st);
    if (with_loss) hipLaunchKernelGGL(k_fm_r2_fwd_loss, dim3((unsigned)((npix + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, r2, *with_loss);
    else hipLaunchKernelGGL(k_fm_r2_fwd, dim3((unsigned)((npix + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, r2);
  }
  return check_launch("k_fm_r2_fwd");
}

// training 1: MSE, its gradient in y2, and (with grad != null) the bias gradient of conv_refine_2; training 3: `cur` is
// d loss / d residual from the caller; 0 / 2: outputs only
static FmLossArgs fm_loss_args(const void* cur, const void* fut, bool u8, int64_t n, int training, float* resid_out, const FmWs& ws) {
  FmLossArgs a;
  a.u8 = u8 ? 1 : 0;
  a.y2 = ws.t[FMT_Y2]; a.cur = cur; a.fut = fut; a.resid_out = resid_out; a.partial = ws.loss_partial;
  a.npix = n * 16384; a.training = training;
  return a;
}
// (already_in_forward: the per-pixel pass ran inside the forward pass' last launch, k_fm_r2_fwd_loss)
static int fm_loss(hipStream_t st, const void* cur, const void* fut, bool u8, int64_t n, int training, float* resid_out,
                   float* loss, float* loss_sum, float* grad, const FmWs& ws, bool already_in_forward = false) {
  const FmLossArgs a = fm_loss_args(cur, fut, u8, n, training, resid_out, ws);
  const int nblocks = (int)(n * 64);
  int rc = NDP_OK;
  if (!already_in_forward) {
    KTimer kt("k_fm_loss", st);
    hipLaunchKernelGGL(k_fm_loss, dim3((unsigned)nblocks), dim3(kThreads), 0, st, a);
    rc = check_launch("k_fm_loss");
  }
  if (rc || (training != 1 && training != 3)) return rc;
  hipLaunchKernelGGL(k_fm_loss_final, dim3(1), dim3(kThreads), 0, st, (const float*)ws.loss_partial, nblocks,
                     1.0 / (3.0 * (double)a.npix), training == 1 ? loss : (float*)nullptr,
                     training == 1 ? loss_sum : (float*)nullptr, grad + fm_param_offset(kFmNet, 13, true));
  return check_launch("k_fm_loss_final");
}

// The weight gradient of a layer and its data gradient both start from d(raw output) and do not depend on each other: the
// weight gradients run on a second stream (one per device, created on first use) beside the chain data gradient ->
// BatchNorm backward -> next layer, whose many short launches they fill in around.  Fork: the side stream waits for an
// event recorded where d(raw) is complete; join: the launch stream waits for the side stream before the slab sums.
// ndp_fm_side_stream(0) keeps everything on the launch stream.
struct FmSide { hipStream_t stream; hipEvent_t fork, join; bool ok; };
static FmSide g_fm_side[kMaxDevices];
static std::once_flag g_fm_side_once[kMaxDevices];
static int g_fm_side_enabled = 1;                                   // ndp_fm_side_stream
static FmSide* fm_side() {
  if (!g_fm_side_enabled) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
  FmSide* sd = &g_fm_side[dev];
  std::call_once(g_fm_side_once[dev], [sd] {
    int lo = 0, hi = 0;                                             // lowest priority: the chain's launches go first
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = 0;
    sd->ok = hipStreamCreateWithPriority(&sd->stream, hipStreamNonBlocking, lo) == hipSuccess &&
             hipEventCreateWithFlags(&sd->fork, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&sd->join, hipEventDisableTiming) == hipSuccess;
  });
  return sd->ok ? sd : nullptr;
}

// Gradient bucket b of a network (the tables: beside its layers) as a range of the flat gradient
static void fm_bucket_range(const FmNet& net, int b, int64_t* offset, int64_t* count) {
  if (net.bucket_first[b] < 0) {
    *offset = fm_bn_offset(net, 0, false);
    *count = fm_param_floats(net) - *offset;
  } else {
    *offset = fm_param_offset(net, net.bucket_first[b], false);
    *count = fm_param_offset(net, net.bucket_end[b], false) - *offset;
  }
}
// One event per bucket, per device and network, created on first use.  `recorded`: set once a pass has recorded all of
// them (fm_bucket_wait refuses before).
constexpr int kFmMaxBuckets = 8;
struct FmBucketEvents { hipEvent_t ev[kFmMaxBuckets]; bool ok; std::atomic<bool> recorded; };
struct FmBucketEventSet { FmBucketEvents dev[kMaxDevices]; std::once_flag once[kMaxDevices]; };
static FmBucketEventSet g_fm_buckets;
static FmBucketEvents* fm_bucket_events(FmBucketEventSet& set, const FmNet& net) {
  static_assert(kFmBuckets <= kFmMaxBuckets, "FmBucketEvents::ev");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
  FmBucketEvents* be = &set.dev[dev];
  const int n = net.buckets;
  std::call_once(set.once[dev], [be, n] {
    be->ok = true;
    for (int i = 0; i < n; ++i) be->ok = be->ok && hipEventCreateWithFlags(&be->ev[i], hipEventDisableTiming) == hipSuccess;
  });
  return be->ok ? be : nullptr;
}
// the body of ndp_fm_bucket_wait / ndp_ae_bucket_wait: `stream` waits for bucket `bucket` of the most recent pass on the
// current device; `who`: the entry point, for its error strings
static int fm_bucket_wait(FmBucketEventSet& set, const FmNet& net, int bucket, void* stream, const char* who) {
  NDP_CHECK_ARG(bucket >= 0 && bucket < net.buckets, "%s: bucket out of range", who);
  int dev = -1;
  NDP_CHECK_ARG(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDevices, "%s: no current device", who);
  FmBucketEvents& be = set.dev[dev];
  NDP_CHECK_ARG(be.recorded.load(), "%s: no pass has recorded the bucket events on this device", who);
  if (hipStreamWaitEvent((hipStream_t)stream, be.ev[bucket], 0) != hipSuccess)
    return fail(NDP_E_LAUNCH, "%s: hipStreamWaitEvent failed", who);
  return NDP_OK;
}

// conv1's data gradient (d_cur) and the action columns of dz (d_actions), either may be null: one launch behind the
// chain's last BatchNorm backward, where m.raw[0] holds d loss / d raw1 and m.din[6] is dz.  ident: the eval-mode output
// is state_cur + residual, so d_out joins d_cur (k_fm_conv1_dgrad<true>); training mode: d_out is not read.
static int fm_conv1_dgrad(const FmRun& r, bool ident, const float* d_out, float* d_cur, float* d_actions) {
  if (d_cur == nullptr && d_actions == nullptr) return NDP_OK;
  FmC1DgArgs c1;
  memset(&c1, 0, sizeof(c1));
  c1.dz = r.m.din[6].p; c1.d_actions = d_actions; c1.nimg = r.n;
  if (d_cur != nullptr) { c1.draw1 = r.m.raw[0].p; c1.w = fm_w1(r, 0); c1.d_out = d_out; c1.d_cur = d_cur; c1.nimg_rows = r.n * 64; }
  const int64_t copy_blocks = d_actions != nullptr ? (r.n * 4 + kThreads - 1) / kThreads : 0;
  const dim3 grid((unsigned)(c1.nimg_rows + copy_blocks));
  KTimer kt("k_fm_conv1_dgrad", r.st);
  if (!ident) hipLaunchKernelGGL(k_fm_conv1_dgrad<false>, grid, dim3(kThreads), 0, r.st, c1);
  else hipLaunchKernelGGL(k_fm_conv1_dgrad<true>, grid, dim3(kThreads), 0, r.st, c1);
  return check_launch("k_fm_conv1_dgrad");
}

// backward pass: from d loss / d (pre-tanh output) in y2 to every gradient in `grad` (flat, the parameters' layout).
// d_cur / d_actions (ndp_fm_backward_inputs, either may be null): the gradient with respect to the image through the
// network alone and to the actions, one more launch on `st` behind the chain's last BatchNorm backward; `grad` and the
// launches that produce it are the same with and without them.
static int fm_backward(hipStream_t st, const float* params, int64_t n, float* grad, const FmWs& ws, const FmStatSync* sync,
                       bool cleared = false, float* d_cur = nullptr, float* d_actions = nullptr) {
  FmSide* side = fm_side();
  hipStream_t sw = side ? side->stream : st;                        // where the weight gradients go
  FmBucketEvents* buckets = fm_bucket_events(g_fm_buckets, kFmNet);
  // everything launched on `st` so far is complete for what the side stream launches after this
  auto fork = [&]() {
    if (side) {
      hipEventRecord(side->fork, st);
      hipStreamWaitEvent(side->stream, side->fork, 0);
    }
  };
  const FmMaps m = fm_maps(ws);
  const FmRun r = {st, kFmNet, m, ws, n, params, nullptr, grad, sync};
  const int64_t npix = n * 16384;
  int rc;
  FmSlabPlan plan = fm_plan_new();
  // bucket b is complete behind everything launched on the weight-gradient stream so far: the row-chunk slabs of its
  // layers are summed now (on that stream), then its event is recorded there
  auto close_bucket = [&](int b) -> int {
    const int rs = fm_slab_sums(sw, plan);
    fm_plan_reset(plan);
    if (rs == NDP_OK && buckets) hipEventRecord(buckets->ev[b], sw);
    return rs;
  };
  if (!cleared) FM_TRY(fm_stat_clear(st, ws, 10, kFmStatSlots));
  // conv_refine_2
  fork();
  {
    // weight gradient: one slab per block of pixels, added by fm_slab_sums with the other layers' (k_fm_r2_wgrad)
    FmR2Args r2;
    memset(&r2, 0, sizeof(r2));
    const int64_t slab = 4 * 9 * 32;
    int64_t nblk = 256;                                               // one block of pixels per CU
    if (nblk > (kFmSlabCap - plan.used) / slab) nblk = (kFmSlabCap - plan.used) / slab;
    r2.rows_per_block = (int)((npix + nblk - 1) / nblk);
    nblk = (npix + r2.rows_per_block - 1) / r2.rows_per_block;
    r2.r1 = m.in[13].p; r2.y2 = m.raw[13].p; r2.npix = npix;
    r2.slabs = fm_plan_append(plan, ws, grad + fm_param_offset(kFmNet, 13, false), nblk, slab, slab / 4);
    KTimer kt("k_fm_r2_wgrad", sw);
    hipLaunchKernelGGL(k_fm_r2_wgrad, dim3((unsigned)nblk), dim3(kThreads), 0, sw, r2);
  }
  FM_TRY(check_launch("k_fm_r2_wgrad"));
  // (the bias gradient of conv_refine_2 came out of the loss kernels)
  {
    // data gradient of conv_refine_2 + the BatchNorm-backward sums of conv_refine_1_bn over it
    FmR2Args r2;
    memset(&r2, 0, sizeof(r2));
    r2.y2 = m.raw[13].p; r2.w = fm_w1(r, 13); r2.dr1 = m.din[13].p; r2.npix = npix;
    const int nblk = (int)((npix + kThreads - 1) / kThreads);
    fm_ep_fill(r2.ep, fm_ep_bn_bwd_of(r, 12), ws);
    KTimer kt("k_fm_r2_dgrad", st);
    hipLaunchKernelGGL(k_fm_r2_dgrad, dim3((unsigned)nblk), dim3(kThreads), 0, st, r2);
  }
  FM_TRY(check_launch("k_fm_r2_dgrad"));
  // Every data gradient below leaves, on its way out, the sums the NEXT BatchNorm / ReLU backward needs (FmEpReq).
  // conv_refine_1
  FM_TRY(fm_layer_bn_bwd(r, 12));
  fork();
  FM_TRY(fm_layer_wgrad(r, sw, 12, plan));
  FM_TRY(fm_r1(st, kFmLabels[12].of[FM_DGRAD], true, m.raw[12].p, fm_w2(r, 12), nullptr, m.din[12].p, n, fm_ep_bn_bwd_of(r, 11), ws));
  // deconv6 .. deconv2: dense = the layer's input map, gathered = d(raw output) at the 4x4 stride-2 taps
  for (int l = 11; l >= 7; --l) {
    FM_TRY(fm_layer_bn_bwd(r, l));
    fork();
    FM_TRY(fm_layer_wgrad(r, sw, l, plan));
    if (l <= 9) FM_TRY(close_bucket(9 - l));                          // bucket 0 ends with deconv4, 1 with deconv3, 2 with deconv2
    FM_TRY(fm_layer_dgrad(r, l, 0, fm_ep_bn_bwd_of(r, l - 1)));
  }
  // deconv1: a 4x4 "image" of d(raw) per row of z
  FM_TRY(fm_layer_bn_bwd(r, 6));
  fork();
  FM_TRY(fm_layer_wgrad(r, sw, 6, plan));
  // conv6: d code = dz[:, 0:128], whose column sums are conv6's bias gradient; its data gradient joins the skip gradient
  // of feat_5 in dcat2
  FM_TRY(fm_layer_dgrad(r, 6, 0, fm_ep_bias(4, 20, {nullptr, 0})));
  fork();
  FM_TRY(fm_bias_finish(r, sw, 0));
  FM_TRY(fm_layer_wgrad(r, sw, 5, plan));
  FM_TRY(close_bucket(3));
  // conv5, conv4 (ReLU, no BatchNorm): the ReLU's backward is applied as the finished gradient is written
  FM_TRY(fm_layer_dgrad(r, 5, 1, fm_ep_bias(3, 21, m.in[5])));
  fork();
  FM_TRY(fm_bias_finish(r, sw, 1));
  FM_TRY(fm_layer_wgrad(r, sw, 4, plan));
  FM_TRY(close_bucket(4));
  FM_TRY(fm_layer_dgrad(r, 4, 1, fm_ep_bias(3, 22, m.in[4])));
  fork();
  FM_TRY(fm_bias_finish(r, sw, 2));
  FM_TRY(fm_layer_wgrad(r, sw, 3, plan));
  FM_TRY(fm_layer_dgrad(r, 3, 1, fm_ep_bn_bwd_of(r, 2)));
  // conv3 .. conv1 (conv1's weight gradient: its columns)
  for (int l = 2; l >= 0; --l) {
    FM_TRY(fm_layer_bn_bwd(r, l));
    fork();
    FM_TRY(fm_layer_wgrad(r, sw, l, plan));
    if (l > 0) FM_TRY(fm_layer_dgrad(r, l, 1, fm_ep_bn_bwd_of(r, l - 1)));
  }
  // m.raw[0] holds d loss / d raw1 since fm_layer_bn_bwd(r, 0): the data gradient of conv1 reads it on `st` while
  // k_fm_wgrad[conv1] reads it on the side stream -- neither writes it; dz is complete since k_fm_dgrad[deconv1]
  FM_TRY(fm_conv1_dgrad(r, false, nullptr, d_cur, d_actions));
  if (side) {
    hipEventRecord(side->join, side->stream);
    hipStreamWaitEvent(st, side->join, 0);
  }
  FM_TRY(fm_slab_sums(st, plan));
  if (buckets) {
    hipEventRecord(buckets->ev[5], st);
    hipEventRecord(buckets->ev[6], st);
    buckets->recorded.store(true);
  }
  return NDP_OK;
}

// the BatchNorm + ReLU behind layer l backward with running statistics (k_fm_bn_eval_bwd_apply): m.raw[l] := d loss / d raw
static int fm_layer_bn_eval_bwd(const FmRun& r, int l) {
  const int b = fm_bn_of(r.net, l), C = kFmBnC[b];
  const int64_t P = fm_out_pixels(r, l);
  FmEltArgs e;
  memset(&e, 0, sizeof(e));
  e.y = r.m.in[l + 1].p; e.y_ld = r.m.in[l + 1].ld; e.dy = r.m.din[l + 1].p; e.dy_ld = r.m.din[l + 1].ld;
  e.out = r.m.raw[l].p; e.out_ld = r.m.raw[l].ld;
  e.invstd = r.ws.bn_invstd + fm_bn_stat_index(b);
  e.gamma = r.params + fm_bn_offset(r.net, b, false);
  e.C = C; e.P = (int)P;
  e.iters = fm_elt_iters(P, C);
  KTimer kt("k_fm_bn_eval_bwd_apply", r.st);
  hipLaunchKernelGGL(k_fm_bn_eval_bwd_apply, fm_elt_grid(P, C), dim3(kThreads), 0, r.st, e);
  return check_launch("k_fm_bn_eval_bwd_apply");
}

// Input gradients of the eval-mode forward pass (ndp_fm_input_grads): fm_backward's data-gradient chain alone, from
// d loss / d (pre-tanh output) in y2 to d_actions (the action columns of dz) and, when d_cur != null, on through the encoder
// to the image.  No weight gradient, no slab, no side stream, no bucket event, no statistics epilogue but the ReLU backward
// of conv4 / conv5 (whose bias sums land in accumulators nobody reads); BatchNorm backward with the running statistics.
static int fm_input_grads(hipStream_t st, const float* params, const float* d_out, int64_t n, float* d_cur, float* d_actions,
                          const FmWs& ws) {
  fm_attrs();
  const FmMaps m = fm_maps(ws);
  const FmRun r = {st, kFmNet, m, ws, n, params, nullptr, nullptr, nullptr};
  const int64_t npix = n * 16384;
  int rc;
  const FmEpReq none = fm_ep_none();
  {
    FmR2Args r2;
    memset(&r2, 0, sizeof(r2));
    r2.y2 = m.raw[13].p; r2.w = fm_w1(r, 13); r2.dr1 = m.din[13].p; r2.npix = npix;
    KTimer kt("k_fm_r2_dgrad", st);
    hipLaunchKernelGGL(k_fm_r2_dgrad, dim3((unsigned)((npix + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, r2);
  }
  FM_TRY(check_launch("k_fm_r2_dgrad"));
  FM_TRY(fm_layer_bn_eval_bwd(r, 12));
  FM_TRY(fm_r1(st, kFmLabels[12].of[FM_DGRAD], true, m.raw[12].p, fm_w2(r, 12), nullptr, m.din[12].p, n, none, ws));
  for (int l = 11; l >= 6; --l) {                                      // deconv6 .. deconv1
    FM_TRY(fm_layer_bn_eval_bwd(r, l));
    FM_TRY(fm_layer_dgrad(r, l, 0, none));
  }
  if (d_cur != nullptr) {
    // the encoder half: conv6, conv5, conv4 (ReLU backward in the epilogue), conv3 .. conv1 (BatchNorm backward between)
    FM_TRY(fm_layer_dgrad(r, 5, 1, fm_ep_bias(3, 21, m.in[5])));
    FM_TRY(fm_layer_dgrad(r, 4, 1, fm_ep_bias(3, 22, m.in[4])));
    FM_TRY(fm_layer_dgrad(r, 3, 1, none));
    for (int l = 2; l >= 1; --l) {
      FM_TRY(fm_layer_bn_eval_bwd(r, l));
      FM_TRY(fm_layer_dgrad(r, l, 1, none));
    }
    FM_TRY(fm_layer_bn_eval_bwd(r, 0));
  }
  return fm_conv1_dgrad(r, true, d_out, d_cur, d_actions);
}

// Which workspaces hold the activations of an eval-mode forward pass that no later call has touched (ndp_fm_input_grads
// consumes them): workspace pointer -> images.  Host-side bookkeeping only; every entry point that writes activations
// drops the workspace's entry first.
static std::mutex g_fm_eval_mutex;
static std::unordered_map<const float*, int64_t> g_fm_eval_fresh;
static void fm_eval_forget(const float* ws) {
  std::lock_guard<std::mutex> lock(g_fm_eval_mutex);
  g_fm_eval_fresh.erase(ws);
}
static void fm_eval_mark(const float* ws, int64_t n) {
  std::lock_guard<std::mutex> lock(g_fm_eval_mutex);
  g_fm_eval_fresh[ws] = n;
}
// takes the entry: the images of the fresh eval-mode forward in ws, or 0
static int64_t fm_eval_take(const float* ws) {
  std::lock_guard<std::mutex> lock(g_fm_eval_mutex);
  auto it = g_fm_eval_fresh.find(ws);
  if (it == g_fm_eval_fresh.end()) return 0;
  const int64_t n = it->second;
  g_fm_eval_fresh.erase(it);
  return n;
}

// the body of ndp_fm_layout / ndp_ae_layout (include/ndp.h); `who`: the entry point, for its error strings
static int fm_layout(const FmNet& net, const char* who, int what, int index, int64_t* offset, int64_t* dims) {
  NDP_CHECK_ARG(offset && dims, "%s: null pointer", who);
  if (what == 0 || what == 1) {
    NDP_CHECK_ARG(index >= 0 && index < net.layers, "%s: layer index out of range", who);
    const FmLayer& L = net.layer[index];
    *offset = fm_param_offset(net, index, what == 1);
    dims[0] = what == 0 ? fm_w_rows(net, index) : L.cout_pad; dims[1] = what == 0 ? L.ksz * L.ksz : 1;
    dims[2] = what == 0 ? fm_w_cols(net, index) : 1; dims[3] = L.kind; dims[4] = L.cin; dims[5] = L.cout;
    return NDP_OK;
  }
  NDP_CHECK_ARG(what >= 2 && what <= 5 && index >= 0 && index < net.bns, "%s: bad BatchNorm query", who);
  *offset = what < 4 ? fm_bn_offset(net, index, what == 3) : fm_stat_offset(index, what == 5);
  dims[0] = kFmBnC[index]; dims[1] = dims[2] = 1; dims[3] = kFmBnLayer[index]; dims[4] = dims[5] = kFmBnC[index];
  return NDP_OK;
}

}  // namespace ndp

extern "C" {

int64_t ndp_fm_param_floats(void) { return ndp::fm_param_floats(ndp::kFmNet); }
int64_t ndp_fm_stat_floats(void) { return ndp::fm_stat_offset(ndp::kFmBns, false); }
int64_t ndp_fm_workspace_floats(int64_t n_images) { return n_images < 1 ? 0 : ndp::fm_ws_floats(n_images); }

int ndp_fm_layout(int what, int index, int64_t* offset, int64_t* dims) {
  return ndp::fm_layout(ndp::kFmNet, "ndp_fm_layout", what, index, offset, dims);
}

int64_t ndp_fm_workspace_offset(int64_t n_images, int tensor) {
  if (n_images < 1 || tensor < 0 || tensor >= ndp::FMT_COUNT) return -1;
  return ndp::fm_tensor_offset(n_images, tensor);
}

int ndp_fm_pack_params(const float* params, float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(params && workspace && aligned16(params) && aligned16(workspace), "ndp_fm_pack_params: bad arguments");
  return fm_pack((hipStream_t)stream, kFmNet, params, fm_ws(workspace, 1));
}

static int fm_forward_any(const float* params, float* running_stats, const void* state_cur, bool u8, const float* actions,
                          int64_t n_images, int training, float* out, float* workspace, void* stream, const char* who,
                          const uint16_t* lp = nullptr) {
  using namespace ndp;
  NDP_CHECK_ARG(params && state_cur && actions && out && workspace && n_images >= 1, "%s: bad arguments", who);
  NDP_CHECK_ARG(training || running_stats, "%s: eval mode needs the running statistics", who);
  NDP_CHECK_ARG(n_images <= 8192, "%s: more than 8192 images per call", who);
  NDP_CHECK_ARG(aligned16(params) && (u8 || aligned16(state_cur)) && aligned16(out) && aligned16(workspace) &&
                (!running_stats || aligned16(running_stats)), "%s: buffers must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  const FmWs ws = fm_ws(workspace, n_images);
  fm_eval_forget(workspace);
  int rc = fm_forward(st, params, running_stats, state_cur, u8, actions, n_images, training, ws, nullptr, false, nullptr, lp);
  if (rc) return rc;
  if (!training) {
    rc = fm_loss(st, state_cur, nullptr, u8, n_images, 0, out, nullptr, nullptr, nullptr, ws);
    if (rc == NDP_OK && lp == nullptr) fm_eval_mark(workspace, n_images);     // ndp_fm_input_grads may follow (fp32 passes only)
    return rc;
  }
  // training mode returns the residual (forward_encoder.py:111-112): y2 -> NCHW
  FmLossArgs a;
  memset(&a, 0, sizeof(a));
  a.y2 = ws.t[FMT_Y2]; a.resid_out = out; a.npix = n_images * 16384;
  a.training = 2;
  hipLaunchKernelGGL(k_fm_loss, dim3((unsigned)(n_images * 64)), dim3(kThreads), 0, st, a);
  return check_launch("k_fm_loss");
}
int ndp_fm_forward(const float* params, float* running_stats, const float* state_cur, const float* actions, int64_t n_images,
                   int training, float* out, float* workspace, void* stream) {
  return fm_forward_any(params, running_stats, state_cur, false, actions, n_images, training, out, workspace, stream, "ndp_fm_forward");
}
int ndp_fm_forward_u8(const float* params, float* running_stats, const uint8_t* frames_cur, const float* actions, int64_t n_images,
                      int training, float* out, float* workspace, void* stream) {
  return fm_forward_any(params, running_stats, frames_cur, true, actions, n_images, training, out, workspace, stream,
                        "ndp_fm_forward_u8");
}

int64_t ndp_fm_lp_weight_bytes(void) { return 2 * ndp::fm_lp_offset(ndp::kFmNet, ndp::kFmNet.layers); }
int ndp_fm_pack_params_lp(const float* params, const float* workspace, void* lp_weights, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(params && workspace && lp_weights && aligned16(params) && aligned16(workspace) && aligned16(lp_weights),
                "ndp_fm_pack_params_lp: bad arguments");
  return fm_pack_lp((hipStream_t)stream, kFmNet, params, fm_ws(const_cast<float*>(workspace), 1), (uint16_t*)lp_weights);
}
int ndp_fm_forward_lp(const float* params, const float* running_stats, const float* state_cur, const uint8_t* frames_u8,
                      const float* actions, int64_t n_images, int precision, const void* lp_weights, float* out, float* workspace,
                      void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(precision == NDP_FM_FP32 || precision == NDP_FM_BF16, "ndp_fm_forward_lp: precision %d is neither NDP_FM_FP32 nor "
                "NDP_FM_BF16", precision);
  NDP_CHECK_ARG((state_cur != nullptr) != (frames_u8 != nullptr), "ndp_fm_forward_lp: exactly one of state_cur and frames_u8");
  NDP_CHECK_ARG(running_stats, "ndp_fm_forward_lp: eval mode needs the running statistics");
  NDP_CHECK_ARG(precision == NDP_FM_FP32 || (lp_weights && aligned16(lp_weights)),
                "ndp_fm_forward_lp: NDP_FM_BF16 needs the 16-byte aligned bf16 weights of ndp_fm_pack_params_lp");
  const bool u8 = frames_u8 != nullptr;
  return fm_forward_any(params, const_cast<float*>(running_stats), u8 ? (const void*)frames_u8 : (const void*)state_cur, u8, actions,
                        n_images, 0, out, workspace, stream, "ndp_fm_forward_lp",
                        precision == NDP_FM_BF16 ? (const uint16_t*)lp_weights : nullptr);
}

static int fm_train_grads_any(const float* params, float* running_stats, const void* state_cur, const void* state_fut, bool u8,
                              const float* actions, int64_t n_images, float* grad, float* loss, float* loss_sum,
                              float* resid_out, float* workspace, void* stream, const ndp::FmStatSync* sync, const char* who) {
  using namespace ndp;
  NDP_CHECK_ARG(params && state_cur && state_fut && actions && grad && loss && workspace && n_images >= 1, "%s: bad arguments", who);
  NDP_CHECK_ARG(n_images <= 8192, "%s: more than 8192 images per call", who);
  NDP_CHECK_ARG(aligned16(params) && (u8 || (aligned16(state_cur) && aligned16(state_fut))) && aligned16(grad) &&
                aligned16(workspace) && (!running_stats || aligned16(running_stats)) && (!resid_out || aligned16(resid_out)),
                "%s: buffers must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  const FmWs ws = fm_ws(workspace, n_images);
  const FmLossArgs la = fm_loss_args(state_cur, state_fut, u8, n_images, 1, resid_out, ws);
  fm_eval_forget(workspace);
  int rc = fm_forward(st, params, running_stats, state_cur, u8, actions, n_images, 1, ws, sync, true, &la);
  if (rc) return rc;
  rc = fm_loss(st, state_cur, state_fut, u8, n_images, 1, resid_out, loss, loss_sum, grad, ws, true);
  if (rc) return rc;
  return fm_backward(st, params, n_images, grad, ws, sync, true);
}
int ndp_fm_train_grads(const float* params, float* running_stats, const float* state_cur, const float* state_fut,
                       const float* actions, int64_t n_images, float* grad, float* loss, float* loss_sum, float* resid_out,
                       float* workspace, void* stream) {
  return fm_train_grads_any(params, running_stats, state_cur, state_fut, false, actions, n_images, grad, loss, loss_sum, resid_out,
                            workspace, stream, nullptr, "ndp_fm_train_grads");
}
int ndp_fm_train_grads_u8(const float* params, float* running_stats, const uint8_t* frames_cur, const uint8_t* frames_fut,
                          const float* actions, int64_t n_images, float* grad, float* loss, float* loss_sum, float* resid_out,
                          float* workspace, void* stream) {
  return fm_train_grads_any(params, running_stats, frames_cur, frames_fut, true, actions, n_images, grad, loss, loss_sum, resid_out,
                            workspace, stream, nullptr, "ndp_fm_train_grads_u8");
}
int ndp_fm_train_grads_dp(const float* params, float* running_stats, const void* frames_cur, const void* frames_fut, int frames_u8,
                          const float* actions, int64_t n_images, float* grad, float* loss, float* loss_sum, float* resid_out,
                          float* workspace, void* stream, ndp_fm_stat_sync_fn stat_sync, void* stat_ctx, int world) {
  NDP_CHECK_ARG(world >= 1 && world <= 4096, "ndp_fm_train_grads_dp: bad world size");
  const ndp::FmStatSync sync = {stat_sync, stat_ctx, world};
  return fm_train_grads_any(params, running_stats, frames_cur, frames_fut, frames_u8 != 0, actions, n_images, grad, loss, loss_sum,
                            resid_out, workspace, stream, ndp::fm_sync_on(&sync) ? &sync : nullptr, "ndp_fm_train_grads_dp");
}

int ndp_fm_grad_buckets(int64_t* offsets, int64_t* counts, int capacity) {
  using namespace ndp;
  NDP_CHECK_ARG(offsets && counts && capacity >= kFmBuckets, "ndp_fm_grad_buckets: need room for 7 buckets");
  for (int b = 0; b < kFmBuckets; ++b) fm_bucket_range(kFmNet, b, offsets + b, counts + b);
  return kFmBuckets;
}

int ndp_fm_bucket_wait(int bucket, void* stream) {
  return ndp::fm_bucket_wait(ndp::g_fm_buckets, ndp::kFmNet, bucket, stream, "ndp_fm_bucket_wait");
}

int ndp_fm_side_stream(int on) {
  const int before = ndp::g_fm_side_enabled;
  ndp::g_fm_side_enabled = on ? 1 : 0;
  return before;
}

int ndp_fm_backward(const float* params, const float* d_resid, int64_t n_images, float* grad, float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(params && d_resid && grad && workspace && n_images >= 1 && n_images <= 8192, "ndp_fm_backward: bad arguments");
  NDP_CHECK_ARG(aligned16(params) && aligned16(d_resid) && aligned16(grad) && aligned16(workspace),
                "ndp_fm_backward: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const FmWs ws = fm_ws(workspace, n_images);
  fm_eval_forget(workspace);
  int rc = fm_loss(st, d_resid, nullptr, false, n_images, 3, nullptr, nullptr, nullptr, grad, ws);
  if (rc) return rc;
  return fm_backward(st, params, n_images, grad, ws, nullptr);
}

int ndp_fm_backward_inputs(const float* params, const float* d_resid, int64_t n_images, float* grad, float* d_state_cur,
                           float* d_actions, float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(params && d_resid && grad && workspace && n_images >= 1 && n_images <= 8192, "ndp_fm_backward_inputs: bad arguments");
  NDP_CHECK_ARG(aligned16(params) && aligned16(d_resid) && aligned16(grad) && aligned16(workspace) &&
                (!d_state_cur || aligned16(d_state_cur)), "ndp_fm_backward_inputs: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const FmWs ws = fm_ws(workspace, n_images);
  fm_eval_forget(workspace);
  int rc = fm_loss(st, d_resid, nullptr, false, n_images, 3, nullptr, nullptr, nullptr, grad, ws);
  if (rc) return rc;
  return fm_backward(st, params, n_images, grad, ws, nullptr, false, d_state_cur, d_actions);
}

static int fm_rollout_link_args(ndp::fm_rollout::LinkArgs& a, const void* target, int target_u8, int64_t stride, int64_t n_images,
                                const char* who) {
  using namespace ndp;
  NDP_CHECK_ARG(target && n_images >= 1 && n_images <= 8192, "%s: bad arguments", who);
  NDP_CHECK_ARG(target_u8 ? (stride >= fm_rollout::kValues && stride % 4 == 0 && ((uintptr_t)target & 3) == 0)
                          : (stride >= fm_rollout::kValues && stride % 4 == 0 && aligned16(target)),
                "%s: frames must be 16-byte (bytes: 4-byte) aligned, their image stride a multiple of 4 and at least one image", who);
  memset(&a, 0, sizeof(a));
  a.target = target; a.target_u8 = target_u8 ? 1 : 0; a.stride = stride; a.nquads = n_images * fm_rollout::kQuads;
  return NDP_OK;
}

int ndp_fm_rollout_begin(const void* frames, int frames_u8, int64_t image_stride, int64_t n_images, float* state, void* stream) {
  using namespace ndp;
  fm_rollout::LinkArgs a;
  int rc = fm_rollout_link_args(a, frames, frames_u8, image_stride, n_images, "ndp_fm_rollout_begin");
  if (rc) return rc;
  NDP_CHECK_ARG(state && aligned16(state), "ndp_fm_rollout_begin: state must be a 16-byte aligned buffer");
  a.state_next = state;
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_fm_rollout_begin", st);
  hipLaunchKernelGGL(k_fm_rollout_begin, dim3((unsigned)fm_rollout::link_blocks(n_images)), dim3(kThreads), 0, st, a);
  return check_launch("k_fm_rollout_begin");
}

int ndp_fm_rollout_advance(const float* state, const float* resid, const void* target, int target_u8, int64_t image_stride,
                           int64_t n_images, int step, int steps, float* state_next, float* local_next, float* step_losses,
                           float* loss, float* loss_sum, float* workspace, void* stream) {
  using namespace ndp;
  fm_rollout::LinkArgs a;
  int rc = fm_rollout_link_args(a, target, target_u8, image_stride, n_images, "ndp_fm_rollout_advance");
  if (rc) return rc;
  NDP_CHECK_ARG(state && resid && state_next && local_next && step_losses && loss && workspace, "ndp_fm_rollout_advance: null pointer");
  NDP_CHECK_ARG(steps >= 1 && step >= 0 && step < steps, "ndp_fm_rollout_advance: step %d of %d", step, steps);
  NDP_CHECK_ARG(aligned16(state) && aligned16(resid) && aligned16(state_next) && aligned16(local_next) && aligned16(workspace),
                "ndp_fm_rollout_advance: buffers must be 16-byte aligned");
  const FmWs ws = fm_ws(workspace, n_images);
  a.state = state; a.resid = resid; a.state_next = state_next; a.local_next = local_next;
  a.partial = reinterpret_cast<double*>(ws.loss_partial);              // n x 256 floats: room for the n x 16 sums
  a.scale = fm_rollout::loss_scale(n_images, steps);
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = fm_rollout::link_blocks(n_images);
  {
    KTimer kt("k_fm_rollout_advance", st);
    hipLaunchKernelGGL(k_fm_rollout_advance, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
  }
  rc = check_launch("k_fm_rollout_advance");
  if (rc) return rc;
  KTimer kt("k_fm_rollout_loss_final", st);
  hipLaunchKernelGGL(k_fm_rollout_loss_final, dim3(1), dim3(kThreads), 0, st, (const double*)a.partial, blocks,
                     n_images * (int64_t)fm_rollout::kValues, step, steps, step_losses, loss, loss_sum);
  return check_launch("k_fm_rollout_loss_final");
}

int ndp_fm_rollout_chain(const float* local, const float* g_next, const float* d_state_cur, int64_t n_images, float* g, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(local && g_next && d_state_cur && g && n_images >= 1 && n_images <= 8192, "ndp_fm_rollout_chain: bad arguments");
  NDP_CHECK_ARG(aligned16(local) && aligned16(g_next) && aligned16(d_state_cur) && aligned16(g),
                "ndp_fm_rollout_chain: buffers must be 16-byte aligned");
  const int64_t n4 = n_images * fm_rollout::kValues / 4;
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_fm_rollout_chain", st);
  hipLaunchKernelGGL(k_fm_rollout_chain, dim3((unsigned)((n4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, local, g_next,
                     d_state_cur, g, n4);
  return check_launch("k_fm_rollout_chain");
}

int ndp_fm_grad_sum(const float* grads, int64_t stride, int count, int64_t floats, float* out, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(grads && out && count >= 1 && count <= 64 && floats >= 1 && floats <= ((int64_t)1 << 36), "ndp_fm_grad_sum: bad arguments");
  NDP_CHECK_ARG(aligned16(grads) && aligned16(out) && stride % 4 == 0 && (count == 1 || stride >= floats),
                "ndp_fm_grad_sum: vectors must be 16-byte aligned, `stride` floats apart (a multiple of 4, no overlap)");
  const int64_t threads = fm_rollout::sum_threads(floats);
  hipStream_t st = (hipStream_t)stream;
  KTimer kt("k_fm_grad_sum", st);
  hipLaunchKernelGGL(k_fm_grad_sum, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, grads, stride, count,
                     floats, out);
  return check_launch("k_fm_grad_sum");
}

int ndp_fm_input_grads(const float* params, const float* d_out, int64_t n_images, float* d_state_cur, float* d_actions,
                       float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(params && d_out && workspace && n_images >= 1 && n_images <= 8192, "ndp_fm_input_grads: bad arguments");
  NDP_CHECK_ARG(d_state_cur || d_actions, "ndp_fm_input_grads: neither d_state_cur nor d_actions is asked for");
  NDP_CHECK_ARG(aligned16(params) && aligned16(d_out) && aligned16(workspace), "ndp_fm_input_grads: buffers must be 16-byte aligned");
  const int64_t fresh = fm_eval_take(workspace);
  if (fresh != n_images)
    return fail(NDP_E_UNSUPPORTED, "ndp_fm_input_grads: the workspace does not hold the activations of an eval-mode ndp_fm_forward "
                "on %lld images (another call ran in between, or they were consumed already)", (long long)n_images);
  hipStream_t st = (hipStream_t)stream;
  const FmWs ws = fm_ws(workspace, n_images);
  // d out / d residual = 1 (out = state_cur + residual): y2 := d_out * (1 - y2^2), the gradient at the pre-tanh output
  FmLossArgs a;
  memset(&a, 0, sizeof(a));
  a.y2 = ws.t[FMT_Y2]; a.cur = d_out; a.partial = ws.loss_partial; a.npix = n_images * 16384; a.training = 3;
  {
    KTimer kt("k_fm_loss", st);
    hipLaunchKernelGGL(k_fm_loss, dim3((unsigned)(n_images * 64)), dim3(kThreads), 0, st, a);
  }
  int rc = check_launch("k_fm_loss");
  if (rc) return rc;
  return fm_input_grads(st, params, d_out, n_images, d_state_cur, d_actions, ws);
}

int ndp_fm_apply_adam(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int32_t* step_count, float lr,
                      float beta1, float beta2, float eps, float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(params && grad && exp_avg && exp_avg_sq && step_count && workspace, "ndp_fm_apply_adam: null pointer");
  NDP_CHECK_ARG(aligned16(params) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq),
                "ndp_fm_apply_adam: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(1), 0, st, step_count, lr, beta1, beta2);
  return fm_adam_pack(st, kFmNet, params, grad, exp_avg, exp_avg_sq, step_count, beta1, beta2, eps, fm_ws(workspace, 1));
}

}  // extern "C"
