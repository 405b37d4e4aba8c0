// ndp_autoencoder.inc -- one training iteration of the reference's image autoencoder (train_autoencoder.py:79-94):
//   models/image_autoencoder.py:14-49   Encoder: conv1..5 (3x3 s2 p1, 3 -> 64 -> 128 -> 256 -> 512 -> 1024), BatchNorm after
//                                       conv1..3 only (conv4_bn / conv5_bn are constructed and never applied), ReLU; conv6
//                                       (4x4 on the 4x4 map) -> 128-d code
//   :53-87    Decoder: deconv1 (128 -> 1024, 4x4 on the 1x1 code), deconv2..5 (ConvTranspose2d(c, c/2, 4, 2, 1)), each +
//             BatchNorm + ReLU; deconv6 (64 -> 3, 4x4 s2 p1) + tanh
//   train_autoencoder.py:84-90          loss = mse(decoder(encoder(x)), x); zero_grad; backward; Adam step
// Included at the end of ndp_kernels.hip, after ndp_forward_model.inc.
//
// The network is the forward model without its skip connections and refinement head, so every layer but the output
// layer runs on the forward model's kernels and host helpers (k_fm_gemm, k_fm_deconv32, k_fm_rows_cls, k_fm_wgrad,
// k_fm_splitk_reduce, k_fm_slab_sum, the epilogue statistics, k_fm_bn_apply / k_fm_bn_bwd_apply, k_fm_pack /
// k_fm_adam_pack).  Its maps are NHWC with the channel count as the pixel stride (nothing is concatenated).  Its eight
// BatchNorms have the channel counts of the forward model's first eight (conv1..3_bn, deconv1..5_bn), so they use those
// BatchNorm indices, statistics slots and scratch; where their tensors live comes from FmBnAt.  What this file says about
// the network is its table (kAeNet: layers, launch labels, BatchNorm count, gradient buckets), its workspace tensors and
// where the maps live in them (ae_maps), the output layer's kernels and the two launch sequences, which name layers and
// no sizes; every size, offset, pack and optimizer segment and the geometry of every layer launch comes from the table
// through the helpers of ndp_forward_model.inc (fm_geom, fm_layer_fwd / _dgrad / _wgrad), which is also how a further
// network of the family would be added -- as the folded decoder below (kAeDecNet, ae_dec_maps) is.
//
// New here: deconv6, 64 -> 3 channels at 128 x 128.  As a GEMM its three output channels would be padded to 32 (ten
// times the MACs, a 32-wide output map); instead three small VALU kernels sized to what they move, as k_fm_r2_*:
//   k_ae_out_fwd_loss  y = tanh(b + deconv6(up5)), the squared error against the image, g = d loss / d (pre-tanh) into
//                      g6 [pixel][4], the per-block sums of the squared error and of g (the bias gradient)
//   k_ae_out_dgrad     d up5 [pixel][64] from g6, and in its epilogue deconv5_bn's backward sums (epilogue mode 2)
//   k_ae_out_wgrad     d W6 [64][16][4] per block of input pixels into slabs, summed in block order by k_fm_slab_sum
//
// Limits: the forward model's argument structs carry pixel counts as int (FmGemmArgs::M, FmEltArgs::P, FmStatFin::P; the
// largest map is n x 4,096 pixels: conv1's output and up5); the new kernels index in 64 bits.  ndp_ae_* accept
// 1 <= n <= kAeMaxImages = 8192 (n x 4,096 < 2^31 with a wide margin; the fixed-point statistics of the largest map stay
// far inside their 2^50 range), as the ndp_fm_* calls do.
//
// Data parallel (ndp_ae_train_grads_dp): the same pass, with the BatchNorm statistics summed over the ranks through the
// caller's per-call function (fm_stat_sync; 8 forward + 8 backward calls) and one event per gradient bucket, recorded
// where the backward pass has written the bucket's last byte (ae_backward's close_bucket; ndp_ae_bucket_wait).

namespace ndp {

constexpr int kAeLayers = 12;
static const FmLayer kAe[kAeLayers] = {
    {FM_CONV, 3, 64, 128, 64, 3, 2, 1, 32, 64, FM_P2_COLUMNS},          // 0  encoder.conv1
    {FM_CONV, 64, 128, 64, 32, 3, 2, 1, 64, 128, FM_P2_CONV_S2},        // 1  encoder.conv2
    {FM_CONV, 128, 256, 32, 16, 3, 2, 1, 128, 256, FM_P2_CONV_S2},      // 2  encoder.conv3
    {FM_CONV, 256, 512, 16, 8, 3, 2, 1, 256, 512, FM_P2_CONV_S2},       // 3  encoder.conv4
    {FM_CONV, 512, 1024, 8, 4, 3, 2, 1, 512, 1024, FM_P2_CONV_S2},      // 4  encoder.conv5
    {FM_CONV, 1024, 128, 4, 1, 4, 1, 0, 1024, 128, FM_P2_CONV6},        // 5  encoder.conv6
    {FM_DECONV, 128, 1024, 1, 4, 4, 1, 0, 128, 1024, FM_P2_DECONV1},    // 6  decoder.deconv1
    {FM_DECONV, 1024, 512, 4, 8, 4, 2, 1, 1024, 512, FM_P2_DECONV_S2},  // 7  decoder.deconv2
    {FM_DECONV, 512, 256, 8, 16, 4, 2, 1, 512, 256, FM_P2_DECONV_S2},   // 8  decoder.deconv3
    {FM_DECONV, 256, 128, 16, 32, 4, 2, 1, 256, 128, FM_P2_DECONV_S2},  // 9  decoder.deconv4
    {FM_DECONV, 128, 64, 32, 64, 4, 2, 1, 128, 64, FM_P2_DECONV_S2},    // 10 decoder.deconv5
    {FM_DECONV, 64, 3, 64, 128, 4, 2, 1, 64, 4, FM_P2_NONE},            // 11 decoder.deconv6
};
// BatchNorms in use: conv1..3_bn, deconv1..5_bn = the forward model's BatchNorms 0..7 (kFmBnC, kFmBnLayer: same channels,
// same layer indices)
constexpr int kAeBns = 8;
constexpr int64_t kAeMaxImages = 8192;
// Gradient buckets of ndp_ae_train_grads_dp: ranges of the flat gradient in the order ae_backward completes them (weight
// gradients last layer first; a layer's bias gradient is final before its weight gradient starts).  Each is closed as
// fm_backward closes its buckets: the row-chunk slabs of its layers are summed, then its event is recorded.
//   bucket 0  layers 8..11 (deconv3..6)        3  layer 4 (conv5)
//          1  layer 7 (deconv2: 8.4 M floats)  4  layers 0..3 (conv1..4)
//          2  layers 5, 6 (conv6, deconv1)     5  the BatchNorm weights and biases (final after conv1_bn's backward)
constexpr int kAeBuckets = 6;
static const int kAeBucketFirst[kAeBuckets] = {8, 7, 5, 4, 0, -1};
static const int kAeBucketEnd[kAeBuckets] = {12, 8, 7, 5, 4, -1};
static const FmLabels kAeLabels[kAeLayers] = {
    FM_LABELS("ae.conv1"), FM_LABELS("ae.conv2"), FM_LABELS("ae.conv3"), FM_LABELS("ae.conv4"), FM_LABELS("ae.conv5"),
    FM_LABELS("ae.conv6"), FM_LABELS("ae.deconv1"), FM_LABELS("ae.deconv2"), FM_LABELS("ae.deconv3"), FM_LABELS("ae.deconv4"),
    FM_LABELS("ae.deconv5"), FM_LABELS("ae.deconv6")};
// the table every host helper of ndp_forward_model.inc reads (sizes, offsets, fm_pack, fm_adam_pack, fm_layout, buckets,
// the layer launches); deconv6 has no second weight order (FM_P2_NONE): the kernels below read P1
static const FmNet kAeNet = {kAe, kAeLayers, kAeBns, kAeBucketFirst, kAeBucketEnd, kAeBuckets, kAeLabels};
static_assert(kAeBuckets <= kFmMaxBuckets, "FmBucketEvents::ev");
static FmBucketEventSet g_ae_buckets;

// ------------------------------------------------------------------------------------------ deconv6 (64 -> 3, 4x4 s2 p1)
// Output pixel (oy, ox) of image i takes the taps ky = ((oy + 1) & 1) + 2 a (a = 0, 1) at source row iy = (oy + 1 - ky) / 2,
// the same in x: four taps per pixel, 4 x 64 x 3 MACs.  W: P1 [ci 64][ky * 4 + kx][co 4] (co = 3 is zero padding),
// staged in LDS (16 KB).  up5 [pixel][64] (n x 64 x 64), g6 [pixel][4] (n x 128 x 128).
constexpr int kAeOutW = 64 * 16 * 4;
struct AeOutArgs {
  const float* up5; const float* w; const float* bias; const float* img;   // img: [n][3][128][128]
  float* g6; float* recon; float* partial;                                 // recon: NCHW output (nullable); partial [block][4]
  float* du5; float* slabs;
  int64_t npix;                     // k_ae_out_fwd_loss: output pixels n x 16,384; dgrad / wgrad: input pixels n x 4,096
  int64_t rows_per_block;           // dgrad / wgrad: input pixels per workgroup
  FmStatEp ep;                      // dgrad: deconv5_bn's backward sums (mode 2; x = raw deconv5 output, y = up5)
};
__device__ __forceinline__ void ae_out_stage_weights(float* Ws, const float* __restrict__ w) {
  for (int i = threadIdx.x; i < kAeOutW / 4; i += kThreads)
    reinterpret_cast<f32x4*>(Ws)[i] = reinterpret_cast<const f32x4*>(w)[i];
  __syncthreads();
}

// acc = bias + the (at most) four taps' 64-channel sums of output pixel (oy, ox) of image img: the arithmetic of deconv6,
// shared by the training kernel (k_ae_out_fwd_loss) and the eval-mode one (k_ae_out_fwd) -- one order of fmaf per channel
__device__ __forceinline__ void ae_out_pixel(float (&acc)[3], const float* up5, const float* Ws, const float* bias,
                                             int64_t img, int oy, int ox) {
  acc[0] = bias[0]; acc[1] = bias[1]; acc[2] = bias[2];
#pragma unroll
  for (int ay = 0; ay < 2; ++ay) {
    const int ky = ((oy + 1) & 1) + 2 * ay, iy = (oy + 1 - ky) >> 1;
    if ((unsigned)iy >= 64u) continue;
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
      const int kx = ((ox + 1) & 1) + 2 * ax, ix = (ox + 1 - kx) >> 1;
      if ((unsigned)ix >= 64u) continue;
      const float* src = up5 + ((img << 12) + iy * 64 + ix) * 64;
      const float* wt = Ws + (ky * 4 + kx) * 4;
#pragma unroll 4
      for (int c4 = 0; c4 < 16; ++c4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wt + (4 * c4 + e) * 64);
          acc[0] = fmaf(v[e], wv[0], acc[0]);
          acc[1] = fmaf(v[e], wv[1], acc[1]);
          acc[2] = fmaf(v[e], wv[2], acc[2]);
        }
      }
    }
  }
}

// one thread per output pixel
__global__ __launch_bounds__(kThreads) void k_ae_out_fwd_loss(AeOutArgs a) {
  __shared__ __attribute__((aligned(16))) float Ws[kAeOutW];
  __shared__ float red[4];
  ae_out_stage_weights(Ws, a.w);
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  float sq = 0.f;
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  if (p < a.npix) {
    const int64_t img = p >> 14;
    const int oy = (int)(p >> 7) & 127, ox = (int)p & 127;
    float acc[3];
    ae_out_pixel(acc, a.up5, Ws, a.bias, img, oy, ox);
    const float scale = 2.0f / (3.0f * (float)a.npix);
    const int64_t base = img * 3 * 16384 + (p & 16383);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float y = tanhf(acc[e]);
      const float d = y - a.img[base + e * 16384];
      sq += d * d;
      g[e] = scale * d * (1.f - y * y);
      if (a.recon != nullptr) a.recon[base + e * 16384] = y;
    }
    *reinterpret_cast<f32x4*>(a.g6 + p * 4) = g;
  }
  sq = block_sum(sq, red);
  const float g0 = block_sum(g[0], red), g1 = block_sum(g[1], red), g2 = block_sum(g[2], red);
  if (threadIdx.x == 0) *reinterpret_cast<f32x4*>(a.partial + 4 * (size_t)blockIdx.x) = f32x4{sq, g0, g1, g2};
}

// ------------------------------------------------------------------------------------------ eval-mode output layer
// y = tanh(b + deconv6(up5)) with nothing of the training loss in it: no g6, no gradient sums.  One thread per output
// pixel, the arithmetic of k_ae_out_fwd_loss (ae_out_pixel).  Outputs, each optional: floats NCHW [n][3][128][128] and
// bytes HWC [n][128][128][3] = trunc(((y + 1) / 2) * 255) in fp32, the reference's denorm(...).astype(np.uint8)
// (train_autoencoder.py:42-43, 97-100).  TGT: what the reconstruction is compared with -- 0 nothing, 1 floats NCHW,
// 2 byte frames HWC normalised through u8_norm_table (the floats the loader would have uploaded) -- and then the
// workgroup's squared-error sum goes to partial[block].  A workgroup is 256 consecutive pixels of ONE image (16,384 =
// 64 x 256), so partial[64 i .. 64 i + 63] are image i's; a workgroup's 768 bytes (in and out) are contiguous and 4-byte
// aligned: they pass through LDS as 192 dwords.
struct AeEvalOutArgs {
  const float* up5; const float* w; const float* bias;
  const float* tgt_f32; const unsigned char* tgt_u8;
  float* recon; unsigned char* recon_u8; float* partial;
};
template <int TGT>
__global__ __launch_bounds__(kThreads) void k_ae_out_fwd(AeEvalOutArgs a) {
  __shared__ __attribute__((aligned(16))) float Ws[kAeOutW];
  __shared__ float red[4];
  __shared__ float lut[TGT == 2 ? 256 : 1];
  __shared__ unsigned int tin[TGT == 2 ? 192 : 1];
  __shared__ unsigned int tout[192];
  const int t = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * kThreads + t;               // (the grid is exactly n x 64 workgroups)
  if (TGT == 2) {
    u8_norm_table(lut);
    if (t < 192) tin[t] = reinterpret_cast<const unsigned int*>(a.tgt_u8 + (int64_t)blockIdx.x * (kThreads * 3))[t];
  }
  ae_out_stage_weights(Ws, a.w);                                       // (ends with a barrier: lut and tin are visible)
  const int64_t img = p >> 14;
  const int oy = (int)(p >> 7) & 127, ox = (int)p & 127;
  float acc[3];
  ae_out_pixel(acc, a.up5, Ws, a.bias, img, oy, ox);
  const int64_t base = img * 3 * 16384 + (p & 16383);
  float sq = 0.f;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const float y = tanhf(acc[e]);
    if (a.recon != nullptr) a.recon[base + e * 16384] = y;
    if (a.recon_u8 != nullptr)
      reinterpret_cast<unsigned char*>(tout)[3 * t + e] = (unsigned char)(int)(((y + 1.0f) / 2.0f) * 255.0f);
    if (TGT != 0) {
      const float x = TGT == 1 ? a.tgt_f32[base + e * 16384] : lut[reinterpret_cast<const unsigned char*>(tin)[3 * t + e]];
      const float d = y - x;
      sq += d * d;
    }
  }
  if (a.recon_u8 != nullptr) {                                         // (uniform)
    __syncthreads();
    if (t < 192) reinterpret_cast<unsigned int*>(a.recon_u8 + (int64_t)blockIdx.x * (kThreads * 3))[t] = tout[t];
  }
  if (TGT != 0) {
    sq = block_sum(sq, red);
    if (t == 0) a.partial[blockIdx.x] = sq;
  }
}

// The errors of one pass of np images: thread i sums image i's 64 partial sums in index order (fp32) -> sq_err[i] =
// sum / 49,152; thread 0 then adds the pass's per-image values, in image order, to the call's running sum -- a double,
// so that the batch mean is the correctly rounded mean of the fp32 per-image values whatever the batch size -- and the
// last pass writes mean_err = running / n.  No atomics: two runs give the same bits.
constexpr int kAeDecPass = 128;                                        // images per pass of ndp_ae_decode
struct AeErrArgs { const float* partial; float* sq_err; float* mean_err; double* running; int np, first, last; int64_t n; };
__global__ __launch_bounds__(kThreads) void k_ae_err_finish(AeErrArgs a) {
  __shared__ float vals[kAeDecPass];
  const int i = threadIdx.x;
  if (i < a.np) {
    const f32x4* src = reinterpret_cast<const f32x4*>(a.partial + 64 * i);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const f32x4 v = src[j];
      s += v[0]; s += v[1]; s += v[2]; s += v[3];
    }
    s = s / 49152.0f;
    vals[i] = s;
    if (a.sq_err != nullptr) a.sq_err[i] = s;
  }
  __syncthreads();
  if (i == 0) {
    double r = a.first ? 0.0 : *a.running;
    for (int j = 0; j < a.np; ++j) r += (double)vals[j];
    *a.running = r;
    if (a.last && a.mean_err != nullptr) *a.mean_err = (float)(r / (double)a.n);
  }
}

// d up5 [i][ci] = sum over the 16 taps (ky, kx) and co < 3 of g6[(2 iy - 1 + ky, 2 ix - 1 + kx)][co] * W[ci][ky kx][co].
// Wave w owns channels 16 w .. 16 w + 15 of the workgroup's pixels, a lane one pixel per pass (weights: wave-uniform LDS
// reads).  Epilogue: deconv5_bn's backward sums over the workgroup's pixels, lanes by shuffles in a fixed order.
constexpr int kAeDgradRows = 256;                          // input pixels per workgroup (4 passes of 64)
__global__ __launch_bounds__(kThreads) void k_ae_out_dgrad(AeOutArgs a) {
  __shared__ __attribute__((aligned(16))) float Ws[kAeOutW];
  __shared__ __attribute__((aligned(16))) float sums[2 * 64];
  ae_out_stage_weights(Ws, a.w);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ch0 = wave * 16;
  const bool stat = a.ep.mode != 0;
  f32x4 s1[4], s2[4], mu[4], is[4];
#pragma unroll
  for (int c4 = 0; c4 < 4; ++c4) {
    s1[c4] = s2[c4] = mu[c4] = is[c4] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (stat) {
      mu[c4] = *reinterpret_cast<const f32x4*>(a.ep.mean + ch0 + 4 * c4);
      is[c4] = *reinterpret_cast<const f32x4*>(a.ep.invstd + ch0 + 4 * c4);
    }
  }
  const int64_t r0 = (int64_t)blockIdx.x * kAeDgradRows;
  for (int pass = 0; pass < kAeDgradRows / 64; ++pass) {
    const int64_t i = r0 + pass * 64 + lane;
    if (i >= a.npix) break;                                // (the tail: the remaining lanes idle, no barrier below)
    const int64_t img = i >> 12;
    const int iy = (int)(i >> 6) & 63, ix = (int)i & 63;
    f32x4 xv[4], yv[4];
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {                       // operands of the statistics: in flight during the sums
      xv[c4] = yv[c4] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (stat) {
        xv[c4] = *reinterpret_cast<const f32x4*>(a.ep.x + i * a.ep.x_ld + ch0 + 4 * c4);
        yv[c4] = *reinterpret_cast<const f32x4*>(a.ep.y + i * a.ep.y_ld + ch0 + 4 * c4);
      }
    }
    f32x4 acc[4];
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) acc[c4] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      const int oy = 2 * iy - 1 + ky;
      if ((unsigned)oy >= 128u) continue;
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        const int ox = 2 * ix - 1 + kx;
        if ((unsigned)ox >= 128u) continue;
        const f32x4 d = *reinterpret_cast<const f32x4*>(a.g6 + ((img << 14) + oy * 128 + ox) * 4);
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(Ws + ((ch0 + 4 * c4 + e) * 16 + ky * 4 + kx) * 4);
            acc[c4][e] = fmaf(d[0], wv[0], acc[c4][e]);
            acc[c4][e] = fmaf(d[1], wv[1], acc[c4][e]);
            acc[c4][e] = fmaf(d[2], wv[2], acc[c4][e]);
          }
      }
    }
    float* o = a.du5 + i * 64 + ch0;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      *reinterpret_cast<f32x4*>(o + 4 * c4) = acc[c4];
      if (stat) fm_stat_terms(a.ep.mode, acc[c4], yv[c4], xv[c4], mu[c4], is[c4], s1[c4], s2[c4]);
    }
  }
  if (!stat) return;
#pragma unroll
  for (int c4 = 0; c4 < 4; ++c4)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v1 = wave_sum(s1[c4][e]), v2 = wave_sum(s2[c4][e]);
      if (lane == 0) {
        sums[ch0 + 4 * c4 + e] = v1;
        sums[64 + ch0 + 4 * c4 + e] = v2;
      }
    }
  __syncthreads();
  fm_stat_publish(a.ep, (int)blockIdx.x, 0, 64, sums);
}

// d W[ci][ky kx][co] = sum over input pixels i of up5[i][ci] * g6[(2 iy - 1 + ky, 2 ix - 1 + kx)][co].  Thread = (ci: lane,
// ky: wave), the four kx and three co in registers; a workgroup walks its block of input pixels in order (four in
// flight), and writes its [64][16][4] sums to its slab.
__global__ __launch_bounds__(kThreads) void k_ae_out_wgrad(AeOutArgs a) {
  const int ci = threadIdx.x & 63, ky = threadIdx.x >> 6;
  const int64_t p0 = (int64_t)blockIdx.x * a.rows_per_block;
  const int64_t p1 = p0 + a.rows_per_block < a.npix ? p0 + a.rows_per_block : a.npix;
  f32x4 acc[4];
#pragma unroll
  for (int kx = 0; kx < 4; ++kx) acc[kx] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t pb = p0; pb < p1; pb += 4) {
    float u[4];
    f32x4 d[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t i = pb + q;
      const bool live = i < p1;
      const int64_t ic = live ? i : p0;
      const int64_t img = ic >> 12;
      const int iy = (int)(ic >> 6) & 63, ix = (int)ic & 63;
      const int oy = 2 * iy - 1 + ky;
      u[q] = live ? a.up5[ic * 64 + ci] : 0.f;
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        const int ox = 2 * ix - 1 + kx;
        const bool ok = (unsigned)oy < 128u && (unsigned)ox < 128u;
        d[q][kx] = *reinterpret_cast<const f32x4*>(a.g6 + ((img << 14) + (ok ? oy * 128 + ox : 0)) * 4);
        if (!ok) d[q][kx] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) acc[kx] += d[q][kx] * u[q];
  }
  float* slab = a.slabs + (size_t)blockIdx.x * kAeOutW + ci * 64 + ky * 16;
#pragma unroll
  for (int kx = 0; kx < 4; ++kx) {
    f32x4 v = acc[kx];
    v[3] = 0.f;                                            // (the padded output channel)
    *reinterpret_cast<f32x4*>(slab + 4 * kx) = v;
  }
}

// ------------------------------------------------------------------------------------------ host side
// Workspace (floats): [P2 weights][BatchNorm scratch + statistics accumulators (the forward model's)][per-image maps x n]
// [loss partial sums][split-K partial sums][weight-gradient slabs][this rank's copy of the accumulators (cross-rank
// statistics: FmWs::stat_acc_local)]
enum AeTensor {
  AET_COLS = 0, AET_RAW1, AET_A1, AET_RAW2, AET_A2, AET_RAW3, AET_A3, AET_A4, AET_A5, AET_Z,
  AET_RAWU1, AET_U1, AET_RAWU2, AET_U2, AET_RAWU3, AET_U3, AET_RAWU4, AET_U4, AET_RAWU5, AET_U5, AET_G6,
  AET_DU5, AET_DU4, AET_DU3, AET_DU2, AET_DU1, AET_DZ, AET_DA5, AET_DA4, AET_DA3, AET_DA2, AET_DA1, AET_COUNT
};
static const int64_t kAeTensorFloats[AET_COUNT] = {          // per image
    4096 * 32, 4096 * 64, 4096 * 64, 1024 * 128, 1024 * 128, 256 * 256, 256 * 256, 64 * 512, 16 * 1024, 128,
    16 * 1024, 16 * 1024, 64 * 512, 64 * 512, 256 * 256, 256 * 256, 1024 * 128, 1024 * 128, 4096 * 64, 4096 * 64, 16384 * 4,
    4096 * 64, 1024 * 128, 256 * 256, 64 * 512, 16 * 1024, 128, 16 * 1024, 64 * 512, 256 * 256, 1024 * 128, 4096 * 64};
static int64_t ae_fixed_floats() {
  return fm_p2_offset(kAeNet, kAeLayers) + 3 * kFmBnChannels + 2 * fm_stat_offset_words(kFmStatSlots);
}
static int64_t ae_tensor_offset(int64_t n, int t) {
  int64_t o = ae_fixed_floats();
  for (int i = 0; i < t; ++i) o += fm_round4(n * kAeTensorFloats[i]);
  return o;
}
static int64_t ae_ws_floats(int64_t n) {
  return ae_tensor_offset(n, AET_COUNT) + fm_round4(n * 256) /* loss partial sums */ + kFmPartCap + kFmSlabCap +
         2 * fm_stat_offset_words(kFmStatSlots);
}
struct AeWs { FmWs fm; float* t[AET_COUNT]; };
static AeWs ae_ws(float* ws, int64_t n) {
  AeWs w;
  memset(&w, 0, sizeof(w));
  fm_ws_head(w.fm, ws, kAeNet);
  for (int i = 0; i < AET_COUNT; ++i) w.t[i] = ws + ae_tensor_offset(n, i);
  w.fm.loss_partial = ws + ae_tensor_offset(n, AET_COUNT);
  w.fm.part = w.fm.loss_partial + fm_round4(n * 256);
  w.fm.slabs = w.fm.part + kFmPartCap;
  w.fm.stat_acc_local = reinterpret_cast<long long*>(w.fm.slabs + kFmSlabCap);
  return w;
}

// where the maps live (FmMaps): nothing is concatenated, every map's pixel stride is its channel count
static FmMaps ae_maps(const AeWs& aw) {
  float* const* t = aw.t;
  auto at = [&](int tensor, int ld) { return FmView{t[tensor], ld}; };
  FmMaps m;
  memset(&m, 0, sizeof(m));
  m.in[0] = at(AET_COLS, 32);   m.raw[0] = at(AET_RAW1, 64);                                       // conv1
  m.in[1] = at(AET_A1, 64);     m.raw[1] = at(AET_RAW2, 128);    m.din[1] = at(AET_DA1, 64);       // conv2
  m.in[2] = at(AET_A2, 128);    m.raw[2] = at(AET_RAW3, 256);    m.din[2] = at(AET_DA2, 128);      // conv3
  m.in[3] = at(AET_A3, 256);                                     m.din[3] = at(AET_DA3, 256);      // conv4
  m.in[4] = at(AET_A4, 512);                                     m.din[4] = at(AET_DA4, 512);      // conv5
  m.in[5] = at(AET_A5, 1024);                                    m.din[5] = at(AET_DA5, 1024);     // conv6
  m.in[6] = at(AET_Z, 128);     m.raw[6] = at(AET_RAWU1, 1024);  m.din[6] = at(AET_DZ, 128);       // deconv1
  m.in[7] = at(AET_U1, 1024);   m.raw[7] = at(AET_RAWU2, 512);   m.din[7] = at(AET_DU1, 1024);     // deconv2
  m.in[8] = at(AET_U2, 512);    m.raw[8] = at(AET_RAWU3, 256);   m.din[8] = at(AET_DU2, 512);      // deconv3
  m.in[9] = at(AET_U3, 256);    m.raw[9] = at(AET_RAWU4, 128);   m.din[9] = at(AET_DU3, 256);      // deconv4
  m.in[10] = at(AET_U4, 128);   m.raw[10] = at(AET_RAWU5, 64);   m.din[10] = at(AET_DU4, 128);     // deconv5
  m.in[11] = at(AET_U5, 64);                                     m.din[11] = at(AET_DU5, 64);      // deconv6 (k_ae_out_*)
  m.in[12] = at(AET_G6, 4);                                                                        // (d loss / d pre-tanh output)
  fm_maps_close(m, kAeNet);
  return m;
}

// forward pass, training mode, through the loss: g6 = d loss / d (pre-tanh output), loss partial sums
static int ae_forward_loss(hipStream_t st, const float* params, float* running, const float* images, int64_t n, float* recon,
                           const AeWs& aw, const FmStatSync* sync) {
  fm_attrs();
  const FmWs& ws = aw.fm;
  const FmMaps m = ae_maps(aw);
  const FmRun r = {st, kAeNet, m, ws, n, params, running, nullptr, sync};
  int rc;
  {
    // conv1's columns, and every statistics accumulator of the step zeroed (k_fm_image_cols without actions)
    KTimer kt("k_fm_image_cols", st);
    const int64_t opix = n * 4096;
    const int64_t zero_words = fm_stat_offset_words(kFmStatSlots);
    const unsigned blocks = (unsigned)((opix + kThreads - 1) / kThreads + (zero_words / 2 + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_fm_image_cols<false>, dim3(blocks), dim3(kThreads), 0, st, (const void*)images, opix, m.in[0].p,
                       (const float*)nullptr, (int64_t)0, (float*)nullptr, ws.stat_acc, zero_words);
  }
  FM_TRY(check_launch("k_fm_image_cols"));
  const FmEpReq none = fm_ep_none();
  // ---- encoder (image_autoencoder.py:36-49): conv1 (its columns) .. conv3 + BatchNorm, conv4 / conv5 + ReLU, conv6
  for (int l = 0; l < 3; ++l) {
    FM_TRY(fm_layer_fwd(r, l, 0, fm_ep_bn_fwd(fm_bn_of(kAeNet, l))));
    FM_TRY(fm_layer_bn_fwd(r, l, 1));
  }
  FM_TRY(fm_layer_fwd(r, 3, 1, none));
  FM_TRY(fm_layer_fwd(r, 4, 1, none));
  FM_TRY(fm_layer_fwd(r, 5, 0, none));
  // ---- decoder (image_autoencoder.py:80-87): deconv1 .. deconv5 + BatchNorm, the output layer with the loss
  for (int l = 6; l < 11; ++l) {
    FM_TRY(fm_layer_fwd(r, l, 0, fm_ep_bn_fwd(fm_bn_of(kAeNet, l))));
    FM_TRY(fm_layer_bn_fwd(r, l, 1));
  }
  {
    AeOutArgs o;
    memset(&o, 0, sizeof(o));
    o.up5 = m.in[11].p; o.w = fm_w1(r, 11); o.bias = fm_bias(r, 11); o.img = images;
    o.g6 = m.in[12].p; o.recon = recon; o.partial = ws.loss_partial; o.npix = n * 16384;
    KTimer kt("k_ae_out_fwd_loss", st);
    hipLaunchKernelGGL(k_ae_out_fwd_loss, dim3((unsigned)((o.npix + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, o);
  }
  return check_launch("k_ae_out_fwd_loss");
}

// backward pass: from g6 to every gradient in `grad` (the bias gradient of deconv6 comes from the loss' partial sums).
// buckets: record the gradient buckets' events (ndp_ae_train_grads_dp); null: one slab-sum launch at the end
static int ae_backward(hipStream_t st, const float* params, int64_t n, float* grad, const AeWs& aw, const FmStatSync* sync,
                       FmBucketEvents* buckets) {
  const FmWs& ws = aw.fm;
  const FmMaps m = ae_maps(aw);
  const FmRun r = {st, kAeNet, m, ws, n, params, nullptr, grad, sync};
  int rc;
  FmSlabPlan plan = fm_plan_new();
  // bucket b is complete behind everything launched so far but the row-chunk slabs of its layers: sum them now, then
  // record its event
  auto close_bucket = [&](int b) -> int {
    if (buckets == nullptr) return NDP_OK;
    const int rs = fm_slab_sums(st, plan);
    fm_plan_reset(plan);
    if (rs != NDP_OK) return rs;
    if (hipEventRecord(buckets->ev[b], st) != hipSuccess) return fail(NDP_E_LAUNCH, "autoencoder: hipEventRecord failed");
    return NDP_OK;
  };
  const int64_t in_pix = n * 4096;
  {
    // deconv6's weight gradient: one slab per block of input pixels (at most 1,024 blocks), summed with the others' slabs
    AeOutArgs o;
    memset(&o, 0, sizeof(o));
    int64_t nblk = 1024;
    if (nblk > kFmSlabCap / kAeOutW) nblk = kFmSlabCap / kAeOutW;
    o.rows_per_block = (in_pix + nblk - 1) / nblk;
    nblk = (in_pix + o.rows_per_block - 1) / o.rows_per_block;
    o.up5 = m.in[11].p; o.g6 = m.in[12].p; o.npix = in_pix;
    o.slabs = fm_plan_append(plan, ws, grad + fm_param_offset(kAeNet, 11, false), nblk, kAeOutW, kAeOutW / 4);
    KTimer kt("k_ae_out_wgrad", st);
    hipLaunchKernelGGL(k_ae_out_wgrad, dim3((unsigned)nblk), dim3(kThreads), 0, st, o);
  }
  FM_TRY(check_launch("k_ae_out_wgrad"));
  {
    // deconv6's data gradient + the BatchNorm-backward sums of deconv5_bn over it
    AeOutArgs o;
    memset(&o, 0, sizeof(o));
    o.w = fm_w1(r, 11); o.g6 = m.in[12].p; o.du5 = m.din[11].p; o.npix = in_pix;
    fm_ep_fill(o.ep, fm_ep_bn_bwd_of(r, 10), ws);
    KTimer kt("k_ae_out_dgrad", st);
    hipLaunchKernelGGL(k_ae_out_dgrad, dim3((unsigned)((in_pix + kAeDgradRows - 1) / kAeDgradRows)), dim3(kThreads), 0, st, o);
  }
  FM_TRY(check_launch("k_ae_out_dgrad"));
  // deconv5 .. deconv2: dense = the layer's input map, gathered = d(raw output) at the 4x4 stride-2 taps; every data
  // gradient leaves the sums the next BatchNorm backward needs
  for (int l = 10; l >= 7; --l) {
    FM_TRY(fm_layer_bn_bwd(r, l));
    FM_TRY(fm_layer_wgrad(r, st, l, plan));
    if (l <= 8) FM_TRY(close_bucket(8 - l));                            // bucket 0 ends with deconv3, 1 with deconv2
    FM_TRY(fm_layer_dgrad(r, l, 0, fm_ep_bn_bwd_of(r, l - 1)));
  }
  // deconv1: a 4x4 "image" of d(raw) per code
  FM_TRY(fm_layer_bn_bwd(r, 6));
  FM_TRY(fm_layer_wgrad(r, st, 6, plan));
  // conv6: d code, whose column sums are conv6's bias gradient
  FM_TRY(fm_layer_dgrad(r, 6, 0, fm_ep_bias(4, 20, {nullptr, 0})));
  FM_TRY(fm_bias_finish(r, st, 0));
  FM_TRY(fm_layer_wgrad(r, st, 5, plan));
  FM_TRY(close_bucket(2));
  // conv5, conv4 (ReLU, no BatchNorm): the ReLU's backward is applied as the finished gradient is written
  FM_TRY(fm_layer_dgrad(r, 5, 0, fm_ep_bias(3, 21, m.in[5])));
  FM_TRY(fm_bias_finish(r, st, 1));
  FM_TRY(fm_layer_wgrad(r, st, 4, plan));
  FM_TRY(close_bucket(3));
  FM_TRY(fm_layer_dgrad(r, 4, 0, fm_ep_bias(3, 22, m.in[4])));
  FM_TRY(fm_bias_finish(r, st, 2));
  FM_TRY(fm_layer_wgrad(r, st, 3, plan));
  FM_TRY(fm_layer_dgrad(r, 3, 0, fm_ep_bn_bwd_of(r, 2)));
  // conv3 .. conv1 (the images need no gradient: conv1's data gradient is skipped; its weight gradient: the columns)
  for (int l = 2; l >= 0; --l) {
    FM_TRY(fm_layer_bn_bwd(r, l));
    FM_TRY(fm_layer_wgrad(r, st, l, plan));
    if (l > 0) FM_TRY(fm_layer_dgrad(r, l, 0, fm_ep_bn_bwd_of(r, l - 1)));
  }
  if (buckets == nullptr) return fm_slab_sums(st, plan);
  FM_TRY(close_bucket(4));
  return close_bucket(5);                                              // (nothing left to sum: the BatchNorm parameters)
}

// one training iteration's gradients: ndp_ae_train_grads (sync, buckets null) and ndp_ae_train_grads_dp
static int ae_train_grads(const char* name, const float* params, float* running_stats, const float* images, int64_t n_images,
                          float* grad, float* loss, float* loss_sum, float* recon_out, float* workspace, void* stream,
                          const FmStatSync* sync, FmBucketEvents* buckets) {
  NDP_CHECK_ARG(params && images && grad && loss && workspace && n_images >= 1, "%s: bad arguments", name);
  NDP_CHECK_ARG(n_images <= kAeMaxImages, "%s: more than %d images per call", name, (int)kAeMaxImages);
  NDP_CHECK_ARG(aligned16(params) && aligned16(images) && aligned16(grad) && aligned16(workspace) &&
                (!running_stats || aligned16(running_stats)) && (!recon_out || aligned16(recon_out)),
                "%s: buffers must be 16-byte aligned", name);
  hipStream_t st = (hipStream_t)stream;
  const AeWs ws = ae_ws(workspace, n_images);
  int rc = ae_forward_loss(st, params, running_stats, images, n_images, recon_out, ws, sync);
  if (rc) return rc;
  const int nblocks = (int)(n_images * 64);
  hipLaunchKernelGGL(k_fm_loss_final, dim3(1), dim3(kThreads), 0, st, (const float*)ws.fm.loss_partial, nblocks,
                     1.0 / (3.0 * (double)(n_images * 16384)), loss, loss_sum, grad + fm_param_offset(kAeNet, 11, true));
  rc = check_launch("k_fm_loss_final");
  if (rc) return rc;
  return ae_backward(st, params, n_images, grad, ws, sync, buckets);
}

// ------------------------------------------------------------------------------------------ eval-mode decoder
// Decoder.forward in eval mode (image_autoencoder.py:80-87) with the BatchNorms folded into the transposed convolutions on
// the host (models/image_autoencoder.py: fold_decoder_params; relu(bn(deconv(x))) = relu(deconv'(x)) with w' = w * scale,
// b' = (b - running_mean) * scale + beta, scale = gamma / sqrt(running_var + eps)).  The folded decoder is a network of
// its own in the sense of ndp_forward_model.inc's tables: deconv1..6, NO BatchNorm, no gradient buckets; its parameter
// vector is [W (P1)][bias] per layer, the second weight order of deconv1..5 is made from it by k_fm_pack into the head of
// the decode workspace.  Launches per pass: deconv1 (mode 3; k_fm_rows_cls up to 4 images), deconv2..4 (mode 1, K split
// where fm_gemm chooses it: + k_fm_splitk_reduce), deconv5 (k_fm_deconv32<true> from 16 images, else mode 1), every one
// with bias + ReLU in its epilogue, writing the next layer's input map; k_ae_out_fwd; with a target k_ae_err_finish.
// Not one BatchNorm launch, not one map written twice.
constexpr int kAeDecLayers = 6;
static const FmLayer kAeDec[kAeDecLayers] = {
    {FM_DECONV, 128, 1024, 1, 4, 4, 1, 0, 128, 1024, FM_P2_DECONV1},    // 0 deconv1
    {FM_DECONV, 1024, 512, 4, 8, 4, 2, 1, 1024, 512, FM_P2_DECONV_S2},  // 1 deconv2
    {FM_DECONV, 512, 256, 8, 16, 4, 2, 1, 512, 256, FM_P2_DECONV_S2},   // 2 deconv3
    {FM_DECONV, 256, 128, 16, 32, 4, 2, 1, 256, 128, FM_P2_DECONV_S2},  // 3 deconv4
    {FM_DECONV, 128, 64, 32, 64, 4, 2, 1, 128, 64, FM_P2_DECONV_S2},    // 4 deconv5
    {FM_DECONV, 64, 3, 64, 128, 4, 2, 1, 64, 4, FM_P2_NONE},            // 5 deconv6 (k_ae_out_fwd reads P1)
};
static const FmLabels kAeDecLabels[kAeDecLayers] = {
    FM_LABELS("aed.deconv1"), FM_LABELS("aed.deconv2"), FM_LABELS("aed.deconv3"), FM_LABELS("aed.deconv4"),
    FM_LABELS("aed.deconv5"), FM_LABELS("aed.deconv6")};
static const FmNet kAeDecNet = {kAeDec, kAeDecLayers, 0, nullptr, nullptr, 0, kAeDecLabels};
// Workspace (floats): [P2 of deconv1..5][up1..up5 x min(n, kAeDecPass) images][squared-error partial sums: 64 per image
// of a pass][the running sum of the per-image errors: one double][split-K partial sums]
enum AeDecTensor { ADT_U1 = 0, ADT_U2, ADT_U3, ADT_U4, ADT_U5, ADT_COUNT };
static const int64_t kAeDecTensorFloats[ADT_COUNT] = {16 * 1024, 64 * 512, 256 * 256, 1024 * 128, 4096 * 64};   // per image
static int64_t ae_dec_cap(int64_t n) { return n < kAeDecPass ? n : kAeDecPass; }
static int64_t ae_dec_tensor_offset(int64_t cap, int t) {
  int64_t o = fm_p2_offset(kAeDecNet, kAeDecLayers);
  for (int i = 0; i < t; ++i) o += cap * kAeDecTensorFloats[i];
  return o;
}
static int64_t ae_dec_ws_floats(int64_t n) {
  const int64_t cap = ae_dec_cap(n);
  return ae_dec_tensor_offset(cap, ADT_COUNT) + cap * 64 + 4 + kFmPartCap;
}

// where a pass' maps live (FmMaps): the caller's codes, then up1 .. up5 (t: the workspace tensors), each layer writing the next one's input
static FmMaps ae_dec_maps(const float* codes, float* const* t) {
  FmMaps m;
  memset(&m, 0, sizeof(m));
  m.in[0] = {const_cast<float*>(codes), 128};
  for (int i = 0; i < ADT_COUNT; ++i) m.in[i + 1] = {t[i], kAeDec[i].cout_pad};
  fm_maps_close(m, kAeDecNet);
  return m;
}

// one pass: np <= kAeDecPass codes -> up5 in the workspace; every layer with bias + ReLU in its epilogue
static int ae_decode_pass(hipStream_t st, const float* P, const float* codes, int64_t np, const FmWs& ws, float* const* t) {
  const FmMaps m = ae_dec_maps(codes, t);
  const FmRun r = {st, kAeDecNet, m, ws, np, P, nullptr, nullptr, nullptr};
  int rc;
  for (int l = 0; l < 5; ++l) FM_TRY(fm_layer_fwd(r, l, 1, fm_ep_none()));
  return NDP_OK;
}

static int ae_decode(const float* params, const float* codes, int64_t n, float* recon_f32, unsigned char* recon_u8,
                     const float* target_f32, const unsigned char* target_u8, float* sq_err, float* mean_err,
                     float* workspace, void* stream) {
  NDP_CHECK_ARG(params && codes && workspace && n >= 1, "ndp_ae_decode: bad arguments");
  NDP_CHECK_ARG(!(target_f32 && target_u8), "ndp_ae_decode: at most one target");
  const bool tgt = target_f32 || target_u8;
  NDP_CHECK_ARG(tgt || (!sq_err && !mean_err), "ndp_ae_decode: sq_err / mean_err need a target");
  NDP_CHECK_ARG(recon_f32 || recon_u8 || sq_err || mean_err, "ndp_ae_decode: no output requested");
  NDP_CHECK_ARG(aligned16(params) && aligned16(codes) && aligned16(workspace) && (!recon_f32 || aligned16(recon_f32)) &&
                (!target_f32 || aligned16(target_f32)), "ndp_ae_decode: float buffers must be 16-byte aligned");
  NDP_CHECK_ARG((reinterpret_cast<uintptr_t>(recon_u8) & 3) == 0 && (reinterpret_cast<uintptr_t>(target_u8) & 3) == 0,
                "ndp_ae_decode: byte buffers must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  fm_attrs();
  const int64_t cap = ae_dec_cap(n);
  FmWs ws;
  memset(&ws, 0, sizeof(ws));
  ws.p2 = workspace;
  float* t[ADT_COUNT];
  for (int i = 0; i < ADT_COUNT; ++i) t[i] = workspace + ae_dec_tensor_offset(cap, i);
  float* partial = workspace + ae_dec_tensor_offset(cap, ADT_COUNT);
  double* running = reinterpret_cast<double*>(partial + cap * 64);
  ws.part = partial + cap * 64 + 4;
  const bool errs = tgt && (sq_err || mean_err);
  for (int64_t i0 = 0; i0 < n; i0 += kAeDecPass) {
    const int64_t np = n - i0 < kAeDecPass ? n - i0 : kAeDecPass;
    int rc = ae_decode_pass(st, params, codes + i0 * 128, np, ws, t);
    if (rc) return rc;
    AeEvalOutArgs o;
    memset(&o, 0, sizeof(o));
    o.up5 = t[ADT_U5]; o.w = params + fm_param_offset(kAeDecNet, 5, false); o.bias = params + fm_param_offset(kAeDecNet, 5, true);
    o.recon = recon_f32 ? recon_f32 + i0 * 49152 : nullptr;
    o.recon_u8 = recon_u8 ? recon_u8 + i0 * 49152 : nullptr;
    o.partial = partial;
    const dim3 grid((unsigned)(np * 64));
    {
      KTimer kt("k_ae_out_fwd", st);
      if (errs && target_f32) {
        o.tgt_f32 = target_f32 + i0 * 49152;
        hipLaunchKernelGGL(k_ae_out_fwd<1>, grid, dim3(kThreads), 0, st, o);
      } else if (errs) {
        o.tgt_u8 = target_u8 + i0 * 49152;
        hipLaunchKernelGGL(k_ae_out_fwd<2>, grid, dim3(kThreads), 0, st, o);
      } else {
        hipLaunchKernelGGL(k_ae_out_fwd<0>, grid, dim3(kThreads), 0, st, o);
      }
    }
    rc = check_launch("k_ae_out_fwd");
    if (rc) return rc;
    if (!errs) continue;
    AeErrArgs e;
    memset(&e, 0, sizeof(e));
    e.partial = partial; e.sq_err = sq_err ? sq_err + i0 : nullptr; e.mean_err = mean_err; e.running = running;
    e.np = (int)np; e.first = i0 == 0; e.last = i0 + np == n; e.n = n;
    KTimer kt("k_ae_err_finish", st);
    hipLaunchKernelGGL(k_ae_err_finish, dim3(1), dim3(kThreads), 0, st, e);
    rc = check_launch("k_ae_err_finish");
    if (rc) return rc;
  }
  return NDP_OK;
}

#undef FM_TRY

}  // namespace ndp

extern "C" {

int64_t ndp_ae_decoder_param_floats(void) { return ndp::fm_param_floats(ndp::kAeDecNet); }
int ndp_ae_decoder_layout(int what, int index, int64_t* offset, int64_t* dims) {
  return ndp::fm_layout(ndp::kAeDecNet, "ndp_ae_decoder_layout", what, index, offset, dims);
}
int64_t ndp_ae_decode_pass_images(void) { return ndp::kAeDecPass; }
int64_t ndp_ae_decode_workspace_floats(int64_t n_images) { return n_images < 1 ? 0 : ndp::ae_dec_ws_floats(n_images); }

int ndp_ae_decode_pack(const float* folded_params, float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(folded_params && workspace && aligned16(folded_params) && aligned16(workspace), "ndp_ae_decode_pack: bad arguments");
  FmWs ws;
  memset(&ws, 0, sizeof(ws));
  ws.p2 = workspace;
  return fm_pack((hipStream_t)stream, kAeDecNet, folded_params, ws);
}

int ndp_ae_decode(const float* folded_params, const float* codes, int64_t n_images, float* recon_f32, unsigned char* recon_u8,
                  const float* target_f32, const unsigned char* target_u8, float* sq_err, float* mean_err, float* workspace,
                  void* stream) {
  return ndp::ae_decode(folded_params, codes, n_images, recon_f32, recon_u8, target_f32, target_u8, sq_err, mean_err,
                        workspace, stream);
}

int64_t ndp_ae_param_floats(void) { return ndp::fm_param_floats(ndp::kAeNet); }
int64_t ndp_ae_stat_floats(void) { return ndp::fm_stat_offset(ndp::kAeBns, false); }
int64_t ndp_ae_workspace_floats(int64_t n_images) {
  return n_images < 1 || n_images > ndp::kAeMaxImages ? 0 : ndp::ae_ws_floats(n_images);
}

int64_t ndp_ae_workspace_offset(int64_t n_images, int tensor) {
  if (n_images < 1 || n_images > ndp::kAeMaxImages || tensor < 0 || tensor >= ndp::AET_COUNT) return -1;
  return ndp::ae_tensor_offset(n_images, tensor);
}

int ndp_ae_layout(int what, int index, int64_t* offset, int64_t* dims) {
  return ndp::fm_layout(ndp::kAeNet, "ndp_ae_layout", what, index, offset, dims);
}

int ndp_ae_pack_params(const float* params, float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(params && workspace && aligned16(params) && aligned16(workspace), "ndp_ae_pack_params: bad arguments");
  return fm_pack((hipStream_t)stream, kAeNet, params, ae_ws(workspace, 1).fm);
}

int ndp_ae_train_grads(const float* params, float* running_stats, const float* images, int64_t n_images, float* grad,
                       float* loss, float* loss_sum, float* recon_out, float* workspace, void* stream) {
  return ndp::ae_train_grads("ndp_ae_train_grads", params, running_stats, images, n_images, grad, loss, loss_sum, recon_out,
                             workspace, stream, nullptr, nullptr);
}

int ndp_ae_train_grads_dp(const float* params, float* running_stats, const float* images, int64_t n_images, float* grad,
                          float* loss, float* loss_sum, float* recon_out, float* workspace, void* stream,
                          ndp_fm_stat_sync_fn stat_sync, void* stat_ctx, int world) {
  using namespace ndp;
  NDP_CHECK_ARG(world >= 1 && world <= 4096, "ndp_ae_train_grads_dp: bad world size");
  NDP_CHECK_ARG(params && images && grad && loss && workspace && n_images >= 1 && n_images <= kAeMaxImages,
                "ndp_ae_train_grads_dp: bad arguments");
  FmBucketEvents* buckets = fm_bucket_events(g_ae_buckets, kAeNet);
  if (buckets == nullptr) return fail(NDP_E_LAUNCH, "ndp_ae_train_grads_dp: could not create the bucket events");
  const FmStatSync sync = {stat_sync, stat_ctx, world};
  const int rc = ae_train_grads("ndp_ae_train_grads_dp", params, running_stats, images, n_images, grad, loss, loss_sum,
                                recon_out, workspace, stream, fm_sync_on(&sync) ? &sync : nullptr, buckets);
  if (rc == NDP_OK) buckets->recorded.store(true);
  return rc;
}

int ndp_ae_grad_buckets(int64_t* offsets, int64_t* counts, int capacity, int* n_buckets) {
  using namespace ndp;
  NDP_CHECK_ARG(offsets && counts && n_buckets, "ndp_ae_grad_buckets: null pointer");
  NDP_CHECK_ARG(capacity >= kAeBuckets, "ndp_ae_grad_buckets: need room for %d buckets", kAeBuckets);
  for (int b = 0; b < kAeBuckets; ++b) fm_bucket_range(kAeNet, b, offsets + b, counts + b);
  *n_buckets = kAeBuckets;
  return NDP_OK;
}

int ndp_ae_bucket_wait(int bucket, void* stream) {
  return ndp::fm_bucket_wait(ndp::g_ae_buckets, ndp::kAeNet, bucket, stream, "ndp_ae_bucket_wait");
}

int ndp_ae_apply_adam(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int32_t* step_count, float lr,
                      float beta1, float beta2, float eps, float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(params && grad && exp_avg && exp_avg_sq && step_count && workspace, "ndp_ae_apply_adam: null pointer");
  NDP_CHECK_ARG(aligned16(params) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(workspace),
                "ndp_ae_apply_adam: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(1), 0, st, step_count, lr, beta1, beta2);
  return fm_adam_pack(st, kAeNet, params, grad, exp_avg, exp_avg_sq, step_count, beta1, beta2, eps, ae_ws(workspace, 1).fm);
}

}  // extern "C"
