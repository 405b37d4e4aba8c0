// ndp_encoder.inc -- the frozen image encoder that produces the GAN's condition codes
// (reference models/image_autoencoder.py:14-49, eval mode, no gradient: train_gan.py:75-76, 152-153)
// as gfx950 kernels.  Included at the end of ndp_kernels.hip, after ndp_capi.inc.
//
//   conv1  3 -> 64, 3x3 s2 p1 (+BN folded, ReLU)       one 32-wide K step on the matrix pipe, reads NCHW, writes NHWC
//   conv2..5  64->128->256->512->1024, 3x3 s2 p1        implicit GEMM on the fp32 MFMA pipe:
//                                                       C[M = n*OH*OW][Cout] = A[M][K = 9 Cin] . W[Cout][K]^T
//   conv6  1024 -> 128, 4x4 on the 4x4 map              the same GEMM with K = 16,384 split over blockIdx.y
//
// Activations are NHWC so that a 32-wide K chunk of the im2col row (one filter tap, 32 consecutive input
// channels) is 128 contiguous bytes.  Workgroup tile 128 x 128, K step 32, both operands staged through LDS
// (double-buffered, next step's global loads in flight during the 128 MFMAs per wave of the current one);
// the 4 waves own 64 x 64 quadrants; lane (c, q) reads 4 consecutive k of "its" row with one ds_read_b128 and
// MFMA step s pairs element s of the A and the B vector (a permutation of the k order, as in ndp_device.h).
//
// Precision NDP_ENC_BF16 (ndp_encoder_forward_lp; the definition is in include/ndp.h): the same six launches with conv1
// storing its map as bf16 and conv2..6 through k_conv_gemm_bf16 -- bf16 maps and bf16 weights straight into the bf16 MFMA,
// fp32 accumulation, fp32 partial sums and codes.

namespace ndp {

#ifndef NDP_ENC_BK
#define NDP_ENC_BK 32
#endif
constexpr int kEncBM = 128, kEncBN = 128, kEncBK = NDP_ENC_BK, kEncLD = kEncBK + 4;
constexpr int conv_gemm_lds_floats() { return 2 * (kEncBM + kEncBN) * kEncLD; }

struct ConvGemmArgs {
  const float* in;        // NHWC [n][H][W][Cin]
  const float* w;         // [Cout][K], k = (kh*KW + kw)*Cin + ci  (BatchNorm folded in)
  const float* bias;      // [Cout] (BatchNorm folded in); ignored when nsplit > 1
  float* out;             // NHWC [M][Cout]; nsplit > 1: partial sums [split][M][Cout]
  int H, W, Cin, OH, OW, Cout;
  int KW, stride, pad;
  int M, K;
  int relu;
  int nsplit, k_per_split;
  int mtiles, ntiles;
};

__global__ __launch_bounds__(kThreads, (kEncBK >= 32 ? 2 : 3)) void k_conv_gemm(ConvGemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int BM = kEncBM, BN = kEncBN, BK = kEncBK, LD = kEncLD;
  // XCD-aware order: workgroups are dealt round-robin over the 8 XCDs; the ntiles column tiles of one row tile
  // read the same im2col rows, so they run on the same XCD (one fetch into that L2)
  // (with fewer than 8 row tiles -- a handful of images -- plain order: the padded scheme would put every workgroup that
  // has work on XCD 0)
  int n_tile, m_tile;
  if (a.mtiles >= 8) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    n_tile = j % a.ntiles;
    m_tile = (j / a.ntiles) * 8 + xcd;
    if (m_tile >= a.mtiles) return;
  } else {
    n_tile = blockIdx.x % a.ntiles;
    m_tile = blockIdx.x / a.ntiles;
  }
  const int split = blockIdx.y;
  const int kbeg = split * a.k_per_split;
  const int kend = kbeg + a.k_per_split < a.K ? kbeg + a.k_per_split : a.K;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;

  // global -> LDS assignment: 4 rows (r0 + 32 u) x one 4-float quad (kq) of each operand per thread and step
  constexpr int QPR = BK / 4, RPP = kThreads / QPR, NU = BM / RPP;   // quads per row, rows per pass, passes
  const int r0 = t / QPR, kq = t % QPR;
  const float* a_img[NU];
  int a_ih0[NU], a_iw0[NU], a_base[NU];
  const float* b_row[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    int m = m_tile * BM + r0 + RPP * u;
    const bool valid = m < a.M;
    m = valid ? m : a.M - 1;
    const int n = m / (a.OH * a.OW), rem = m - n * (a.OH * a.OW);
    const int oh = rem / a.OW, ow = rem - oh * a.OW;
    a_img[u] = a.in + (size_t)n * a.H * a.W * a.Cin + 4 * kq;
    a_ih0[u] = valid ? oh * a.stride - a.pad : -(1 << 20);       // rows past M: every tap out of bounds -> zeros
    a_iw0[u] = ow * a.stride - a.pad;
    a_base[u] = ((oh * a.stride - a.pad) * a.W + a_iw0[u]) * a.Cin;   // + tap offset = element offset in the image
    b_row[u] = a.w + (size_t)(n_tile * BN + r0 + RPP * u) * a.K + 4 * kq;
  }
  f32x4 ra[NU], rb[NU];
  bool ra_ok[NU];          // padding taps: the loaded value is replaced by zero when it is WRITTEN to LDS, so that
                          // nothing consumes a load before the step's MFMAs (hipcc would wait for it at once)
  auto fetch = [&](int k0) {
    const int tap = k0 / a.Cin, ci0 = k0 - tap * a.Cin;          // uniform: one tap, 32 consecutive channels
    const int kh = tap / a.KW, kw = tap - kh * a.KW;
    const int tapoff = (kh * a.W + kw) * a.Cin + ci0;            // uniform
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const bool ok = (unsigned)(a_ih0[u] + kh) < (unsigned)a.H && (unsigned)(a_iw0[u] + kw) < (unsigned)a.W;
      ra[u] = ldg4<4>(a_img[u] + (ok ? a_base[u] + tapoff : 0));   // unconditional load from a valid address
      ra_ok[u] = ok;
      rb[u] = ldg4<4>(b_row[u] + k0);
    }
    pin_vmem();
  };
  auto stage = [&](int buf) {
    float* As = smem + buf * (BM + BN) * LD;
    float* Bs = As + BM * LD;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      *reinterpret_cast<f32x4*>(As + (r0 + RPP * u) * LD + 4 * kq) = ra_ok[u] ? ra[u] : f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(Bs + (r0 + RPP * u) * LD + 4 * kq) = rb[u];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jn = 0; jn < 4; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(kbeg);
  stage(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    const bool more = k0 + BK < kend;
    if (more) fetch(k0 + BK);                                    // in flight during this step's 128 MFMAs
    const float* As = smem + buf * (BM + BN) * LD + (wm * 64 + c) * LD + 4 * q;
    const float* Bs = smem + buf * (BM + BN) * LD + BM * LD + (wn * 64 + c) * LD + 4 * q;
    constexpr int NH = BK / 16;
    f32x4 af[NH][4], bf[NH][4];                                    // all 16-wide parts of the step up front
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[h][i] = *reinterpret_cast<const f32x4*>(As + i * 16 * LD + 16 * h);
        bf[h][i] = *reinterpret_cast<const f32x4*>(Bs + i * 16 * LD + 16 * h);
      }
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jn = 0; jn < 4; ++jn) acc[i][jn] = mfma16(bf[h][jn][s], af[h][i][s], acc[i][jn]);   // C^T tile: see epilogue
    pin_vmem();
    if (more) stage(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // epilogue: the MFMAs computed the TRANSPOSED 16 x 16 tiles (weights as the A operand), so a lane holds output
  // row (pixel) c and 4 consecutive channels 4q..4q+3 of each tile: one 16-byte store per tile
  float* out = a.out + (a.nsplit > 1 ? (size_t)split * a.M * a.Cout : 0);
  const bool fin = a.nsplit == 1;
#pragma unroll
  for (int jn = 0; jn < 4; ++jn) {
    const int col = n_tile * BN + wn * 64 + jn * 16 + 4 * q;
    const f32x4 bv = fin ? *reinterpret_cast<const f32x4*>(a.bias + col) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m_tile * BM + wm * 64 + i * 16 + c;
      if (m < a.M) {
        f32x4 v = acc[i][jn] + bv;
        if (a.relu && fin) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
        *reinterpret_cast<f32x4*>(out + (size_t)m * a.Cout + col) = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ k_conv_gemm_bf16
// k_conv_gemm with bf16 MFMA operands (precision NDP_ENC_BF16; the definition is in include/ndp.h):
// out = act(bias + sum bf16(x) . bf16(w)), products exact, the sum in fp32 in the accumulator of v_mfma_f32_16x16x32_bf16.
// Same ConvGemmArgs -- a.in is the bf16 map its producer stored (the rounding of this layer's operand, done once), a.w the
// layer's bf16 weights (k_enc_pack_lp) -- same 128 x 128 tile, XCD order, K split and epilogue.  The operand path:
//   load   both operands come as bf16 and go to LDS as they come: a 32-wide K chunk of an im2col row (one tap, 32
//          consecutive channels) is 64 contiguous bytes, 16 bytes per thread and load; a padding tap is zeroed where it
//          is written to LDS;
//   LDS    row stride 48 values = 96 bytes, the conflict-free stride of k_fm_gemm_bf16 (any 8 consecutive rows on the 8
//          even 16-byte slots, the rows at q + 1 on the odd ones);
//   read   k_fm_gemm_bf16's fragments: one 16-byte read per operand tile and 32-wide K step, lane l = 16 q + c holds row c,
//          k = 8 q .. 8 q + 7; the weights are the A operand, so a lane ends with output pixel c and channels 4 q .. 4 q + 3.
// OUT_LP: the finished map is stored as bf16 (conv2..conv5; 8 bytes per lane and tile); conv6 stores fp32 codes.  Partial
// sums of a split layer are fp32 either way.
// ReLU of the bf16 pass: a NaN stays a NaN, as the definition's torch.relu has it (fmaxf(NaN, 0) is 0: the fp32 pass,
// whose bits are pinned, drops a NaN at its first ReLU)
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

constexpr int kEncLpBK = 32, kEncLpLD = 48;             // (a K step of 64 was measured and lost at small n: DESIGN 5t)
constexpr int conv_gemm_bf16_lds_bytes() { return 2 * (kEncBM + kEncBN) * kEncLpLD * 2; }

template <bool OUT_LP>
__global__ __launch_bounds__(kThreads, 2) void k_conv_gemm_bf16(ConvGemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t smem_enc_lp[];
  constexpr int BM = kEncBM, BN = kEncBN, BK = kEncLpBK, LD = kEncLpLD;
  int n_tile, m_tile;                                                  // (k_conv_gemm's order)
  if (a.mtiles >= 8) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    n_tile = j % a.ntiles;
    m_tile = (j / a.ntiles) * 8 + xcd;
    if (m_tile >= a.mtiles) return;
  } else {
    n_tile = blockIdx.x % a.ntiles;
    m_tile = blockIdx.x / a.ntiles;
  }
  const int split = blockIdx.y;
  const int kbeg = split * a.k_per_split;
  const int kend = kbeg + a.k_per_split < a.K ? kbeg + a.k_per_split : a.K;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;

  // global -> LDS assignment: NU rows (r0 + RPP u) x one 8-value quad (16 bytes, kq) of each operand per thread and step
  constexpr int QPR = BK / 8, RPP = kThreads / QPR, NU = BM / RPP;
  const int r0 = t / QPR, kq = t % QPR;
  const uint16_t* in_lp = reinterpret_cast<const uint16_t*>(a.in);
  const uint16_t* w_lp = reinterpret_cast<const uint16_t*>(a.w);
  const uint16_t* a_img[NU];
  int a_ih0[NU], a_iw0[NU], a_base[NU];
  const uint16_t* b_row[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    int m = m_tile * BM + r0 + RPP * u;
    const bool valid = m < a.M;
    m = valid ? m : a.M - 1;
    const int n = m / (a.OH * a.OW), rem = m - n * (a.OH * a.OW);
    const int oh = rem / a.OW, ow = rem - oh * a.OW;
    a_img[u] = in_lp + (size_t)n * a.H * a.W * a.Cin + 8 * kq;
    a_ih0[u] = valid ? oh * a.stride - a.pad : -(1 << 20);       // rows past M: every tap out of bounds -> zeros
    a_iw0[u] = ow * a.stride - a.pad;
    a_base[u] = ((oh * a.stride - a.pad) * a.W + a_iw0[u]) * a.Cin;
    b_row[u] = w_lp + (size_t)(n_tile * BN + r0 + RPP * u) * a.K + 8 * kq;
  }
  u32x4 ra[NU], rb[NU];
  bool ra_ok[NU];
  auto fetch = [&](int k0) {
    const int tap = k0 / a.Cin, ci0 = k0 - tap * a.Cin;          // uniform: one tap, BK consecutive channels
    const int kh = tap / a.KW, kw = tap - kh * a.KW;
    const int tapoff = (kh * a.W + kw) * a.Cin + ci0;            // uniform
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const bool ok = (unsigned)(a_ih0[u] + kh) < (unsigned)a.H && (unsigned)(a_iw0[u] + kw) < (unsigned)a.W;
      ra[u] = *reinterpret_cast<const u32x4*>(a_img[u] + (ok ? a_base[u] + tapoff : 0));   // always a valid address
      ra_ok[u] = ok;
      rb[u] = *reinterpret_cast<const u32x4*>(b_row[u] + k0);
    }
    pin_vmem();
  };
  auto stage = [&](int buf) {
    uint16_t* As = smem_enc_lp + buf * (BM + BN) * LD;
    uint16_t* Bs = As + BM * LD;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      *reinterpret_cast<u32x4*>(As + (r0 + RPP * u) * LD + 8 * kq) = ra_ok[u] ? ra[u] : u32x4{0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4*>(Bs + (r0 + RPP * u) * LD + 8 * kq) = rb[u];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jn = 0; jn < 4; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(kbeg);
  stage(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    const bool more = k0 + BK < kend;
    if (more) fetch(k0 + BK);                                    // in flight during this step's MFMAs
    const uint16_t* As = smem_enc_lp + buf * (BM + BN) * LD + (wm * 64 + c) * LD + 8 * q;
    const uint16_t* Bs = smem_enc_lp + buf * (BM + BN) * LD + BM * LD + (wn * 64 + c) * LD + 8 * q;
    bf16x8 af[4], bf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[i] = *reinterpret_cast<const bf16x8*>(As + i * 16 * LD);
      bf[i] = *reinterpret_cast<const bf16x8*>(Bs + i * 16 * LD);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jn = 0; jn < 4; ++jn)
        acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[jn], af[i], acc[i][jn], 0, 0, 0);   // transposed tiles
    pin_vmem();
    if (more) stage(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // k_conv_gemm's epilogue: a lane holds output row (pixel) c and the channels 4q .. 4q+3 of each tile
  const bool fin = a.nsplit == 1;
  float* out = a.out + (fin ? 0 : (size_t)split * a.M * a.Cout);
#pragma unroll
  for (int jn = 0; jn < 4; ++jn) {
    const int col = n_tile * BN + wn * 64 + jn * 16 + 4 * q;
    const f32x4 bv = fin ? *reinterpret_cast<const f32x4*>(a.bias + col) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m_tile * BM + wm * 64 + i * 16 + c;
      if (m < a.M) {
        f32x4 v = acc[i][jn] + bv;
        if (a.relu && fin) v = f32x4{relu_keep_nan(v[0]), relu_keep_nan(v[1]), relu_keep_nan(v[2]), relu_keep_nan(v[3])};
        const size_t at = (size_t)m * a.Cout + col;
        if (OUT_LP && fin) *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(out) + at) = u32x2{fm_bf16_pair(v[0], v[1]), fm_bf16_pair(v[2], v[3])};
        else *reinterpret_cast<f32x4*>(out + at) = v;
      }
    }
  }
}

// out[m][co] = act(bias[co] + sum_s part[s][m][co])  (fixed order: bitwise reproducible)
__device__ __forceinline__ float splitk_sum(const float* part, int nsplit, int64_t mc, const float* bias, int cout, int64_t i) {
  float s = bias[i % cout];
  int sp = 0;
  for (; sp + 8 <= nsplit; sp += 8) {      // 8 loads in flight, summed in split order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(sp + u) * mc + i];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; sp < nsplit; ++sp) s += part[(size_t)sp * mc + i];
  return s;
}
__global__ __launch_bounds__(kThreads) void k_splitk_reduce(const float* part, int nsplit, int64_t mc, const float* bias,
                                                            int cout, int relu, float* out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= mc) return;
  const float s = splitk_sum(part, nsplit, mc, bias, cout, i);
  out[i] = relu ? fmaxf(s, 0.f) : s;
}
// ... the finished map stored as bf16 (the split layers of a NDP_ENC_BF16 pass; conv6's codes keep the fp32 one)
__global__ __launch_bounds__(kThreads) void k_splitk_reduce_bf16(const float* part, int nsplit, int64_t mc, const float* bias,
                                                                 int cout, int relu, __bf16* out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= mc) return;
  const float s = splitk_sum(part, nsplit, mc, bias, cout, i);
  out[i] = (__bf16)(relu ? relu_keep_nan(s) : s);
}

// the weights of conv2..conv6 as bf16, one launch (pack_lp_body, ndp_device.h: k_fm_pack_lp's body)
__global__ __launch_bounds__(kThreads) void k_enc_pack_lp(PackLpArgs a) { pack_lp_body(a); }

// conv1: 3 -> 64 channels, 3x3 stride 2 pad 1, 128x128 -> 64x64, BatchNorm folded, ReLU; reads the reference's NCHW
// images, writes NHWC.  K = 27 (padded to 32 with zero weights) is a single 32-wide K step of the matrix pipe:
// workgroup = 2 output rows of one image = 128 pixels x 64 channels; the im2col tile [128][32] is gathered into LDS
// (thread = pixel x 16 k), the weights [64][32] sit beside it; wave w computes pixels 32 w .. 32 w + 31 (2 x 4 tiles x
// 8 MFMAs, transposed as in k_conv_gemm so that a lane stores 4 consecutive channels).  2 % of the encoder's MACs:
// the layer is its 537 MB of output per 512 images.
struct Conv1Args { const void* img; const float* w; const float* bias; float* out; int64_t n; };
constexpr int kC1LD = 36, kC1InLD = 132;
constexpr int kC1Pairs = 4, kC1Groups = 32 / kC1Pairs;   // row pairs per workgroup; workgroups per image

// Decoded camera frames are bytes, height x width x RGB (what PIL hands the reference's loader); the reference turns them
// into its [-1, 1] float tensors on the host, utils/hdf5_load.py:9-11: (ToTensor()(image) - 0.5) * 2.0 with ToTensor =
// byte -> float32, / 255.  The same three fp32 operations per byte value, as a 256-entry table in LDS: a kernel that
// gathers from the byte frames (U8) computes on exactly the floats the reference would have uploaded, from a quarter
// of the bytes and with no host conversion.
__device__ __forceinline__ void u8_norm_table(float* lut) {
  for (int i = threadIdx.x; i < 256; i += blockDim.x) lut[i] = ((float)i / 255.0f - 0.5f) * 2.0f;
}

// U8 = false: img is the reference's float tensor [n][3][128][128]; true: byte frames [n][128][128][3]
// LP (precision NDP_ENC_BF16): the same fp32 arithmetic, the map stored as bf16 -- a.out is then a bf16 map, and a lane's
// 4 consecutive channels are one 8-byte store
template <bool U8, bool LP = false>
__global__ __launch_bounds__(kThreads) void k_enc_conv1(Conv1Args a) {
  __shared__ __attribute__((aligned(16))) float As[128 * kC1LD];     // [pixel][k]
  __shared__ __attribute__((aligned(16))) float Ws[64 * kC1LD];      // [co][k], k = ci*9 + kh*3 + kw, 27..31 zero
  __shared__ float lut[256];
  __shared__ float In[3 * 5 * kC1InLD];                               // [ci][input row][1 + 128 + 1 columns]
  if (U8) u8_norm_table(lut);                                         // (visible behind the first barrier below)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int64_t n = blockIdx.x / kC1Groups;
  const int oh_first = (int)(blockIdx.x - n * kC1Groups) * (2 * kC1Pairs);
  // weights [27][64] -> Ws[co][k]: consecutive threads read consecutive co (one 256-byte row per k); once per workgroup
  for (int i = t; i < 64 * 32; i += kThreads) {
    const int co = i & 63, k = i >> 6;
    Ws[co * kC1LD + k] = k < 27 ? a.w[k * 64 + co] : 0.f;
  }
  // Two output rows read input rows 2 oh0 - 1 .. 2 oh0 + 3: staged in LDS with coalesced loads (a row is 512 contiguous
  // bytes per channel, or 384 bytes of interleaved RGB), one zero column on either side and a zero row above the image,
  // so that the im2col gather needs no bounds checks and no scattered global loads (round 2 gathered 16 scalars per
  // thread from global memory: the kernel was its gather, 58 % of its wave-cycles parked).  A workgroup walks kC1Pairs
  // row pairs; the loads of the next pair's rows are in flight under the MFMAs and the stores of this one.
  for (int i = t; i < 3 * 5 * kC1InLD; i += kThreads) In[i] = 0.f;   // row -1 is only ever needed by the first pair
  const unsigned char* img8 = static_cast<const unsigned char*>(a.img) + (size_t)n * 3 * 128 * 128;
  const float* img = static_cast<const float*>(a.img) + (size_t)n * 3 * 128 * 128;
  // this thread's two staging slots: U8: word wv of row r; float: float4 x4 of (channel, row) cr
  int slot_r[2], slot_x[2], slot_ci[2];
  bool slot_on[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = t + u * kThreads;
    slot_on[u] = i < 480;
    if (U8) { slot_r[u] = i / 96; slot_x[u] = i - 96 * slot_r[u]; slot_ci[u] = 0; }
    else { const int cr = i >> 5; slot_x[u] = i & 31; slot_ci[u] = cr / 5; slot_r[u] = cr - 5 * slot_ci[u]; }
  }
  uint32_t w8[2] = {0u, 0u};
  f32x4 wf[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  bool have[2] = {false, false};
  auto fetch = [&](int oh0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int ih = oh0 * 2 - 1 + slot_r[u];
      have[u] = slot_on[u] && (unsigned)ih < 128u;
      if (!have[u]) continue;
      if (U8) w8[u] = *reinterpret_cast<const uint32_t*>(img8 + (size_t)ih * 384 + 4 * slot_x[u]);
      else wf[u] = *reinterpret_cast<const f32x4*>(img + ((size_t)slot_ci[u] * 128 + ih) * 128 + 4 * slot_x[u]);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!have[u]) continue;
      if (U8) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int byte_idx = 4 * slot_x[u] + e, iw = byte_idx / 3, ci = byte_idx - 3 * iw;
          In[(ci * 5 + slot_r[u]) * kC1InLD + iw + 1] = lut[(w8[u] >> (8 * e)) & 0xffu];
        }
      } else {
        float* dst = In + (slot_ci[u] * 5 + slot_r[u]) * kC1InLD + 4 * slot_x[u] + 1;
        dst[0] = wf[u][0]; dst[1] = wf[u][1]; dst[2] = wf[u][2]; dst[3] = wf[u][3];
      }
    }
  };
  fetch(oh_first);
  __syncthreads();                                                   // zeros, table
  stage();
  f32x4 bv[4];
#pragma unroll
  for (int jn = 0; jn < 4; ++jn) bv[jn] = *reinterpret_cast<const f32x4*>(a.bias + jn * 16 + 4 * q);
  for (int pair = 0; pair < kC1Pairs; ++pair) {
    const int oh0 = oh_first + 2 * pair;
    __syncthreads();                                                 // In holds this pair's rows; As is free
    {
      const int p = t >> 1, half = t & 1;                            // pixel p = (row p >> 6, column p & 63)
      const int orow = p >> 6, ow = p & 63;
      float v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k = 16 * half + j;
        const int kk = k < 27 ? k : 0;
        const int ci = kk / 9, r9 = kk - 9 * ci, kh = r9 / 3, kw = r9 - 3 * kh;
        const float x = In[(ci * 5 + 2 * orow + kh) * kC1InLD + 2 * ow + kw];   // column iw + 1 = 2 ow - 1 + kw + 1
        v[j] = k < 27 ? x : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 16; j += 4)
        *reinterpret_cast<f32x4*>(As + p * kC1LD + 16 * half + j) = f32x4{v[j], v[j + 1], v[j + 2], v[j + 3]};
    }
    if (pair + 1 < kC1Pairs) fetch(oh0 + 2);
    __syncthreads();                                                 // As complete; In is free
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jn = 0; jn < 4; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 af[2], bf[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const f32x4*>(As + (wave * 32 + i * 16 + c) * kC1LD + 16 * h + 4 * q);
#pragma unroll
      for (int jn = 0; jn < 4; ++jn) bf[jn] = *reinterpret_cast<const f32x4*>(Ws + (jn * 16 + c) * kC1LD + 16 * h + 4 * q);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int jn = 0; jn < 4; ++jn) acc[i][jn] = mfma16(bf[jn][s], af[i][s], acc[i][jn]);
    }
#pragma unroll
    for (int jn = 0; jn < 4; ++jn) {
      const int col = jn * 16 + 4 * q;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int p = wave * 32 + i * 16 + c;
        const f32x4 v = acc[i][jn] + bv[jn];
        if (LP) {
          uint16_t* dst = reinterpret_cast<uint16_t*>(a.out) + (((size_t)n * 64 + oh0 + (p >> 6)) * 64 + (p & 63)) * 64 + col;
          *reinterpret_cast<u32x2*>(dst) =
              u32x2{fm_bf16_pair(relu_keep_nan(v[0]), relu_keep_nan(v[1])), fm_bf16_pair(relu_keep_nan(v[2]), relu_keep_nan(v[3]))};
        } else {
          float* dst = a.out + (((size_t)n * 64 + oh0 + (p >> 6)) * 64 + (p & 63)) * 64 + col;
          *reinterpret_cast<f32x4*>(dst) = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
        }
      }
    }
    if (pair + 1 < kC1Pairs) stage();                                // (row 0 of In: overwritten, every later pair has ih >= 0)
  }
}

// ---------------------------------------------------------------- host side
// Packed parameter buffer (fp32), produced by ndivplanning_amd.models.image_autoencoder.pack_encoder_params:
//   conv1: w [27][64] (k = ci*9 + kh*3 + kw), bias [64]
//   conv l = 2..6: w [Cout][KH][KW][Cin], bias [Cout]        (BatchNorm of conv1..3 folded into w and bias)
struct EncLayer { int cin, cout, hin, hout, ksz, stride, pad; };
static const EncLayer kEnc[6] = {
    {3, 64, 128, 64, 3, 2, 1},   {64, 128, 64, 32, 3, 2, 1},    {128, 256, 32, 16, 3, 2, 1},
    {256, 512, 16, 8, 3, 2, 1},  {512, 1024, 8, 4, 3, 2, 1},    {1024, 128, 4, 1, 4, 1, 0}};
constexpr int kEncChunk = 512;          // images per pass (activations of a pass: 0.5 M floats = 2 MB per image)
constexpr int kEncPartBlocks = 1024;    // split-K partial sums: at most this many 128 x 128 output tiles in flight

static int64_t enc_w_floats(int l) { return (int64_t)kEnc[l].cout * kEnc[l].ksz * kEnc[l].ksz * kEnc[l].cin; }
static int64_t enc_param_offset(int l, bool bias) {
  int64_t o = 0;
  for (int i = 0; i < l; ++i) o += enc_w_floats(i) + kEnc[i].cout;
  return o + (bias ? enc_w_floats(l) : 0);
}
static int64_t enc_act_floats(int l) { return (int64_t)kEnc[l].hout * kEnc[l].hout * kEnc[l].cout; }   // per image
static int64_t enc_ws_floats(int64_t n) {
  const int64_t c = n < kEncChunk ? n : kEncChunk;
  int64_t per = 0;
  for (int l = 0; l < 5; ++l) per += enc_act_floats(l);
  return c * per + (int64_t)kEncPartBlocks * kEncBM * kEncBN;
}

// K split of layer l for n images: the deep layers have few output tiles when n is small (conv5: 8 per 8 images);
// the smallest divisor d of K / 32 that gives >= 512 workgroups (2 per CU), with tiles * d <= kEncPartBlocks
// (bk: the K step of the kernel that runs the layer -- k_conv_gemm's kEncBK is a build option, NDP_ENC_BK, and may differ
// from k_conv_gemm_bf16's 32: a split must be whole steps of the kernel it is for)
static int enc_split(int l, int64_t n, int bk = kEncBK) {
  const EncLayer& L = kEnc[l];
  const int64_t m = n * L.hout * L.hout;
  const int64_t tiles = ((m + kEncBM - 1) / kEncBM) * (L.cout / kEncBN);
  const int steps = L.ksz * L.ksz * L.cin / bk;
  int best = 1;
  for (int d = 1; d <= steps && d <= 128; ++d) {
    if (steps % d != 0 || tiles * d > kEncPartBlocks) continue;
    best = d;
    if (tiles * d >= 512) break;
  }
  return best;
}

static std::once_flag g_enc_attr_once[kMaxDevices];

// layer l of n images as a GEMM launch: the geometry, the bias, the K split (the operands and the output: the caller's)
static ConvGemmArgs conv_gemm_args(int l, const float* params, int64_t n, int nsplit) {
  const EncLayer& L = kEnc[l];
  ConvGemmArgs a;
  a.in = nullptr; a.w = nullptr; a.bias = params + enc_param_offset(l, true); a.out = nullptr;
  a.H = a.W = L.hin; a.Cin = L.cin; a.OH = a.OW = L.hout; a.Cout = L.cout;
  a.KW = L.ksz; a.stride = L.stride; a.pad = L.pad;
  a.M = (int)(n * L.hout * L.hout); a.K = L.ksz * L.ksz * L.cin;
  a.relu = l < 5 ? 1 : 0;
  a.nsplit = nsplit; a.k_per_split = a.K / nsplit;
  a.mtiles = (a.M + kEncBM - 1) / kEncBM; a.ntiles = L.cout / kEncBN;
  return a;
}
static dim3 conv_gemm_grid(const ConvGemmArgs& a) {
  return dim3((unsigned)(a.mtiles >= 8 ? 8 * ((a.mtiles + 7) / 8) * a.ntiles : a.mtiles * a.ntiles), (unsigned)a.nsplit);
}

static int launch_conv_gemm(int l, const float* in, const float* params, float* out, int64_t n, float* part, hipStream_t st) {
  const int nsplit = enc_split(l, n);
  float* final_out = out;
  if (nsplit > 1) out = part;
  std::call_once(device_once(g_enc_attr_once), [] { allow_lds(k_conv_gemm, conv_gemm_lds_floats() * 4); });
  ConvGemmArgs a = conv_gemm_args(l, params, n, nsplit);
  a.in = in; a.w = params + enc_param_offset(l, false); a.out = out;
  const dim3 grid = conv_gemm_grid(a);
  KTimer kt(l == 5 ? "k_conv_gemm[6]" : (l == 1 ? "k_conv_gemm[2]" : (l == 2 ? "k_conv_gemm[3]" : (l == 3 ? "k_conv_gemm[4]" : "k_conv_gemm[5]"))), st);
  hipLaunchKernelGGL(k_conv_gemm, grid, dim3(kThreads), conv_gemm_lds_floats() * 4, st, a);
  int rc = check_launch("k_conv_gemm");
  if (rc || nsplit == 1) return rc;
  const int64_t mc = (int64_t)a.M * a.Cout;
  KTimer kt2("k_splitk_reduce", st);
  hipLaunchKernelGGL(k_splitk_reduce, dim3((unsigned)((mc + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     part, nsplit, mc, a.bias, a.Cout, a.relu, final_out);
  return check_launch("k_splitk_reduce");
}

// ---- precision NDP_ENC_BF16
static std::once_flag g_enc_lp_attr_once[kMaxDevices];
static const char* const kEncLpLabel[6] = {"k_enc_conv1_bf16", "k_conv_gemm_bf16[2]", "k_conv_gemm_bf16[3]", "k_conv_gemm_bf16[4]",
                                           "k_conv_gemm_bf16[5]", "k_conv_gemm_bf16[6]"};
static int64_t enc_lp_w_offset(int l) {        // conv l + 1's bf16 weights (l = 1..5; 6: the end), in bf16 elements
  int64_t o = 0;
  for (int i = 1; i < l; ++i) o += enc_w_floats(i);
  return o;
}
static int64_t enc_lp_act_offset(int l, int64_t n) {   // map l (0..4; 5: the end) of a pass of n images, in bf16 elements
  int64_t o = 0;
  for (int i = 0; i < l; ++i) o += n * enc_act_floats(i);
  return o;
}

// layer l = 1..5 with bf16 operands: `in` the bf16 map of layer l - 1, `out` a bf16 map (l < 5) or the fp32 codes (l == 5)
static int launch_conv_gemm_bf16(int l, const uint16_t* in, const float* params, const uint16_t* lp, void* out, int64_t n,
                                 float* part, hipStream_t st) {
  const int nsplit = enc_split(l, n, kEncLpBK);
  std::call_once(device_once(g_enc_lp_attr_once), [] {
    allow_lds(k_conv_gemm_bf16<true>, conv_gemm_bf16_lds_bytes());
    allow_lds(k_conv_gemm_bf16<false>, conv_gemm_bf16_lds_bytes());
  });
  ConvGemmArgs a = conv_gemm_args(l, params, n, nsplit);
  a.in = reinterpret_cast<const float*>(in); a.w = reinterpret_cast<const float*>(lp + enc_lp_w_offset(l));
  a.out = nsplit > 1 ? part : static_cast<float*>(out);
  {
    KTimer kt(kEncLpLabel[l], st);
    if (l < 5) hipLaunchKernelGGL(k_conv_gemm_bf16<true>, conv_gemm_grid(a), dim3(kThreads), conv_gemm_bf16_lds_bytes(), st, a);
    else hipLaunchKernelGGL(k_conv_gemm_bf16<false>, conv_gemm_grid(a), dim3(kThreads), conv_gemm_bf16_lds_bytes(), st, a);
  }
  int rc = check_launch("k_conv_gemm_bf16");
  if (rc || nsplit == 1) return rc;
  const int64_t mc = (int64_t)a.M * a.Cout;
  if (l < 5) {
    KTimer kt2("k_splitk_reduce_bf16", st);
    hipLaunchKernelGGL(k_splitk_reduce_bf16, dim3((unsigned)((mc + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       part, nsplit, mc, a.bias, a.Cout, a.relu, static_cast<__bf16*>(out));
    return check_launch("k_splitk_reduce_bf16");
  }
  KTimer kt2("k_splitk_reduce", st);
  hipLaunchKernelGGL(k_splitk_reduce, dim3((unsigned)((mc + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     part, nsplit, mc, a.bias, a.Cout, a.relu, static_cast<float*>(out));
  return check_launch("k_splitk_reduce");
}

static int enc_pack_lp(const float* params, uint16_t* lp, hipStream_t st) {
  PackLpArgs a;
  memset(&a, 0, sizeof(a));
  a.dst = lp;
  for (int l = 1; l < 6; ++l) {
    const int i = a.nseg++;
    a.src[i] = params + enc_param_offset(l, false);
    a.dst_off[i] = enc_lp_w_offset(l); a.count[i] = enc_w_floats(l);
    a.block_begin[i + 1] = a.block_begin[i] + (int)((a.count[i] + 4095) / 4096);
  }
  KTimer kt("k_enc_pack_lp", st);
  hipLaunchKernelGGL(k_enc_pack_lp, dim3((unsigned)a.block_begin[a.nseg]), dim3(kThreads), 0, st, a);
  return check_launch("k_enc_pack_lp");
}

}  // namespace ndp

extern "C" {

int64_t ndp_encoder_param_floats(void) { return ndp::enc_param_offset(6, false); }

int64_t ndp_encoder_workspace_floats(int64_t n_images) { return n_images < 1 ? 0 : ndp::enc_ws_floats(n_images); }

// lp: the bf16 weights of ndp_encoder_pack_params_lp -> a NDP_ENC_BF16 pass (bf16 maps at the head of the workspace, the
// fp32 partial sums behind them); null: the fp32 pass
static int encoder_forward_any(const float* packed_params, const void* images, bool u8, int64_t n_images, float* codes,
                               float* workspace, void* stream, const uint16_t* lp = nullptr) {
  using namespace ndp;
  hipStream_t st = (hipStream_t)stream;
  for (int64_t n0 = 0; n0 < n_images; n0 += kEncChunk) {
    const int64_t n = n_images - n0 < kEncChunk ? n_images - n0 : kEncChunk;
    if (lp != nullptr) {
      uint16_t* maps = reinterpret_cast<uint16_t*>(workspace);
      float* part = reinterpret_cast<float*>(maps + enc_lp_act_offset(5, n));
      const size_t first = (size_t)n0 * 3 * 128 * 128;
      Conv1Args c1{u8 ? (const void*)(static_cast<const unsigned char*>(images) + first)
                      : (const void*)(static_cast<const float*>(images) + first),
                   packed_params + enc_param_offset(0, false), packed_params + enc_param_offset(0, true),
                   reinterpret_cast<float*>(maps), n};
      {
        KTimer kt(kEncLpLabel[0], st);
        if (u8) hipLaunchKernelGGL((k_enc_conv1<true, true>), dim3((unsigned)(n * kC1Groups)), dim3(kThreads), 0, st, c1);
        else hipLaunchKernelGGL((k_enc_conv1<false, true>), dim3((unsigned)(n * kC1Groups)), dim3(kThreads), 0, st, c1);
      }
      int rc = check_launch("k_enc_conv1_bf16");
      if (rc) return rc;
      for (int l = 1; l < 6; ++l) {
        void* out = l < 5 ? (void*)(maps + enc_lp_act_offset(l, n)) : (void*)(codes + n0 * 128);
        rc = launch_conv_gemm_bf16(l, maps + enc_lp_act_offset(l - 1, n), packed_params, lp, out, n, part, st);
        if (rc) return rc;
      }
      continue;
    }
    float* act[5];
    float* p = workspace;
    for (int l = 0; l < 5; ++l) { act[l] = p; p += n * enc_act_floats(l); }
    float* part = p;
    {
      const size_t first = (size_t)n0 * 3 * 128 * 128;
      Conv1Args c1{u8 ? (const void*)(static_cast<const unsigned char*>(images) + first)
                      : (const void*)(static_cast<const float*>(images) + first),
                   packed_params + enc_param_offset(0, false), packed_params + enc_param_offset(0, true), act[0], n};
      KTimer kt("k_enc_conv1", st);
      if (u8) hipLaunchKernelGGL(k_enc_conv1<true>, dim3((unsigned)(n * kC1Groups)), dim3(kThreads), 0, st, c1);
      else hipLaunchKernelGGL(k_enc_conv1<false>, dim3((unsigned)(n * kC1Groups)), dim3(kThreads), 0, st, c1);
      int rc = check_launch("k_enc_conv1");
      if (rc) return rc;
    }
    for (int l = 1; l < 6; ++l) {
      int rc = launch_conv_gemm(l, act[l - 1], packed_params, l < 5 ? act[l] : codes + n0 * 128, n, part, st);
      if (rc) return rc;
    }
  }
  return NDP_OK;
}

int ndp_encoder_forward(const float* packed_params, const float* images, int64_t n_images, float* codes,
                        float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(packed_params && images && codes && workspace && n_images >= 1, "ndp_encoder_forward: bad arguments");
  NDP_CHECK_ARG(aligned16(packed_params) && aligned16(images) && aligned16(codes) && aligned16(workspace),
                "ndp_encoder_forward: buffers must be 16-byte aligned");
  return encoder_forward_any(packed_params, images, false, n_images, codes, workspace, stream);
}

int ndp_encoder_forward_u8(const float* packed_params, const uint8_t* frames_hwc, int64_t n_images, float* codes,
                           float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(packed_params && frames_hwc && codes && workspace && n_images >= 1, "ndp_encoder_forward_u8: bad arguments");
  NDP_CHECK_ARG(aligned16(packed_params) && aligned16(codes) && aligned16(workspace),
                "ndp_encoder_forward_u8: buffers must be 16-byte aligned");
  return encoder_forward_any(packed_params, frames_hwc, true, n_images, codes, workspace, stream);
}

int64_t ndp_encoder_lp_weight_bytes(void) { return 2 * ndp::enc_lp_w_offset(6); }

int64_t ndp_encoder_lp_act_offset(int layer, int64_t n_images) {
  if (layer < 0 || layer > 4 || n_images < 1) return -1;
  return ndp::enc_lp_act_offset(layer, n_images < ndp::kEncChunk ? n_images : ndp::kEncChunk);
}

int ndp_encoder_pack_params_lp(const float* packed_params, void* lp_weights, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(packed_params && lp_weights, "ndp_encoder_pack_params_lp: bad arguments");
  NDP_CHECK_ARG(aligned16(packed_params) && aligned16(lp_weights), "ndp_encoder_pack_params_lp: buffers must be 16-byte aligned");
  return enc_pack_lp(packed_params, static_cast<uint16_t*>(lp_weights), (hipStream_t)stream);
}

int ndp_encoder_forward_lp(const float* packed_params, const float* images, const uint8_t* frames_hwc, int64_t n_images,
                           int precision, const void* lp_weights, float* codes, float* workspace, void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(precision == NDP_ENC_FP32 || precision == NDP_ENC_BF16, "ndp_encoder_forward_lp: precision %d is neither "
                "NDP_ENC_FP32 nor NDP_ENC_BF16", precision);
  NDP_CHECK_ARG((images != nullptr) != (frames_hwc != nullptr), "ndp_encoder_forward_lp: exactly one of images and frames_hwc");
  NDP_CHECK_ARG(packed_params && codes && workspace && n_images >= 1, "ndp_encoder_forward_lp: bad arguments");
  NDP_CHECK_ARG(aligned16(packed_params) && aligned16(codes) && aligned16(workspace) && (images == nullptr || aligned16(images)),
                "ndp_encoder_forward_lp: buffers must be 16-byte aligned");
  NDP_CHECK_ARG(precision == NDP_ENC_FP32 || (lp_weights != nullptr && aligned16(lp_weights)),
                "ndp_encoder_forward_lp: NDP_ENC_BF16 needs the 16-byte aligned bf16 weights of ndp_encoder_pack_params_lp");
  const bool u8 = frames_hwc != nullptr;
  return encoder_forward_any(packed_params, u8 ? (const void*)frames_hwc : (const void*)images, u8, n_images, codes, workspace,
                             stream, precision == NDP_ENC_BF16 ? static_cast<const uint16_t*>(lp_weights) : nullptr);
}

}  // extern "C"
