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
// storing its map as bf16 and conv2..6 through k_conv_gemm's bf16 operand path (EncBf16; the paths are described in
// ndp_device.h) -- bf16 maps and bf16 weights straight into the bf16 MFMA, fp32 accumulation, fp32 partial sums and codes:
// out = act(bias + sum bf16(x) . bf16(w)), where the bf16 map is what its producer stored (the rounding of this layer's
// operand, done once) and the weights are the k_pack_lp copy.  A 32-wide K chunk of an im2col row is then 64 contiguous
// bytes, 16 bytes per thread and load.

namespace ndp {

// (a K step of 64 was measured for the bf16 path and lost at small n: DESIGN 5t)
constexpr int kEncBM = 128, kEncBN = 128, kEncBK = 32, kEncLD = kEncBK + 4;
using EncF32 = PathF32<kEncLD>;
using EncBf16 = PathEncBf16;

struct ConvGemmArgs {
  const void* in;         // NHWC [n][H][W][Cin], P::A::elem of the launched path P
  const void* w;          // [Cout][K], k = (kh*KW + kw)*Cin + ci  (BatchNorm folded in), P::B::elem
  const float* bias;      // [Cout] (BatchNorm folded in); ignored when nsplit > 1
  void* out;              // NHWC [M][Cout], bf16 with OUT_LP, else fp32; nsplit > 1: fp32 partial sums [split][M][Cout]
  int H, W, Cin, OH, OW, Cout;
  int KW, stride, pad;
  int M, K;
  int relu;
  int nsplit, k_per_split;
  int mtiles, ntiles;
};

// ReLU of the bf16 pass: a NaN stays a NaN, as the definition's torch.relu has it (fmaxf(NaN, 0) is 0: the fp32 pass,
// whose bits are pinned, drops a NaN at its first ReLU)
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

// The bf16 instantiations differ from the fp32 one outside the operand path, deliberately, in this: their ReLU keeps a NaN
// (relu_keep_nan; the fp32 one is fmaxf), and with OUT_LP the finished map is stored as bf16 (conv2..conv5; 8 bytes per lane
// and tile) -- conv6 stores fp32 codes, and the partial sums of a split layer are fp32 either way.
template <class P, bool OUT_LP>
__global__ __launch_bounds__(kThreads, 2) void k_conv_gemm(ConvGemmArgs a) {
  using SA = typename P::A; using SB = typename P::B; using Mma = typename P::Mma;
  static_assert(P::kLp || !OUT_LP, "k_conv_gemm: bf16 maps come from the bf16 pass");
  constexpr int BM = kEncBM, BN = kEncBN, BK = kEncBK, LD = Mma::LD, V = P::V;
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

  // global -> LDS assignment: NU rows (r0 + RPP u) x one quad of V values (kq) of each operand per thread and step
  constexpr int QPR = BK / V, RPP = kThreads / QPR, NU = BM / RPP;   // quads per row, rows per pass, passes
  const int r0 = t / QPR, kq = t % QPR;
  const typename SA::elem* a_img[NU];
  int a_ih0[NU], a_iw0[NU], a_base[NU];
  const typename SB::elem* b_row[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    int m = m_tile * BM + r0 + RPP * u;
    const bool valid = m < a.M;
    m = valid ? m : a.M - 1;
    const int n = m / (a.OH * a.OW), rem = m - n * (a.OH * a.OW);
    const int oh = rem / a.OW, ow = rem - oh * a.OW;
    a_img[u] = static_cast<const typename SA::elem*>(a.in) + (size_t)n * a.H * a.W * a.Cin + V * kq;
    a_ih0[u] = valid ? oh * a.stride - a.pad : -(1 << 20);       // rows past M: every tap out of bounds -> zeros
    a_iw0[u] = ow * a.stride - a.pad;
    a_base[u] = ((oh * a.stride - a.pad) * a.W + a_iw0[u]) * a.Cin;   // + tap offset = element offset in the image
    b_row[u] = static_cast<const typename SB::elem*>(a.w) + (size_t)(n_tile * BN + r0 + RPP * u) * a.K + V * kq;
  }
  typename SA::reg ra[NU];
  typename SB::reg rb[NU];
  bool ra_ok[NU];          // padding taps: zeroed where the quad is written to LDS (the Stages of ndp_device.h)
  auto fetch = [&](int k0) {
    const int tap = k0 / a.Cin, ci0 = k0 - tap * a.Cin;          // uniform: one tap, 32 consecutive channels
    const int kh = tap / a.KW, kw = tap - kh * a.KW;
    const int tapoff = (kh * a.W + kw) * a.Cin + ci0;            // uniform
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const bool ok = (unsigned)(a_ih0[u] + kh) < (unsigned)a.H && (unsigned)(a_iw0[u] + kw) < (unsigned)a.W;
      ra[u] = SA::load(a_img[u] + (ok ? a_base[u] + tapoff : 0));   // unconditional load from a valid address
      ra_ok[u] = ok;
      rb[u] = SB::load(b_row[u] + k0);
    }
    pin_vmem();
  };
  auto stage = [&](int buf) {
    typename P::lds* As = Mma::tiles() + buf * (BM + BN) * LD;
    typename P::lds* Bs = As + BM * LD;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      *reinterpret_cast<typename SA::quad*>(As + (r0 + RPP * u) * LD + V * kq) = SA::staged(ra[u], ra_ok[u]);
      *reinterpret_cast<typename SB::quad*>(Bs + (r0 + RPP * u) * LD + V * kq) = SB::staged(rb[u]);
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
    const typename P::lds* As = Mma::tiles() + buf * (BM + BN) * LD + (wm * 64 + c) * LD + Mma::KQ * q;
    const typename P::lds* Bs = Mma::tiles() + buf * (BM + BN) * LD + BM * LD + (wn * 64 + c) * LD + Mma::KQ * q;
    typename Mma::frag af[4], bf[4];                               // all parts of the step up front
#pragma unroll
    for (int h = 0; h < Mma::PARTS; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Mma::read(af[i], As + i * 16 * LD, h);
        Mma::read(bf[i], Bs + i * 16 * LD, h);
      }
#pragma unroll
    for (int ks = 0; ks < Mma::KSUB; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) acc[i][jn] = Mma::mma(bf[jn], af[i], acc[i][jn], ks);   // C^T tile: see epilogue
    pin_vmem();
    if (more) stage(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // epilogue: the MFMAs computed the TRANSPOSED 16 x 16 tiles (weights as the A operand), so a lane holds output
  // row (pixel) c and 4 consecutive channels 4q..4q+3 of each tile: one 16-byte store per tile
  float* out = static_cast<float*>(a.out) + (a.nsplit > 1 ? (size_t)split * a.M * a.Cout : 0);
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
        if (a.relu && fin) {
          if constexpr (P::kLp) v = f32x4{relu_keep_nan(v[0]), relu_keep_nan(v[1]), relu_keep_nan(v[2]), relu_keep_nan(v[3])};
          else v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
        }
        const size_t at = (size_t)m * a.Cout + col;
        if (OUT_LP && fin) *reinterpret_cast<u32x2*>(static_cast<uint16_t*>(a.out) + at) = u32x2{fm_bf16_pair(v[0], v[1]), fm_bf16_pair(v[2], v[3])};
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
// OUT = float: conv6's codes, and every split layer of the fp32 pass; OUT = __bf16: the finished map of a split layer of a
// NDP_ENC_BF16 pass.  Each output type keeps its ReLU (see relu_keep_nan).
template <class OUT>
__global__ __launch_bounds__(kThreads) void k_splitk_reduce(const float* part, int nsplit, int64_t mc, const float* bias,
                                                            int cout, int relu, OUT* out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= mc) return;
  const float s = splitk_sum(part, nsplit, mc, bias, cout, i);
  if constexpr (sizeof(OUT) == sizeof(float)) out[i] = relu ? fmaxf(s, 0.f) : s;
  else out[i] = (OUT)(relu ? relu_keep_nan(s) : s);
}

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
// (a split is whole K steps of k_conv_gemm: 32 in both precisions)
static int enc_split(int l, int64_t n) {
  const EncLayer& L = kEnc[l];
  const int64_t m = n * L.hout * L.hout;
  const int64_t tiles = ((m + kEncBM - 1) / kEncBM) * (L.cout / kEncBN);
  const int steps = L.ksz * L.ksz * L.cin / kEncBK;
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

// ---- precision NDP_ENC_BF16
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

// layer l = 1..5: split, launch, reduce.  lp == null, the fp32 pass: `in` and `out` are fp32 maps (l == 5: the codes) and the
// weights come from `params`.  lp != null, NDP_ENC_BF16: `in` is the bf16 map of layer l - 1, the weights are lp's, `out` is
// a bf16 map (l < 5) or the fp32 codes (l == 5).  Partial sums of a split layer are fp32 in `part` either way.
static int launch_conv_gemm(int l, const void* in, const float* params, const uint16_t* lp, void* out, int64_t n, float* part,
                            hipStream_t st) {
  static const char* const kEncLabel[6] = {"k_enc_conv1", "k_conv_gemm[2]", "k_conv_gemm[3]", "k_conv_gemm[4]", "k_conv_gemm[5]",
                                           "k_conv_gemm[6]"};
  const int nsplit = enc_split(l, n);
  const bool out_lp = lp != nullptr && l < 5;
  std::call_once(device_once(g_enc_attr_once), [] {
    allow_lds((k_conv_gemm<EncF32, false>), EncF32::lds_bytes(kEncBM + kEncBN));
    allow_lds((k_conv_gemm<EncBf16, true>), EncBf16::lds_bytes(kEncBM + kEncBN));
    allow_lds((k_conv_gemm<EncBf16, false>), EncBf16::lds_bytes(kEncBM + kEncBN));
  });
  ConvGemmArgs a = conv_gemm_args(l, params, n, nsplit);
  a.in = in; a.out = nsplit > 1 ? part : out;
  if (lp != nullptr) a.w = lp + enc_lp_w_offset(l);
  else a.w = params + enc_param_offset(l, false);
  const dim3 grid = conv_gemm_grid(a);
  {
    KTimer kt(lp != nullptr ? kEncLpLabel[l] : kEncLabel[l], st);
    if (lp == nullptr) hipLaunchKernelGGL((k_conv_gemm<EncF32, false>), grid, dim3(kThreads), EncF32::lds_bytes(kEncBM + kEncBN), st, a);
    else if (out_lp) hipLaunchKernelGGL((k_conv_gemm<EncBf16, true>), grid, dim3(kThreads), EncBf16::lds_bytes(kEncBM + kEncBN), st, a);
    else hipLaunchKernelGGL((k_conv_gemm<EncBf16, false>), grid, dim3(kThreads), EncBf16::lds_bytes(kEncBM + kEncBN), st, a);
  }
  int rc = check_launch(lp != nullptr ? "k_conv_gemm_bf16" : "k_conv_gemm");
  if (rc || nsplit == 1) return rc;
  const int64_t mc = (int64_t)a.M * a.Cout;
  const dim3 rgrid((unsigned)((mc + kThreads - 1) / kThreads));
  const char* rlabel = out_lp ? "k_splitk_reduce_bf16" : "k_splitk_reduce";
  KTimer kt2(rlabel, st);
  if (out_lp) hipLaunchKernelGGL(k_splitk_reduce<__bf16>, rgrid, dim3(kThreads), 0, st, part, nsplit, mc, a.bias, a.Cout, a.relu, static_cast<__bf16*>(out));
  else hipLaunchKernelGGL(k_splitk_reduce<float>, rgrid, dim3(kThreads), 0, st, part, nsplit, mc, a.bias, a.Cout, a.relu, static_cast<float*>(out));
  return check_launch(rlabel);
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
  hipLaunchKernelGGL(k_pack_lp, dim3((unsigned)a.block_begin[a.nseg]), dim3(kThreads), 0, st, a);
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
        rc = launch_conv_gemm(l, maps + enc_lp_act_offset(l - 1, n), packed_params, lp, out, n, part, st);
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
      int rc = launch_conv_gemm(l, act[l - 1], packed_params, nullptr, l < 5 ? act[l] : codes + n0 * 128, n, part, st);
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
