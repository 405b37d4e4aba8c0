// ndp_resize.inc -- camera frames [n][H][W][3] bytes -> [n][128][128][3] bytes, bit-identical to Pillow's
// `Image.resize((128, 128), Image.LANCZOS)` on an 8-bit RGB image (MPC_gym_eval.py:68-77 and
// generate_trajectories.py:113-118 of the reference; Pillow's ImagingResample).  DESIGN.md section 5h.
//
// Pillow's 8-bit resampler is integer arithmetic on a table of fixed-point coefficients (22 fractional bits) that is
// computed in double: the table is built on the host by build_axis (plain C++, what tests/resize_host_driver.hip runs
// under the sanitizers), the kernel does only the integer part.  Two separable passes, horizontal first, each rounded
// to bytes; a pass whose input and output sizes agree is skipped.
//
//   k_resize_lanczos   one launch.  A workgroup takes (image, band of rb output rows): the vertical bounds of the
//                      band's first and last row give the input rows it needs; each of its four waves brings one input
//                      row at a time into LDS with dword loads and filters it horizontally into the band's byte tile
//                      [rows][384]; then the vertical pass runs out of that tile, four bytes per thread, and a finished
//                      row leaves as 96 dwords.  Optionally the normalised floats [n][3][128][128] of the same bytes
//                      (u8_norm_table: what k_eval_frames_u8 makes of them) are written by the same launch.
// Integer arithmetic and no atomics: every run gives the same bits, whatever rb.  Included at the end of
// ndp_kernels.hip, after ndp_jpeg.inc.

namespace ndp {
namespace resize {

constexpr int kOut = 128;                        // output rows and columns
constexpr int kRowBytes = kOut * 3;              // one output (or horizontally filtered) row
constexpr int kMaxIn = 2048;                     // largest input height / width
constexpr int kMaxImages = 65536;
constexpr int kPrecBits = 22;                    // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int32_t kHalf = 1 << (kPrecBits - 1);
constexpr int kRsThreads = 256;
constexpr int kRsWaves = kRsThreads / 64;
constexpr int kHdrInts = 8;                      // magic, H, W, kx, ky, 0, 0, 0
constexpr int32_t kMagic = 0x525a4c33;
constexpr int kLdsBudget = 64 * 1024;            // dynamic LDS that needs no opt-in
constexpr int kLutBytes = 256 * 4;

// The tables of one (H, W): int32 hdr[8] | xb[128][2] | yb[128][2] | kx[128][ksize_x] | ky[128][ksize_y]
// (bounds: first input sample and tap count of every output sample; coefficients: fixed point, zero past the count).
struct Plan {
  int h, w, kx, ky;
  int64_t xb, yb, kxc, kyc, ints;                // offsets in int32
};

__host__ __device__ inline double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * 3.14159265358979323846;
  return sin(x) / x;
}

__host__ __device__ inline double lanczos_filter(double x) {
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}

__host__ __device__ inline int axis_ksize(int in) {
  const double scale = (double)in / (double)kOut;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(3.0 * filterscale) * 2 + 1;
}

__host__ __device__ inline bool make_plan(int64_t h, int64_t w, Plan* p) {
  if (h < 1 || h > kMaxIn || w < 1 || w > kMaxIn) return false;
  p->h = (int)h;
  p->w = (int)w;
  p->kx = axis_ksize((int)w);
  p->ky = axis_ksize((int)h);
  p->xb = kHdrInts;
  p->yb = p->xb + 2 * kOut;
  p->kxc = p->yb + 2 * kOut;
  p->kyc = p->kxc + (int64_t)kOut * p->kx;
  p->ints = p->kyc + (int64_t)kOut * p->ky;
  return true;
}

// First input sample and tap count of output sample xx (Pillow's precompute_coeffs).
__host__ __device__ inline void axis_bounds(int in, int xx, int* xmin, int* n) {
  const double scale = (double)in / (double)kOut;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 3.0 * filterscale;
  const double center = (xx + 0.5) * scale;
  int lo = (int)(center - support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + support + 0.5);
  if (hi > in) hi = in;
  *xmin = lo;
  *n = hi - lo;
}

// One axis: bounds [128][2] and coefficients [128][ksize].  `w` is scratch of ksize doubles.  Returns the largest
// magnitude an accumulator can reach over the axis' rows (kHalf + 255 * the larger of the positive and the negative
// coefficient sums): below 2^31 for every valid table.
__host__ __device__ inline int64_t build_axis(int in, int ksize, int32_t* bounds, int32_t* coefs, double* w) {
  const double scale = (double)in / (double)kOut;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double ss = 1.0 / filterscale;
  int64_t worst = 0;
  for (int xx = 0; xx < kOut; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin, n;
    axis_bounds(in, xx, &xmin, &n);
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = lanczos_filter((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    int64_t pos = 0, neg = 0;
    for (int x = 0; x < ksize; ++x) {
      int32_t k = 0;
      if (x < n) {
        double v = w[x];
        if (ww != 0.0) v /= ww;
        k = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << kPrecBits)) : (int32_t)(0.5 + v * (double)(1 << kPrecBits));
      }
      coefs[(int64_t)xx * ksize + x] = k;
      if (k > 0) pos += k; else neg -= k;
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
    const int64_t m = (int64_t)kHalf + 255 * (pos > neg ? pos : neg);
    if (m > worst) worst = m;
  }
  return worst;
}

// The tables of plan p into t (p.ints int32).  Returns build_axis' bound over both axes.
__host__ __device__ inline int64_t build_tables(const Plan& p, int32_t* t, double* scratch) {
  t[0] = kMagic; t[1] = p.h; t[2] = p.w; t[3] = p.kx; t[4] = p.ky; t[5] = t[6] = t[7] = 0;
  const int64_t a = build_axis(p.w, p.kx, t + p.xb, t + p.kxc, scratch);
  const int64_t b = build_axis(p.h, p.ky, t + p.yb, t + p.kyc, scratch);
  return a > b ? a : b;
}

__host__ __device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// clip8(acc >> 22) with an arithmetic shift (acc starts at kHalf), written as the clamp of acc to [0, 2^30 - 1] followed
// by the shift, which is the same number.  In the shift-then-clamp form the compiler packs two of the vertical pass's
// four results with v_ashr_pk_u8_i32 and ORs the other two into that register's upper half as if it were zero; on an
// MI355X bytes 2 and 3 of every output dword then came out with stray bits (DESIGN.md section 5h).
__host__ __device__ inline uint32_t finish(int32_t acc) {
  return (uint32_t)clampi(acc, 0, (256 << kPrecBits) - 1) >> kPrecBits;
}

// One output sample: n taps, `stride` bytes apart.
__host__ __device__ inline uint8_t sample(const uint8_t* p, int stride, const int32_t* k, int n) {
  int32_t acc = kHalf;
  for (int x = 0; x < n; ++x) acc += (int32_t)p[x * stride] * k[x];
  return (uint8_t)finish(acc);
}

// Bounds of one output sample as the kernel uses them: whatever the table holds, the taps stay inside [0, in) and
// inside the table's row.
__host__ __device__ inline void safe_bounds(const int32_t* b, int xx, int in, int ksize, int* xmin, int* n) {
  const int lo = clampi(b[2 * xx], 0, in);
  *xmin = lo;
  *n = clampi(b[2 * xx + 1], 0, ksize < in - lo ? ksize : in - lo);
}

// Input rows [r0, r1) that the band of output rows y0 .. y0 + rb - 1 reads.
__host__ __device__ inline void band_rows(const int32_t* yb, int y0, int rb, int h, int ky, bool vpass, int* r0, int* r1) {
  if (!vpass) { *r0 = y0; *r1 = y0 + rb; return; }
  int lo, n, lo2, n2;
  safe_bounds(yb, y0, h, ky, &lo, &n);
  safe_bounds(yb, y0 + rb - 1, h, ky, &lo2, &n2);
  *r0 = lo;
  *r1 = lo2 + n2 > lo ? lo2 + n2 : lo;
}

__host__ __device__ inline int raw_stride(int w) { return (w * 3 + 6 + 15) / 16 * 16; }

// Dynamic LDS of a launch: the table of floats, the band's output rows, its tile, one raw input row per wave.
__host__ __device__ inline int lds_bytes(int rb, int tile_rows, int w) {
  return kLutBytes + rb * kRowBytes + tile_rows * kRowBytes + (w != kOut ? kRsWaves * raw_stride(w) : 0);
}

// Host: the tallest tile over the bands of rb rows (from the bounds alone, no table needed).
inline int tile_rows_for(int h, int rb) {
  if (h == kOut) return rb;
  int worst = 0;
  for (int y0 = 0; y0 < kOut; y0 += rb) {
    int lo, n, lo2, n2;
    axis_bounds(h, y0, &lo, &n);
    axis_bounds(h, y0 + rb - 1, &lo2, &n2);
    const int rows = lo2 + n2 - lo;
    if (rows > worst) worst = rows;
  }
  return worst;
}

// Host: rows per band.  Few images: short bands, so that there are workgroups for every CU; many images: tall bands,
// which repeat less of the horizontal pass (a band of rb rows reads about ksize + scale * (rb - 1) input rows).
// PROVISIONAL: the thresholds below are reasoned from the workgroup count against the chip's 256 CUs, not picked from
// timings; scripts/bench_resize.py times every split at n = 1 and n = 64 (rows_per_band overrides this choice).
inline int choose_rb(int64_t n, int h, int w) {
  int rb = n >= 32 ? 8 : (n >= 16 ? 4 : (n >= 8 ? 2 : 1));
  while (rb > 1 && lds_bytes(rb, tile_rows_for(h, rb), w) > kLdsBudget) rb >>= 1;
  return rb;
}

struct Args {
  const uint8_t* frames;
  const int32_t* tab;
  uint8_t* out;
  float* outf;                                   // NULL, or [n][3][128][128]
  int64_t n;
  int h, w, kx, ky, rb, tile_rows, raw_stride;
};

}  // namespace resize

// Row `p` (row_bytes bytes, at byte offset `mis` from a dword boundary) into dst as whole dwords, so that the row's byte
// i lands at dst[mis + i].  A dword that lies inside the row is one load; the first and the last are put together from
// the bytes that belong to the row.
__device__ __forceinline__ void resize_load_row(const uint8_t* p, int mis, int row_bytes, uint8_t* dst, int lane) {
  const uint8_t* base = p - mis;
  const int end = mis + row_bytes;
  const int ndw = (end + 3) >> 2;
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  for (int i = lane; i < ndw; i += 64) {
    const int b0 = 4 * i;
    uint32_t v;
    if (b0 >= mis && b0 + 4 <= end) {
      v = *reinterpret_cast<const uint32_t*>(base + b0);
    } else {
      v = 0;
      for (int j = 0; j < 4; ++j)
        if (b0 + j >= mis && b0 + j < end) v |= (uint32_t)base[b0 + j] << (8 * j);
    }
    d[i] = v;
  }
}

__global__ __launch_bounds__(resize::kRsThreads) void k_resize_lanczos(resize::Args a) {
  using namespace resize;
  extern __shared__ __attribute__((aligned(16))) uint8_t resize_lds[];
  float* lut = reinterpret_cast<float*>(resize_lds);
  uint8_t* obuf = resize_lds + kLutBytes;
  uint8_t* tile = obuf + a.rb * kRowBytes;
  uint8_t* raw = tile + a.tile_rows * kRowBytes;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int bands = kOut / a.rb;
  const int64_t img = blockIdx.x / bands;
  const int y0 = (int)(blockIdx.x - img * bands) * a.rb;
  if (img >= a.n) return;
  if (a.outf) u8_norm_table(lut);
  const int32_t* xb = a.tab + kHdrInts;
  const int32_t* yb = xb + 2 * kOut;
  const int32_t* kxc = yb + 2 * kOut;
  const int32_t* kyc = kxc + kOut * a.kx;
  const bool hpass = a.w != kOut, vpass = a.h != kOut;
  int r0, r1;
  band_rows(yb, y0, a.rb, a.h, a.ky, vpass, &r0, &r1);
  if (r1 - r0 > a.tile_rows) r1 = r0 + a.tile_rows;
  const int nrows = r1 - r0;
  const int row_bytes = a.w * 3;
  const int64_t img_off = img * a.h * (int64_t)row_bytes;

  // horizontal pass: input rows r0 .. r1 - 1 into the tile, one row per wave at a time
  for (int g = 0; g < nrows; g += kRsWaves) {
    const int lr = g + wave;
    const int64_t off = img_off + (int64_t)(r0 + lr) * row_bytes;
    const int mis = (int)(off & 3);              // `frames` is dword-aligned
    if (lr < nrows) resize_load_row(a.frames + off, mis, row_bytes, hpass ? raw + wave * a.raw_stride : tile + lr * kRowBytes, lane);
    if (hpass) {
      __syncthreads();
      if (lr < nrows) {
        const uint8_t* rw = raw + wave * a.raw_stride + mis;
        for (int o = lane; o < kRowBytes; o += 64) {
          const int xx = o / 3, c = o - 3 * xx;
          int xmin, n;
          safe_bounds(xb, xx, a.w, a.kx, &xmin, &n);
          tile[lr * kRowBytes + o] = sample(rw + xmin * 3 + c, 3, kxc + xx * a.kx, n);
        }
      }                                          // (a wave reads only its own raw row: no barrier before the next load)
    }
  }
  __syncthreads();

  // vertical pass: one dword (four bytes of an output row) per thread and step
  for (int task = t; task < a.rb * (kRowBytes / 4); task += kRsThreads) {
    const int row = task / (kRowBytes / 4), q = task - row * (kRowBytes / 4);
    const int yy = y0 + row;
    uint32_t word;
    if (vpass) {
      int ymin, n;
      safe_bounds(yb, yy, a.h, a.ky, &ymin, &n);
      ymin = clampi(ymin, r0, r1);
      if (n > r1 - ymin) n = r1 - ymin;
      const uint32_t* col = reinterpret_cast<const uint32_t*>(tile + (ymin - r0) * kRowBytes) + q;
      const int32_t* k = kyc + yy * a.ky;
      int32_t a0 = kHalf, a1 = kHalf, a2 = kHalf, a3 = kHalf;
      for (int y = 0; y < n; ++y) {
        const uint32_t v = col[y * (kRowBytes / 4)];
        const int32_t c = k[y];
        a0 += (int32_t)(v & 255u) * c;
        a1 += (int32_t)((v >> 8) & 255u) * c;
        a2 += (int32_t)((v >> 16) & 255u) * c;
        a3 += (int32_t)(v >> 24) * c;
      }
      word = finish(a0) | finish(a1) << 8 | finish(a2) << 16 | finish(a3) << 24;
    } else {
      word = row < nrows ? reinterpret_cast<const uint32_t*>(tile + row * kRowBytes)[q] : 0u;
    }
    reinterpret_cast<uint32_t*>(a.out + (img * kOut + yy) * kRowBytes)[q] = word;
    if (a.outf) reinterpret_cast<uint32_t*>(obuf)[task] = word;
  }
  if (a.outf) {
    __syncthreads();
    for (int i = t; i < a.rb * kRowBytes; i += kRsThreads) {
      const int row = i / kRowBytes, rem = i - row * kRowBytes;
      const int c = rem >> 7, x = rem & 127;
      a.outf[((img * 3 + c) * kOut + y0 + row) * kOut + x] = lut[obuf[row * kRowBytes + x * 3 + c]];
    }
  }
}

}  // namespace ndp

extern "C" {

int64_t ndp_resize_workspace_bytes(int64_t height, int64_t width) {
  ndp::resize::Plan p;
  return ndp::resize::make_plan(height, width, &p) ? p.ints * 4 : 0;
}

int ndp_resize_build_tables(int64_t height, int64_t width, void* tables_host, int64_t bytes) {
  using namespace ndp;
  using namespace ndp::resize;
  NDP_CHECK_ARG(tables_host, "ndp_resize_build_tables: null pointer");
  Plan p;
  NDP_CHECK_ARG(make_plan(height, width, &p), "ndp_resize_build_tables: frames of %lld x %lld are outside 1..%d",
                (long long)height, (long long)width, kMaxIn);
  NDP_CHECK_ARG(bytes >= p.ints * 4, "ndp_resize_build_tables: %lld bytes are below the %lld the tables need",
                (long long)bytes, (long long)(p.ints * 4));
  NDP_CHECK_ARG((reinterpret_cast<uintptr_t>(tables_host) & 3) == 0, "ndp_resize_build_tables: tables must be 4-byte aligned");
  double scratch[2 * (3 * kMaxIn / kOut) + 1];
  static_assert(sizeof(scratch) / sizeof(double) == 97, "ksize of the largest input");
  const int64_t worst = build_tables(p, static_cast<int32_t*>(tables_host), scratch);
  if (worst >= ((int64_t)1 << 31))
    return fail(NDP_E_UNSUPPORTED, "ndp_resize_build_tables: an accumulator could reach %lld", (long long)worst);
  return NDP_OK;
}

int ndp_resize_lanczos_u8(const uint8_t* frames_hwc, int64_t n_images, int64_t height, int64_t width, const void* tables,
                          int64_t table_bytes, int rows_per_band, uint8_t* out_hwc, float* images, void* stream) {
  using namespace ndp;
  using namespace ndp::resize;
  NDP_CHECK_ARG(frames_hwc && tables && out_hwc, "ndp_resize_lanczos_u8: null pointer");
  NDP_CHECK_ARG(n_images >= 1 && n_images <= kMaxImages, "ndp_resize_lanczos_u8: bad image count %lld", (long long)n_images);
  Plan p;
  NDP_CHECK_ARG(make_plan(height, width, &p), "ndp_resize_lanczos_u8: frames of %lld x %lld are outside 1..%d",
                (long long)height, (long long)width, kMaxIn);
  NDP_CHECK_ARG(table_bytes >= p.ints * 4, "ndp_resize_lanczos_u8: tables of %lld bytes are below the %lld that %d x %d needs",
                (long long)table_bytes, (long long)(p.ints * 4), p.h, p.w);
  NDP_CHECK_ARG(((reinterpret_cast<uintptr_t>(frames_hwc) | reinterpret_cast<uintptr_t>(tables) |
                  reinterpret_cast<uintptr_t>(out_hwc) | reinterpret_cast<uintptr_t>(images)) & 3) == 0,
                "ndp_resize_lanczos_u8: frames, tables and outputs must be 4-byte aligned");
  NDP_CHECK_ARG(rows_per_band == 0 || rows_per_band == 1 || rows_per_band == 2 || rows_per_band == 4 || rows_per_band == 8 ||
                rows_per_band == 16, "ndp_resize_lanczos_u8: rows_per_band %d is not 0 (automatic), 1, 2, 4, 8 or 16",
                rows_per_band);
  const int rb = rows_per_band ? rows_per_band : choose_rb(n_images, p.h, p.w);
  const int tile_rows = tile_rows_for(p.h, rb);
  const int lds = lds_bytes(rb, tile_rows, p.w);
  NDP_CHECK_ARG(lds <= kLdsBudget, "ndp_resize_lanczos_u8: bands of %d rows of a %d x %d frame need %d bytes of LDS (at most %d)",
                rb, p.h, p.w, lds, kLdsBudget);
  hipStream_t st = (hipStream_t)stream;
  Args a{frames_hwc, static_cast<const int32_t*>(tables), out_hwc, images, n_images, p.h, p.w, p.kx, p.ky, rb, tile_rows,
         raw_stride(p.w)};
  KTimer kt("k_resize_lanczos", st);
  hipLaunchKernelGGL(k_resize_lanczos, dim3((unsigned)(n_images * (kOut / rb))), dim3(kRsThreads), (size_t)lds, st, a);
  return check_launch("k_resize_lanczos");
}

}  // extern "C"
