// image_quality.inc -- the image-quality kernels (k_image_quality, k_image_quality_finish, csrc/ndp_eval.inc)
// run on the CPU, for tests/test_image_quality_host.py.  main.hip includes it behind the library's source (see there); it
// calls the __host__ __device__ functions the kernels call (image_quality::tap, unit, product, filter, ssim_at, sq_diff,
// bands, band_rows, h_item, ssim_slot, psnr_slot, ssim_of, psnr_of; fm_score::row_of, norm_u8) by the kernels' schedule:
// one "workgroup" of 16 * rows threads per (pair, channel, band), the two operands' rows scaled "into LDS", the band's own
// rows' squared differences summed per row by 16 lanes and folded, the five maps filtered along the rows, 16 lanes per
// output row filtering down the columns, S, the lane's fp64 sum in column order, the fold; then per pair the fixed tree
// over the 354 and 384 row sums.  What the kernels do outside those functions -- the loops, the barriers' phases, the
// folds -- is restated here and tested as a copy; a slip in the device's own form of those is seen only by the GPU tests
// (tests/test_gpu_image_quality.py).  It makes no HIP runtime call and needs no GPU.
//
// Usage: host_driver image_quality IN OUT
//   IN   int32 cases, then per case 8 int32 (n_pairs, n_a, n_b, a kind 1 floats / 2 bytes, b kind, index maps: bit 0
//        a_idx, bit 1 b_idx, output rows per band, wanted: bit 0 ssim, bit 1 psnr), a (n_a x 49,152 floats or bytes), b,
//        a_idx [n_pairs] int32 if present, b_idx [n_pairs] int32 if present
//   OUT  per case ssim [n_pairs] floats, psnr [n_pairs] floats (the sentinel -7 where not wanted)
// Every buffer -- inputs, outputs, index maps, the workspace, each LDS array -- is an allocation of exactly its size, so a
// sanitizer sees any access past it.  Exit 3: the tap table is not the double computation rounded once.
namespace host::image_quality {

using namespace ndp::image_quality;
using ndp::fm_score::norm_u8;
using ndp::fm_score::row_of;

struct Case {
  int32_t n_pairs, n_a, n_b, a_kind, b_kind, maps, rows, want;
};

struct Operand {
  const float* f32;
  const unsigned char* u8;
};

// iq_stage
void stage(const Operand& o, int64_t row, int c, int r0, int in_rows, const float* lut, float* dst) {
  if (o.f32) {
    const float* src = o.f32 + row * kValues + c * kPlane + r0 * kSide;
    for (int i = 0; i < in_rows * (kSide / 4); ++i) {
      float v[4];
      memcpy(v, src + 4 * i, 16);
      for (int e = 0; e < 4; ++e) dst[4 * i + e] = unit(v[e]);
    }
  } else {
    const unsigned char* src = o.u8 + row * kValues + (int64_t)r0 * kSide * 3 + c;
    for (int i = 0; i < in_rows * kSide; ++i) dst[i] = unit(lut[src[3 * i]]);
  }
}

// iq_row_fold, lane 0's value
double fold(double* v) {
  for (int w = kRowLanes / 2; w > 0; w >>= 1)
    for (int j = 0; j < w; ++j) v[j] += v[j + w];
  return v[0];
}

// k_image_quality<rows> for the workgroup of (pair, c, band)
void band_block(const Case& k, const Operand& a, const int32_t* a_idx, const Operand& b, const int32_t* b_idx,
                int64_t pair, int c, int band, double* sums) {
  const int rows = k.rows, in_max = rows + kHalo;
  const int64_t ra = row_of(a_idx, pair, k.n_a), rb = row_of(b_idx, pair, k.n_b);
  if (ra < 0 || rb < 0) return;
  Exact<float> xs((size_t)in_max * kSide), ys((size_t)in_max * kSide), lut(256);
  Exact<float> h0((size_t)in_max * kOut), h1((size_t)in_max * kOut), h2((size_t)in_max * kOut), h3((size_t)in_max * kOut),
      h4((size_t)in_max * kOut);
  int r0, out_rows, in_rows, own_rows;
  band_rows(band, rows, &r0, &out_rows, &in_rows, &own_rows);
  for (int i = 0; i < 256; ++i) lut.p[i] = norm_u8(i);
  stage(a, ra, c, r0, in_rows, lut.p, xs.p);
  stage(b, rb, c, r0, in_rows, lut.p, ys.p);
  Exact<double> lanes(kRowLanes);
  if (k.want & 2) {
    for (int group = 0; group < rows; ++group)
      for (int r = group; r < own_rows; r += rows) {
        for (int lane = 0; lane < kRowLanes; ++lane) {
          double s = 0.0;
          for (int col = lane; col < kSide; col += kRowLanes) s += sq_diff(xs.p[r * kSide + col], ys.p[r * kSide + col]);
          lanes.p[lane] = s;
        }
        sums[psnr_slot(pair, c, r0 + r)] = fold(lanes.p);
      }
  }
  if (!(k.want & 1)) return;
  for (int i = 0; i < in_rows * kOut; ++i) {
    int row, col;
    h_item(i, &row, &col);
    float x[kTaps], y[kTaps], xx[kTaps], yy[kTaps], xy[kTaps];
    for (int t = 0; t < kTaps; ++t) {
      x[t] = xs.p[row * kSide + col + t];
      y[t] = ys.p[row * kSide + col + t];
      xx[t] = product(x[t], x[t]);
      yy[t] = product(y[t], y[t]);
      xy[t] = product(x[t], y[t]);
    }
    h0.p[i] = filter(x, 1);
    h1.p[i] = filter(y, 1);
    h2.p[i] = filter(xx, 1);
    h3.p[i] = filter(yy, 1);
    h4.p[i] = filter(xy, 1);
  }
  for (int group = 0; group < out_rows; ++group) {
    for (int lane = 0; lane < kRowLanes; ++lane) {
      double s = 0.0;
      for (int col = lane; col < kOut; col += kRowLanes) {
        const int at = group * kOut + col;
        s += (double)ssim_at(filter(h0.p + at, kOut), filter(h1.p + at, kOut), filter(h2.p + at, kOut),
                             filter(h3.p + at, kOut), filter(h4.p + at, kOut));
      }
      lanes.p[lane] = s;
    }
    sums[ssim_slot(pair, c, r0 + group)] = fold(lanes.p);
  }
}

// iq_finish_sum
double finish_sum(const double* v, int n) {
  constexpr int T = kFinishThreads;
  Exact<double> red(T);
  for (int t = 0; t < T; ++t) red.p[t] = (t < n ? v[t] : 0.0) + (t + T < n ? v[t + T] : 0.0);
  for (int w = T / 2; w > 0; w >>= 1)
    for (int t = 0; t < w; ++t) red.p[t] += red.p[t + w];
  return red.p[0];
}

// k_image_quality_finish for the workgroup of `pair`
void finish_block(const Case& k, const int32_t* a_idx, const int32_t* b_idx, int64_t pair, const double* sums, float* ssim,
                  float* psnr) {
  const bool ok = row_of(a_idx, pair, k.n_a) >= 0 && row_of(b_idx, pair, k.n_b) >= 0;
  if (!ok) {
    if (k.want & 1) ssim[pair] = NAN;
    if (k.want & 2) psnr[pair] = NAN;
    return;
  }
  if (k.want & 1) ssim[pair] = ssim_of(finish_sum(sums + ssim_slot(pair, 0, 0), kSsimRows));
  if (k.want & 2) psnr[pair] = psnr_of(finish_sum(sums + psnr_slot(pair, 0, 0), kPsnrRows));
}

bool taps_are_the_double_computation() {
  double g[kTaps], sum = 0.0;
  for (int i = 0; i < kTaps; ++i) sum += g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
  for (int i = 0; i < kTaps; ++i)
    if (tap(i) != (float)(g[i] / sum)) return false;
  return true;
}

int run(int argc, char** argv) {
  static_assert(kRowSums == 3 * 118 + 3 * 128 && kSsimRows <= 2 * kFinishThreads && kPsnrRows <= 2 * kFinishThreads &&
                    kSsimValues == 41772 && kValues == 49152, "the schedule");
  if (!taps_are_the_double_computation()) return 3;
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  int32_t cases = 0;
  if (!read_pod(in, &cases) || cases < 0) return kBadInput;
  for (int32_t ci = 0; ci < cases; ++ci) {
    Case k;
    if (!read_pod(in, &k)) return kBadInput;
    if (k.n_pairs < 1 || k.n_a < 1 || k.n_b < 1 || k.rows < 1 || k.rows > kOut || !(k.want & 3)) return kBadInput;
    const size_t n = (size_t)k.n_pairs;
    Exact<float> a_f32(k.a_kind == 1 ? (size_t)k.n_a * kValues : 0), b_f32(k.b_kind == 1 ? (size_t)k.n_b * kValues : 0);
    Exact<unsigned char> a_u8(k.a_kind == 2 ? (size_t)k.n_a * kValues : 0), b_u8(k.b_kind == 2 ? (size_t)k.n_b * kValues : 0);
    Exact<int32_t> a_idx(k.maps & 1 ? n : 0), b_idx(k.maps & 2 ? n : 0);
    if (!a_f32.read(in) || !a_u8.read(in) || !b_f32.read(in) || !b_u8.read(in) || !a_idx.read(in) || !b_idx.read(in))
      return kBadInput;
    const Operand a{k.a_kind == 1 ? a_f32.p : nullptr, k.a_kind == 2 ? a_u8.p : nullptr};
    const Operand b{k.b_kind == 1 ? b_f32.p : nullptr, k.b_kind == 2 ? b_u8.p : nullptr};
    const int32_t* ai = k.maps & 1 ? a_idx.p : nullptr;
    const int32_t* bi = k.maps & 2 ? b_idx.p : nullptr;
    Exact<double> sums(n * kRowSums);
    Exact<float> ssim(n), psnr(n);
    sums.fill(-7.0);
    ssim.fill(-7.0f);
    psnr.fill(-7.0f);
    const int nb = bands(k.rows);
    for (int64_t block = 0; block < (int64_t)n * 3 * nb; ++block)
      band_block(k, a, ai, b, bi, block / (3 * nb), (int)((block / nb) % 3), (int)(block % nb), sums.p);
    for (int64_t pair = 0; pair < k.n_pairs; ++pair) finish_block(k, ai, bi, pair, sums.p, ssim.p, psnr.p);
    ssim.write(out);
    psnr.write(out);
  }
  return close_files(in, out);
}

}  // namespace host::image_quality
