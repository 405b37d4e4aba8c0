// fm_score_host_driver.hip -- the forward-model scoring kernel (k_fm_score, csrc/ndp_eval.inc) run on the CPU, for
// tests/test_fm_score_host.py.  It includes the library's source as the library build does and calls the __host__
// __device__ functions the kernel calls (fm_score::row_of, thread_elems, tile_byte, norm_u8, sq_diff, to_byte) by the
// kernel's schedule: one "workgroup" of 768 threads per prediction, 16 tiles, per tile the staging of the HWC bytes "in
// LDS", the threads' four elements, the byte tile written back, then the fixed 768 -> 512 -> 256 .. 1 tree over the
// threads' fp64 sums.  What k_fm_score does outside those functions -- the loops, the barriers' phases, the tree -- is
// restated here and tested as a copy; a slip in the device's own form of those is seen only by the GPU tests
// (tests/test_gpu_forward_model_eval.py).  It makes no HIP runtime call and needs no GPU.
//
// Usage: fm_score_host_driver IN OUT
//   IN   int32 cases, then per case 8 int32 (n, n_target, n_base, target kind 1 floats / 2 bytes, base kind 0 none / 1 / 2,
//        has target_idx, has base_idx, want bytes), pred n x 49,152 floats, the targets (n_target x 49,152 floats or
//        bytes), the base frames, target_idx [n] int32 if present, base_idx [n] int32 if present
//   OUT  per case pred_err [n] floats, base_err [n] floats (the sentinel -7 where there is no base), bytes [n x 49,152]
//        (0xA5 where not wanted)
// Every buffer -- inputs, outputs, index maps, each LDS array -- is an allocation of exactly its size, so a sanitizer sees
// any access past it.
#include "../ndivplanning_amd/csrc/ndp_kernels.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

using namespace ndp::fm_score;

template <class T>
struct Exact {
  T* p;
  size_t n;
  explicit Exact(size_t count) : p(static_cast<T*>(malloc(count ? count * sizeof(T) : 1))), n(count) {}
  ~Exact() { free(p); }
  Exact(const Exact&) = delete;
  bool read(FILE* f) { return fread(p, sizeof(T), n, f) == n; }
};

struct Case {
  int32_t n, n_target, n_base, tgt_kind, base_kind, has_tidx, has_bidx, want_bytes;
};

// k_fm_score<tgt_kind, base_kind> for the workgroup of image `img`
void score_image(const Case& c, int64_t img, const float* pred, const float* tgt_f32, const unsigned char* tgt_u8,
                 const int32_t* tidx, const float* base_f32, const unsigned char* base_u8, const int32_t* bidx,
                 float* pred_err, float* base_err, unsigned char* pred_u8) {
  Exact<float> lut(256);
  Exact<unsigned char> tin(kTileBytes), bin(kTileBytes), tout(kTileBytes);
  Exact<double> red(kScoreThreads), sp(kScoreThreads), sb(kScoreThreads);
  Exact<float> y(4 * kScoreThreads), x(4 * kScoreThreads), b(4 * kScoreThreads);
  for (int i = 0; i < 256; ++i) lut.p[i] = norm_u8(i);
  const int64_t tr = row_of(tidx, img, c.n_target);
  const int64_t br = c.base_kind != 0 ? row_of(bidx, img, c.n_base) : -1;
  const bool do_pred = tr >= 0;
  const bool do_base = c.base_kind != 0 && tr >= 0 && br >= 0;
  const bool do_tgt = do_pred || do_base;
  const bool do_bytes = c.want_bytes != 0;
  for (int t = 0; t < kScoreThreads; ++t) sp.p[t] = sb.p[t] = 0.0;
  for (int tile = 0; tile < kTiles; ++tile) {
    for (int t = 0; t < kScoreThreads; ++t) {                       // up to the first barrier
      int plane, lp0, off;
      thread_elems(t, tile, &plane, &lp0, &off);
      if (c.tgt_kind == 2 && do_tgt) memcpy(tin.p + 4 * t, tgt_u8 + tr * kValues + (int64_t)tile * kTileBytes + 4 * t, 4);
      if (c.base_kind == 2 && do_base) memcpy(bin.p + 4 * t, base_u8 + br * kValues + (int64_t)tile * kTileBytes + 4 * t, 4);
      memcpy(y.p + 4 * t, pred + img * kValues + off, 16);
      if (c.tgt_kind == 1 && do_tgt) memcpy(x.p + 4 * t, tgt_f32 + tr * kValues + off, 16);
      if (c.base_kind == 1 && do_base) memcpy(b.p + 4 * t, base_f32 + br * kValues + off, 16);
    }
    for (int t = 0; t < kScoreThreads; ++t) {                       // between the barriers
      int plane, lp0, off;
      thread_elems(t, tile, &plane, &lp0, &off);
      for (int e = 0; e < 4; ++e) {
        const int byte = tile_byte(lp0 + e, plane);
        if (c.tgt_kind == 2 && do_tgt) x.p[4 * t + e] = lut.p[tin.p[byte]];
        if (c.base_kind == 2 && do_base) b.p[4 * t + e] = lut.p[bin.p[byte]];
        if (do_pred) sp.p[t] += sq_diff(y.p[4 * t + e], x.p[4 * t + e]);
        if (do_base) sb.p[t] += sq_diff(b.p[4 * t + e], x.p[4 * t + e]);
        if (do_bytes) tout.p[byte] = to_byte(y.p[4 * t + e]);
      }
    }
    if (do_bytes)                                                   // behind the second barrier
      for (int t = 0; t < kScoreThreads; ++t) memcpy(pred_u8 + img * kValues + (int64_t)tile * kTileBytes + 4 * t, tout.p + 4 * t, 4);
  }
  for (int pass = 0; pass < 2; ++pass) {                            // fm_score_block_sum
    if (pass == 1 && c.base_kind == 0) break;
    for (int t = 0; t < kScoreThreads; ++t) red.p[t] = pass == 0 ? sp.p[t] : sb.p[t];
    for (int t = 0; t < 256; ++t) red.p[t] += red.p[t + 512];
    for (int w = 256; w > 0; w >>= 1)
      for (int t = 0; t < w; ++t) red.p[t] += red.p[t + w];
    const bool ok = pass == 0 ? do_pred : do_base;
    (pass == 0 ? pred_err : base_err)[img] = ok ? (float)(red.p[0] / (double)kValues) : NAN;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
    return 2;
  }
  static_assert(kScoreThreads * 4 == kTileBytes && kTiles * kTilePixels == kPlane && kValues == 49152, "the schedule");
  int32_t cases = 0;
  if (fread(&cases, 4, 1, in) != 1 || cases < 0) return 2;
  for (int32_t ci = 0; ci < cases; ++ci) {
    Case c;
    if (fread(&c, sizeof(c), 1, in) != 1) return 2;
    if (c.n < 1 || c.n_target < 1 || (c.base_kind != 0 && c.n_base < 1)) return 2;
    const size_t n = (size_t)c.n;
    Exact<float> pred(n * kValues);
    Exact<float> tgt_f32(c.tgt_kind == 1 ? (size_t)c.n_target * kValues : 0);
    Exact<unsigned char> tgt_u8(c.tgt_kind == 2 ? (size_t)c.n_target * kValues : 0);
    Exact<float> base_f32(c.base_kind == 1 ? (size_t)c.n_base * kValues : 0);
    Exact<unsigned char> base_u8(c.base_kind == 2 ? (size_t)c.n_base * kValues : 0);
    Exact<int32_t> tidx(c.has_tidx ? n : 0), bidx(c.has_bidx ? n : 0);
    if (!pred.read(in) || !tgt_f32.read(in) || !tgt_u8.read(in) || !base_f32.read(in) || !base_u8.read(in) ||
        !tidx.read(in) || !bidx.read(in))
      return 2;
    Exact<float> pred_err(n), base_err(n);
    Exact<unsigned char> bytes(n * kValues);
    for (size_t i = 0; i < n; ++i) pred_err.p[i] = base_err.p[i] = -7.0f;
    memset(bytes.p, 0xA5, n * kValues);
    for (int64_t img = 0; img < c.n; ++img)
      score_image(c, img, pred.p, c.tgt_kind == 1 ? tgt_f32.p : nullptr, c.tgt_kind == 2 ? tgt_u8.p : nullptr,
                  c.has_tidx ? tidx.p : nullptr, c.base_kind == 1 ? base_f32.p : nullptr,
                  c.base_kind == 2 ? base_u8.p : nullptr, c.has_bidx ? bidx.p : nullptr, pred_err.p, base_err.p, bytes.p);
    fwrite(pred_err.p, 4, n, out);
    fwrite(base_err.p, 4, n, out);
    fwrite(bytes.p, 1, n * kValues, out);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  return 0;
}
