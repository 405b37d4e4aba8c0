// fm_score.inc -- the forward-model scoring kernel (k_fm_score, csrc/ndp_eval.inc) run on the CPU, for
// tests/test_fm_score_host.py.  main.hip includes it behind the library's source (see there); it calls the __host__
// __device__ functions the kernel calls (fm_score::row_of, thread_elems, tile_byte, norm_u8, sq_diff, to_byte) by the
// kernel's schedule: one "workgroup" of 768 threads per prediction, 16 tiles, per tile the staging of the HWC bytes "in
// LDS", the threads' four elements, the byte tile written back, then the fixed 768 -> 512 -> 256 .. 1 tree over the
// threads' fp64 sums.  What k_fm_score does outside those functions -- the loops, the barriers' phases, the tree -- is
// restated here and tested as a copy; a slip in the device's own form of those is seen only by the GPU tests
// (tests/test_gpu_forward_model_eval.py).  It makes no HIP runtime call and needs no GPU.
//
// Usage: host_driver fm_score IN OUT
//   IN   int32 cases, then per case 8 int32 (n, n_target, n_base, target kind 1 floats / 2 bytes, base kind 0 none / 1 / 2,
//        has target_idx, has base_idx, want bytes), pred n x 49,152 floats, the targets (n_target x 49,152 floats or
//        bytes), the base frames, target_idx [n] int32 if present, base_idx [n] int32 if present
//   OUT  per case pred_err [n] floats, base_err [n] floats (the sentinel -7 where there is no base), bytes [n x 49,152]
//        (0xA5 where not wanted)
// Every buffer -- inputs, outputs, index maps, each LDS array -- is an allocation of exactly its size, so a sanitizer sees
// any access past it.
namespace host::fm_score {

using namespace ndp::fm_score;

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

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  static_assert(kScoreThreads * 4 == kTileBytes && kTiles * kTilePixels == kPlane && kValues == 49152, "the schedule");
  int32_t cases = 0;
  if (!read_pod(in, &cases) || cases < 0) return kBadInput;
  for (int32_t ci = 0; ci < cases; ++ci) {
    Case c;
    if (!read_pod(in, &c)) return kBadInput;
    if (c.n < 1 || c.n_target < 1 || (c.base_kind != 0 && c.n_base < 1)) return kBadInput;
    const size_t n = (size_t)c.n;
    Exact<float> pred(n * kValues);
    Exact<float> tgt_f32(c.tgt_kind == 1 ? (size_t)c.n_target * kValues : 0);
    Exact<unsigned char> tgt_u8(c.tgt_kind == 2 ? (size_t)c.n_target * kValues : 0);
    Exact<float> base_f32(c.base_kind == 1 ? (size_t)c.n_base * kValues : 0);
    Exact<unsigned char> base_u8(c.base_kind == 2 ? (size_t)c.n_base * kValues : 0);
    Exact<int32_t> tidx(c.has_tidx ? n : 0), bidx(c.has_bidx ? n : 0);
    if (!pred.read(in) || !tgt_f32.read(in) || !tgt_u8.read(in) || !base_f32.read(in) || !base_u8.read(in) ||
        !tidx.read(in) || !bidx.read(in))
      return kBadInput;
    Exact<float> pred_err(n), base_err(n);
    Exact<unsigned char> bytes(n * kValues);
    pred_err.fill(-7.0f);
    base_err.fill(-7.0f);
    bytes.fill(0xA5);
    for (int64_t img = 0; img < c.n; ++img)
      score_image(c, img, pred.p, c.tgt_kind == 1 ? tgt_f32.p : nullptr, c.tgt_kind == 2 ? tgt_u8.p : nullptr,
                  c.has_tidx ? tidx.p : nullptr, c.base_kind == 1 ? base_f32.p : nullptr,
                  c.base_kind == 2 ? base_u8.p : nullptr, c.has_bidx ? bidx.p : nullptr, pred_err.p, base_err.p, bytes.p);
    pred_err.write(out);
    base_err.write(out);
    bytes.write(out);
  }
  return close_files(in, out);
}

}  // namespace host::fm_score
