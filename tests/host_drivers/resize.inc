// resize.inc -- the Lanczos resize (csrc/ndp_resize.inc) run on the CPU, for tests/test_resize_core_host.py.
// main.hip includes it behind the library's source (see there); it calls the __host__ __device__ functions the kernel
// calls (make_plan, build_tables, safe_bounds, band_rows, sample, finish) and the host functions of the launch
// (choose_rb, tile_rows_for, lds_bytes); it makes no HIP runtime call and needs no GPU.  What k_resize_lanczos does
// outside those functions is restated here and tested as a copy: the loop over a band's input rows, the placement of
// the horizontally filtered rows in the tile, the vertical pass out of the tile.  A slip in the device's own form of
// those (the dword loads of a misaligned row, the four-bytes-per-thread vertical pass, the float output) is seen only
// by the GPU tests (tests/test_gpu_resize.py).
//
// Usage: host_driver resize IN OUT
//   IN   int32 n, then n x (int32 H, int32 W, H*W*3 bytes of frame, 128*128*3 bytes expected)
//   OUT  per case kRecordInts int32 (see Record), then the 128x128x3 bytes of the resize by the n = 1 schedule
// Every frame is resized by every band split the launch can choose (n = 1 .. 64 images) that fits LDS.  The frame, every
// raw input row "in LDS", every band's tile and the tables live in allocations of exactly their own size, so a sanitizer
// sees any access past them.
namespace host::resize {

using namespace ndp::resize;

struct Record {
  int32_t equal;           // 1: every schedule gave the expected bytes
  int32_t mismatches;      // bytes that differ from the expected ones, over all schedules
  int32_t schedules;       // band splits run
  int32_t kx, ky;          // taps per output sample
  int32_t worst_lo;        // the largest magnitude an accumulator can reach over the tables (build_tables),
  int32_t worst_hi;        //   low and high 32 bits
  int32_t max_tile_rows;   // the tallest tile over the schedules
};
constexpr int kRecordInts = sizeof(Record) / 4;
constexpr int kFrame = kOut * kRowBytes;

// k_resize_lanczos for one frame with bands of rb rows.  Returns false where a band needs more rows than the launch
// would have allocated.
bool resize_frame(const uint8_t* frame, const Plan& p, const int32_t* tab, int rb, uint8_t* out, int* max_rows) {
  const int32_t* xb = tab + p.xb;
  const int32_t* yb = tab + p.yb;
  const int32_t* kxc = tab + p.kxc;
  const int32_t* kyc = tab + p.kyc;
  const bool hpass = p.w != kOut, vpass = p.h != kOut;
  const int tile_rows = tile_rows_for(p.h, rb);
  const int row_bytes = p.w * 3;
  if (tile_rows > *max_rows) *max_rows = tile_rows;
  for (int y0 = 0; y0 < kOut; y0 += rb) {
    int r0, r1;
    band_rows(yb, y0, rb, p.h, p.ky, vpass, &r0, &r1);
    if (r1 - r0 > tile_rows) return false;
    const int nrows = r1 - r0;
    Exact<uint8_t> tile((size_t)nrows * kRowBytes);
    for (int lr = 0; lr < nrows; ++lr) {
      Exact<uint8_t> raw(row_bytes);
      memcpy(raw.p, frame + (size_t)(r0 + lr) * row_bytes, row_bytes);
      if (!hpass) {
        memcpy(tile.p + (size_t)lr * kRowBytes, raw.p, kRowBytes);
        continue;
      }
      for (int o = 0; o < kRowBytes; ++o) {
        const int xx = o / 3, c = o - 3 * xx;
        int xmin, n;
        safe_bounds(xb, xx, p.w, p.kx, &xmin, &n);
        tile.p[(size_t)lr * kRowBytes + o] = sample(raw.p + xmin * 3 + c, 3, kxc + xx * p.kx, n);
      }
    }
    for (int row = 0; row < rb; ++row) {
      const int yy = y0 + row;
      uint8_t* dst = out + (size_t)yy * kRowBytes;
      if (!vpass) {
        memcpy(dst, tile.p + (size_t)row * kRowBytes, kRowBytes);
        continue;
      }
      int ymin, n;
      safe_bounds(yb, yy, p.h, p.ky, &ymin, &n);
      ymin = clampi(ymin, r0, r1);
      if (n > r1 - ymin) n = r1 - ymin;
      for (int o = 0; o < kRowBytes; ++o)
        dst[o] = sample(tile.p + (size_t)(ymin - r0) * kRowBytes + o, kRowBytes, kyc + yy * p.ky, n);
    }
  }
  return true;
}

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  int32_t n = 0;
  if (!read_pod(in, &n) || n < 0) return kBadInput;
  for (int32_t i = 0; i < n; ++i) {
    int32_t hw[2];
    if (!read_pod(in, &hw)) return kBadInput;
    Plan p;
    if (!make_plan(hw[0], hw[1], &p)) return kBadInput;
    if (ndp_resize_workspace_bytes(hw[0], hw[1]) != p.ints * 4) return 3;
    const size_t bytes = (size_t)p.h * p.w * 3;
    Exact<uint8_t> frame(bytes), want(kFrame), got(kFrame), first(kFrame);
    if (!frame.read(in) || !want.read(in)) return kBadInput;
    Exact<int32_t> tab((size_t)p.ints);
    Exact<double> scratch((size_t)(p.kx > p.ky ? p.kx : p.ky));
    const int64_t worst = build_tables(p, tab.p, scratch.p);
    // the library's own entry builds the same table
    Exact<int32_t> tab2((size_t)p.ints);
    if (ndp_resize_build_tables(p.h, p.w, tab2.p, p.ints * 4) != 0 || memcmp(tab.p, tab2.p, (size_t)p.ints * 4) != 0) return 3;
    Record rec;
    memset(&rec, 0, sizeof(rec));
    rec.equal = 1;
    rec.kx = p.kx;
    rec.ky = p.ky;
    rec.worst_lo = (int32_t)(worst & 0xFFFFFFFFll);
    rec.worst_hi = (int32_t)(worst >> 32);
    int last_rb = 0;
    for (int64_t images = 1; images <= 64; images *= 2) {
      const int rb = choose_rb(images, p.h, p.w);
      if (rb == last_rb) continue;
      last_rb = rb;
      if (lds_bytes(rb, tile_rows_for(p.h, rb), p.w) > kLdsBudget) return 4;
      memset(got.p, 0xA5, kFrame);
      if (!resize_frame(frame.p, p, tab.p, rb, got.p, &rec.max_tile_rows)) return 5;
      int bad = 0;
      for (int j = 0; j < kFrame; ++j) bad += got.p[j] != want.p[j];
      rec.mismatches += bad;
      if (bad) rec.equal = 0;
      if (rec.schedules == 0) memcpy(first.p, got.p, kFrame);
      ++rec.schedules;
    }
    static_assert(kRecordInts == 8, "tests/test_resize_core_host.py reads 8 int32 per case");
    fwrite(&rec, sizeof(rec), 1, out);
    fwrite(first.p, 1, kFrame, out);
  }
  return close_files(in, out);
}

}  // namespace host::resize
