// jpeg.inc -- the JPEG decoder's core (csrc/ndp_jpeg.inc) run on the CPU, for tests/test_jpeg_core_host.py
// and tests/golden/make_golden_jpeg_edges.py.  main.hip includes it behind the library's source (see there); it calls the
// __host__ __device__ functions the kernels call (parse_headers, derive_table, lut_entry, marker_at, stuffed_at, eoi_at,
// chunk_bits, Lane, sync_chunk, write_chunk, idct_islow, ycc_pixel); it makes no HIP runtime call and needs no GPU.
// What the kernels do outside those functions is restated here, not shared, and is tested as a copy: the round loop
// and the scans of k_jpeg_entropy (entropy_chunked, dc_sums), k_jpeg_parse's search for the marker and its placement of
// the unstuffed bytes (parse), k_jpeg_idct's dequantisation with its packed int4 loads and its block-to-plane placement
// (pixels).  A slip in the device's own form of those (a round cap, the flags hand-off, the int4 unpacking) is seen
// only by the GPU tests, which compare with PIL (tests/test_gpu_jpeg_edges.py, tests/test_gpu_jpeg.py).
//
// Usage: host_driver jpeg IN OUT [frames]
//   IN   int32 n, then n x (int32 len, len bytes): the streams
//   OUT  per stream kRecordInts int32 (see Record), then, with `frames`, the 128x128x3 bytes of the chunked decode and of
//        the serial decode
// Every stream is decoded twice.  Chunked: k_jpeg_entropy's schedule run serially (the same chunk length, Jacobi rounds
// of sync_chunk over the dirty chunks, at most nchunks + 1 of them, block placement from the per-chunk counts, write_chunk
// per chunk, DC running sums per component).  Serial: one Lane from bit 0, 384 blocks one after the other.  Both then go
// through idct_islow and ycc_pixel.  Each stream, its staged head, its unstuffed data and the part of them "in LDS" live
// in allocations of exactly their own size, so a sanitizer sees any read past them.
namespace host::jpeg {

using namespace ndp::jpeg;

struct Record {
  int32_t status;          // the chunked decode's NDP_JPEG_* status
  int32_t status_serial;   // the serial decode's
  int32_t frames_equal;    // 1: both decodes gave the same 128x128x3 bytes
  int32_t rounds;          // sync rounds run (0: rejected before the entropy stage)
  int32_t nchunks;
  int32_t ncompact;        // unstuffed bytes
  int32_t max_dc_cat;      // census of the serial decode: the largest DC category,
  int32_t zrl;             //   ZRL symbols,
  int32_t no_eob;          //   blocks that end at coefficient 63 without an EOB,
  int32_t slow;            //   symbols whose code is longer than kLook bits,
  int32_t max_abs;         //   the largest |coefficient| (DC as its value)
  int32_t reserved;
};
constexpr int kRecordInts = sizeof(Record) / 4;
constexpr int kFrame = kSize * kSize * 3;

struct Tables {
  uint16_t qt[3][64];
  uint16_t lut[4 << kLook];
  int32_t maxc[4 * 18], voff[4 * 18];
  uint8_t hval[4 * 256];
};

// What k_jpeg_parse does for one frame.  Returns the status; on NDP_JPEG_OK the tables and the unstuffed data (padded
// with zeros to a whole word) are filled in.
int parse(const uint8_t* s, int32_t len, Tables* T, std::vector<uint8_t>* compact, int32_t* ncompact) {
  const int nstage = len < kStage ? len : kStage;
  Exact<uint8_t> stage(nstage);
  if (nstage) memcpy(stage.p, s, nstage);
  Header h;
  memset(&h, 0xA5, sizeof(h));
  int st = parse_headers(stage.p, s, len, &h);
  if (st != NDP_JPEG_OK) return st;
  for (int t = 0; t < 4; ++t) {
    const int slot = (t & 1) ? 4 + h.ta[t >> 1 ? 1 : 0] : h.td[t >> 1 ? 1 : 0];
    if (!derive_table(&h, slot, (t & 1) == 0, T->maxc + 18 * t, T->voff + 18 * t, T->hval + 256 * t)) st = NDP_JPEG_CORRUPT;
  }
  if (st != NDP_JPEG_OK) return st;
  for (int c = 0; c < 3; ++c) memcpy(T->qt[c], h.qt[h.tq[c]], sizeof(T->qt[c]));
  const int32_t e0 = h.sos_end;
  int32_t mark = len;
  for (int32_t p = e0; p < len; ++p) {
    if (marker_at(stage.p, s, p, len)) { mark = p; break; }
  }
  for (int i = 0; i < (4 << kLook); ++i) {
    const int t = i >> kLook;
    T->lut[i] = lut_entry(T->maxc + 18 * t, T->voff + 18 * t, T->hval + 256 * t, i & ((1 << kLook) - 1));
  }
  compact->clear();
  for (int32_t p = e0; p < mark; ++p) {
    if (!stuffed_at(stage.p, s, p, e0)) compact->push_back((uint8_t)rd(stage.p, s, p));
  }
  *ncompact = (int32_t)compact->size();
  while (compact->size() & 3) compact->push_back(0);
  return eoi_at(stage.p, s, mark, len) ? NDP_JPEG_OK : NDP_JPEG_CORRUPT;
}

template <bool FAR>
Lane<FAR> make_lane(const uint32_t* words, const uint32_t* far, int32_t nbytes, const Tables& T) {
  return Lane<FAR>{words, kStreamLdsBytes / 4, far, (nbytes + 3) >> 2, T.lut, T.maxc, T.voff, T.hval};
}

void dc_sums(int16_t* coef, const int32_t* dcd) {
  int32_t acc[3] = {0, 0, 0};
  for (int g = 0; g < kBlocks; ++g) {
    const int mcu = g / 6, bi = g - 6 * mcu;
    const int comp = bi < 4 ? 0 : bi - 3;
    const int blk = bi < 4 ? (2 * (mcu >> 3) + (bi >> 1)) * 16 + 2 * (mcu & 7) + (bi & 1) : 256 + (bi - 4) * 64 + mcu;
    acc[comp] += dcd[g];
    coef[blk * 64] = (int16_t)acc[comp];
  }
}

// k_jpeg_entropy's schedule for one frame, run serially.  Returns the status.
template <bool FAR>
int entropy_chunked(const uint32_t* words, const uint32_t* far, int32_t nbytes, const Tables& T, int16_t* coef,
                    Record* rec) {
  const int32_t avail = nbytes * 8;
  const int32_t chunk = chunk_bits(avail);
  const int nchunks = (avail + chunk - 1) / chunk;
  rec->nchunks = nchunks;
  Lane<FAR> ln = make_lane<FAR>(words, far, nbytes, T);
  std::vector<EState> mine(kEntropyThreads), exits(kEntropyThreads);
  std::vector<int> nblk(kEntropyThreads, 0), dirty(kEntropyThreads, 0);
  std::vector<int32_t> end(kEntropyThreads);
  for (int c = 0; c < kEntropyThreads; ++c) {
    mine[c] = EState{c * chunk, 0, 0};
    exits[c] = EState{0, 0, 0};
    dirty[c] = c < nchunks;
    end[c] = (c + 1) * chunk < avail ? (c + 1) * chunk : avail;
  }
  int rounds = 0;
  for (int round = 0; round <= nchunks; ++round) {
    ++rounds;
    for (int c = 0; c < nchunks; ++c) {
      if (dirty[c]) exits[c] = sync_chunk(ln, mine[c], end[c], &nblk[c]);
      dirty[c] = 0;
    }
    bool any = false;
    for (int c = nchunks - 1; c > 0; --c) {             // every chunk against this round's exits
      if (!same_state(exits[c - 1], mine[c])) {
        mine[c] = exits[c - 1];
        dirty[c] = 1;
        any = true;
      }
    }
    if (!any) break;
  }
  rec->rounds = rounds;
  int32_t dcd[kBlocks];
  memset(dcd, 0, sizeof(dcd));
  bool error = false;
  int32_t last_end = -1;
  int first = 0;
  for (int c = 0; c < nchunks; ++c) {
    int32_t last = -1;
    if (!write_chunk(ln, mine[c], end[c], first, coef, dcd, &last)) error = true;
    if (last >= 0) last_end = last;
    first += nblk[c];
  }
  if (error || last_end < 0 || last_end > avail) return NDP_JPEG_CORRUPT;
  dc_sums(coef, dcd);
  return NDP_JPEG_OK;
}

// The next 16 bits at bit `pos` of the unstuffed data (zeros past it): the census reads the stream by itself.
int peek16(const std::vector<uint8_t>& data, int32_t nbytes, int32_t pos) {
  int v = 0;
  for (int i = 0; i < 3; ++i) {
    const int32_t b = (pos >> 3) + i;
    v = (v << 8) | (b < nbytes ? data[b] : 0);
  }
  return (v >> (8 - (pos & 7))) & 0xFFFF;
}

// One Lane from bit 0, block after block, no chunking.  Returns the status; fills the census.
template <bool FAR>
int entropy_serial(const uint32_t* words, const uint32_t* far, const std::vector<uint8_t>& data, int32_t nbytes,
                   const Tables& T, int16_t* coef, Record* rec) {
  const int32_t avail = nbytes * 8;
  Lane<FAR> ln = make_lane<FAR>(words, far, nbytes, T);
  ln.seek(EState{0, 0, 0});
  int32_t dcd[kBlocks];
  for (int g = 0; g < kBlocks; ++g) {
    const int mcu = g / 6, bi = g - 6 * mcu;
    const int blk = bi < 4 ? (2 * (mcu >> 3) + (bi >> 1)) * 16 + 2 * (mcu & 7) + (bi & 1) : 256 + (bi - 4) * 64 + mcu;
    for (int i = 0; i < 64; ++i) {
      // the census finds the symbol's code by itself: jdhuff.c's loop over the code lengths
      const int t = (ln.st.bp < 4 ? 0 : 2) + (ln.st.k ? 1 : 0);
      const int bits = peek16(data, nbytes, ln.st.pos);
      int clen = 0, csym = 0;
      for (int l = 1; l <= 16 && !clen; ++l) {
        const int code = bits >> (16 - l);
        if (code <= T.maxc[t * 18 + l]) {
          clen = l;
          csym = T.hval[t * 256 + ((code + T.voff[t * 18 + l]) & 255)];
        }
      }
      const bool ac = ln.st.k != 0;
      int v, zz;
      if (!ln.symbol(&v, &zz)) return NDP_JPEG_CORRUPT;
      rec->slow += clen > kLook;
      rec->zrl += ac && csym == 0xF0;
      if (zz == 0) {
        dcd[g] = v;
        int cat = 0;
        for (int a = v < 0 ? -v : v; a; a >>= 1) ++cat;
        if (cat > rec->max_dc_cat) rec->max_dc_cat = cat;
      } else if (zz > 0) {
        coef[blk * 64 + kNatural[zz]] = (int16_t)v;
        if (zz == 63) ++rec->no_eob;
      }
      if (ln.st.k == 0) break;
    }
    if (ln.st.k != 0) return NDP_JPEG_CORRUPT;
  }
  if (ln.st.pos > avail) return NDP_JPEG_CORRUPT;
  dc_sums(coef, dcd);
  for (int i = 0; i < kBlocks * 64; ++i) {
    const int a = coef[i] < 0 ? -coef[i] : coef[i];
    if (a > rec->max_abs) rec->max_abs = a;
  }
  return NDP_JPEG_OK;
}

// k_jpeg_idct and k_jpeg_color for one frame.
void pixels(const int16_t* coef, const Tables& T, uint8_t* rgb) {
  std::vector<uint8_t> planes(kPlaneBytes);
  for (int b = 0; b < kBlocks; ++b) {
    const int comp = b < 256 ? 0 : (b < 320 ? 1 : 2);
    int x[64];
    uint8_t px[64];
    for (int i = 0; i < 64; ++i) x[i] = (int)coef[b * 64 + i] * (int)T.qt[comp][i];
    idct_islow(x, px);
    uint8_t* plane = planes.data();
    int stride, by, bx;
    if (comp == 0) { stride = 128; by = b >> 4; bx = b & 15; }
    else { plane += 16384 + (comp - 1) * 4096; stride = 64; by = (b - 256 - (comp - 1) * 64) >> 3; bx = (b - 256) & 7; }
    for (int r = 0; r < 8; ++r) memcpy(plane + (by * 8 + r) * stride + bx * 8, px + 8 * r, 8);
  }
  const uint8_t* pl = planes.data();
  for (int y = 0; y < kSize; ++y)
    for (int x = 0; x < kSize; ++x) ycc_pixel(pl, pl + 16384, pl + 16384 + 4096, y, x, rgb + (y * kSize + x) * 3);
}

void decode(const uint8_t* s, int32_t len, Record* rec, uint8_t* chunked, uint8_t* serial) {
  memset(rec, 0, sizeof(*rec));
  memset(chunked, 0, kFrame);
  memset(serial, 0, kFrame);
  Tables T;
  std::vector<uint8_t> compact;
  int32_t nbytes = 0;
  const int st = parse(s, len, &T, &compact, &nbytes);
  rec->status = rec->status_serial = st;
  rec->frames_equal = 1;
  if (st != NDP_JPEG_OK) return;
  rec->ncompact = nbytes;
  // the whole unstuffed data (the workspace on the device) and its first 24 KB (LDS), each exactly as long as it is
  const int32_t nwords = (nbytes + 3) >> 2, nlds = nwords < kStreamLdsBytes / 4 ? nwords : kStreamLdsBytes / 4;
  Exact<uint32_t> far(nwords), words(nlds);
  if (nwords) {
    memcpy(far.p, compact.data(), (size_t)nwords * 4);
    memcpy(words.p, compact.data(), (size_t)nlds * 4);
  }
  std::vector<int16_t> ca(kBlocks * 64, 0), cb(kBlocks * 64, 0);
  if (nbytes <= kStreamLdsBytes) {
    rec->status = entropy_chunked<false>(words.p, far.p, nbytes, T, ca.data(), rec);
    rec->status_serial = entropy_serial<false>(words.p, far.p, compact, nbytes, T, cb.data(), rec);
  } else {
    rec->status = entropy_chunked<true>(words.p, far.p, nbytes, T, ca.data(), rec);
    rec->status_serial = entropy_serial<true>(words.p, far.p, compact, nbytes, T, cb.data(), rec);
  }
  if (rec->status == NDP_JPEG_OK) pixels(ca.data(), T, chunked);
  if (rec->status_serial == NDP_JPEG_OK) pixels(cb.data(), T, serial);
  rec->frames_equal = memcmp(chunked, serial, kFrame) == 0;
}

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  const bool with_frames = argc > 3 && strcmp(argv[3], "frames") == 0;
  int32_t n = 0;
  if (!read_pod(in, &n) || n < 0) return kBadInput;
  std::vector<uint8_t> chunked(kFrame), serial(kFrame);
  for (int32_t i = 0; i < n; ++i) {
    int32_t len = 0;
    if (!read_pod(in, &len) || len < 0 || len >= (1 << 28)) return kBadInput;
    Exact<uint8_t> s((size_t)len);
    if (!s.read(in)) return kBadInput;
    Record rec;
    decode(s.p, len, &rec, chunked.data(), serial.data());
    static_assert(kRecordInts == 12, "tests/test_jpeg_core_host.py reads 12 int32 per stream");
    fwrite(&rec, sizeof(rec), 1, out);
    if (with_frames) {
      fwrite(chunked.data(), 1, kFrame, out);
      fwrite(serial.data(), 1, kFrame, out);
    }
  }
  return close_files(in, out);
}

}  // namespace host::jpeg
