// jpeg_enc.inc -- the JPEG encoder's core (csrc/ndp_jpeg_enc.inc) run on the CPU, for
// tests/test_jpeg_encode_core_host.py.  main.hip includes it behind the library's source (see there); it calls the
// __host__ __device__ functions the kernels call (block_coefs, dc_predecessor, encode_block with BitCounter and
// BitWriter, pad_bits, stuff_chunk, entropy_byte) and reads the tables the kernels read (kT); it makes no HIP runtime
// call and needs no GPU.  What k_jpeg_enc_dct and k_jpeg_enc_pack do outside those functions is restated here, not shared,
// and is tested as a copy: the two scans, the zeroing of the bit buffer, the placement of the stuffed bytes.
// k_jpeg_enc_offsets (the scan of the frame lengths against the capacity, its tile carry) has no part here: only the GPU
// tests cover it (tests/test_gpu_jpeg_encode.py: 1,025 frames, the capacity cuts, the retry).
//
// Usage: host_driver jpeg_enc IN OUT
//   IN   int32 nf, nf x 49152 bytes (frames [128][128][3]), int32 nc, nc x 24576 int16 (coefficient sets [384][64]:
//        blocks in scan order, zig-zag order, DC as values -- what k_jpeg_enc_dct leaves in the workspace)
//   OUT  per item kRecordInts int32 (see Record), then the stream of the kernels' schedule (Record::len bytes)
// Every item is written twice.  Scheduled: k_jpeg_enc_pack's steps run serially, lane by lane (bit counts, exclusive scan,
// bits ORed into words, padding, 0xFF counts per lane, scan, stuffed bytes).  Serial: one bit writer from bit 0, block
// after block, stuffing as it goes (jchuff.c's emit_bits), with its own walk over the coefficients.  The bit buffer is
// an allocation of exactly its own size, so a sanitizer sees any access past it.
namespace host::jpeg_enc {

using namespace ndp::jpegenc;

struct Record {
  int32_t len;             // bytes of the scheduled stream
  int32_t len_serial;      // bytes of the serial stream
  int32_t equal;           // 1: the same bytes
  int32_t total_bits;      // entropy bits before padding
  int32_t entropy_bytes;   // bytes between the header and EOI (stuffing included)
  int32_t stuffed;         // 0x00 bytes inserted
  int32_t last_ff;         // 1: the last entropy byte (padded) is 0xFF, so 0x00 sits directly before EOI
  int32_t zrl;             // ZRL symbols
  int32_t eob_only;        // blocks coded as a DC symbol and EOB
  int32_t max_dc_cat;      // the largest DC category
  int32_t max_stream;      // ndp_jpeg_encode_max_stream_bytes()
  int32_t reserved;
};
constexpr int kRecordInts = sizeof(Record) / 4;
constexpr int kFrame = kSize * kSize * 3;
constexpr int kCoefs = kBlocks * 64;

template <class T>
using Exact = host::Exact<T, 16>;

// k_jpeg_enc_pack<true> for one frame's coefficients.
void scheduled(const int16_t* coef, std::vector<uint8_t>* out, Record* rec) {
  int32_t bits[kPackThreads], scan[kPackThreads], pred[kPackThreads];
  for (int t = 0; t < kPackThreads; ++t) {
    const int pg = dc_predecessor(t);
    pred[t] = pg >= 0 ? coef[pg * 64] : 0;
    const int tab = (t % 6) < 4 ? 0 : 2;
    BitCounter cnt = {0};
    encode_block(coef + t * 64, pred[t], kT.huff[tab], kT.huff[tab + 1], cnt);
    bits[t] = cnt.bits;
  }
  int32_t run = 0;
  for (int t = 0; t < kPackThreads; ++t) {
    scan[t] = run;
    run += bits[t];
  }
  const int32_t total_bits = run;
  const int32_t nbytes = (total_bits + 7) >> 3;
  const int32_t nwords = (nbytes + 3) >> 2 < kBitWords ? (nbytes + 3) >> 2 : kBitWords;
  Exact<uint32_t> words((size_t)nwords);
  for (int i = 0; i < nwords; ++i) words.p[i] = 0;
  for (int t = kPackThreads - 1; t >= 0; --t) {          // any order: OR commutes
    const int tab = (t % 6) < 4 ? 0 : 2;
    BitWriter wr;
    wr.start(words.p, nwords, scan[t]);
    encode_block(coef + t * 64, pred[t], kT.huff[tab], kT.huff[tab + 1], wr);
    wr.finish();
  }
  if (pad_bits(total_bits) && (total_bits >> 5) < nwords) words.p[total_bits >> 5] |= pad_bits(total_bits);
  const int32_t chunk = stuff_chunk(nbytes);
  int32_t ff[kPackThreads], c0[kPackThreads], c1[kPackThreads], total_ff = 0;
  for (int t = 0; t < kPackThreads; ++t) {
    c0[t] = t * chunk < nbytes ? t * chunk : nbytes;
    c1[t] = c0[t] + chunk < nbytes ? c0[t] + chunk : nbytes;
    ff[t] = 0;
    for (int32_t k = c0[t]; k < c1[t]; ++k) ff[t] += entropy_byte(words.p, k) == 0xFF;
    scan[t] = total_ff;
    total_ff += ff[t];
  }
  const int32_t len = kHeaderBytes + nbytes + total_ff + 2;
  Exact<uint8_t> stream((size_t)len);
  memset(stream.p, 0xA5, (size_t)len);
  memcpy(stream.p, kT.header, kHeaderBytes);
  for (int t = 0; t < kPackThreads; ++t) {
    int32_t o = kHeaderBytes + c0[t] + scan[t];
    for (int32_t k = c0[t]; k < c1[t]; ++k) {
      const int b = entropy_byte(words.p, k);
      stream.p[o++] = (uint8_t)b;
      if (b == 0xFF) stream.p[o++] = 0;
    }
  }
  stream.p[len - 2] = 0xFF;
  stream.p[len - 1] = 0xD9;
  out->assign(stream.p, stream.p + len);
  rec->len = len;
  rec->total_bits = total_bits;
  rec->entropy_bytes = nbytes + total_ff;
  rec->stuffed = total_ff;
  rec->last_ff = nbytes > 0 && entropy_byte(words.p, nbytes - 1) == 0xFF;
}

// jchuff.c's way: one accumulator, bytes out as they fill, a 0x00 after each 0xFF.
struct SerialWriter {
  std::vector<uint8_t>* out;
  uint32_t acc = 0;
  int fill = 0;
  void put(uint32_t code, int len) {
    for (int i = len - 1; i >= 0; --i) {
      acc = (acc << 1) | ((code >> i) & 1u);
      if (++fill == 8) {
        out->push_back((uint8_t)acc);
        if ((acc & 0xFF) == 0xFF) out->push_back(0);
        acc = 0;
        fill = 0;
      }
    }
  }
};

int category(int v) {
  int a = v < 0 ? -v : v, s = 0;
  for (; a; a >>= 1) ++s;
  return s;
}

void serial(const int16_t* coef, std::vector<uint8_t>* out, Record* rec) {
  out->assign(kT.header, kT.header + kHeaderBytes);
  SerialWriter w{out};
  int last_dc[3] = {0, 0, 0};
  for (int g = 0; g < kBlocks; ++g) {
    const int bi = g % 6, comp = bi < 4 ? 0 : bi - 3, tab = bi < 4 ? 0 : 2;
    const int16_t* zz = coef + g * 64;
    int diff = zz[0] - last_dc[comp];
    last_dc[comp] = zz[0];
    diff = diff < -2047 ? -2047 : (diff > 2047 ? 2047 : diff);
    int s = category(diff);
    if (s > rec->max_dc_cat) rec->max_dc_cat = s;
    uint32_t e = kT.huff[tab][s];
    w.put(e & 0xFFFF, (int)(e >> 16));
    if (s) w.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
    int run = 0, symbols = 0;
    for (int k = 1; k < 64; ++k) {
      int v = zz[k];
      if (v == 0) { ++run; continue; }
      while (run > 15) {
        e = kT.huff[tab + 1][0xF0];
        w.put(e & 0xFFFF, (int)(e >> 16));
        run -= 16;
        ++rec->zrl;
        ++symbols;
      }
      v = v < -1023 ? -1023 : (v > 1023 ? 1023 : v);
      s = category(v);
      e = kT.huff[tab + 1][(run << 4) | s];
      w.put(e & 0xFFFF, (int)(e >> 16));
      w.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
      run = 0;
      ++symbols;
    }
    if (run > 0) {
      e = kT.huff[tab + 1][0];
      w.put(e & 0xFFFF, (int)(e >> 16));
      if (symbols == 0) ++rec->eob_only;
    }
  }
  if (w.fill) w.put((1u << (8 - w.fill)) - 1, 8 - w.fill);
  out->push_back(0xFF);
  out->push_back(0xD9);
  rec->len_serial = (int32_t)out->size();
}

void encode(const int16_t* coef, FILE* out) {
  Record rec;
  memset(&rec, 0, sizeof(rec));
  std::vector<uint8_t> a, b;
  scheduled(coef, &a, &rec);
  serial(coef, &b, &rec);
  rec.equal = a == b;
  rec.max_stream = (int32_t)ndp_jpeg_encode_max_stream_bytes();
  static_assert(kRecordInts == 12, "tests/jpeg_enc_core_host.py reads 12 int32 per item");
  fwrite(&rec, sizeof(rec), 1, out);
  fwrite(a.data(), 1, a.size(), out);
}

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  int32_t nf = 0, nc = 0;
  if (!read_pod(in, &nf) || nf < 0) return kBadInput;
  Exact<uint8_t> frame(kFrame);
  Exact<int16_t> coef(kCoefs);
  for (int32_t i = 0; i < nf; ++i) {
    if (!frame.read(in)) return kBadInput;
    for (int g = 0; g < kBlocks; ++g) block_coefs(frame.p, g, coef.p + g * 64);      // k_jpeg_enc_dct
    encode(coef.p, out);
  }
  if (!read_pod(in, &nc) || nc < 0) return kBadInput;
  for (int32_t i = 0; i < nc; ++i) {
    if (!coef.read(in)) return kBadInput;
    encode(coef.p, out);
  }
  return close_files(in, out);
}

}  // namespace host::jpeg_enc
