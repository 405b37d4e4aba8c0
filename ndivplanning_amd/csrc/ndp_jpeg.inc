// ndp_jpeg.inc -- device-side JPEG decode of the trajectory frames (generate_trajectories.py:113-122 of the reference:
// PIL, quality 95, 4:2:0, 128x128), bit-identical to PIL (libjpeg-turbo: islow IDCT, fancy h2v2 upsampling, fixed-point
// YCbCr -> RGB).  Four launches per batch:
//   k_jpeg_parse    one workgroup per frame: lane 0 walks the markers (SOI .. SOS) and keeps the DQT / DHT contents in
//                   LDS; the workgroup then builds the frame's descriptor (quantisation tables per component, 9-bit
//                   Huffman lookahead tables, the slow-path tables), finds the marker that ends the entropy data and
//                   writes the data with its 0xFF00 stuffing removed, word-aligned, into the workspace
//   k_jpeg_entropy  one workgroup per frame, its tables and unstuffed data staged in LDS: the bit stream is decoded
//                   in up to 256 chunks in parallel by self-synchronising subsequences (see EState below), a scan of
//                   the blocks per chunk places them, a last pass writes the coefficients (natural order, int16), and
//                   a segmented scan turns the DC differences into values
//   k_jpeg_idct     one thread per 8x8 block: dequantise + libjpeg's integer islow IDCT into the Y / Cb / Cr planes
//   k_jpeg_color    one thread per output pixel: libjpeg-turbo's h2v2 "fancy" (triangular) chroma upsampling and the
//                   fixed-point YCbCr -> RGB tables, [n][128][128][3] bytes; a frame with a nonzero status gets zeros
// Reads stay inside [offsets[i], offsets[i+1]), writes inside frame i's slices; every loop has a fixed bound.  Integer
// arithmetic only, no atomics outside LDS: two runs give the same bits.  Included at the end of ndp_kernels.hip.

namespace ndp {
namespace jpeg {

constexpr int kSize = 128;                     // frame height and width
constexpr int kBlocks = 384;                   // 64 MCUs x (4 Y + Cb + Cr)
constexpr int kLook = 9;                       // lookahead bits of the Huffman tables
constexpr int kDescBytes = 6144;
constexpr int kCoefBytes = kBlocks * 64 * 2;
constexpr int kPlaneBytes = kSize * kSize + 2 * (kSize / 2) * (kSize / 2);
constexpr int64_t kFrameBytes = (int64_t)kDescBytes + kCoefBytes + kPlaneBytes;
constexpr int64_t kMaxImages = 65536;
constexpr int kParseThreads = 256;
constexpr int kStage = 2048;                   // stream bytes staged in LDS for the header walk
constexpr int kEntropyThreads = 256;           // k_jpeg_entropy: one workgroup per frame, one lane per chunk
constexpr int kStreamLdsBytes = 24576;         // entropy bytes per frame held in LDS (larger streams read the rest)
constexpr int kMinChunkBits = 128;             // chunks are at least this long (and a multiple of 32 bits)
constexpr int kMaxSegments = 256;              // marker segments walked before SOS

// zig-zag index -> natural (row-major) index
constexpr uint8_t kNatural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Per-frame descriptor in the workspace.  Huffman tables: 0 Y DC, 1 Y AC, 2 chroma DC, 3 chroma AC.
struct Desc {
  int32_t status;
  int32_t ncompact;                            // entropy bytes after unstuffing
  int64_t cstart;                              // their offset in the workspace's stream area (4-byte aligned)
  uint16_t qt[3][64];                          // per component, natural order
  uint16_t lut[4][1 << kLook];                 // (code length << 8) | symbol; 0: longer than kLook bits or no code
  int32_t maxcode[4][18];                      // largest code of each length, -1 if none (libjpeg's jdhuff.c)
  int32_t valoff[4][18];                       // huffval index of a length-l code = code + valoff[l]
  uint8_t huffval[4][256];
};
static_assert(sizeof(Desc) <= kDescBytes, "descriptor outgrew its slot");

// What lane 0 gathers from the headers (LDS).
struct Header {
  uint16_t qt[4][64];                          // DQT slots, natural order
  uint8_t bits[8][17];                         // DHT slots (class * 4 + id): counts per length 1..16
  uint8_t vals[8][256];
  uint8_t qt_set, ht_set;                      // bit masks of the slots defined
  uint8_t tq[3], td[3], ta[3];                 // per component: quantisation and Huffman table slots
  int32_t sos_end;                             // first byte of the entropy data (relative to the stream)
};

__host__ __device__ inline int rd(const uint8_t* stage, const uint8_t* s, int64_t p) {
  return p < kStage ? stage[p] : s[p];
}

// The rules of the entropy data [e0, mark) of a stream of `len` bytes, shared by k_jpeg_parse and the host driver of the
// tests (tests/jpeg_host_driver.hip).  A marker: a 0xFF not followed by 0x00 (fill bytes and a 0xFF that ends the stream
// included); the first one at or after e0 ends the data.
__host__ __device__ inline bool marker_at(const uint8_t* stage, const uint8_t* s, int32_t p, int32_t len) {
  return rd(stage, s, p) == 0xFF && (p + 1 >= len || rd(stage, s, p + 1) != 0x00);
}

// A stuffed byte: the 0x00 after a 0xFF of the data; unstuffing drops it.
__host__ __device__ inline bool stuffed_at(const uint8_t* stage, const uint8_t* s, int32_t p, int32_t e0) {
  return p > e0 && rd(stage, s, p) == 0x00 && rd(stage, s, p - 1) == 0xFF;
}

// The data must end at EOI, after any fill bytes (a truncated stream, or another marker inside the scan, is corrupt).
__host__ __device__ inline bool eoi_at(const uint8_t* stage, const uint8_t* s, int32_t mark, int32_t len) {
  int32_t p = mark;
  for (int fill = 0; fill < 64 && p < len && rd(stage, s, p) == 0xFF; ++fill) ++p;
  return p > mark && p < len && rd(stage, s, p) == 0xD9;
}

// The marker walk SOI .. SOS.  Returns an NDP_JPEG_* status; on NDP_JPEG_OK, h describes the frame.  `stage` holds the
// first min(len, kStage) bytes of `s` (the same bytes: it only saves global reads).
__host__ __device__ inline int parse_headers(const uint8_t* stage, const uint8_t* s, int64_t len, Header* h) {
  h->qt_set = 0;
  h->ht_set = 0;
  if (len < 4 || rd(stage, s, 0) != 0xFF || rd(stage, s, 1) != 0xD8) return NDP_JPEG_CORRUPT;
  int64_t p = 2;
  bool sof = false;
  uint8_t cid[3] = {0, 0, 0};
  for (int seg = 0; seg < kMaxSegments; ++seg) {
    if (p + 4 > len || rd(stage, s, p) != 0xFF) return NDP_JPEG_CORRUPT;
    int m = 0xFF;
    for (int fill = 0; fill < 64 && m == 0xFF; ++fill) {        // fill bytes before a marker
      ++p;
      if (p >= len) return NDP_JPEG_CORRUPT;
      m = rd(stage, s, p);
    }
    ++p;
    if (m == 0xFF || m == 0x00 || m == 0x01 || m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7)) return NDP_JPEG_CORRUPT;
    if (p + 2 > len) return NDP_JPEG_CORRUPT;
    const int seglen = (rd(stage, s, p) << 8) | rd(stage, s, p + 1);
    if (seglen < 2 || p + seglen > len) return NDP_JPEG_CORRUPT;
    const int64_t q0 = p + 2, qe = p + seglen;                  // segment body [q0, qe)
    if (m == 0xC0 || m == 0xC1) {                                // baseline / extended sequential, Huffman
      if (sof || seglen < 8) return NDP_JPEG_CORRUPT;
      sof = true;
      const int prec = rd(stage, s, q0);
      const int hgt = (rd(stage, s, q0 + 1) << 8) | rd(stage, s, q0 + 2);
      const int wid = (rd(stage, s, q0 + 3) << 8) | rd(stage, s, q0 + 4);
      const int nf = rd(stage, s, q0 + 5);
      if (seglen != 8 + 3 * nf) return NDP_JPEG_CORRUPT;
      if (prec != 8 || nf != 3) return NDP_JPEG_UNSUPPORTED;
      for (int c = 0; c < 3; ++c) {
        cid[c] = (uint8_t)rd(stage, s, q0 + 6 + 3 * c);
        const int hv = rd(stage, s, q0 + 7 + 3 * c);
        const int tq = rd(stage, s, q0 + 8 + 3 * c);
        if (hv != (c == 0 ? 0x22 : 0x11)) return NDP_JPEG_UNSUPPORTED;
        if (tq > 3) return NDP_JPEG_CORRUPT;
        h->tq[c] = (uint8_t)tq;
      }
      if (cid[0] == cid[1] || cid[0] == cid[2] || cid[1] == cid[2]) return NDP_JPEG_CORRUPT;
      if (hgt != kSize || wid != kSize) return NDP_JPEG_SIZE;
    } else if (m == 0xDB) {                                      // DQT
      int64_t q = q0;
      for (int t = 0; t < 4 && q < qe; ++t) {
        const int pq = rd(stage, s, q) >> 4, id = rd(stage, s, q) & 15;
        if (pq > 1 || id > 3 || q + 1 + 64 * (pq + 1) > qe) return NDP_JPEG_CORRUPT;
        for (int k = 0; k < 64; ++k) {
          const int v = pq ? (rd(stage, s, q + 1 + 2 * k) << 8) | rd(stage, s, q + 2 + 2 * k) : rd(stage, s, q + 1 + k);
          h->qt[id][kNatural[k]] = (uint16_t)v;
        }
        h->qt_set |= (uint8_t)(1 << id);
        q += 1 + 64 * (pq + 1);
      }
      if (q != qe) return NDP_JPEG_CORRUPT;
    } else if (m == 0xC4) {                                      // DHT
      int64_t q = q0;
      for (int t = 0; t < 8 && q < qe; ++t) {
        const int tc = rd(stage, s, q) >> 4, th = rd(stage, s, q) & 15;
        if (tc > 1 || th > 3 || q + 17 > qe) return NDP_JPEG_CORRUPT;
        const int slot = tc * 4 + th;
        int total = 0;
        h->bits[slot][0] = 0;
        for (int l = 1; l <= 16; ++l) {
          h->bits[slot][l] = (uint8_t)rd(stage, s, q + l);
          total += h->bits[slot][l];
        }
        if (total > 256 || q + 17 + total > qe) return NDP_JPEG_CORRUPT;
        for (int i = 0; i < total; ++i) h->vals[slot][i] = (uint8_t)rd(stage, s, q + 17 + i);
        h->ht_set |= (uint8_t)(1 << slot);
        q += 17 + total;
      }
      if (q != qe) return NDP_JPEG_CORRUPT;
    } else if (m == 0xDD) {                                      // DRI: restart intervals are not supported
      if (seglen != 4) return NDP_JPEG_CORRUPT;
      if (((rd(stage, s, q0) << 8) | rd(stage, s, q0 + 1)) != 0) return NDP_JPEG_UNSUPPORTED;
    } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {         // APPn, COM: skipped
    } else if (m == 0xDA) {                                      // SOS
      if (!sof || seglen < 8) return NDP_JPEG_CORRUPT;
      const int ns = rd(stage, s, q0);
      if (seglen != 6 + 2 * ns) return NDP_JPEG_CORRUPT;
      if (ns != 3) return NDP_JPEG_UNSUPPORTED;                 // one interleaved scan only
      for (int c = 0; c < 3; ++c) {
        if (rd(stage, s, q0 + 1 + 2 * c) != cid[c]) return NDP_JPEG_UNSUPPORTED;
        const int t = rd(stage, s, q0 + 2 + 2 * c);
        h->td[c] = (uint8_t)(t >> 4);
        h->ta[c] = (uint8_t)(t & 15);
        if (h->td[c] > 3 || h->ta[c] > 3) return NDP_JPEG_CORRUPT;
      }
      if (rd(stage, s, q0 + 7) != 0 || rd(stage, s, q0 + 8) != 63 || rd(stage, s, q0 + 9) != 0) return NDP_JPEG_CORRUPT;
      // the chroma components share their Huffman tables (every PIL stream does)
      if (h->td[1] != h->td[2] || h->ta[1] != h->ta[2]) return NDP_JPEG_UNSUPPORTED;
      for (int c = 0; c < 3; ++c) {
        if (!(h->qt_set >> h->tq[c] & 1) || !(h->ht_set >> h->td[c] & 1) || !(h->ht_set >> (4 + h->ta[c]) & 1))
          return NDP_JPEG_CORRUPT;
      }
      h->sos_end = (int32_t)qe;
      return NDP_JPEG_OK;
    } else {                                                     // progressive, arithmetic, lossless, hierarchical ...
      return NDP_JPEG_UNSUPPORTED;
    }
    p = qe;
  }
  return NDP_JPEG_CORRUPT;
}

// jdhuff.c's derived tables for slot `slot` of h: maxcode / valoff / huffval.  Returns false where jdhuff.c raises
// JERR_BAD_HUFF_TABLE: an over-subscribed table, an all-ones code, a DC symbol above 15.
__host__ __device__ inline bool derive_table(const Header* h, int slot, bool dc, int32_t* maxcode, int32_t* valoff,
                                             uint8_t* huffval) {
  int code = 0, k = 0;
  maxcode[0] = -1;
  valoff[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = h->bits[slot][l];
    valoff[l] = k - code;
    k += cnt;
    code += cnt;
    if (code >= (1 << l)) return false;              // no code may be all ones (jdhuff.c)
    maxcode[l] = cnt ? code - 1 : -1;
    code <<= 1;
  }
  maxcode[17] = 0x7FFFFFFF;
  valoff[17] = 0;
  for (int i = 0; i < 256; ++i) {
    huffval[i] = i < k ? h->vals[slot][i] : 0;
    if (dc && i < k && huffval[i] > 15) return false;
  }
  return true;
}

// Lookahead entry e (the next kLook bits of the stream, MSB first) of a derived table.
__host__ __device__ inline uint16_t lut_entry(const int32_t* maxcode, const int32_t* valoff, const uint8_t* huffval,
                                              int e) {
  for (int l = 1; l <= kLook; ++l) {
    const int code = e >> (kLook - l);
    if (code <= maxcode[l] && code + valoff[l] >= 0) {
      // codes of length l are [maxcode - count + 1, maxcode]; a shorter prefix was not a code, so code >= mincode
      return (uint16_t)((l << 8) | huffval[code + valoff[l]]);
    }
  }
  return 0;
}

// Entropy decoding of one frame by self-synchronising subsequences (Klein & Wiseman 2003; Weissenberger & Schmidt
// 2018).  The unstuffed bits are cut into chunks; the decoder state at a symbol boundary is (bit position, zig-zag index
// k -- 0: a DC symbol is next --, block within the MCU).  Lane c decodes the symbols that start in chunk c from an entry
// state; the first boundary at or after the chunk's end is its exit state, the next chunk's entry.  Chunk 0's entry is
// exact; the others start from a guess (their first bit, k 0, block 0) and are decoded again from the previous exit
// until no entry changes, so every entry is exact by induction; garbage decoded from a wrong guess only delays that.
// A scan of the blocks each chunk starts places them, and a last pass decodes each block once more and writes it.
struct EState {
  int32_t pos;                                   // bit position in the unstuffed data
  int32_t k;                                     // zig-zag index of the next symbol within the block (0: DC)
  int32_t bp;                                    // block within the MCU: 0..3 Y, 4 Cb, 5 Cr
};

__host__ __device__ inline bool same_state(const EState& a, const EState& b) {
  return a.pos == b.pos && a.k == b.k && a.bp == b.bp;
}

// Chunk length in bits for `avail` bits of unstuffed data: at most kEntropyThreads chunks, each a multiple of 32 bits
// and at least kMinChunkBits long.
__host__ __device__ inline int32_t chunk_bits(int32_t avail) {
  const int32_t even = ((avail + kEntropyThreads - 1) / kEntropyThreads + 31) & ~31;
  return even > kMinChunkBits ? even : kMinChunkBits;
}

// The one-lane bit reader and symbol loop: a 64-bit MSB-first buffer refilled a word at a time, the next word already
// loaded.  `words` (LDS on the device) holds the first `split` words; a stream longer than that reads the rest from `far`
// (FAR = true; a separate instantiation, so the common one has no global load whose wait would also wait for the
// block stores in flight).  Words past the data read as zero.
template <bool FAR>
struct Lane {
  const uint32_t* words; int32_t split; const uint32_t* far; int32_t nwords;
  const uint16_t* lut; const int32_t* maxcode; const int32_t* valoff; const uint8_t* huffval;
  uint64_t buf, next;
  int cnt;                                       // valid bits in buf
  int32_t wpos;                                  // index of the word in `next`
  EState st;

  __host__ __device__ uint64_t load(int32_t w) const {
    const uint32_t v = (w >= 0 && w < nwords) ? ((!FAR || w < split) ? words[w] : far[w]) : 0u;
    return (uint64_t)__builtin_bswap32(v);
  }
  __host__ __device__ void seek(const EState& e) {
    st = e;
    const int32_t w = e.pos >> 5, off = e.pos & 31;
    buf = ((load(w) << 32) | load(w + 1)) << off;
    cnt = 64 - off;
    wpos = w + 2;
    next = load(wpos);
  }
  // One symbol: returns false for a code that is not in the table or a coefficient past the block; on success st is
  // advanced, *v is the coefficient and *zz its zig-zag index (-1 for EOB / ZRL, which write nothing).
  __host__ __device__ bool symbol(int* v, int* zz) {
    if (cnt < 32) {                              // at most 16 code bits + 15 value bits per symbol
      buf |= next << (32 - cnt);
      cnt += 32;
      ++wpos;
      next = load(wpos);
    }
    const int t = (st.bp < 4 ? 0 : 2) + (st.k ? 1 : 0);
    const uint16_t e = lut[t * (1 << kLook) + (int)(buf >> (64 - kLook))];
    int len = e >> 8, sym = e & 255;
    if (!e) {                                    // codes longer than kLook bits
      for (int l = kLook + 1; l <= 16; ++l) {
        const int code = (int)(buf >> (64 - l));
        if (code <= maxcode[t * 18 + l]) {
          len = l;
          sym = huffval[t * 256 + ((code + valoff[t * 18 + l]) & 255)];
          break;
        }
      }
      if (len == 0) return false;
    }
    buf <<= len;
    cnt -= len;
    const int r = sym >> 4, sz = sym & 15;
    int val = 0;
    if (sz) {
      const int bits = (int)(buf >> (64 - sz));
      buf <<= sz;
      cnt -= sz;
      val = bits < (1 << (sz - 1)) ? bits - (1 << sz) + 1 : bits;
    }
    st.pos += len + sz;
    *v = val;
    *zz = -1;
    if (st.k == 0) {
      if (sym > 11) return false;
      *zz = 0;
      st.k = 1;
      return true;
    }
    if (sz) {
      st.k += r;
      if (st.k > 63) return false;
      *zz = st.k;
      ++st.k;
    } else if (r == 15) {
      st.k += 16;
    } else {
      st.k = 64;                                 // EOB
    }
    if (st.k >= 64) {
      st.k = 0;
      st.bp = st.bp == 5 ? 0 : st.bp + 1;
    }
    return true;
  }
};

// Sync pass of one chunk: from `entry`, the symbols that start before `end`; returns the exit state and the number of
// blocks whose DC symbol starts in the chunk.  An undecodable symbol (a wrong guess, or corrupt data: the write pass
// tells them apart) restarts the guess one bit further on.
template <bool FAR>
__host__ __device__ inline EState sync_chunk(Lane<FAR>& ln, const EState& entry, int32_t end, int* nblk) {
  ln.seek(entry);
  int blocks = 0;
  for (int it = 0; it < end - entry.pos + 1 && ln.st.pos < end; ++it) {   // every symbol takes at least one bit
    int v, zz;
    const int32_t at = ln.st.pos;
    const bool dc = ln.st.k == 0;
    if (!ln.symbol(&v, &zz)) {
      const EState g = {at + 1, 0, ln.st.bp};
      ln.seek(g);
    } else if (dc) {
      ++blocks;
    }
  }
  *nblk = blocks;
  return ln.st;
}

// Write pass of one chunk from its exact entry: skips the tail of a block begun in the previous chunk, then decodes each
// block that starts before `end` (first global index `first`; blocks from 384 on are past the frame) to its end and
// writes it, natural order, not dequantised, DC as the difference (into dcd, decode order).  Returns false on a
// decoding error inside a block of the frame; *last_end: where block 383 ended, if this chunk wrote it.
template <bool FAR>
__host__ __device__ inline bool write_chunk(Lane<FAR>& ln, const EState& entry, int32_t end, int first, int16_t* coef,
                                            int32_t* dcd, int32_t* last_end) {
  ln.seek(entry);
  int v, zz;
  for (int i = 0; i < 64 && ln.st.k != 0; ++i) {
    if (!ln.symbol(&v, &zz)) return first >= kBlocks;      // the previous chunk's block: it reports the error
  }
  for (int g = first; g < kBlocks && ln.st.pos < end; ++g) {
    const int mcu = g / 6, bi = g - 6 * mcu;
    const int blk = bi < 4 ? (2 * (mcu >> 3) + (bi >> 1)) * 16 + 2 * (mcu & 7) + (bi & 1) : 256 + (bi - 4) * 64 + mcu;
    int4* dst = reinterpret_cast<int4*>(coef + blk * 64);
    for (int i = 0; i < 8; ++i) dst[i] = make_int4(0, 0, 0, 0);
    for (int i = 0; i < 64; ++i) {
      if (!ln.symbol(&v, &zz)) return false;
      if (zz == 0) dcd[g] = v;
      else if (zz > 0) coef[blk * 64 + kNatural[zz]] = (int16_t)v;
      if (ln.st.k == 0) break;
    }
    if (ln.st.k != 0) return false;
    if (g == kBlocks - 1) *last_end = ln.st.pos;
  }
  return true;
}

// libjpeg's jidctint.c (islow), CONST_BITS 13, PASS1_BITS 2; the output clamp of libjpeg-turbo's SIMD IDCT.  The sums
// and products are taken modulo 2^32 (unsigned, then an arithmetic shift of the same bits): the same results wherever
// jidctint.c's int arithmetic is defined, i.e. for every stream an encoder writes, and defined results for the
// coefficients of a corrupt one (any int16 times any uint16).
#define NDP_JPEG_IDCT_1D(I0, I1, I2, I3, I4, I5, I6, I7, O0, O1, O2, O3, O4, O5, O6, O7, RND, SH)   \
  do {                                                                                             \
    typedef uint32_t U;                                                                            \
    U z2 = (U)(I2), z3 = (U)(I6);                                                                  \
    U z1 = (z2 + z3) * 4433u;                                                                      \
    U tmp2 = z1 + z3 * (U)-15137, tmp3 = z1 + z2 * 6270u;                                          \
    z2 = (U)(I0); z3 = (U)(I4);                                                                    \
    U tmp0 = (z2 + z3) * 8192u, tmp1 = (z2 - z3) * 8192u;                                          \
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;    \
    tmp0 = (U)(I7); tmp1 = (U)(I5); tmp2 = (U)(I3); tmp3 = (U)(I1);                                \
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;                                          \
    U z4 = tmp1 + tmp3;                                                                            \
    const U z5 = (z3 + z4) * 9633u;                                                                \
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;                                 \
    z1 *= (U)-7373; z2 *= (U)-20995; z3 *= (U)-16069; z4 *= (U)-3196;                              \
    z3 += z5; z4 += z5;                                                                            \
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;                            \
    O0 = (int)(tmp10 + tmp3 + (U)(RND)) >> (SH); O7 = (int)(tmp10 - tmp3 + (U)(RND)) >> (SH);      \
    O1 = (int)(tmp11 + tmp2 + (U)(RND)) >> (SH); O6 = (int)(tmp11 - tmp2 + (U)(RND)) >> (SH);      \
    O2 = (int)(tmp12 + tmp1 + (U)(RND)) >> (SH); O5 = (int)(tmp12 - tmp1 + (U)(RND)) >> (SH);      \
    O3 = (int)(tmp13 + tmp0 + (U)(RND)) >> (SH); O4 = (int)(tmp13 - tmp0 + (U)(RND)) >> (SH);      \
  } while (0)

__host__ __device__ inline uint8_t clamp_u8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// One block: x = dequantised coefficients (natural order) in, 64 samples out (row-major).
__host__ __device__ inline void idct_islow(int* x, uint8_t* px) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {                      // pass 1: columns, into x (scaled by 2^PASS1_BITS)
    NDP_JPEG_IDCT_1D(x[c], x[8 + c], x[16 + c], x[24 + c], x[32 + c], x[40 + c], x[48 + c], x[56 + c],
                     x[c], x[8 + c], x[16 + c], x[24 + c], x[32 + c], x[40 + c], x[48 + c], x[56 + c],
                     1 << 10, 11);
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {                      // pass 2: rows, descaled by CONST_BITS + PASS1_BITS + 3
    int* w = x + 8 * r;
    int o0, o1, o2, o3, o4, o5, o6, o7;
    NDP_JPEG_IDCT_1D(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o0, o1, o2, o3, o4, o5, o6, o7, 1 << 17, 18);
    px[8 * r + 0] = clamp_u8(o0 + 128); px[8 * r + 1] = clamp_u8(o1 + 128);
    px[8 * r + 2] = clamp_u8(o2 + 128); px[8 * r + 3] = clamp_u8(o3 + 128);
    px[8 * r + 4] = clamp_u8(o4 + 128); px[8 * r + 5] = clamp_u8(o5 + 128);
    px[8 * r + 6] = clamp_u8(o6 + 128); px[8 * r + 7] = clamp_u8(o7 + 128);
  }
}
#undef NDP_JPEG_IDCT_1D

// Output pixel (y, x) of a decoded frame from its planes Y [128][128], Cb / Cr [64][64]: jdsample.c h2v2_fancy_upsample
// (the nearer chroma row weighs 3, the farther 1, edges replicated, bias 8 on even columns and 7 on odd ones) and
// jdcolor.c ycc_rgb_convert (SCALEBITS 16).
__host__ __device__ inline void ycc_pixel(const uint8_t* yp, const uint8_t* cbp, const uint8_t* crp, int y, int x,
                                          uint8_t* rgb) {
  const int ci = y >> 1, cj = x >> 1;
  const int rn = (y & 1) ? (ci < 63 ? ci + 1 : 63) : (ci > 0 ? ci - 1 : 0);
  const int cn = (x & 1) ? (cj < 63 ? cj + 1 : 63) : (cj > 0 ? cj - 1 : 0);
  const int bias = (x & 1) ? 7 : 8;
  const int cb = (3 * (3 * cbp[ci * 64 + cj] + cbp[rn * 64 + cj]) + 3 * cbp[ci * 64 + cn] + cbp[rn * 64 + cn] + bias) >> 4;
  const int cr = (3 * (3 * crp[ci * 64 + cj] + crp[rn * 64 + cj]) + 3 * crp[ci * 64 + cn] + crp[rn * 64 + cn] + bias) >> 4;
  const int yy = yp[y * 128 + x];
  const int xr = cr - 128, xb = cb - 128;
  // FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554, ONE_HALF = 1 << 15
  const int r_off = (91881 * xr + 32768) >> 16;
  const int b_off = (116130 * xb + 32768) >> 16;
  const int g_off = (-46802 * xr + (-22554 * xb + 32768)) >> 16;
  rgb[0] = clamp_u8(yy + r_off);
  rgb[1] = clamp_u8(yy + g_off);
  rgb[2] = clamp_u8(yy + b_off);
}

struct Layout {
  Desc* desc;
  int16_t* coef;
  uint8_t* planes;
  uint8_t* compact;
  int64_t compact_bytes;
};

__host__ __device__ inline int64_t fixed_bytes(int64_t n) { return n * kFrameBytes; }

__host__ __device__ inline int64_t compact_need(int64_t n, int64_t stream_bytes) {
  return (stream_bytes + 4 * n + 8 + 255) / 256 * 256;
}

inline Layout layout(void* ws, int64_t ws_bytes, int64_t n) {
  uint8_t* b = static_cast<uint8_t*>(ws);
  Layout L;
  L.desc = reinterpret_cast<Desc*>(b);
  L.coef = reinterpret_cast<int16_t*>(b + n * kDescBytes);
  L.planes = b + n * (kDescBytes + (int64_t)kCoefBytes);
  L.compact = b + fixed_bytes(n);
  L.compact_bytes = ws_bytes - fixed_bytes(n);
  return L;
}

}  // namespace jpeg

__global__ __launch_bounds__(jpeg::kParseThreads) void k_jpeg_parse(const uint8_t* __restrict__ streams,
                                                                     const int64_t* __restrict__ offsets,
                                                                     jpeg::Layout L) {
  using namespace jpeg;
  __shared__ uint8_t stage[kStage];
  __shared__ Header h;
  __shared__ int32_t maxc[4][18], voff[4][18];
  __shared__ uint8_t hval[4][256];
  __shared__ int32_t s_status, s_mark;
  __shared__ int32_t s_scan[kParseThreads];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x;
  const int64_t beg = offsets[f], end = offsets[f + 1], o0 = offsets[0];
  Desc* d = L.desc + f;
  const bool sane = end >= beg && beg >= o0 && end - beg < (1 << 28);
  const int64_t len = sane ? end - beg : 0;
  const uint8_t* s = streams + beg;
  const int nstage = (int)(len < kStage ? len : kStage);
  for (int i = tid; i < nstage; i += kParseThreads) stage[i] = s[i];
  __syncthreads();
  if (tid == 0) {
    int st = sane ? parse_headers(stage, s, len, &h) : NDP_JPEG_CORRUPT;
    const int64_t cstart = ((beg - o0) + 4 * f + 3) & ~(int64_t)3;
    if (st == NDP_JPEG_OK && cstart + len + 4 > L.compact_bytes) st = NDP_JPEG_WORKSPACE;
    d->cstart = cstart;
    s_status = st;
    s_mark = (int32_t)len;
  }
  __syncthreads();
  if (s_status != NDP_JPEG_OK) {
    if (tid == 0) d->status = s_status;
    return;
  }
  if (tid < 4) {
    const int slot = (tid & 1) ? 4 + h.ta[tid >> 1 ? 1 : 0] : h.td[tid >> 1 ? 1 : 0];
    if (!derive_table(&h, slot, (tid & 1) == 0, maxc[tid], voff[tid], hval[tid])) atomicExch(&s_status, NDP_JPEG_CORRUPT);
  }
  for (int i = tid; i < 3 * 64; i += kParseThreads) d->qt[i >> 6][i & 63] = h.qt[h.tq[i >> 6]][i & 63];
  // the marker that ends the entropy data: the first 0xFF not followed by 0x00 (fill bytes included)
  const int32_t e0 = h.sos_end;
  const int32_t span = (int32_t)len - e0;
  const int32_t chunk = (span + kParseThreads - 1) / kParseThreads;
  const int32_t c0 = e0 + tid * chunk, c1 = c0 + chunk < (int32_t)len ? c0 + chunk : (int32_t)len;
  for (int32_t p = c0; p < c1; ++p) {
    if (marker_at(stage, s, p, (int32_t)len)) {
      atomicMin(&s_mark, p);
      break;
    }
  }
  __syncthreads();
  if (s_status != NDP_JPEG_OK) {
    if (tid == 0) d->status = s_status;
    return;
  }
  for (int i = tid; i < 4 * (1 << kLook); i += kParseThreads) {
    const int t = i >> kLook;
    d->lut[t][i & ((1 << kLook) - 1)] = lut_entry(maxc[t], voff[t], hval[t], i & ((1 << kLook) - 1));
  }
  for (int i = tid; i < 4 * 18; i += kParseThreads) {
    d->maxcode[i / 18][i % 18] = maxc[i / 18][i % 18];
    d->valoff[i / 18][i % 18] = voff[i / 18][i % 18];
  }
  for (int i = tid; i < 4 * 256; i += kParseThreads) d->huffval[i >> 8][i & 255] = hval[i >> 8][i & 255];
  // unstuff [e0, mark): drop the 0x00 after each 0xFF; a block-wide exclusive scan places each thread's bytes
  const int32_t mark = s_mark;
  const int32_t u1 = c1 < mark ? c1 : mark;
  int32_t keep = 0;
  for (int32_t p = c0; p < u1; ++p) keep += !stuffed_at(stage, s, p, e0);
  s_scan[tid] = keep;
  __syncthreads();
  for (int off = 1; off < kParseThreads; off <<= 1) {
    const int32_t v = tid >= off ? s_scan[tid - off] : 0;
    __syncthreads();
    s_scan[tid] += v;
    __syncthreads();
  }
  uint8_t* out = L.compact + d->cstart;
  int32_t o = s_scan[tid] - keep;
  for (int32_t p = c0; p < u1; ++p) {
    if (!stuffed_at(stage, s, p, e0)) out[o++] = (uint8_t)rd(stage, s, p);
  }
  if (tid == kParseThreads - 1) {
    const int32_t total = s_scan[tid];
    for (int32_t p = total; p < ((total + 3) & ~3); ++p) out[p] = 0;      // the last word's tail
    d->ncompact = total;
    d->status = eoi_at(stage, s, mark, (int32_t)len) ? NDP_JPEG_OK : NDP_JPEG_CORRUPT;
  }
}

template <bool FAR>
__device__ inline void entropy_frame(const jpeg::Layout& L, jpeg::Desc* d, int64_t f, const uint32_t* words,
                                     const uint16_t* lut, const int32_t* maxc, const int32_t* voff, const uint8_t* hval,
                                     jpeg::EState* exits, int32_t* cnt, int32_t* dcd, int32_t* flags) {
  using namespace jpeg;
  const int c = threadIdx.x;
  const int32_t nbytes = d->ncompact;
  const int32_t avail = nbytes * 8;
  const int32_t chunk = chunk_bits(avail);
  const int nchunks = (avail + chunk - 1) / chunk;
  const int32_t end = min((c + 1) * chunk, avail);
  Lane<FAR> ln{words, kStreamLdsBytes / 4, reinterpret_cast<const uint32_t*>(L.compact + d->cstart), (nbytes + 3) >> 2,
               lut, maxc, voff, hval};
  EState mine = {c * chunk, 0, 0};
  int nblk = 0;
  bool dirty = c < nchunks;
  // sync rounds: after round r the entries of chunks 0..r are exact, so nchunks + 1 rounds always suffice
  for (int round = 0; round <= nchunks; ++round) {
    if (dirty) exits[c] = sync_chunk(ln, mine, end, &nblk);
    dirty = false;
    if (c == 0) flags[round & 1] = 0;
    __syncthreads();
    if (c > 0 && c < nchunks && !same_state(exits[c - 1], mine)) {
      mine = exits[c - 1];
      dirty = true;
      flags[round & 1] = 1;
    }
    __syncthreads();
    if (!flags[round & 1]) break;
  }
  // block index of each chunk's first block: exclusive scan of the counts
  cnt[c] = c < nchunks ? nblk : 0;
  __syncthreads();
  for (int off = 1; off < kEntropyThreads; off <<= 1) {
    const int32_t v = c >= off ? cnt[c - off] : 0;
    __syncthreads();
    cnt[c] += v;
    __syncthreads();
  }
  const int first = cnt[c] - (c < nchunks ? nblk : 0);
  if (c == 0) {
    flags[2] = 0;                                          // decoding error
    flags[3] = -1;                                         // where block 383 ended
  }
  __syncthreads();
  int16_t* coef = L.coef + f * (kBlocks * 64);
  if (c < nchunks) {
    int32_t last = -1;
    if (!write_chunk(ln, mine, end, first, coef, dcd, &last)) flags[2] = 1;
    if (last >= 0) flags[3] = last;
  }
  __syncthreads();
  if (flags[2] || flags[3] < 0 || flags[3] > avail) {     // an error, fewer than 384 blocks, or past the data
    if (c == 0) d->status = NDP_JPEG_CORRUPT;
    return;
  }
  // DC: running sums of the differences per component, in decode order (segmented scan over Y 256, Cb 64, Cr 64)
  int32_t* acc = cnt;                                      // 256 entries: Y; the chroma scans reuse dcd below
  __shared__ int32_t chroma[128];
  for (int g = c; g < kBlocks; g += kEntropyThreads) {
    const int mcu = g / 6, bi = g - 6 * mcu;
    if (bi < 4) acc[mcu * 4 + bi] = dcd[g];
    else chroma[(bi - 4) * 64 + mcu] = dcd[g];
  }
  __syncthreads();
  for (int off = 1; off < kEntropyThreads; off <<= 1) {
    const int32_t vy = c >= off ? acc[c - off] : 0;
    const int32_t vc = (c < 128 && (c & 63) >= off) ? chroma[c - off] : 0;
    __syncthreads();
    acc[c] += vy;
    if (c < 128) chroma[c] += vc;
    __syncthreads();
  }
  {
    const int mcu = c >> 2, bi = c & 3;                    // Y block c of decode order
    coef[((2 * (mcu >> 3) + (bi >> 1)) * 16 + 2 * (mcu & 7) + (bi & 1)) * 64] = (int16_t)acc[c];
    if (c < 128) coef[(256 + c) * 64] = (int16_t)chroma[c];
  }
}

__global__ __launch_bounds__(jpeg::kEntropyThreads) void k_jpeg_entropy(jpeg::Layout L, int64_t n) {
  using namespace jpeg;
  constexpr int kLutWords = 4 * (1 << kLook) / 2;
  constexpr int kStreamWords = kStreamLdsBytes / 4;
  __shared__ uint32_t lut[kLutWords];
  __shared__ int32_t maxc[4 * 18], voff[4 * 18];
  __shared__ uint8_t hval[4 * 256];
  __shared__ uint32_t words[kStreamWords];
  __shared__ EState exits[kEntropyThreads];
  __shared__ int32_t cnt[kEntropyThreads], dcd[kBlocks], flags[4];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x;
  Desc* d = L.desc + f;
  if (d->status != NDP_JPEG_OK) return;                     // uniform over the workgroup
  for (int i = tid; i < kLutWords; i += kEntropyThreads) lut[i] = reinterpret_cast<const uint32_t*>(d->lut)[i];
  for (int i = tid; i < 4 * 18; i += kEntropyThreads) {
    maxc[i] = d->maxcode[i / 18][i % 18];
    voff[i] = d->valoff[i / 18][i % 18];
  }
  for (int i = tid; i < 4 * 256; i += kEntropyThreads) hval[i] = d->huffval[i >> 8][i & 255];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(L.compact + d->cstart);
  const int32_t nbytes = d->ncompact;
  const int32_t nw = min((nbytes + 3) >> 2, kStreamWords);
  for (int i = tid; i < nw; i += kEntropyThreads) words[i] = src[i];
  __syncthreads();
  if (nbytes <= kStreamLdsBytes)
    entropy_frame<false>(L, d, f, words, reinterpret_cast<const uint16_t*>(lut), maxc, voff, hval, exits, cnt,
                         dcd, flags);
  else
    entropy_frame<true>(L, d, f, words, reinterpret_cast<const uint16_t*>(lut), maxc, voff, hval, exits, cnt,
                        dcd, flags);
}

__global__ __launch_bounds__(256) void k_jpeg_idct(jpeg::Layout L, int64_t n) {
  using namespace jpeg;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n * kBlocks) return;
  const int64_t f = g / kBlocks;
  const int b = (int)(g % kBlocks);
  const Desc* d = L.desc + f;
  if (d->status != NDP_JPEG_OK) return;
  const int comp = b < 256 ? 0 : (b < 320 ? 1 : 2);
  const int4* cp = reinterpret_cast<const int4*>(L.coef + g * 64);
  const int4* qp = reinterpret_cast<const int4*>(d->qt[comp]);
  int x[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int4 c = cp[i], q = qp[i];
    const int cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[8 * i + 2 * j] = (int)(int16_t)(cw[j] & 0xFFFF) * (int)(qw[j] & 0xFFFF);
      x[8 * i + 2 * j + 1] = (cw[j] >> 16) * (int)((uint32_t)qw[j] >> 16);
    }
  }
  uint8_t px[64];
  idct_islow(x, px);
  uint8_t* plane = L.planes + f * kPlaneBytes;
  int stride, by, bx;
  if (comp == 0) { stride = 128; by = b >> 4; bx = b & 15; }
  else { plane += 16384 + (comp - 1) * 4096; stride = 64; by = (b - 256 - (comp - 1) * 64) >> 3; bx = (b - 256) & 7; }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    uint2 w;
    w.x = px[8 * r] | px[8 * r + 1] << 8 | px[8 * r + 2] << 16 | (uint32_t)px[8 * r + 3] << 24;
    w.y = px[8 * r + 4] | px[8 * r + 5] << 8 | px[8 * r + 6] << 16 | (uint32_t)px[8 * r + 7] << 24;
    *reinterpret_cast<uint2*>(plane + (by * 8 + r) * stride + bx * 8) = w;
  }
}

__global__ __launch_bounds__(256) void k_jpeg_color(jpeg::Layout L, int64_t n, uint8_t* __restrict__ frames,
                                                    int32_t* __restrict__ status) {
  using namespace jpeg;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n * kSize * kSize) return;
  const int64_t f = g >> 14;
  const int y = (int)(g >> 7) & 127, x = (int)g & 127;
  const int st = L.desc[f].status;
  if (y == 0 && x == 0) status[f] = st;
  uint8_t rgb[3] = {0, 0, 0};
  if (st == NDP_JPEG_OK) {
    const uint8_t* pl = L.planes + f * kPlaneBytes;
    ycc_pixel(pl, pl + 16384, pl + 16384 + 4096, y, x, rgb);
  }
  uint8_t* o = frames + g * 3;
  o[0] = rgb[0];
  o[1] = rgb[1];
  o[2] = rgb[2];
}

}  // namespace ndp

extern "C" {

int64_t ndp_jpeg_workspace_bytes(int64_t n_images, int64_t stream_bytes) {
  using namespace ndp::jpeg;
  if (n_images < 1 || n_images > kMaxImages || stream_bytes < 0 || stream_bytes > ((int64_t)1 << 40)) return 0;
  return fixed_bytes(n_images) + compact_need(n_images, stream_bytes);
}

int ndp_jpeg_decode_u8(const uint8_t* streams, const int64_t* offsets, int64_t n_images, uint8_t* frames_hwc,
                       int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ndp;
  using namespace ndp::jpeg;
  NDP_CHECK_ARG(streams && offsets && frames_hwc && status && workspace, "ndp_jpeg_decode_u8: null pointer");
  NDP_CHECK_ARG(n_images >= 1 && n_images <= kMaxImages, "ndp_jpeg_decode_u8: bad image count %lld",
                (long long)n_images);
  NDP_CHECK_ARG(workspace_bytes >= fixed_bytes(n_images) + compact_need(n_images, 0),
                "ndp_jpeg_decode_u8: workspace of %lld bytes is below the %lld that %lld images need",
                (long long)workspace_bytes, (long long)(fixed_bytes(n_images) + compact_need(n_images, 0)),
                (long long)n_images);
  NDP_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "ndp_jpeg_decode_u8: workspace must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  Layout L = layout(workspace, workspace_bytes, n_images);
  {
    KTimer kt("k_jpeg_parse", st);
    hipLaunchKernelGGL(k_jpeg_parse, dim3((unsigned)n_images), dim3(kParseThreads), 0, st, streams, offsets, L);
  }
  int rc = check_launch("k_jpeg_parse");
  if (rc) return rc;
  {
    KTimer kt("k_jpeg_entropy", st);
    hipLaunchKernelGGL(k_jpeg_entropy, dim3((unsigned)n_images), dim3(kEntropyThreads), 0, st, L, n_images);
  }
  if ((rc = check_launch("k_jpeg_entropy"))) return rc;
  {
    KTimer kt("k_jpeg_idct", st);
    hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)((n_images * kBlocks + 255) / 256)), dim3(256), 0, st, L, n_images);
  }
  if ((rc = check_launch("k_jpeg_idct"))) return rc;
  KTimer kt("k_jpeg_color", st);
  hipLaunchKernelGGL(k_jpeg_color, dim3((unsigned)(n_images * kSize * kSize / 256)), dim3(256), 0, st, L, n_images,
                     frames_hwc, status);
  return check_launch("k_jpeg_color");
}

}  // extern "C"
