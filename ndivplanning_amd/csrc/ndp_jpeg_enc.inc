// ndp_jpeg_enc.inc -- device-side JPEG encode of trajectory frames, byte-identical to the reference's writer
// (generate_trajectories.py:113-122: PIL `im.save(format="jpeg", quality=95)`, i.e. libjpeg-turbo: baseline, 8-bit,
// 128x128, 4:2:0, the Annex K tables scaled for quality 95, the standard Huffman tables, no restart markers).  The
// output is the layout `pack_jpegs` makes and ndp_jpeg_decode_u8 reads: one byte buffer plus int64 offsets[n+1].
// Four launches per batch:
//   k_jpeg_enc_dct      one thread per 8x8 block: jccolor.c's fixed-point RGB -> YCbCr, jcsample.c's h2v2 box
//                       downsampling of the chroma, jfdctint.c's integer "islow" forward DCT, sign-magnitude quantisation;
//                       int16 coefficients in zig-zag order, blocks in scan order (MCU by MCU: Y00 Y01 Y10 Y11 Cb Cr)
//   k_jpeg_enc_pack<0>  one workgroup per frame, one lane per block: bit count per block (the DC predecessor is the
//                       previous block's coefficient, so nothing is carried), exclusive scan over the 384 blocks, the bits
//                       ORed into a bit buffer in LDS, 0xFF bytes counted; writes the frame's stream length only
//   k_jpeg_enc_offsets  one workgroup: scan of the n lengths in tiles of 1024 into offsets[n+1], against `capacity`
//   k_jpeg_enc_pack<1>  the same work again; writes header, stuffed entropy data and EOI at the frame's offset
// No workgroup waits for another, every loop has a fixed bound, atomics touch LDS only (atomicOr: commutative, so the
// bytes do not depend on the order of the lanes), integer arithmetic only: two runs give the same bytes.
// Included at the end of ndp_kernels.hip, after ndp_jpeg.inc.

namespace ndp {
namespace jpegenc {

using jpeg::kBlocks;
using jpeg::kMaxImages;
using jpeg::kNatural;
using jpeg::kSize;

constexpr int kHeaderBytes = 623;              // SOI .. SOS, the same for every frame
constexpr int kCoefBytes = kBlocks * 64 * 2;   // per frame in the workspace
constexpr int kDctThreads = 128;               // k_jpeg_enc_dct: 3 workgroups per frame (2 of Y blocks, 1 of chroma)
constexpr int kPackThreads = kBlocks;          // k_jpeg_enc_pack: one lane per block
constexpr int kScanTile = 1024;                // k_jpeg_enc_offsets: lengths per pass of its one workgroup
constexpr int kMaxDcBits = 11;                 // the standard DC tables code categories 0..11
constexpr int kMaxAcBits = 10;                 // the standard AC tables code sizes 1..10

// Annex K.1 / K.2 quantisation tables, natural order, before scaling.
constexpr uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3 Huffman tables: codes per length 1..16, then the symbols in code order.  0 Y DC, 1 Y AC, 2 chroma DC,
// 3 chroma AC (the decoder's numbering).
constexpr uint8_t kHuffBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                      {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                      {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                      {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr int kHuffCount[4] = {12, 162, 12, 162};
constexpr uint8_t kHuffVals[4][162] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// Everything derived from the tables above, at compile time.
struct Tables {
  uint16_t q8[2][64];            // 8 * the quality-95 quantiser, natural order (jcdctmgr.c: the islow DCT's output is
                                 // scaled by 8)
  uint32_t huff[4][256];         // symbol -> (code length << 16) | code; 0: the table has no such symbol
  uint8_t header[kHeaderBytes];  // SOI, JFIF APP0, DQT x 2, SOF0, DHT x 4, SOS
  int32_t block_bits[2];         // the most bits one block can take: Y, chroma
};

constexpr Tables make_tables() {
  Tables t = {};
  uint8_t q[2][64] = {};
  for (int c = 0; c < 2; ++c) {
    for (int i = 0; i < 64; ++i) {                       // jpeg_quality_scaling(95) = 200 - 2 * 95 = 10
      int v = (kBaseQ[c][i] * 10 + 50) / 100;
      v = v < 1 ? 1 : (v > 255 ? 255 : v);
      q[c][i] = (uint8_t)v;
      t.q8[c][i] = (uint16_t)(8 * v);
    }
  }
  for (int h = 0; h < 4; ++h) {                          // jchuff.c jpeg_make_c_derived_tbl
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < kHuffBits[h][l - 1]; ++i) {
        t.huff[h][kHuffVals[h][k]] = ((uint32_t)l << 16) | (uint32_t)code;
        ++code;
        ++k;
      }
      code <<= 1;
    }
  }
  for (int c = 0; c < 2; ++c) {                          // the entropy bound of one block
    int dc = 0, ac = 0;
    for (int s = 0; s <= kMaxDcBits; ++s) {
      const int len = (int)(t.huff[2 * c][s] >> 16) + s;
      dc = len > dc ? len : dc;
    }
    for (int r = 0; r < 16; ++r) {
      for (int s = 1; s <= kMaxAcBits; ++s) {
        const int len = (int)(t.huff[2 * c + 1][(r << 4) | s] >> 16) + s;
        ac = len > ac ? len : ac;
      }
    }
    t.block_bits[c] = dc + 63 * ac;                      // 63 nonzero coefficients: no ZRL, no EOB
  }
  int p = 0;
  uint8_t* o = t.header;
  const uint8_t app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (int i = 0; i < 20; ++i) o[p++] = app0[i];
  for (int c = 0; c < 2; ++c) {
    o[p++] = 0xFF; o[p++] = 0xDB; o[p++] = 0; o[p++] = 67; o[p++] = (uint8_t)c;
    for (int k = 0; k < 64; ++k) o[p++] = q[c][kNatural[k]];
  }
  const uint8_t sof[] = {0xFF, 0xC0, 0, 17, 8, 0, kSize, 0, kSize, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
  for (int i = 0; i < 19; ++i) o[p++] = sof[i];
  for (int h = 0; h < 4; ++h) {
    o[p++] = 0xFF; o[p++] = 0xC4; o[p++] = 0; o[p++] = (uint8_t)(19 + kHuffCount[h]);
    o[p++] = (uint8_t)(((h & 1) << 4) | (h >> 1));       // class (0 DC, 1 AC) << 4 | table id
    for (int l = 0; l < 16; ++l) o[p++] = kHuffBits[h][l];
    for (int i = 0; i < kHuffCount[h]; ++i) o[p++] = kHuffVals[h][i];
  }
  const uint8_t sos[] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  for (int i = 0; i < 14; ++i) o[p++] = sos[i];
  if (p != kHeaderBytes) t.block_bits[0] = -1;           // caught by the static_assert below
  return t;
}

constexpr Tables kT = make_tables();
static_assert(kT.block_bits[0] > 0 && kT.block_bits[1] > 0, "header length or Huffman tables are off");

// The entropy data of one frame before stuffing: at most this many bits, whatever the coefficients (encode_block clamps
// them to what the tables can code).  Every byte can be 0xFF, so stuffing at most doubles it.
constexpr int kMaxEntropyBits = 256 * kT.block_bits[0] + 128 * kT.block_bits[1];
constexpr int kMaxEntropyBytes = (kMaxEntropyBits + 7) / 8;
constexpr int kBitWords = (kMaxEntropyBytes + 3) / 4;
constexpr int64_t kMaxStreamBytes = (int64_t)kHeaderBytes + 2 * kMaxEntropyBytes + 2;
static_assert(kBitWords * 4 + 4 * 256 * 4 + 2 * kPackThreads * 4 + 64 <= 160 * 1024, "k_jpeg_enc_pack's LDS");

// ---------------------------------------------------------------- colour, downsampling, DCT, quantisation
// jccolor.c rgb_ycc_convert (SCALEBITS 16): FIX(0.29900) = 19595, FIX(0.58700) = 38470, FIX(0.11400) = 7471,
// FIX(0.16874) = 11059, FIX(0.33126) = 21709, FIX(0.5) = 32768, FIX(0.41869) = 27439, FIX(0.08131) = 5329.
__host__ __device__ inline int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__host__ __device__ inline int ycc_cb(int r, int g, int b) {
  return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
__host__ __device__ inline int ycc_cr(int r, int g, int b) {
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// `count` (a multiple of 4) bytes from a 4-byte aligned address, a word at a time.
template <int COUNT>
__host__ __device__ inline void load_bytes(const uint8_t* p, uint8_t* out) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int i = 0; i < COUNT / 4; ++i) {
    const uint32_t v = w[i];
    out[4 * i] = (uint8_t)v;
    out[4 * i + 1] = (uint8_t)(v >> 8);
    out[4 * i + 2] = (uint8_t)(v >> 16);
    out[4 * i + 3] = (uint8_t)(v >> 24);
  }
}

// The 64 samples (minus 128) of scan-order block g of `frame` ([128][128][3] bytes, 4-byte aligned).
__host__ __device__ inline void block_samples(const uint8_t* frame, int g, int* d) {
  const int mcu = g / 6, bi = g - 6 * mcu;
  const int my = mcu >> 3, mx = mcu & 7;
  if (bi < 4) {
    const int y0 = 16 * my + 8 * (bi >> 1), x0 = 16 * mx + 8 * (bi & 1);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      uint8_t px[24];
      load_bytes<24>(frame + ((y0 + r) * kSize + x0) * 3, px);
#pragma unroll
      for (int c = 0; c < 8; ++c) d[8 * r + c] = ycc_y(px[3 * c], px[3 * c + 1], px[3 * c + 2]) - 128;
    }
  } else {
    // jcsample.c h2v2_downsample: the 2x2 box of the converted samples, bias 1 in even output columns, 2 in odd ones
    const bool cb = bi == 4;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      uint8_t p0[48], p1[48];
      load_bytes<48>(frame + ((16 * my + 2 * r) * kSize + 16 * mx) * 3, p0);
      load_bytes<48>(frame + ((16 * my + 2 * r + 1) * kSize + 16 * mx) * 3, p1);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        int sum = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint8_t* a = p0 + 3 * (2 * c + j);
          const uint8_t* b = p1 + 3 * (2 * c + j);
          sum += cb ? ycc_cb(a[0], a[1], a[2]) + ycc_cb(b[0], b[1], b[2])
                    : ycc_cr(a[0], a[1], a[2]) + ycc_cr(b[0], b[1], b[2]);
        }
        d[8 * r + c] = ((sum + 1 + (c & 1)) >> 2) - 128;
      }
    }
  }
}

// jfdctint.c (islow), CONST_BITS 13, PASS1_BITS 2.  One 1-D pass over I0..I7 in place; the even outputs 0 and 4 are
// `<< 2` in the row pass (EVEN_UP) and descaled by 2 in the column pass, the others descaled by SH.
#define NDP_JPEG_FDCT_1D(I0, I1, I2, I3, I4, I5, I6, I7, ROWS, SH)                                                  \
  do {                                                                                                             \
    const int t0 = I0 + I7, t7 = I0 - I7, t1 = I1 + I6, t6 = I1 - I6;                                              \
    const int t2 = I2 + I5, t5 = I2 - I5, t3 = I3 + I4, t4 = I3 - I4;                                              \
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;                                          \
    const int rnd = 1 << ((SH) - 1);                                                                               \
    I0 = (ROWS) ? (t10 + t11) * 4 : (t10 + t11 + 2) >> 2;                                                          \
    I4 = (ROWS) ? (t10 - t11) * 4 : (t10 - t11 + 2) >> 2;                                                          \
    int z1 = (t12 + t13) * 4433;                                                                                   \
    I2 = (z1 + t13 * 6270 + rnd) >> (SH);                                                                          \
    I6 = (z1 - t12 * 15137 + rnd) >> (SH);                                                                         \
    z1 = t4 + t7;                                                                                                  \
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;                                                                  \
    const int z5 = (z3 + z4) * 9633;                                                                               \
    const int m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;                                   \
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;                                        \
    I7 = (m4 + z1 + z3 + rnd) >> (SH);                                                                             \
    I5 = (m5 + z2 + z4 + rnd) >> (SH);                                                                             \
    I3 = (m6 + z2 + z3 + rnd) >> (SH);                                                                             \
    I1 = (m7 + z1 + z4 + rnd) >> (SH);                                                                             \
  } while (0)

__host__ __device__ inline void fdct_islow(int* d) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int* w = d + 8 * r;
    NDP_JPEG_FDCT_1D(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], true, 11);
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    NDP_JPEG_FDCT_1D(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c], false, 15);
  }
}
#undef NDP_JPEG_FDCT_1D

// jcdctmgr.c quantize: on the magnitude, rounded half up, the sign put back.
__host__ __device__ inline int quantize(int c, int q8) {
  const int a = c < 0 ? -c : c;
  const int v = (a + (q8 >> 1)) / q8;
  return c < 0 ? -v : v;
}

// Scan-order block g of `frame` -> 64 quantised coefficients, zig-zag order.
__host__ __device__ inline void block_coefs(const uint8_t* frame, int g, int16_t* zz) {
  int d[64];
  block_samples(frame, g, d);
  fdct_islow(d);
  const int comp = (g % 6) < 4 ? 0 : 1;
#pragma unroll
  for (int k = 0; k < 64; ++k) zz[k] = (int16_t)quantize(d[kNatural[k]], kT.q8[comp][kNatural[k]]);
}

// ---------------------------------------------------------------- entropy coding
__host__ __device__ inline int bit_length(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }
__host__ __device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Scan-order index of the block whose DC value predicts block g's (the previous block of the same component), -1: none.
__host__ __device__ inline int dc_predecessor(int g) {
  const int mcu = g / 6, bi = g - 6 * mcu;
  if (bi >= 1 && bi <= 3) return g - 1;
  if (mcu == 0) return -1;
  return bi == 0 ? g - 3 : g - 6;
}

struct BitCounter {
  int32_t bits;
  __host__ __device__ void put(uint32_t, int len) { bits += len; }
};

// Bits MSB first into 32-bit words whose bit 31 is the earliest: a 64-bit accumulator aligned to the first bit's place,
// each completed word ORed into `words` (shared with the blocks before and after, hence OR; atomic on the device).
// Nothing is written at or beyond words[nwords].
struct BitWriter {
  uint32_t* words;
  int32_t nwords, w;
  uint64_t acc;
  int fill;
  __host__ __device__ void start(uint32_t* base, int32_t n, int32_t bitpos) {
    words = base; nwords = n; w = bitpos >> 5; fill = bitpos & 31; acc = 0;
  }
  __host__ __device__ void flush_word() {
    const uint32_t v = (uint32_t)(acc >> 32);
    if (v && w < nwords) {
#if defined(__HIP_DEVICE_COMPILE__)
      atomicOr(&words[w], v);
#else
      words[w] |= v;
#endif
    }
  }
  __host__ __device__ void put(uint32_t code, int len) {          // len <= 27, fill <= 31
    acc |= (uint64_t)code << (64 - fill - len);
    fill += len;
    if (fill >= 32) {
      flush_word();
      ++w;
      acc <<= 32;
      fill -= 32;
    }
  }
  __host__ __device__ void finish() { if (fill) flush_word(); }
};

// jchuff.c encode_one_block: zz = one block's coefficients in zig-zag order (16-byte aligned), pred = the DC predictor,
// dc / ac = its Huffman tables (Tables::huff rows).  The difference is clamped to what category 11 holds (+-2047) and the
// AC values to category 10 (+-1023).  No frame reaches either clamp: the quality-95 DC quantiser is 2 (q8 = 16), so a DC
// value lies in -512..508 and a difference within +-1020 (category 10; with a quantiser of 1 it would reach category 11,
// still inside the clamp), and an AC value stays below 1024 because the DCT's gain for an AC basis function is at most
// 928 / 128.  So any 64 int16 values stay within Tables::block_bits.
template <class Sink>
__host__ __device__ inline void encode_block(const int16_t* zz, int pred, const uint32_t* dc, const uint32_t* ac,
                                             Sink& sink) {
  int run = 0;
  for (int i = 0; i < 8; ++i) {
    const int4 pack = *reinterpret_cast<const int4*>(zz + 8 * i);
    const int pw[4] = {pack.x, pack.y, pack.z, pack.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int v = (j & 1) ? (pw[j >> 1] >> 16) : (int)(int16_t)(pw[j >> 1] & 0xFFFF);
      if (i == 0 && j == 0) {
        v = clampi(v - pred, -2047, 2047);
        const int s = bit_length(v < 0 ? -v : v);
        const uint32_t e = dc[s];
        sink.put(((e & 0xFFFF) << s) | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << s) - 1)), (int)(e >> 16) + s);
        continue;
      }
      if (v == 0) {
        ++run;
        continue;
      }
      for (int z = 0; z < 3 && run >= 16; ++z) {                  // ZRL: a run is at most 62
        sink.put(ac[0xF0] & 0xFFFF, (int)(ac[0xF0] >> 16));
        run -= 16;
      }
      v = clampi(v, -1023, 1023);
      const int s = bit_length(v < 0 ? -v : v);
      const uint32_t e = ac[(run << 4) | s];
      sink.put(((e & 0xFFFF) << s) | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << s) - 1)), (int)(e >> 16) + s);
      run = 0;
    }
  }
  if (run > 0) sink.put(ac[0] & 0xFFFF, (int)(ac[0] >> 16));      // EOB
}

// Byte k of the bit buffer.
__host__ __device__ inline int entropy_byte(const uint32_t* words, int32_t k) {
  return (int)(words[k >> 2] >> (24 - 8 * (k & 3))) & 0xFF;
}

// The 1-bits that pad the last byte of `total_bits` bits, as (word index, value to OR); value 0: no padding.
__host__ __device__ inline uint32_t pad_bits(int32_t total_bits) {
  const int pad = (8 - (total_bits & 7)) & 7;
  return pad ? ((1u << pad) - 1u) << (32 - (total_bits & 31) - pad) : 0u;
}

// Bytes per lane in the stuffing pass over `nbytes` entropy bytes.
__host__ __device__ inline int32_t stuff_chunk(int32_t nbytes) { return (nbytes + kPackThreads - 1) / kPackThreads; }

// Workspace: coefficients [n][384][64] int16, then the stream lengths [n] int64.
__host__ __device__ inline int64_t workspace_bytes(int64_t n) {
  return n * kCoefBytes + (n * 8 + 255) / 256 * 256;
}

}  // namespace jpegenc

__global__ __launch_bounds__(jpegenc::kDctThreads) void k_jpeg_enc_dct(const uint8_t* __restrict__ frames,
                                                                       int16_t* __restrict__ coef) {
  using namespace jpegenc;
  const int64_t f = blockIdx.x / (kBlocks / kDctThreads);
  const int t = (int)(blockIdx.x % (kBlocks / kDctThreads)) * kDctThreads + threadIdx.x;   // Y row-major, Cb, Cr
  int g;
  if (t < 256) {
    const int by = t >> 4, bx = t & 15;
    g = ((by >> 1) * 8 + (bx >> 1)) * 6 + (by & 1) * 2 + (bx & 1);
  } else {
    g = ((t - 256) & 63) * 6 + 4 + ((t - 256) >> 6);
  }
  int16_t zz[64];
  block_coefs(frames + f * (kSize * kSize * 3), g, zz);
  int4* dst = reinterpret_cast<int4*>(coef + (f * kBlocks + g) * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int4 v;
    v.x = (uint16_t)zz[8 * i] | ((uint32_t)(uint16_t)zz[8 * i + 1] << 16);
    v.y = (uint16_t)zz[8 * i + 2] | ((uint32_t)(uint16_t)zz[8 * i + 3] << 16);
    v.z = (uint16_t)zz[8 * i + 4] | ((uint32_t)(uint16_t)zz[8 * i + 5] << 16);
    v.w = (uint16_t)zz[8 * i + 6] | ((uint32_t)(uint16_t)zz[8 * i + 7] << 16);
    dst[i] = v;
  }
}

// WRITE false: lens[f] = the frame's stream length.  WRITE true: the stream itself at streams + offsets[f], where
// offsets[f+1] - offsets[f] is that length (k_jpeg_enc_offsets made it so); a frame that got no room is skipped.
template <bool WRITE>
__global__ __launch_bounds__(jpegenc::kPackThreads) void k_jpeg_enc_pack(const int16_t* __restrict__ coef,
                                                                        int64_t* __restrict__ lens,
                                                                        const int64_t* __restrict__ offsets,
                                                                        uint8_t* __restrict__ streams, int64_t capacity) {
  using namespace jpegenc;
  __shared__ uint32_t words[kBitWords];
  __shared__ uint32_t huff[4 * 256];
  __shared__ int32_t scan[kPackThreads];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x;
  int64_t beg = 0, room = 0;
  if (WRITE) {
    beg = offsets[f];
    room = offsets[f + 1] - beg;
    if (room <= 0) return;                                         // status 4: uniform over the workgroup
  }
  for (int i = tid; i < 4 * 256; i += kPackThreads) huff[i] = kT.huff[i >> 8][i & 255];
  const int16_t* frame_coef = coef + f * (kBlocks * 64);
  const int16_t* zz = frame_coef + tid * 64;
  const int pg = dc_predecessor(tid);
  const int pred = pg >= 0 ? frame_coef[pg * 64] : 0;
  const int tab = (tid % 6) < 4 ? 0 : 2;
  __syncthreads();
  BitCounter cnt = {0};
  encode_block(zz, pred, huff + tab * 256, huff + (tab + 1) * 256, cnt);
  scan[tid] = cnt.bits;
  __syncthreads();
  for (int off = 1; off < kPackThreads; off <<= 1) {
    const int32_t v = tid >= off ? scan[tid - off] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const int32_t start = scan[tid] - cnt.bits;
  const int32_t total_bits = scan[kPackThreads - 1];               // <= kMaxEntropyBits: encode_block's clamps
  const int32_t nbytes = (total_bits + 7) >> 3;
  const int32_t nwords = min((nbytes + 3) >> 2, kBitWords);
  __syncthreads();                                                 // scan is reused below
  for (int i = tid; i < nwords; i += kPackThreads) words[i] = 0;
  __syncthreads();
  BitWriter wr;
  wr.start(words, nwords, start);
  encode_block(zz, pred, huff + tab * 256, huff + (tab + 1) * 256, wr);
  wr.finish();
  if (tid == 0 && pad_bits(total_bits) && (total_bits >> 5) < nwords) atomicOr(&words[total_bits >> 5], pad_bits(total_bits));
  __syncthreads();
  // stuffing: a 0x00 after every 0xFF byte; a scan of the 0xFF counts places each lane's bytes
  const int32_t chunk = stuff_chunk(nbytes);
  const int32_t c0 = min(tid * chunk, nbytes), c1 = min(c0 + chunk, nbytes);
  int32_t ff = 0;
  for (int32_t k = c0; k < c1; ++k) ff += entropy_byte(words, k) == 0xFF;
  scan[tid] = ff;
  __syncthreads();
  for (int off = 1; off < kPackThreads; off <<= 1) {
    const int32_t v = tid >= off ? scan[tid - off] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const int64_t len = (int64_t)kHeaderBytes + nbytes + scan[kPackThreads - 1] + 2;
  if (!WRITE) {
    if (tid == 0) lens[f] = len;
    return;
  }
  if (room != len || beg < 0 || beg + len > capacity) return;      // cannot happen; nothing is written outside the room
  uint8_t* out = streams + beg;
  for (int i = tid; i < kHeaderBytes; i += kPackThreads) out[i] = kT.header[i];
  int64_t o = (int64_t)kHeaderBytes + c0 + (scan[tid] - ff);
  for (int32_t k = c0; k < c1; ++k) {
    const int b = entropy_byte(words, k);
    out[o++] = (uint8_t)b;
    if (b == 0xFF) out[o++] = 0;
  }
  if (tid == 0) {
    out[len - 2] = 0xFF;
    out[len - 1] = 0xD9;
  }
}

// offsets[0] = 0, offsets[i+1] = offsets[i] + lens[i] while the streams fit `capacity`; the first frame that does not
// fit and every frame after it get status NDP_JPEG_WORKSPACE and length 0.  One workgroup, tiles of kScanTile lengths.
__global__ __launch_bounds__(jpegenc::kScanTile) void k_jpeg_enc_offsets(const int64_t* __restrict__ lens, int64_t n,
                                                                        int64_t capacity, int64_t* __restrict__ offsets,
                                                                        int32_t* __restrict__ status) {
  using namespace jpegenc;
  __shared__ int64_t s[kScanTile];
  __shared__ int64_t s_carry, s_fit_end;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_carry = 0;
    s_fit_end = 0;
    offsets[0] = 0;
  }
  __syncthreads();
  for (int tile = 0; tile < (int)(kMaxImages / kScanTile); ++tile) {
    const int64_t i = (int64_t)tile * kScanTile + tid;
    if ((int64_t)tile * kScanTile >= n) break;                     // uniform
    s[tid] = i < n ? lens[i] : 0;
    __syncthreads();
    for (int off = 1; off < kScanTile; off <<= 1) {
      const int64_t v = tid >= off ? s[tid - off] : 0;
      __syncthreads();
      s[tid] += v;
      __syncthreads();
    }
    const int64_t carry = s_carry;
    const int64_t incl = carry + s[tid];
    const bool fits = incl <= capacity;
    // the last frame that fits (the lengths are positive, so the sums increase) leaves the end of the used bytes
    const bool next_fits = tid + 1 < kScanTile && i + 1 < n && carry + s[tid + 1] <= capacity;
    if (i < n && fits && !next_fits) s_fit_end = incl;
    __syncthreads();
    if (i < n) {
      offsets[i + 1] = fits ? incl : s_fit_end;
      status[i] = fits ? NDP_JPEG_OK : NDP_JPEG_WORKSPACE;
    }
    __syncthreads();
    if (tid == kScanTile - 1) s_carry = incl;
    __syncthreads();
  }
}

}  // namespace ndp

extern "C" {

int64_t ndp_jpeg_encode_workspace_bytes(int64_t n_images) {
  using namespace ndp::jpegenc;
  if (n_images < 1 || n_images > kMaxImages) return 0;
  return workspace_bytes(n_images);
}

int64_t ndp_jpeg_encode_max_stream_bytes(void) { return ndp::jpegenc::kMaxStreamBytes; }

int64_t ndp_jpeg_encode_lengths_offset(int64_t n_images) {
  using namespace ndp::jpegenc;
  if (n_images < 1 || n_images > kMaxImages) return -1;
  return n_images * kCoefBytes;
}

int ndp_jpeg_encode_u8(const uint8_t* frames_hwc, int64_t n_images, uint8_t* streams, int64_t capacity, int64_t* offsets,
                       int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ndp;
  using namespace ndp::jpegenc;
  NDP_CHECK_ARG(frames_hwc && streams && offsets && status && workspace, "ndp_jpeg_encode_u8: null pointer");
  NDP_CHECK_ARG(n_images >= 1 && n_images <= kMaxImages, "ndp_jpeg_encode_u8: bad image count %lld",
                (long long)n_images);
  NDP_CHECK_ARG(capacity >= 0 && capacity <= ((int64_t)1 << 40), "ndp_jpeg_encode_u8: bad capacity %lld",
                (long long)capacity);
  NDP_CHECK_ARG(workspace_bytes >= jpegenc::workspace_bytes(n_images),
                "ndp_jpeg_encode_u8: workspace of %lld bytes is below the %lld that %lld images need",
                (long long)workspace_bytes, (long long)jpegenc::workspace_bytes(n_images), (long long)n_images);
  NDP_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "ndp_jpeg_encode_u8: workspace must be 256-byte aligned");
  NDP_CHECK_ARG((reinterpret_cast<uintptr_t>(frames_hwc) & 3) == 0, "ndp_jpeg_encode_u8: frames must be 4-byte aligned");
  NDP_CHECK_ARG((reinterpret_cast<uintptr_t>(offsets) & 7) == 0, "ndp_jpeg_encode_u8: offsets must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int16_t* coef = static_cast<int16_t*>(workspace);
  int64_t* lens = reinterpret_cast<int64_t*>(static_cast<uint8_t*>(workspace) + n_images * kCoefBytes);
  {
    KTimer kt("k_jpeg_enc_dct", st);
    hipLaunchKernelGGL(k_jpeg_enc_dct, dim3((unsigned)(n_images * (kBlocks / kDctThreads))), dim3(kDctThreads), 0, st,
                       frames_hwc, coef);
  }
  int rc = check_launch("k_jpeg_enc_dct");
  if (rc) return rc;
  {
    KTimer kt("k_jpeg_enc_pack_count", st);
    hipLaunchKernelGGL(k_jpeg_enc_pack<false>, dim3((unsigned)n_images), dim3(kPackThreads), 0, st, coef, lens,
                       (const int64_t*)offsets, streams, capacity);
  }
  if ((rc = check_launch("k_jpeg_enc_pack_count"))) return rc;
  {
    KTimer kt("k_jpeg_enc_offsets", st);
    hipLaunchKernelGGL(k_jpeg_enc_offsets, dim3(1), dim3(kScanTile), 0, st, (const int64_t*)lens, n_images, capacity,
                       offsets, status);
  }
  if ((rc = check_launch("k_jpeg_enc_offsets"))) return rc;
  KTimer kt("k_jpeg_enc_pack_write", st);
  hipLaunchKernelGGL(k_jpeg_enc_pack<true>, dim3((unsigned)n_images), dim3(kPackThreads), 0, st, coef, lens,
                     (const int64_t*)offsets, streams, capacity);
  return check_launch("k_jpeg_enc_pack_write");
}

}  // extern "C"
