// ndp_store.inc -- batch assembly from a device-resident trajectory store (ndp_store_gather, include/ndp.h;
// trajectory_store.py; DESIGN.md section 5m).  Included by ndp_kernels.hip.
//
// The store holds every trajectory of a bundle directory in device memory: one blob of JPEG streams back to back, an
// int64 frame-offset table [N*T+1] (frame f of the store is blob[frame_offsets[f] .. frame_offsets[f+1])), and the float
// tables states [N,T,25], actions [N,T,4], goal [N,3].  A batch is B trajectory indices and a window (seq_start,
// seq_length) of every trajectory; its n = B * seq_length streams, packed back to back in batch order with an int64
// offset table [n+1], are what ndp_jpeg_decode_u8 takes.  Two launches, no host synchronisation, no atomics:
//
//   k_store_scan   workgroup 0: the selected lengths and their exclusive prefix sum -> out_offsets [n+1], and the status
//                  word (bit 0: an index is outside 0..N-1 -- that trajectory gets zero-length streams and zero rows;
//                  bit 1: the streams do not fit `capacity` -- the bytes past it are not written).
//                  1024 threads, each owns a contiguous run of ceil(n / 1024) streams; the run sums are scanned in LDS.
//                  Workgroups 1..: the rows of states / actions / goal, element by element (4-byte words, bit copies).
//   k_store_copy   the bytes.  The DESTINATION is cut into 16-byte words (the output buffer is 16-byte aligned), 256
//                  words to a chunk, chunks dealt round-robin to the workgroups of a fixed-size grid: the number of
//                  chunks is out_offsets[n] / 4096, read on the device.  A long stream is therefore spread over as many
//                  workgroups as it has chunks, and the grid does not depend on the data.  A workgroup finds the streams
//                  of its chunk's first and last byte by binary search in out_offsets (uniform), each thread then its own
//                  word's stream inside that range.  A word that lies inside one stream is one 16-byte store of bytes
//                  read as five aligned 4-byte words around the (unaligned) source range and shifted into place; a word
//                  that crosses a stream boundary, the last word of the batch, and a word whose five source words would
//                  reach past the end of the blob go byte by byte.  Nothing is read outside the blob (no padding of the
//                  allocation is needed: the blob starts 4-byte aligned, so the aligned read never starts before it) and
//                  nothing is written at or past out_offsets[n].
//
// The index, bounds and chunking arithmetic and the per-thread work are in ndp::store, __host__ __device__:
// tests/store_gather_host_driver.hip runs exactly these functions by this schedule on the CPU.
namespace ndp {
namespace store {

constexpr int kStateDim = 25, kActionDim = 4, kGoalDim = 3;
constexpr int kScanThreads = 1024;
constexpr int kCopyThreads = 256;
constexpr int kWordBytes = 16;
constexpr int64_t kChunkBytes = (int64_t)kCopyThreads * kWordBytes;      // 4096
constexpr int kMaxCopyBlocks = 2048;
constexpr int kMaxRowBlocks = 1024;
constexpr int64_t kMaxStreams = 1 << 22;

struct Args {
  const uint8_t* blob; int64_t blob_bytes;
  const int64_t* frame_offsets;                       // [n_traj * steps + 1]
  const uint32_t* states; const uint32_t* actions; const uint32_t* goal;       // float tables as 4-byte words
  int64_t n_traj; int steps;
  const int64_t* indices; int64_t batch; int seq_start; int seq_length;
  uint8_t* out_buffer; int64_t capacity;
  int64_t* out_offsets;                               // [batch * seq_length + 1]
  uint32_t* out_states; uint32_t* out_actions; uint32_t* out_goal;
  int32_t* status;
};

__host__ __device__ inline int64_t n_streams(const Args& a) { return a.batch * (int64_t)a.seq_length; }
__host__ __device__ inline bool valid_index(int64_t idx, int64_t n_traj) { return idx >= 0 && idx < n_traj; }

// the store's frame number of stream s of the batch, or -1 when its trajectory index is out of range
__host__ __device__ inline int64_t source_frame(const Args& a, int64_t s) {
  const uint32_t b = (uint32_t)s / (uint32_t)a.seq_length, t = (uint32_t)s - b * (uint32_t)a.seq_length;    // s < 2^22
  const int64_t idx = a.indices[b];
  if (!valid_index(idx, a.n_traj)) return -1;
  return idx * a.steps + a.seq_start + t;
}

__host__ __device__ inline int64_t stream_length(const Args& a, int64_t s) {
  const int64_t f = source_frame(a, s);
  if (f < 0) return 0;
  const int64_t len = a.frame_offsets[f + 1] - a.frame_offsets[f];
  return len > 0 ? len : 0;
}

// the scan's schedule: thread t owns streams [t * per, min(n, (t + 1) * per))
__host__ __device__ inline int64_t scan_run(int64_t n) { return (n + kScanThreads - 1) / kScanThreads; }

__host__ __device__ inline int64_t scan_run_sum(const Args& a, int64_t n, int t) {
  const int64_t per = scan_run(n), lo = t * per, hi = lo + per < n ? lo + per : n;
  int64_t sum = 0;
  for (int64_t s = lo; s < hi; ++s) sum += stream_length(a, s);
  return sum;
}

// writes the run's offsets from its exclusive base; the thread that owns the last stream also writes out_offsets[n]
__host__ __device__ inline void scan_run_write(const Args& a, int64_t n, int t, int64_t base) {
  const int64_t per = scan_run(n), lo = t * per, hi = lo + per < n ? lo + per : n;
  for (int64_t s = lo; s < hi; ++s) {
    a.out_offsets[s] = base;
    base += stream_length(a, s);
  }
  if (lo < n && hi == n) a.out_offsets[n] = base;
}

__host__ __device__ inline bool any_bad_index(const Args& a, int t) {
  bool bad = false;
  for (int64_t b = t; b < a.batch; b += kScanThreads) bad = bad || !valid_index(a.indices[b], a.n_traj);
  return bad;
}

// the row gather: word e of a table of `width` floats a step (width * seq_length words per trajectory of the batch)
__host__ __device__ inline int64_t row_words(const Args& a) {
  return a.batch * ((int64_t)a.seq_length * (kStateDim + kActionDim) + kGoalDim);
}
__host__ __device__ inline int row_blocks(const Args& a) {
  const int64_t b = (row_words(a) + kScanThreads - 1) / kScanThreads;
  return (int)(b < kMaxRowBlocks ? b : kMaxRowBlocks);
}
__host__ __device__ inline void gather_table(const Args& a, const uint32_t* table, uint32_t* out, int width, int64_t e) {
  const uint32_t per = (uint32_t)a.seq_length * (uint32_t)width;           // e < 2^22 * 25
  const uint32_t b = (uint32_t)e / per, r = (uint32_t)e - b * per;
  const int64_t idx = a.indices[b];
  out[e] = valid_index(idx, a.n_traj) ? table[(idx * a.steps + a.seq_start) * width + r] : 0u;
}
// word e of the three tables laid end to end: states, then actions, then goal
__host__ __device__ inline void gather_row_word(const Args& a, int64_t e) {
  const int64_t ns = a.batch * (int64_t)a.seq_length * kStateDim, na = a.batch * (int64_t)a.seq_length * kActionDim;
  if (e < ns) {
    gather_table(a, a.states, a.out_states, kStateDim, e);
  } else if (e < ns + na) {
    gather_table(a, a.actions, a.out_actions, kActionDim, e - ns);
  } else {
    const int64_t g = e - ns - na;
    const uint32_t b = (uint32_t)g / (uint32_t)kGoalDim, c = (uint32_t)g - b * (uint32_t)kGoalDim;
    const int64_t idx = a.indices[b];
    a.out_goal[g] = valid_index(idx, a.n_traj) ? a.goal[idx * kGoalDim + c] : 0u;
  }
}

// the copy's schedule
__host__ __device__ inline int64_t chunk_count(int64_t total_bytes) { return (total_bytes + kChunkBytes - 1) / kChunkBytes; }
__host__ __device__ inline int copy_blocks(int64_t capacity) {
  const int64_t c = chunk_count(capacity);
  return (int)(c < 1 ? 1 : c < kMaxCopyBlocks ? c : kMaxCopyBlocks);
}

// the stream that holds destination byte d (0 <= d < off[n]): the largest s in [lo, hi] with off[s] <= d; the caller
// guarantees off[lo] <= d.  A zero-length stream never holds a byte: of equal offsets the last one wins.
__host__ __device__ inline int64_t stream_of(const int64_t* off, int64_t lo, int64_t hi, int64_t d) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= d) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// where stream s starts in the blob (s holds at least one byte, so its frame is valid)
__host__ __device__ inline int64_t source_start(const Args& a, int64_t s) { return a.frame_offsets[source_frame(a, s)]; }

struct Word { uint32_t w[4]; };

// 16 bytes from src (any alignment), read as five 4-byte words from src rounded down to a multiple of 4; the caller has
// checked that those 20 bytes lie inside the blob
__host__ __device__ inline Word realigned_read(const uint8_t* blob, int64_t src) {
  const int64_t a0 = src & ~(int64_t)3;
  const int sh = (int)(src & 3) * 8;
  uint32_t r[5];
  __builtin_memcpy(r, __builtin_assume_aligned(blob + a0, 4), sizeof(r));
  Word v;
  for (int i = 0; i < 4; ++i) v.w[i] = (uint32_t)((((uint64_t)r[i + 1] << 32) | r[i]) >> sh);
  return v;
}

// destination bytes [d, min(d + 16, total)), d a multiple of 16; [s_lo, s_hi] brackets the stream of byte d
__host__ __device__ inline void copy_word(const Args& a, int64_t n, int64_t total, int64_t s_lo, int64_t s_hi, int64_t d) {
  if (d >= total) return;
  int64_t s = stream_of(a.out_offsets, s_lo, s_hi, d);
  int64_t begin = a.out_offsets[s], end = a.out_offsets[s + 1];
  int64_t src = source_start(a, s) + (d - begin);
  if (d + kWordBytes <= end && d + kWordBytes <= total && (src & ~(int64_t)3) + 20 <= a.blob_bytes) {
    const Word v = realigned_read(a.blob, src);
    __builtin_memcpy(__builtin_assume_aligned(a.out_buffer + d, 16), v.w, kWordBytes);
    return;
  }
  const int64_t stop = d + kWordBytes < total ? d + kWordBytes : total;
  for (int64_t p = d; p < stop; ++p) {
    if (p >= end) {                                   // the next stream that holds a byte (p < total: there is one)
      do { ++s; } while (s + 1 < n && a.out_offsets[s + 1] <= p);
      begin = a.out_offsets[s];
      end = a.out_offsets[s + 1];
      src = source_start(a, s) + (p - begin);
    }
    if (src >= 0 && src < a.blob_bytes) a.out_buffer[p] = a.blob[src];
    ++src;
  }
}

}  // namespace store

__global__ __launch_bounds__(store::kScanThreads) void k_store_scan(store::Args a) {
  using namespace store;
  const int t = threadIdx.x;
  if (blockIdx.x > 0) {                               // the float tables
    const int64_t words = row_words(a), stride = (int64_t)(gridDim.x - 1) * kScanThreads;
    for (int64_t e = (int64_t)(blockIdx.x - 1) * kScanThreads + t; e < words; e += stride) gather_row_word(a, e);
    return;
  }
  __shared__ int64_t sums[kScanThreads];
  __shared__ int bad;
  if (t == 0) bad = 0;
  const int64_t n = n_streams(a);
  const int64_t mine = scan_run_sum(a, n, t);
  sums[t] = mine;
  __syncthreads();
  if (any_bad_index(a, t)) bad = 1;                   // every writer writes 1
  for (int d = 1; d < kScanThreads; d <<= 1) {        // inclusive scan of the run sums
    const int64_t v = t >= d ? sums[t - d] : 0;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  scan_run_write(a, n, t, sums[t] - mine);
  if (t == 0) *a.status = bad | (sums[kScanThreads - 1] > a.capacity ? 2 : 0);
}

__global__ __launch_bounds__(store::kCopyThreads) void k_store_copy(store::Args a) {
  using namespace store;
  const int64_t n = n_streams(a);
  const int64_t total = a.out_offsets[n] < a.capacity ? a.out_offsets[n] : a.capacity;      // status 2: does not fit
  const int64_t chunks = chunk_count(total);
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t d0 = c * kChunkBytes;
    const int64_t last = d0 + kChunkBytes - 1 < total - 1 ? d0 + kChunkBytes - 1 : total - 1;
    const int64_t s_lo = stream_of(a.out_offsets, 0, n - 1, d0);
    const int64_t s_hi = stream_of(a.out_offsets, s_lo, n - 1, last);
    copy_word(a, n, total, s_lo, s_hi, d0 + (int64_t)threadIdx.x * kWordBytes);
  }
}

}  // namespace ndp

extern "C" {

int ndp_store_gather(const uint8_t* blob, int64_t blob_bytes, const int64_t* frame_offsets, const float* states,
                     const float* actions, const float* goal, int64_t n_traj, int steps, const int64_t* indices,
                     int64_t batch, int seq_start, int seq_length, uint8_t* out_buffer, int64_t capacity,
                     int64_t* out_offsets, float* out_states, float* out_actions, float* out_goal, int32_t* status,
                     void* stream) {
  using namespace ndp;
  NDP_CHECK_ARG(frame_offsets && states && actions && goal && indices && out_offsets && out_states && out_actions &&
                out_goal && status, "ndp_store_gather: null pointer");
  NDP_CHECK_ARG(n_traj >= 1 && steps >= 1 && n_traj * (int64_t)steps <= store::kMaxStreams,
                "ndp_store_gather: bad store size (%lld trajectories of %d steps)", (long long)n_traj, steps);
  NDP_CHECK_ARG(batch >= 1 && seq_start >= 0 && seq_length >= 1 && seq_start + (int64_t)seq_length <= steps,
                "ndp_store_gather: bad window (batch %lld, seq_start %d, seq_length %d of %d steps)", (long long)batch,
                seq_start, seq_length, steps);
  NDP_CHECK_ARG(batch * (int64_t)seq_length <= store::kMaxStreams, "ndp_store_gather: %lld streams in one batch",
                (long long)(batch * (int64_t)seq_length));
  NDP_CHECK_ARG(blob_bytes >= 0 && capacity >= 0 && (blob || blob_bytes == 0) && (out_buffer || capacity == 0),
                "ndp_store_gather: bad buffer sizes (blob %lld, capacity %lld) or null pointer", (long long)blob_bytes,
                (long long)capacity);
  NDP_CHECK_ARG((reinterpret_cast<uintptr_t>(blob) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_buffer) & 15) == 0,
                "ndp_store_gather: blob must be 4-byte aligned and out_buffer 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  store::Args a{blob, blob_bytes, frame_offsets, reinterpret_cast<const uint32_t*>(states),
                reinterpret_cast<const uint32_t*>(actions), reinterpret_cast<const uint32_t*>(goal), n_traj, steps,
                indices, batch, seq_start, seq_length, out_buffer, capacity, out_offsets,
                reinterpret_cast<uint32_t*>(out_states), reinterpret_cast<uint32_t*>(out_actions),
                reinterpret_cast<uint32_t*>(out_goal), status};
  {
    KTimer kt("k_store_scan", st);
    hipLaunchKernelGGL(k_store_scan, dim3(1 + store::row_blocks(a)), dim3(store::kScanThreads), 0, st, a);
    const int rc = check_launch("k_store_scan");
    if (rc != NDP_OK) return rc;
  }
  KTimer kt("k_store_copy", st);
  hipLaunchKernelGGL(k_store_copy, dim3(store::copy_blocks(capacity)), dim3(store::kCopyThreads), 0, st, a);
  return check_launch("k_store_copy");
}

}  // extern "C"
