// store_gather.inc -- the trajectory store's batch gather (k_store_scan, k_store_copy, csrc/ndp_store.inc)
// run on the CPU, for tests/test_store_gather_host.py.  main.hip includes it behind the library's source (see there); it
// calls the __host__ __device__ functions the kernels call (store::scan_run_sum, any_bad_index, scan_run_write,
// row_blocks, gather_row_word, copy_blocks, chunk_count, stream_of, copy_word) by the kernels' schedule: workgroup 0 of
// k_store_scan with its 1024 threads' runs, the row workgroups' grid-stride loops, then k_store_copy's workgroups, each
// walking its chunks and its 256 threads their 16-byte words.  What the kernels do outside those functions -- the LDS
// scan of the 1024 run sums (restated here as a serial prefix sum), the loops over threads and chunks -- is tested as a
// copy; a slip in the device's own form of those is seen only by the GPU test (tests/test_gpu_trajectory_store.py).  It
// makes no HIP runtime call and needs no GPU.
//
// Usage: host_driver store_gather IN OUT
//   IN   int64 N, T, blob bytes; frame offsets int64 [N*T+1]; states float [N*T*25]; actions float [N*T*4]; goal float
//        [N*3]; the blob; int64 cases; per case int64 B, seq_start, seq_length, capacity, then indices int64 [B]
//   OUT  per case: int64 status, int64 count of changed bytes in out_buffer[offsets[n] .. capacity), offsets int64 [n+1],
//        states float [n*25], actions float [n*4], goal float [B*3], then the offsets[n] used bytes of the buffer
// Every buffer is an allocation of exactly its size (the blob is NOT padded: the store does not pad it either), so a
// sanitizer sees any access past it; the output buffer is filled with the canary 0xC5 before the run.
namespace host::store_gather {

using namespace ndp::store;

constexpr uint8_t kCanary = 0xC5;

void run_scan(const Args& a) {
  const int64_t n = n_streams(a);
  Exact<int64_t> sums(kScanThreads);
  int bad = 0;
  for (int t = 0; t < kScanThreads; ++t) sums.p[t] = scan_run_sum(a, n, t);
  for (int t = 0; t < kScanThreads; ++t) if (any_bad_index(a, t)) bad = 1;
  int64_t base = 0;
  for (int t = 0; t < kScanThreads; ++t) {                          // the exclusive scan of the run sums
    scan_run_write(a, n, t, base);
    base += sums.p[t];
  }
  *a.status = bad | (base > a.capacity ? 2 : 0);
  const int blocks = row_blocks(a);
  const int64_t words = row_words(a), stride = (int64_t)blocks * kScanThreads;
  for (int b = 0; b < blocks; ++b)
    for (int t = 0; t < kScanThreads; ++t)
      for (int64_t e = (int64_t)b * kScanThreads + t; e < words; e += stride) gather_row_word(a, e);
}

void run_copy(const Args& a) {
  const int64_t n = n_streams(a);
  const int grid = copy_blocks(a.capacity);
  for (int block = 0; block < grid; ++block) {
    const int64_t total = a.out_offsets[n] < a.capacity ? a.out_offsets[n] : a.capacity;
    const int64_t chunks = chunk_count(total);
    for (int64_t c = block; c < chunks; c += grid) {
      const int64_t d0 = c * kChunkBytes;
      const int64_t last = d0 + kChunkBytes - 1 < total - 1 ? d0 + kChunkBytes - 1 : total - 1;
      const int64_t s_lo = stream_of(a.out_offsets, 0, n - 1, d0);
      const int64_t s_hi = stream_of(a.out_offsets, s_lo, n - 1, last);
      for (int t = 0; t < kCopyThreads; ++t) copy_word(a, n, total, s_lo, s_hi, d0 + (int64_t)t * kWordBytes);
    }
  }
}

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  int64_t head[3];
  if (!read_pod(in, &head)) return kBadInput;
  const int64_t N = head[0], T = head[1], blob_bytes = head[2];
  if (N < 1 || T < 1 || blob_bytes < 0 || N * T > kMaxStreams) return kBadInput;
  const size_t frames = (size_t)(N * T);
  Exact<int64_t> frame_offsets(frames + 1);
  Exact<float> states(frames * kStateDim), actions(frames * kActionDim), goal((size_t)N * kGoalDim);
  Exact<uint8_t> blob((size_t)blob_bytes);
  if (!frame_offsets.read(in) || !states.read(in) || !actions.read(in) || !goal.read(in) || !blob.read(in)) return kBadInput;
  int64_t cases = 0;
  if (!read_pod(in, &cases) || cases < 0) return kBadInput;
  for (int64_t ci = 0; ci < cases; ++ci) {
    int64_t h[4];
    if (!read_pod(in, &h)) return kBadInput;
    const int64_t B = h[0], seq_start = h[1], seq_length = h[2], capacity = h[3];
    if (B < 1 || seq_start < 0 || seq_length < 1 || seq_start + seq_length > T || capacity < 0) return kBadInput;
    const size_t n = (size_t)(B * seq_length);
    if ((int64_t)n > kMaxStreams) return kBadInput;
    Exact<int64_t> indices((size_t)B), out_offsets(n + 1);
    if (!indices.read(in)) return kBadInput;
    Exact<uint8_t> buffer((size_t)capacity);
    buffer.fill(kCanary);
    Exact<float> out_states(n * kStateDim), out_actions(n * kActionDim), out_goal((size_t)B * kGoalDim);
    Exact<int32_t> status(1);
    Args a{blob.p, blob_bytes, frame_offsets.p, reinterpret_cast<const uint32_t*>(states.p),
           reinterpret_cast<const uint32_t*>(actions.p), reinterpret_cast<const uint32_t*>(goal.p), N, (int)T, indices.p, B,
           (int)seq_start, (int)seq_length, buffer.p, capacity, out_offsets.p, reinterpret_cast<uint32_t*>(out_states.p),
           reinterpret_cast<uint32_t*>(out_actions.p), reinterpret_cast<uint32_t*>(out_goal.p), status.p};
    run_scan(a);
    run_copy(a);
    const int64_t used = out_offsets.p[n] < capacity ? out_offsets.p[n] : capacity;
    int64_t changed = 0;
    for (int64_t i = used; i < capacity; ++i) changed += buffer.p[i] != kCanary;
    const int64_t st = status.p[0];
    fwrite(&st, 8, 1, out);
    fwrite(&changed, 8, 1, out);
    out_offsets.write(out);
    out_states.write(out);
    out_actions.write(out);
    out_goal.write(out);
    buffer.write(out, (size_t)used);
  }
  return close_files(in, out);
}

}  // namespace host::store_gather
