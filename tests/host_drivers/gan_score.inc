// gan_score.inc -- the generator scoring kernel (k_gan_score, csrc/ndp_eval.inc) run on the CPU, for
// tests/test_gan_score_host.py.  main.hip includes it behind the library's source (see there); it calls the __host__
// __device__ functions the kernel calls (gan_score::block_threads, rows_per_block, lds_bytes, sample_error, add_squares,
// distance, hinge, sigmoid, better_min, better_max) by the kernel's schedule: blocks of rows_per_block(K) rows, the
// rows' samples, noise and logits staged "in LDS", pass 1 (e_k, the fp32 row sums, the fp64 distance sums), pass 2 (the
// hinge terms), then each row's serial walk over its K samples.  What k_gan_score does outside those functions -- the
// loops, the barriers' phases, the LDS carving -- is restated here and tested as a copy; a slip in the device's own form
// of those is seen only by the GPU tests (tests/test_gpu_gan_eval.py).  It makes no HIP runtime call and needs no GPU.
//
// Usage: host_driver gan_score IN OUT
//   IN   int32 cases, then per case 7 int32 (n, K, nz, has action, has noise, has logits, output mask: bit o set = output
//        o wanted, in the order of ndp_gan_score's arguments), action_hat n x K x 4 floats, action n x 4 floats if
//        present, noise n x K x nz floats if present, logits n x K floats if present
//   OUT  per case the ten outputs in argument order, each of its full size: sample_err [n,K], mean_err [n], best_err [n],
//        best_k [n] int32, best_curve [n,K], spread [n], ndiv [n], d_fake_prob [n], d_pick_k [n] int32, d_pick_err [n];
//        an output that was not wanted holds the sentinel -7
// Every buffer -- inputs, outputs, each LDS array -- is an allocation of exactly its size, so a sanitizer sees any access
// past it; an input or output that is absent is a null pointer.
namespace host::gan_score {

using namespace ndp::gan_score;

// k_gan_score for the workgroup `block`
void score_block(const ndp::GanScoreArgs& a, int64_t block) {
  const int k = a.k, nz = a.nz, G = a.rows_per_block, slots = G * k;
  Exact<double> hs(slots), ds(slots);
  Exact<float> xs((size_t)slots * kActionDim), zs((size_t)slots * nz), sx(slots), sz(slots), es(slots), ls(slots);
  if (lds_bytes(slots, nz) != (hs.n + ds.n) * sizeof(double) + (xs.n + zs.n + sx.n + sz.n + es.n + ls.n) * sizeof(float)) abort();
  const int nthreads = block_threads(k);
  const int64_t n0 = block * G;
  const int nrows = (int)((a.n - n0) < G ? (a.n - n0) : G);
  const int nact = nrows * k;
  const bool pairs = a.spread != nullptr || a.ndiv != nullptr;
  for (int t = 0; t < nthreads; ++t) {                              // up to the first barrier
    for (int idx = t; idx < nact * kActionDim; idx += nthreads) xs.p[idx] = a.x[n0 * k * kActionDim + idx];
    if (a.ndiv != nullptr)
      for (int idx = t; idx < nact * nz; idx += nthreads) zs.p[idx] = a.z[n0 * k * nz + idx];
    if (a.logits != nullptr)
      for (int idx = t; idx < nact; idx += nthreads) ls.p[idx] = a.logits[n0 * k + idx];
  }
  for (int t = 0; t < nact; ++t) {                                  // pass 1
    const int g = t / k;
    const int64_t row = n0 + g;
    if (a.action != nullptr) {
      const float e = sample_error(xs.p + t * kActionDim, a.action + row * kActionDim);
      es.p[t] = e;
      if (a.sample_err != nullptr) a.sample_err[n0 * k + t] = e;
    }
    if (pairs) {
      float ssx = 0.f, ssz = 0.f;
      double dsum = 0.0;
      for (int j = 0; j < k; ++j) {
        const float dx = distance(xs.p + t * kActionDim, xs.p + (g * k + j) * kActionDim, kActionDim);
        ssx += dx;
        dsum += (double)dx;
        if (a.ndiv != nullptr) ssz += distance(zs.p + t * nz, zs.p + (g * k + j) * nz, nz);
      }
      sx.p[t] = ssx;
      sz.p[t] = ssz;
      ds.p[t] = dsum;
    }
  }
  if (a.ndiv != nullptr)
    for (int t = 0; t < nact; ++t) {                                // pass 2
      const int g = t / k;
      const float sxi = sx.p[t], szi = sz.p[t];
      double h = 0.0;
      for (int j = 0; j < k; ++j) {
        const float dx = distance(xs.p + t * kActionDim, xs.p + (g * k + j) * kActionDim, kActionDim);
        const float dz = distance(zs.p + t * nz, zs.p + (g * k + j) * nz, nz);
        h += (double)hinge(dz, szi, dx, sxi);
      }
      hs.p[t] = h;
    }
  for (int g = 0; g < nrows; ++g) {                                 // the row's thread 0
    const int s0 = g * k;
    const int64_t row = n0 + g;
    if (a.action != nullptr) {
      double sum = 0.0;
      float best = es.p[s0];
      int bk = 0;
      for (int i = 0; i < k; ++i) {
        if (a.mean_err != nullptr) sum = add_squares(sum, xs.p + (s0 + i) * kActionDim, a.action + row * kActionDim);
        if (better_min(es.p[s0 + i], best)) { best = es.p[s0 + i]; bk = i; }
        if (a.best_curve != nullptr) a.best_curve[row * k + i] = best;
      }
      if (a.mean_err != nullptr) a.mean_err[row] = (float)(sum / (double)(k * kActionDim));
      if (a.best_err != nullptr) a.best_err[row] = best;
      if (a.best_k != nullptr) a.best_k[row] = bk;
    }
    if (a.spread != nullptr) {
      double sum = 0.0;
      for (int i = 0; i < k; ++i) sum += ds.p[s0 + i];
      a.spread[row] = (float)(sum / ((double)k * (double)(k - 1)));
    }
    if (a.ndiv != nullptr) {
      double sum = 0.0;
      for (int i = 0; i < k; ++i) sum += hs.p[s0 + i];
      a.ndiv[row] = (float)sum;
    }
    if (a.logits != nullptr) {
      double sum = 0.0;
      float top = ls.p[s0];
      int pk = 0;
      for (int i = 0; i < k; ++i) {
        if (a.d_fake_prob != nullptr) sum += (double)sigmoid(ls.p[s0 + i]);
        if (better_max(ls.p[s0 + i], top)) { top = ls.p[s0 + i]; pk = i; }
      }
      if (a.d_fake_prob != nullptr) a.d_fake_prob[row] = (float)(sum / (double)k);
      if (a.d_pick_k != nullptr) a.d_pick_k[row] = pk;
      if (a.d_pick_err != nullptr) a.d_pick_err[row] = es.p[s0 + pk];
    }
  }
}

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  int32_t cases = 0;
  if (!read_pod(in, &cases) || cases < 0) return kBadInput;
  for (int32_t ci = 0; ci < cases; ++ci) {
    int32_t h[7];
    if (!read_pod(in, &h)) return kBadInput;
    const int n = h[0], k = h[1], nz = h[2], mask = h[6];
    if (n < 1 || k < 1 || k > 256 || nz < 1 || nz > kMaxNoise) return kBadInput;
    const size_t rows = (size_t)n, flat = rows * k;
    Exact<float> x(flat * kActionDim), action(h[3] ? rows * kActionDim : 0), noise(h[4] ? flat * nz : 0), logits(h[5] ? flat : 0);
    if (!x.read(in) || !action.read(in) || !noise.read(in) || !logits.read(in)) return kBadInput;
    auto want = [mask](int o) { return (mask >> o) & 1; };
    // exact-size outputs for the kernel (absent: null) and full-size, sentinel-filled ones for the report
    Exact<float> sample_err(want(0) ? flat : 0), mean_err(want(1) ? rows : 0), best_err(want(2) ? rows : 0);
    Exact<int32_t> best_k(want(3) ? rows : 0);
    Exact<float> best_curve(want(4) ? flat : 0), spread(want(5) ? rows : 0), ndiv(want(6) ? rows : 0), d_fake_prob(want(7) ? rows : 0);
    Exact<int32_t> d_pick_k(want(8) ? rows : 0);
    Exact<float> d_pick_err(want(9) ? rows : 0);
    const int G = rows_per_block(k);
    ndp::GanScoreArgs a{x.p, action.p, ndiv.p ? noise.p : nullptr, logits.p, n, k, ndiv.p ? nz : 0, G,
                        sample_err.p, mean_err.p, best_err.p, best_k.p, best_curve.p, spread.p, ndiv.p, d_fake_prob.p,
                        d_pick_k.p, d_pick_err.p};
    for (int64_t b = 0; b < (n + G - 1) / G; ++b) score_block(a, b);
    auto put_f = [&](const Exact<float>& e, size_t count) {
      if (e.p) { e.write(out); return; }
      Exact<float> s(count);
      s.fill(-7.0f);
      s.write(out);
    };
    auto put_i = [&](const Exact<int32_t>& e, size_t count) {
      if (e.p) { e.write(out); return; }
      Exact<int32_t> s(count);
      s.fill(-7);
      s.write(out);
    };
    put_f(sample_err, flat); put_f(mean_err, rows); put_f(best_err, rows); put_i(best_k, rows); put_f(best_curve, flat);
    put_f(spread, rows); put_f(ndiv, rows); put_f(d_fake_prob, rows); put_i(d_pick_k, rows); put_f(d_pick_err, rows);
  }
  return close_files(in, out);
}

}  // namespace host::gan_score
