// step_plan.inc -- what the host decides about a GAN step before it launches anything (csrc/ndp_capi.inc: the network
// tables g_mlp / d_mlp, step_plan, build_jobs, fill_reduce), for tests/test_step_plan_host.py.  main.hip includes it behind
// the library's source.  Host arithmetic only: no kernel is replayed and no HIP runtime call is made; the workspaces, codes
// and noise are address ranges without access rights, so that a pointer can be named as (space, float offset) and a touch
// would fault.
//
// Usage: host_driver step_plan IN OUT
//   IN   int32 queries, then per query 5 int32: kind, flat, K, nz, first
//        kind 0  a step at (flat, K, nz); first: 1 the first D step of an iteration, 0 a repeat
//        kind 1  the module-level backward calls (ndp_g_backward, ndp_d_backward) at m = flat rows, code_rep K, noise_dim nz
//        kind 3  the variant lists of the phase kernels
//        kind 2  the step entry points' answers to a configuration they must refuse (first = -1: a null configuration)
//   OUT  int64 values.  kind 2: the return values of ndp_step_workspace_floats, ndp_step_workspace_offset (tensor 0),
//        ndp_step_d_grads, ndp_step_g_grads, ndp_step_pack_params, ndp_step_apply_adam.  kind 3: the entries of kPhaseA, then
//        per entry (ring, NR); the entries of kPhaseB, then per entry (ring, preload, NR).  kind 0 and 1, in this order:
//          plan     kPlan values (test_step_plan_host.py: PLAN; -1 where the query has no such launch)
//          layouts  per network (G, D): w[5], b[5], total; packed copies fwd[4], dg[4], total
//          offsets  ndp_step_workspace_offset of the 12 tensors (kind 1: -1)
//          regions  kRegions x (space, begin, end): the tensors of the workspaces (REGIONS; space -1: none)
//          jobs     per network: njobs, nwide, wide_chunks, nchunks, then per job kJob values (JOB; pointers as space, offset)
//          reduce   per network: slab count, n, regions, then 4 x (begin, end, slabs)
// Spaces: 0 the step's workspace, 1 codes, 2 noise, 3 / 4 / 5 the acts, G and D workspaces of the module-level calls.
#include <sys/mman.h>

namespace host::step_plan {

constexpr int kPlan = 37, kRegions = 27, kJob = 22, kSpaces = 6;

struct Space {
  float* base = nullptr; size_t bytes = 0;
  explicit Space(int64_t floats) : bytes(((size_t)floats * sizeof(float) + 4095) / 4096 * 4096 + 4096) {
    void* p = mmap(nullptr, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) abort();
    base = static_cast<float*>(p);
  }
  ~Space() { munmap(base, bytes); }
  Space(const Space&) = delete;
};

struct Report {
  int64_t plan[kPlan], layout[2][20], offsets[NDP_STEP_TENSORS], region[kRegions][3];
  ndp::WgradArgs jobs[2];
  ndp::ReduceArgs red[2];
  const float* base[kSpaces]; int64_t floats[kSpaces];
};

static void name(const Report& r, const float* p, int64_t* out) {
  out[0] = -1; out[1] = 0;
  for (int s = 0; s < kSpaces; ++s)
    if (r.base[s] && p >= r.base[s] && p < r.base[s] + r.floats[s]) { out[0] = s; out[1] = p - r.base[s]; }
}

static void layouts(Report& r, int nz) {
  const ndp::Mlp net[2] = {ndp::g_mlp(nz), ndp::d_mlp()};
  for (int n = 0; n < 2; ++n) {
    const ndp::MlpLayout L = ndp::layout(net[n]);
    const ndp::PackOffsets P = ndp::pack_offsets(net[n]);
    int64_t* o = r.layout[n];
    for (int l = 0; l < 5; ++l) { o[l] = l < net[n].layers ? L.w[l] : 0; o[5 + l] = l < net[n].layers ? L.b[l] : 0; }
    o[10] = L.total;
    for (int l = 0; l < 4; ++l) { o[11 + l] = l + 1 < net[n].layers ? P.fwd[l] : -1; o[15 + l] = l + 1 < net[n].layers ? P.dg[l] : -1; }
    o[19] = P.total;
  }
}

// the regions of the three sub-layouts, in the order of REGIONS
static void regions(Report& r, const ndp::GActs& a, int sa, const ndp::GBwdWs& g, int sg, const ndp::DBwdWs& d, int sd) {
  int i = 0;
  auto put = [&](int space, int64_t begin, int64_t end) { r.region[i][0] = space; r.region[i][1] = begin; r.region[i][2] = end; ++i; };
  for (int l = 0; l < 4; ++l) put(sa, a.h[l], l < 3 ? a.h[l + 1] : a.end);
  for (int l = 0; l < 5; ++l) put(sg, g.dy[l], l < 4 ? g.dy[l + 1] : g.slabs);
  put(sg, g.slabs, g.end);
  put(sd, d.xa, d.h[0]);
  for (int l = 0; l < 3; ++l) put(sd, d.h[l], l < 2 ? d.h[l + 1] : d.dy[0]);
  for (int l = 0; l < 4; ++l) put(sd, d.dy[l], l < 3 ? d.dy[l + 1] : d.slabs);
  put(sd, d.slabs, d.lossp);
  put(sd, d.lossp, d.end);
  for (; i < kRegions; ++i) r.region[i][0] = -1, r.region[i][1] = r.region[i][2] = 0;
}

static void chunk_counts(int64_t* plan, const ndp::NetPlan& g, const ndp::NetPlan& d) {
  const int v[8] = {g.heavy, g.light, g.wide, g.slabs, d.heavy, d.light, d.wide, d.slabs};
  for (int i = 0; i < 8; ++i) plan[4 + i] = v[i];
}

static void step(Report& r, const ndp_step_config& c, bool first, float* ws, const float* codes, const float* noise) {
  const ndp::StepPlan p = ndp::step_plan(&c, first);
  const int K = c.num_sample, nz = c.noise_dim;
  ndp::build_g_jobs(r.jobs[0], nz, ws, p.gw, ws, p.acts, codes, ndp::CODE, K, noise, nz, p.m, ws + p.g_seg);
  ndp::build_d_jobs(r.jobs[1], ws, p.dw, codes, ndp::CODE, K, p.m, p.mpad, first ? ws + p.d_seg : nullptr, p.rpad);
  ndp_step_buffers b;
  memset(&b, 0, sizeof(b));
  b.workspace = ws;
  ndp_step_config cfg = c;
  cfg.p2p = nullptr;
  ndp::fill_step_reduce("step_plan", r.red[0], &cfg, &b, p, 1, r.jobs[0]);
  ndp::fill_step_reduce("step_plan", r.red[1], &cfg, &b, p, 0, r.jobs[1]);
  const ndp::Variant<ndp::PhaseBArgs>& vb = ndp::kPhaseB[p.phase_b];
  const int64_t np = ndp::layout(ndp::g_mlp(nz)).total, nd = ndp::layout(ndp::d_mlp()).total;
  const int64_t plan[kPlan] = {
      p.m, p.mpad, p.rpad, p.d_rows, 0, 0, 0, 0, 0, 0, 0, 0, p.seg_s, p.seg_entries, p.ndiv_fused, p.ndiv_threads, p.ndiv_blocks,
      p.d_front_grid, first ? ndp::kPhaseA[p.phase_a].t[0] : -1, first ? ndp::kPhaseA[p.phase_a].t[1] : -1,
      p.phase_b_grid, vb.t[0], vb.t[2], vb.t[1],
      p.wgrad_d_grid, r.jobs[1].nwide != 0, p.wgrad_g_grid, r.jobs[0].nwide != 0, p.reduce_d_grid, p.reduce_g_grid,
      p.ndiv_fused ? 0 : p.ndiv_blocks, ndp::blocks_of(np), ndp::blocks_of(nd), p.loss_count_d, p.loss_count_g, p.ndiv_blocks, p.floats};
  memcpy(r.plan, plan, sizeof(plan));
  chunk_counts(r.plan, p.gw.plan, p.dw.plan);
  for (int t = 0; t < NDP_STEP_TENSORS; ++t) r.offsets[t] = ndp_step_workspace_offset(&c, t);
  regions(r, p.acts, 0, p.gw, 0, p.dw, 0);
  const int64_t rest[8] = {p.d_action, p.nd_grad, p.nd_part, p.g_packed, p.d_packed, p.d_seg, p.g_seg, p.floats};
  for (int i = 0; i < 7; ++i) { r.region[20 + i][0] = 0; r.region[20 + i][1] = rest[i]; r.region[20 + i][2] = rest[i + 1]; }
}

static void module_calls(Report& r, int64_t m, int code_rep, int nz, float* acts, float* gws, float* dws, const float* codes,
                   const float* noise) {
  const int64_t mpad = ndp::pad_rows(m);
  const ndp::GActs a = ndp::g_acts(0, mpad);
  const ndp::GBwdWs g = ndp::g_bwd_ws(0, mpad, nz);
  const ndp::DBwdWs d = ndp::d_bwd_ws(0, mpad);
  ndp::build_g_jobs(r.jobs[0], nz, gws, g, acts, a, codes, ndp::CODE, code_rep, noise, nz, m, nullptr);
  ndp::build_d_jobs(r.jobs[1], dws, d, codes, ndp::CODE, code_rep, m, mpad, nullptr, 0);
  const int64_t np = ndp::layout(ndp::g_mlp(nz)).total, nd = ndp::layout(ndp::d_mlp()).total;
  ndp::fill_reduce("step_plan", r.red[0], gws + g.slabs, g.slab_stride, np, g.plan, &r.jobs[0], nullptr, nullptr, nullptr, nullptr, 1);
  ndp::fill_reduce("step_plan", r.red[1], dws + d.slabs, d.slab_stride, nd, d.plan, &r.jobs[1], nullptr, nullptr, nullptr, nullptr, 0);
  for (int i = 0; i < kPlan; ++i) r.plan[i] = -1;
  r.plan[0] = m; r.plan[1] = mpad;
  chunk_counts(r.plan, g.plan, d.plan);
  r.plan[24] = ndp::wgrad_grid(r.jobs[1].njobs, d.plan, 0); r.plan[25] = r.jobs[1].nwide != 0;
  r.plan[26] = ndp::wgrad_grid(r.jobs[0].njobs, g.plan, 0); r.plan[27] = r.jobs[0].nwide != 0;
  r.plan[28] = ndp::reduce_grid(nd); r.plan[29] = ndp::reduce_grid(np);
  for (int t = 0; t < NDP_STEP_TENSORS; ++t) r.offsets[t] = -1;
  regions(r, a, 3, g, 4, d, 5);
}

static bool write(const Report& r, FILE* out) {
  std::vector<int64_t> v(r.plan, r.plan + kPlan);
  for (int n = 0; n < 2; ++n) v.insert(v.end(), r.layout[n], r.layout[n] + 20);
  v.insert(v.end(), r.offsets, r.offsets + NDP_STEP_TENSORS);
  for (int i = 0; i < kRegions; ++i) v.insert(v.end(), r.region[i], r.region[i] + 3);
  for (int n = 0; n < 2; ++n) {
    const ndp::WgradArgs& w = r.jobs[n];
    const int64_t head[4] = {w.njobs, w.nwide, w.wide_chunks, w.nchunks};
    v.insert(v.end(), head, head + 4);
    for (int i = 0; i < w.njobs + w.nwide; ++i) {
      const ndp::WgradJob& j = w.job[i];
      int64_t f[kJob] = {0, 0, 0, 0, j.lda, j.ldb, j.a_cols, j.b_cols, j.b_rowmod, j.b_rowdiv, j.b_rowmax, j.b_vec, j.dst_off, j.dst_ld,
                         j.bias_off, j.kind, j.rows, j.seg, j.seg_s, j.seg_k, j.seg_wrap, j.nchunks};
      name(r, j.A, f);
      name(r, j.B, f + 2);
      v.insert(v.end(), f, f + kJob);
    }
  }
  for (int n = 0; n < 2; ++n) {
    const ndp::ReduceArgs& a = r.red[n];
    const int64_t head[3] = {a.nchunks, a.n, a.nregions};
    v.insert(v.end(), head, head + 3);
    for (int i = 0; i < 4; ++i) {
      const int64_t reg[3] = {i < a.nregions ? a.reg_begin[i] : 0, i < a.nregions ? a.reg_end[i] : 0, i < a.nregions ? a.reg_slabs[i] : 0};
      v.insert(v.end(), reg, reg + 3);
    }
  }
  return fwrite(v.data(), sizeof(int64_t), v.size(), out) == v.size();
}

// the answers of the step entry points to a configuration that none of them may run; every buffer is there, so that
// the configuration alone is what they refuse
static bool refusals(const ndp_step_config* c, FILE* out) {
  Exact<float, 16> buf(64);
  Exact<int32_t, 16> word(8);
  ndp_step_buffers b;
  memset(&b, 0, sizeof(b));
  b.g_params = b.g_grad = b.g_exp_avg = b.g_exp_avg_sq = b.d_params = b.d_grad = b.d_exp_avg = b.d_exp_avg_sq = buf.p;
  b.losses = b.action_hat = b.workspace = buf.p;
  b.g_step = b.d_step = word.p;
  const int64_t v[6] = {ndp_step_workspace_floats(c), ndp_step_workspace_offset(c, 0),
                        ndp_step_d_grads(c, &b, buf.p, buf.p, buf.p, 1, nullptr), ndp_step_g_grads(c, &b, buf.p, buf.p, buf.p, nullptr),
                        ndp_step_pack_params(c, &b, nullptr), ndp_step_apply_adam(c, &b, 1, nullptr)};
  return fwrite(v, sizeof(v), 1, out) == 1;
}

static bool variants(FILE* out) {
  std::vector<int64_t> v;
  v.push_back(sizeof(ndp::kPhaseA) / sizeof(ndp::kPhaseA[0]));
  for (const auto& a : ndp::kPhaseA) { v.push_back(a.t[0]); v.push_back(a.t[1]); }
  v.push_back(sizeof(ndp::kPhaseB) / sizeof(ndp::kPhaseB[0]));
  for (const auto& b : ndp::kPhaseB) { v.push_back(b.t[0]); v.push_back(b.t[2]); v.push_back(b.t[1]); }
  return fwrite(v.data(), sizeof(int64_t), v.size(), out) == v.size();
}

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  int32_t queries = 0;
  if (!read_pod(in, &queries) || queries < 0 || queries > 4096) return kBadInput;
  for (int32_t q = 0; q < queries; ++q) {
    int32_t h[5];
    if (!read_pod(in, &h)) return kBadInput;
    ndp_step_config c;
    memset(&c, 0, sizeof(c));
    c.flat = h[1]; c.num_sample = h[2]; c.noise_dim = h[3];
    if (h[0] == 2 || h[0] == 3) {
      if (!(h[0] == 3 ? variants(out) : refusals(h[4] == -1 ? nullptr : &c, out))) return kBadInput;
      continue;
    }
    if (h[0] < 0 || h[0] > 3 || !ndp::step_config_ok(&c)) return kBadInput;
    static Report r;
    memset(&r, 0, sizeof(r));
    layouts(r, c.noise_dim);
    const int64_t m = h[0] == 0 ? c.flat * c.num_sample : c.flat, mpad = ndp::pad_rows(m);
    const int64_t floats[kSpaces] = {h[0] == 0 ? ndp_step_workspace_floats(&c) : 0, (h[0] == 0 ? c.flat : m) * ndp::CODE, m * c.noise_dim,
                                     ndp::g_acts(0, mpad).end, ndp::g_bwd_ws(0, mpad, c.noise_dim).end, ndp::d_bwd_ws(0, mpad).end};
    const Space s0(floats[0]), s1(floats[1]), s2(floats[2]), s3(floats[3]), s4(floats[4]), s5(floats[5]);
    const Space* sp[kSpaces] = {&s0, &s1, &s2, &s3, &s4, &s5};
    for (int s = 0; s < kSpaces; ++s) { r.base[s] = sp[s]->base; r.floats[s] = floats[s]; }
    if (h[0] == 0) {
      r.base[3] = r.base[4] = r.base[5] = nullptr;
      step(r, c, h[4] != 0, s0.base, s1.base, s2.base);
    } else {
      r.base[0] = nullptr;
      module_calls(r, m, c.num_sample, c.noise_dim, s3.base, s4.base, s5.base, s1.base, s2.base);
    }
    if (!write(r, out)) return kBadInput;
  }
  return close_files(in, out);
}

}  // namespace host::step_plan
