// fm_geometry.inc -- what the layer launches of the forward model, the autoencoder and its folded decoder hand to fm_gemm,
// fm_deconv32 and fm_wgrad (csrc/ndp_forward_model.inc: fm_geom, fm_layer_views, the per-network FmMaps), for
// tests/test_fm_geometry_host.py.  main.hip includes it behind the library's source.  Host arithmetic only: no kernel is
// replayed, no HIP runtime call is made, no map is read or written -- the workspaces are address ranges without access
// rights, so that the library's own fm_ws / ae_ws / ae_dec_maps lay the tensors out in them and a touch would fault.
//
// Usage: host_driver fm_geometry IN OUT
//   IN   int32 queries, then per query 4 int32: net (0 forward model, 1 autoencoder, 2 folded decoder), layer, direction
//        (0 forward, 1 data gradient, 2 weight gradient), images
//   OUT  per query kFields int32 (see Row) and the launch's label, 32 bytes zero-padded; then per network int32 layers and
//        per layer four views of 3 int32 (tensor, channel offset, pixel stride): in[l], raw[l], din[l], in[l + 1]
// A view is named by the workspace tensor it lies in (its index in FmTensor / AeTensor / AeDecTensor; -1 a null view,
// -2 the caller's codes) and its offset from that tensor's first float.
#include <sys/mman.h>

namespace host::fm_geometry {

constexpr int kFields = 21;
constexpr int kMaxImages = 32;

struct Space {
  float* base = nullptr; size_t bytes = 0;
  explicit Space(int64_t floats) : bytes((size_t)floats * sizeof(float)) {
    void* p = mmap(nullptr, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) abort();
    base = static_cast<float*>(p);
  }
  ~Space() { munmap(base, bytes); }
  Space(const Space&) = delete;
};

// the maps of one network at n images, and how to name a pointer into them
struct Net {
  const ndp::FmNet* net; ndp::FmMaps m; float* const* t; int tensors; const float* codes;
  void name(ndp::FmView v, int32_t* out) const {
    out[0] = -1; out[1] = 0; out[2] = v.ld;
    if (v.p == nullptr) return;
    if (v.p == codes) { out[0] = -2; return; }
    for (int i = 0; i < tensors; ++i)
      if (t[i] <= v.p && (i + 1 == tensors || v.p < t[i + 1])) { out[0] = i; out[1] = (int32_t)(v.p - t[i]); }
  }
};

int run(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, &in, &out)) return kBadInput;
  int32_t queries = 0;
  if (!read_pod(in, &queries) || queries < 0 || queries > 4096) return kBadInput;
  const Space fm_space(ndp::fm_ws_floats(kMaxImages)), ae_space(ndp::ae_ws_floats(kMaxImages)),
      dec_space(ndp::ae_dec_ws_floats(kMaxImages));
  Exact<float> codes((size_t)kMaxImages * 128);
  auto maps_of = [&](int which, int64_t n, ndp::FmWs* fw, ndp::AeWs* aw, float** dt) {
    Net r;
    if (which == 0) {
      *fw = ndp::fm_ws(fm_space.base, n);
      r = Net{&ndp::kFmNet, ndp::fm_maps(*fw), fw->t, ndp::FMT_COUNT, nullptr};
    } else if (which == 1) {
      *aw = ndp::ae_ws(ae_space.base, n);
      r = Net{&ndp::kAeNet, ndp::ae_maps(*aw), aw->t, ndp::AET_COUNT, nullptr};
    } else {
      for (int i = 0; i < ndp::ADT_COUNT; ++i) dt[i] = dec_space.base + ndp::ae_dec_tensor_offset(ndp::ae_dec_cap(n), i);
      r = Net{&ndp::kAeDecNet, ndp::ae_dec_maps(codes.p, dt), dt, ndp::ADT_COUNT, codes.p};
    }
    return r;
  };
  ndp::FmWs fw;
  ndp::AeWs aw;
  float* dt[ndp::ADT_COUNT];
  for (int32_t q = 0; q < queries; ++q) {
    int32_t h[4];
    if (!read_pod(in, &h)) return kBadInput;
    if (h[0] < 0 || h[0] > 2 || h[2] < 0 || h[2] > 2 || h[3] < 1 || h[3] > kMaxImages) return kBadInput;
    const Net r = maps_of(h[0], h[3], &fw, &aw, dt);
    if (h[1] < 0 || h[1] >= r.net->layers) return kBadInput;
    const ndp::FmGeom g = ndp::fm_geom(*r.net, h[1], h[2], h[3]);
    if (g.mode < 0) return kBadInput;                                  // (the layer has no such launch)
    ndp::FmView a, b;
    ndp::fm_layer_views(*r.net, r.m, h[1], h[2], &a, &b);
    int32_t row[kFields] = {h[2] == ndp::FM_WGRAD ? 2 : g.deconv32, g.mode, g.SH, g.ss, g.OH, g.GH, g.C, g.N, g.KH, g.pad, g.p2,
                            g.DH, g.J, g.columns, ndp::fm_bn_of(*r.net, h[1])};
    r.name(a, row + 15);
    r.name(b, row + 18);
    char label[32];
    memset(label, 0, sizeof(label));
    strncpy(label, r.net->label[h[1]].of[h[2]], sizeof(label) - 1);
    if (fwrite(row, sizeof(row), 1, out) != 1 || fwrite(label, sizeof(label), 1, out) != 1) return kBadInput;
  }
  for (int which = 0; which < 3; ++which) {
    const Net r = maps_of(which, 16, &fw, &aw, dt);
    const int32_t layers = r.net->layers;
    if (fwrite(&layers, sizeof(layers), 1, out) != 1) return kBadInput;
    for (int l = 0; l < layers; ++l) {
      int32_t v[12];
      r.name(r.m.in[l], v);
      r.name(r.m.raw[l], v + 3);
      r.name(r.m.din[l], v + 6);
      r.name(r.m.in[l + 1], v + 9);
      if (fwrite(v, sizeof(v), 1, out) != 1) return kBadInput;
    }
  }
  return close_files(in, out);
}

}  // namespace host::fm_geometry
