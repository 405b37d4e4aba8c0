// main.hip -- the one host-driver program (built and run by tests/host_driver.py).  It includes the library's source as
// the library build does, once, and then the driver bodies: each replays one kernel family's schedule on the CPU through
// the __host__ __device__ functions the kernels call, in allocations of exactly their size (exact.h), so that
// AddressSanitizer and UBSan see what the device would not report (fm_geometry and step_plan replay nothing: they report the
// launch arguments the host derives from the network tables).  The program makes no HIP runtime call and needs no GPU; it is an
// ordinary program, started as a child process.
//
// Usage: host_driver NAME IN OUT [flags ...]
// NAME selects the body; each body's header gives the formats of its IN and OUT.
#include "../../ndivplanning_amd/csrc/ndp_kernels.hip"

#include <cmath>
#include <cstring>
#include <vector>

#include "exact.h"

#include "jpeg.inc"
#include "jpeg_enc.inc"
#include "resize.inc"
#include "fm_score.inc"
#include "gan_score.inc"
#include "image_quality.inc"
#include "store_gather.inc"
#include "fm_rollout.inc"
#include "plan_cem.inc"
#include "world.inc"
#include "fm_geometry.inc"
#include "step_plan.inc"

int main(int argc, char** argv) {
  static const struct {
    const char* name;
    int (*run)(int, char**);
  } drivers[] = {
      {"jpeg", host::jpeg::run},
      {"jpeg_enc", host::jpeg_enc::run},
      {"resize", host::resize::run},
      {"fm_score", host::fm_score::run},
      {"gan_score", host::gan_score::run},
      {"image_quality", host::image_quality::run},
      {"store_gather", host::store_gather::run},
      {"fm_rollout", host::fm_rollout::run},
      {"plan_cem", host::plan_cem::run},
      {"world", host::world::run},
      {"fm_geometry", host::fm_geometry::run},
      {"step_plan", host::step_plan::run},
  };
  for (const auto& d : drivers)
    if (argc > 1 && strcmp(argv[1], d.name) == 0) return d.run(argc - 1, argv + 1);
  fprintf(stderr, "usage: %s NAME IN OUT [flags ...], NAME one of:", argv[0]);
  for (const auto& d : drivers) fprintf(stderr, " %s", d.name);
  fprintf(stderr, "\n");
  return host::kBadInput;
}
