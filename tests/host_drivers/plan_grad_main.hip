// plan_grad_main.hip -- a host-driver program of its own for the body plan_grad.inc (built by tests/host_driver.py: build
// on this source, see tests/plan_grad_common.py: build_driver; run by tests/host_driver.py: run).  The body is not a
// row of main.hip's table because the change that added it left every existing test file as it was; a later change
// that may edit main.hip moves the #include and the row there and deletes this file.  Like main.hip it includes the
// library's source as the library build does, once, and then the body, which replays the schedules of k_plan_goal_grad,
// k_plan_grad_gather and k_plan_grad_step on the CPU through the __host__ __device__ functions the kernels call, in
// allocations of exactly their size (exact.h), under AddressSanitizer and UBSan.  The program makes no HIP runtime call
// and needs no GPU; it is an ordinary program, started as a child process.
//
// Usage: host_driver plan_grad IN OUT     (the formats of IN and OUT: plan_grad.inc)
#include "../../ndivplanning_amd/csrc/ndp_kernels.hip"

#include <cmath>
#include <cstring>

#include "exact.h"

#include "plan_grad.inc"

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "plan_grad") == 0) return host::plan_grad::run(argc - 1, argv + 1);
  fprintf(stderr, "usage: %s plan_grad IN OUT\n", argv[0]);
  return host::kBadInput;
}
