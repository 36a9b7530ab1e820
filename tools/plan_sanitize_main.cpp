// plan_sanitize_main.cpp — a stand-alone program that runs the host-side plan (csrc/plan.h: choose_plan + build_plan, no
// HIP runtime call) over .p3w files, for building under -fsanitize=address,undefined and running on a CPU.
//
//   hipcc -O1 -g -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       tools/plan_sanitize_main.cpp p3achygo_amd/csrc/plan.cpp -o plan_sanitize
//   ./plan_sanitize <flags> a.p3w b.p3w ...        (flags: the P3HIP_FLAG_* sum, e.g. 2048 for P3HIP_FLAG_INT8_ANY)
//
// Prints one line per file: the path chosen, the blocks, the quantized tensors and the arena size, or the refusal.
// Exit status 0 when every file was planned or refused cleanly; the sanitizers abort on a finding.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../p3achygo_amd/csrc/plan.h"

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s <flags> file.p3w ...\n", argv[0]);
    return 2;
  }
  const uint32_t flags = (uint32_t)strtoul(argv[1], nullptr, 0);
  const eng::Options opt = eng::Options::from_env();
  for (int i = 2; i < argc; ++i) {
    eng::WeightFile wf;
    eng::Plan plan;
    eng::Arena ar;
    std::string err;
    if (!wf.load(argv[i], err)) {
      printf("%s: load failed: %s\n", argv[i], err.c_str());
      return 1;
    }
    if (!eng::build_plan(wf, flags, opt, plan, ar, err)) {
      printf("%s: refused: %s\n", argv[i], err.c_str());
      continue;
    }
    size_t layers = 0;
    for (const eng::BlockPlan& b : plan.blocks) layers += b.layers.size();
    printf("%s: %s, C %d (file %d) C_b %d (file %d), %zu blocks, %zu layers, %d quantized tensors, arena %zu bytes\n", argv[i],
           eng::path_name(plan.choice.path), wf.C, wf.model_C, wf.Cb, wf.model_Cb, plan.blocks.size(), layers, plan.n_q,
           ar.host.size());
  }
  return 0;
}
