// plan_sanitize_main.cpp — a stand-alone program that runs the host-side plan (csrc/plan.h: choose_plan + build_plan, no
// HIP runtime call) over .p3w files, for building under -fsanitize=address,undefined and running on a CPU, and for
// pinning what the plan decides and packs (tests/test_plan_matrix_cpu.py).
//
//   hipcc -O1 -g -std=c++17 -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       tools/plan_sanitize_main.cpp p3achygo_amd/csrc/plan.cpp -o plan_sanitize
//   (without the sanitizers, --offload-host-only builds it in seconds)
//   ./plan_sanitize <flags> a.p3w b.p3w ...            (flags: the P3HIP_FLAG_* sum, e.g. 2048 for P3HIP_FLAG_INT8_ANY,
//                                                       or several of them, "0,2048,64": every file under each)
//   ./plan_sanitize --choose <flags> a.p3w b.p3w ...   choose_plan alone: works on a file that is only a header
//
// Prints one line per (file, flags).  Plan mode: the path chosen, the blocks, the quantized tensors, the arena's size
// and FNV-1a digest and the PlanChoice, or the refusal.  --choose: the path and the PlanChoice, or the refusal.
// Exit status 0 when every file was planned or refused cleanly; the sanitizers abort on a finding.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../p3achygo_amd/csrc/plan.h"

static std::string choice_fields(const eng::PlanChoice& c) {
  char buf[128];
  snprintf(buf, sizeof buf, "CB %d CPI %d heads_image %d heads_fused %d tfm_heads %d tfm_D %d", c.CB, c.CPI, (int)c.heads_image,
           (int)c.heads_fused, c.tfm_heads, c.tfm_D);
  return buf;
}

int main(int argc, char** argv) {
  const bool choose = argc > 1 && strcmp(argv[1], "--choose") == 0;
  const int first = choose ? 3 : 2;
  if (argc < first + 1) {
    fprintf(stderr, "usage: %s [--choose] <flags>[,<flags>...] file.p3w ...\n", argv[0]);
    return 2;
  }
  std::vector<uint32_t> flag_sets;
  for (const char* p = argv[first - 1]; *p;) {
    char* end = nullptr;
    flag_sets.push_back((uint32_t)strtoul(p, &end, 0));
    if (end == p) { fprintf(stderr, "bad flags: %s\n", argv[first - 1]); return 2; }
    p = *end == ',' ? end + 1 : end;
  }
  const eng::Options opt = eng::Options::from_env();
  for (int i = first; i < argc; ++i) {
    eng::WeightFile wf;
    std::string err;
    if (!wf.load(argv[i], err)) {
      printf("%s: load failed: %s\n", argv[i], err.c_str());
      return 1;
    }
    for (const uint32_t flags : flag_sets) {
      if (choose) {
        const eng::PlanChoice c = eng::choose_plan(wf, flags, opt, err);
        if (c.path == eng::Path::Refused) printf("%s: %u: refused: %s\n", argv[i], flags, err.c_str());
        else printf("%s: %u: %s, %s\n", argv[i], flags, eng::path_name(c.path), choice_fields(c).c_str());
        continue;
      }
      eng::Plan plan;
      eng::Arena ar;
      if (!eng::build_plan(wf, flags, opt, plan, ar, err)) {
        printf("%s: %u: refused: %s\n", argv[i], flags, err.c_str());
        wf.missing.clear();
        continue;
      }
      unsigned long long h = 14695981039346656037ull;   // FNV-1a, 64 bits
      for (const unsigned char c : ar.host) h = (h ^ c) * 1099511628211ull;
      size_t layers = 0;   // the convs of the layer-wise blocks
      for (const eng::BlockPlan& b : plan.blocks)
        if (b.kind == 4) layers += b.layers.size();
      printf("%s: %u: %s, C %d (file %d) C_b %d (file %d), %zu blocks, %zu layers, %d quantized tensors, arena %zu bytes, "
             "digest %016llx, %s\n", argv[i], flags, eng::path_name(plan.choice.path), wf.C, wf.model_C, wf.Cb, wf.model_Cb,
             plan.blocks.size(), layers, plan.n_q, ar.host.size(), h, choice_fields(plan.choice).c_str());
    }
  }
  return 0;
}
