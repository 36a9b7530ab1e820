// dataset_targets_main.cc — opens chunks with the reader (p3achygo_amd/host/tf_reader.h) and prints, per file, the rows, the
// rows that have the trainer's targets and a digest of those targets, for a build with -fsanitize=address,undefined
// (tests/test_loss_cpu.py): the records hold target keys of every wrong length and kind, and the sanitizers must stay
// silent.  Usage: dataset_targets_main FILE...
#include <cstdio>

#include "../../p3achygo_amd/host/tf_reader.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    p3::GoDataset ds;
    const p3::ReadStatus st = ds.Open(argv[a]);
    if (!st.ok()) {
      std::printf("%s: error %d %s\n", argv[a], st.code, st.msg.c_str());
      continue;
    }
    size_t with = 0;
    uint32_t digest = 0;
    for (size_t i = 0; i < ds.size(); ++i) {
      const p3hip_targets* t = ds.targets(i);
      if (!t) continue;
      ++with;
      digest = p3::Crc32c(t, sizeof *t) ^ (digest * 31u);
    }
    std::printf("%s: rows %zu targets %zu digest %08x\n", argv[a], ds.size(), with, (unsigned)digest);
  }
  return 0;
}
