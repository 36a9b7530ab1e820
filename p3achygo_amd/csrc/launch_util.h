// launch_util.h — host-side helpers shared by the kernel launchers (kernels.hip, conv_any.hip, block_i8.hip,
// heads_aux.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace p3 {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE, and the launchers are called from many host threads
// (bench.py: one driver thread per game group; an evaluation match: one engine per player, possibly on two devices):
// one flag per (kernel instantiation, device ordinal), set after the attribute call succeeded.  Racing first calls
// set the same value twice, which is harmless; nobody launches before the attribute is set on ITS device.
struct AttrOnce { std::atomic<bool> done[32]; };
template <class K>
inline hipError_t ensure_lds(AttrOnce& once, K kernel, size_t lds) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32)
    return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (once.done[dev].load(std::memory_order_acquire)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) once.done[dev].store(true, std::memory_order_release);
  return e;
}

// Grid of the kernels that split their NCP output passes across workgroups: a multiple of
// 8 * NCP, at most n_cu, enough for every (position group, pass) pair.
inline int conv_split_grid(int npos, int npos_per_wg, int ncp, int n_cu) {
  const int unit = 8 * ncp;
  const int groups = (npos + npos_per_wg - 1) / npos_per_wg;
  int want = ((groups + 7) / 8) * unit;                 // pairs, padded to whole units
  int cap = (n_cu / unit) * unit;
  if (cap < unit) cap = unit;
  return want < cap ? want : cap;
}

}  // namespace p3
