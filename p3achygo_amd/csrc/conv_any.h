// conv_any.h — the layer-wise conv trunk at any width (include/p3hip.h P3HIP_CONV_SET): the kernels of kernels.hip
// whose width is a template argument there (k_init, k_conv1x1, k_lconv, k_bdense), with the channel counts as launch
// arguments in units of 64 channels.  The engine pads a file's C and C_b to multiples of 64 (engine.cpp
// WeightFile::pad_conv), so every count here is one.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace p3 {

constexpr int kConvAnyMaxC = 512;

// C a multiple of 64, 64 <= C <= kConvAnyMaxC; output passes of 128 channels where C is a multiple of 128, else of 64
// (engine.cpp packs the stream with conv_any_init_pass(C))
constexpr int conv_any_init_pass(int C) { return C % 128 == 0 ? 128 : 64; }
hipError_t launch_init_any(int C, const InitArgs& a, int grid, hipStream_t s);

// K slice of the per-position 1x1 convs (broadcast conv_first / conv_last, head convs): 128 channels where C is a
// multiple of 128 from 256 on, else 64 — what k_conv1x1<C, ..> takes at C = 384 and C = 192
constexpr int conv_any_slice(int C) { return (C >= 256 && C % 128 == 0) ? 128 : 64; }
// which: as launch_conv1x1 (0 conv_first, 1 conv_last, 2 head convs C -> 96)
hipError_t launch_conv1x1_any(int C, int which, const Conv1x1Args& a, int n_cu, hipStream_t s);

// cin, cout multiples of 64 up to kConvAnyMaxC; kw 1 or 3; the flag sets of engine.cpp's layer-wise plan
hipError_t launch_lconv_any(int kw, int cin, int cout, const LConvArgs& a, int n_cu, hipStream_t s);
const char* lconv_any_kernel_name(int kw);

hipError_t launch_bdense_any(int C, const BDenseArgs& a, int grid, hipStream_t s);

}  // namespace p3
