// transformer_ffn_body.inc — the body of k_tfm_ffn<C> (NT = 4) and k_tfm_ffn_split<C, NT> (NT = 1, 2), included inside
// the kernel (transformer_core.h says why as text).  In scope: the constants C, NT and TfmFfnArgs a.
// 16 NT tokens per workgroup of 256 threads: o . Wo + x, RMSNorm_out, silu(x^ . Wgate) * (x^ . Wup), . Wdown + residual.
// C <= 96: x1 = x + o . Wo lives in LDS as fp32 rows beside the o / RMSNorm tile xs and the SwiGLU tile hs.
// C >= 128: x1 stays in the registers of the lanes that computed it (the Wo and Wdown tiles of a wave are the same
// (ct, token tile) pairs), and its fp32 rows pass through hs's space only for RMSNorm_out, before hs is written: LDS is
// xs + hs = 16 NT ((C + 8) 2 + (2 C + 8) 2) bytes, 149.5 KiB at C = 384 and NT = 4.  The values and their rounding are
// the same.  The rows are staged and normalised by waves 0 .. NT - 1, under the test transformer_qkv_body.inc explains.
  constexpr int kTok = 16 * NT, F = 2 * C, kXs = C + 8, kHs = F + 8, kX1 = C + 1, P = C / 4, Cs = tfm_stream_width(C);
  constexpr bool kRegX1 = C > 96;
  constexpr int kX1Lds = kRegX1 ? 1 : kTok * kX1;
  constexpr int kCt = C / 16, kWt = (kCt + 3) / 4;   // output-channel tiles; per wave at most
  __shared__ __attribute__((aligned(16))) _Float16 xs[kTok * kXs];   // o, then RMSNorm_out(x1)
  __shared__ __attribute__((aligned(16))) _Float16 hs[kTok * kHs];   // silu(gate) * up (C >= 128: x1 rows before)
  __shared__ float x1s[kX1Lds];                                      // x + o . Wo, fp32 (C <= 96)
  float* x1 = kRegX1 ? reinterpret_cast<float*>(hs) : x1s;
  f32x4 x1r[kRegX1 ? kWt : 1][NT];
  const int T = a.npos * kTfmL, g0 = blockIdx.x * kTok;
  if (NT == 4 || threadIdx.x < 4 * kTok) {
    const int r = threadIdx.x >> 2, q = threadIdx.x & 3, g = g0 + r;
#pragma unroll
    for (int j = 0; j < P / 8; ++j) {
      h8 h = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (g < T) h = *reinterpret_cast<const h8*>(a.o + (size_t)g * C + P * q + 8 * j);
      *reinterpret_cast<h8*>(xs + r * kXs + P * q + 8 * j) = h;
    }
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4, n = lane & 15;
  if constexpr (!kRegX1) {
    for (int ct = wave; ct < kCt; ct += 4) {
      f32x4 acc[NT];
      gemm_tile<C / 32, NT>(reinterpret_cast<const h8*>(a.wo), ct, xs, kXs, acc);
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const int r = 16 * tt + n, g = g0 + r, c = 16 * ct + 4 * gq;
        h4 res = h4{0, 0, 0, 0};
        if (g < T) res = *reinterpret_cast<const h4*>(a.x + x_index<Cs>(g, c));
#pragma unroll
        for (int i = 0; i < 4; ++i) x1[r * kX1 + c + i] = acc[tt][i] + (float)res[i];
      }
    }
  } else {
#pragma unroll
    for (int w = 0; w < kWt; ++w) {
      const int ct = wave + 4 * w;
      if (ct >= kCt) break;
      f32x4 acc[NT];
      gemm_tile<C / 32, NT>(reinterpret_cast<const h8*>(a.wo), ct, xs, kXs, acc);
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const int r = 16 * tt + n, g = g0 + r, c = 16 * ct + 4 * gq;
        h4 res = h4{0, 0, 0, 0};
        if (g < T) res = *reinterpret_cast<const h4*>(a.x + x_index<Cs>(g, c));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          x1r[w][tt][i] = acc[tt][i] + (float)res[i];
          x1[r * kX1 + c + i] = x1r[w][tt][i];
        }
      }
    }
  }
  __syncthreads();
  if (NT == 4 || threadIdx.x < 4 * kTok) rms_rows<C>([&](int r, int c) { return x1[r * kX1 + c]; }, a.rms_scale, xs);
  __syncthreads();
  for (int c2 = wave; c2 < F / 16; c2 += 4) {   // gate tile c2 and up tile c2 (packed as tiles F / 16 + c2)
    f32x4 gt[NT], up[NT];
    gemm_tile<C / 32, NT>(reinterpret_cast<const h8*>(a.wgu), c2, xs, kXs, gt);
    gemm_tile<C / 32, NT>(reinterpret_cast<const h8*>(a.wgu), F / 16 + c2, xs, kXs, up);
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
      h4 hv;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t = gt[tt][i];
        hv[i] = (_Float16)(t / (1.0f + __expf(-t)) * up[tt][i]);
      }
      *reinterpret_cast<h4*>(hs + (16 * tt + n) * kHs + 16 * c2 + 4 * gq) = hv;
    }
  }
  __syncthreads();
  if constexpr (!kRegX1) {
    for (int ct = wave; ct < kCt; ct += 4) {
      f32x4 acc[NT];
      gemm_tile<F / 32, NT>(reinterpret_cast<const h8*>(a.wdown), ct, hs, kHs, acc);
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const int r = 16 * tt + n, g = g0 + r, c = 16 * ct + 4 * gq;
        if (g >= T) continue;
        h4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = (_Float16)(acc[tt][i] + x1[r * kX1 + c + i]);
        *reinterpret_cast<h4*>(a.x + x_index<Cs>(g, c)) = y;
      }
    }
  } else {
#pragma unroll
    for (int w = 0; w < kWt; ++w) {
      const int ct = wave + 4 * w;
      if (ct >= kCt) break;
      f32x4 acc[NT];
      gemm_tile<F / 32, NT>(reinterpret_cast<const h8*>(a.wdown), ct, hs, kHs, acc);
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const int r = 16 * tt + n, g = g0 + r, c = 16 * ct + 4 * gq;
        if (g >= T) continue;
        h4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = (_Float16)(acc[tt][i] + x1r[w][tt][i]);
        *reinterpret_cast<h4*>(a.x + x_index<Cs>(g, c)) = y;
      }
    }
  }
