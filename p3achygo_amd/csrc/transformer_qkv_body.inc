// transformer_qkv_body.inc — the body of k_tfm_qkv<C, D> (NT = 4) and k_tfm_qkv_split<C, D, NT> (NT = 1, 2), included
// inside the kernel (transformer_core.h says why as text).  In scope: the constants C, D, NT and TfmQkvArgs a.
// 16 NT tokens per workgroup of 256 threads: RMSNorm_in, x^ . [Wq | Wk | Wv], spiral RoPE on q and k  -> q, k, v fp16.
  constexpr int kTok = 16 * NT, kXs = C + 8, P = C / 4, NH = C / D, Cs = tfm_stream_width(C);
  __shared__ __attribute__((aligned(16))) _Float16 xs[kTok * kXs];
  const int T = a.npos * kTfmL, g0 = blockIdx.x * kTok;
  // Waves 0 .. NT - 1 stage and normalise the rows.  At NT = 4 that is every thread and the test has to be a constant:
  // left to run time it changes 28 of the 30 64-token kernels and costs qkv ones 4 to 8 VGPRs (<96, 32>: 136 -> 140).
  if (NT == 4 || threadIdx.x < 4 * kTok) {
    const int r = threadIdx.x >> 2, q = threadIdx.x & 3, g = g0 + r;
    float v[P];
#pragma unroll
    for (int j = 0; j < P / 8; ++j) {
      h8 h = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (g < T) h = *reinterpret_cast<const h8*>(a.x + x_index<Cs>(g, P * q + 8 * j));
#pragma unroll
      for (int e = 0; e < 8; ++e) v[8 * j + e] = (float)h[e];
    }
    rms_rows<C>([&](int, int c) { return v[c - P * q]; }, a.rms_scale, xs);
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4;
  const h8* w = reinterpret_cast<const h8*>(a.wqkv);
  for (int ct = wave; ct < 3 * C / 16; ct += 4) {
    f32x4 acc[NT];
    gemm_tile<C / 32, NT>(w, ct, xs, kXs, acc);
    const int oc = 16 * ct + 4 * gq;             // first of the lane's four output channels
    const int which = oc / C, hc = oc % C;        // 0 q, 1 k, 2 v; channel within the C
    const int head = hc / D, d = hc % D;          // d is a multiple of 4: two RoPE pairs (d, d+1), (d+2, d+3)
    _Float16* dst = which == 0 ? a.q : (which == 1 ? a.k : a.v);
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
      const int g = g0 + 16 * tt + (lane & 15);
      if (g >= T) continue;
      const int p = g / kTfmL, s = g - p * kTfmL;
      f32x4 y = acc[tt];
      if (which < 2) {   // RoPE.call: x'[2j] = x[2j] cos + x[2j+1] sin, x'[2j+1] = x[2j] sin - x[2j+1] cos (a reflection)
        const float* cs = a.rope_cos + s * D + d;
        const float* sn = a.rope_sin + s * D + d;
        // Which product of a b + c d is rounded on its own and which rides in the fma is the compiler's choice under
        // -ffp-contract=fast, and it chooses by the code around the expression.  In every NT = 4 kernel the plain
        // expression comes out as rope4 spells it (tests/test_low_latency_tfm_cpu.py pins that).  In the NT = 1 kernels
        // it comes out otherwise (both x'[2j] fused on the second product: the last bit differs), and rope4 inside the
        // NT = 4 kernels changes the code of all 17 and the registers of six.  Neither spelling serves both, so the
        // 64-token kernels keep the expression they were built and measured with and the split ones take rope4.
        if constexpr (NT == 4) {
          f32x4 z;
          z[0] = y[0] * cs[0] + y[1] * sn[0];
          z[1] = y[0] * sn[1] - y[1] * cs[1];
          z[2] = y[2] * cs[2] + y[3] * sn[2];
          z[3] = y[2] * sn[3] - y[3] * cs[3];
          y = z;
        } else {
          y = rope4(y, cs, sn);
        }
      }
      const h4 o = h4{(_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
      *reinterpret_cast<h4*>(dst + (((size_t)p * NH + head) * kTfmLPad + s) * D + d) = o;
    }
  }
