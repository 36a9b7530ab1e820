// transformer_split.hip — the transformer block's three launches for runs of a few positions (transformer_split.h,
// P3HIP_FLAG_LOW_LATENCY_TFM), for gfx950, on v_mfma_f32_16x16x32_f16:
//   k_tfm_qkv_split<C, D, NT>  16 NT tokens per workgroup (NT = 1, 2) instead of 64
//   k_tfm_attn_split<D>        one workgroup per (position, head, part): K and V^T of the head in LDS as k_tfm_attn stages
//                              them, and the 16-query step on the part's share of the 23 query tiles only
//   k_tfm_ffn_split<C, NT>     16 NT tokens per workgroup
// The bodies restate those of transformer.hip operation for operation with the token-tile count as a parameter (that
// file's kernels, symbols and registers are pinned and stay as they are): per token and per query the same loads, the
// same MFMA chain in the same K order, the same RMSNorm partial sums over the same C / 4 channels and the same two
// __shfl_xor, the same fp32 expressions and the same roundings (RoPE with the contraction k_tfm_qkv's code objects show
// written out: rope4 below).  tests/test_low_latency_tfm_gpu.py holds the two files to equal bytes.  Every element offset
// into q, k, v, o and x is computed in 64 bits.
#include "transformer_split.h"

#include <type_traits>

namespace p3 {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ inline f32x4 mfma(const h8& a, const h8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// address of channel c of token g (= pos * 361 + s) in the residual stream of width Cs
template <int Cs>
__device__ inline size_t x_index(int g, int c) {
  const int p = g / kTfmL, s = g - p * kTfmL;
  return (((size_t)p * (Cs / 8) + (c >> 3)) * kTfmL + s) * 8 + (c & 7);
}

// transformer.hip gemm_tile over the NT token tiles of the workgroup: the K order st = 0 .. NST - 1 of every tile's chain
template <int NST, int NT>
__device__ inline void gemm_tile(const h8* __restrict__ wpack, int ct, const _Float16* t, int ld, f32x4 acc[NT]) {
  const int lane = threadIdx.x & 63;
  for (int tt = 0; tt < NT; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < NST; ++st) {
    const h8 a = wpack[((size_t)ct * NST + st) * 64 + lane];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
      const h8 b = *reinterpret_cast<const h8*>(t + (16 * tt + (lane & 15)) * ld + 32 * st + 8 * (lane >> 4));
      acc[tt] = mfma(a, b, acc[tt]);
    }
  }
}

// transformer.hip rms_rows for the threads 0 .. 4 x tokens - 1 (whole waves: 64 threads per token tile): 4 threads per
// token, C / 4 channels each, in the same order
template <int C, class Src>
__device__ inline void rms_rows(Src src, const float* __restrict__ scale, _Float16* dst) {
  constexpr int P = C / 4;
  const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
  float v[P];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    v[j] = src(r, P * q + j);
    ss += v[j] * v[j];
  }
  ss += __shfl_xor(ss, 1);
  ss += __shfl_xor(ss, 2);
  const float inv = rsqrtf(ss * (1.0f / C) + 1e-6f);
#pragma unroll
  for (int j = 0; j < P; ++j) dst[r * (C + 8) + P * q + j] = (_Float16)(v[j] * inv * scale[P * q + j]);
}

// RoPE.call on the lane's two pairs: x'[2j] = x[2j] cos + x[2j+1] sin, x'[2j+1] = x[2j] sin - x[2j+1] cos (a reflection).
// Which product of a b + c d is rounded on its own and which rides in the fma is the compiler's choice under
// -ffp-contract=fast, and it chooses by the code around the expression: every instantiation of k_tfm_qkv rounds both
// products of x'[0] and adds them, and rounds the second product of x'[1], x'[2] and x'[3] and fuses the first.  Written
// as in transformer.hip this file's NT = 1 kernels came out otherwise (both x'[2j] fused on the second product), so the
// choice of k_tfm_qkv's code objects is spelled out here and contraction is off.
__device__ inline f32x4 rope4(const f32x4& y, const float* cs, const float* sn) {
#pragma clang fp contract(off)
  const float p0 = y[0] * cs[0], p1 = y[1] * sn[0];
  f32x4 z;
  z[0] = p0 + p1;
  z[1] = __builtin_fmaf(y[0], sn[1], -(y[1] * cs[1]));
  z[2] = __builtin_fmaf(y[2], cs[2], y[3] * sn[2]);
  z[3] = __builtin_fmaf(y[2], sn[3], -(y[3] * cs[3]));
  return z;
}

template <int C, int D, int NT>
__global__ __launch_bounds__(256) void k_tfm_qkv_split(TfmQkvArgs a) {
  constexpr int kTok = 16 * NT, kXs = C + 8, P = C / 4, NH = C / D, Cs = tfm_stream_width(C);
  __shared__ __attribute__((aligned(16))) _Float16 xs[kTok * kXs];
  const int T = a.npos * kTfmL, g0 = blockIdx.x * kTok;
  if (threadIdx.x < 4 * kTok) {   // waves 0 .. NT - 1
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
      if (which < 2) y = rope4(y, a.rope_cos + s * D + d, a.rope_sin + s * D + d);
      const h4 o = h4{(_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
      *reinterpret_cast<h4*>(dst + (((size_t)p * NH + head) * kTfmLPad + s) * D + d) = o;
    }
  }
}

// One (position, head, part) per workgroup: blockIdx.x = (position x heads + head) x parts + part.  The part's query tiles
// are the ceil(23 / parts) from part x ceil(23 / parts) on (12 + 11, 8 + 8 + 7, 5 x 4 + 3), a wave takes every fourth (at
// 6 parts one tile per wave: the last part has 3, and its last tile the queries 352 .. 360 and seven masked ones).  Every
// query 0 .. 360 belongs to exactly one part;
// the step on a tile is k_tfm_attn's (the full-row softmax at D = 32, the 64-key online softmax at D = 64).
template <int D>
__global__ __launch_bounds__(256) void k_tfm_attn_split(TfmAttnArgs a, int parts) {
  constexpr int kKs = D + 8, kVt = kTfmLPad + 8;
  __shared__ __attribute__((aligned(16))) _Float16 ks[kTfmLPad * kKs];
  __shared__ __attribute__((aligned(16))) _Float16 vt[D * kVt];
  const int nh = a.heads;
  const int ph = blockIdx.x / parts, part = blockIdx.x - ph * parts;
  const int p = ph / nh, head = ph % nh;
  const int per = (kTfmQTiles + parts - 1) / parts;
  const int qt0 = part * per, qt1 = min(qt0 + per, kTfmQTiles);
  const size_t base = ((size_t)p * nh + head) * kTfmLPad * D;
  for (int i = threadIdx.x; i < kTfmLPad * D / 8; i += 256) {
    const int key = i / (D / 8), d0 = 8 * (i % (D / 8));
    *reinterpret_cast<h8*>(ks + key * kKs + d0) = *reinterpret_cast<const h8*>(a.k + base + key * D + d0);
    const h8 v = *reinterpret_cast<const h8*>(a.v + base + key * D + d0);
#pragma unroll
    for (int e = 0; e < 8; ++e) vt[(d0 + e) * kVt + key] = v[e];
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4, n = lane & 15;
  // log2(e) / sqrt(head_dim)
  const float kScale = D == 32 ? 1.4426950408889634f / 5.656854249492381f : 1.4426950408889634f / 8.0f;
  constexpr int kKt = kTfmLPad / 16;   // 24 key tiles
  constexpr int kQs = D / 32;          // k32 steps of q . k
  constexpr int kDt = D / 16;          // 16-channel tiles of o
  // O^T += V^T . P^T over k32 step j (key tiles 2j, 2j + 1) with P's fp16 fragment bp
  auto pv_step = [&](int j, const h8& bp, f32x4* o) {
#pragma unroll
    for (int dt = 0; dt < kDt; ++dt) {
      const _Float16* row = vt + (16 * dt + n) * kVt + 32 * j + 4 * gq;
      const h4 lo = *reinterpret_cast<const h4*>(row), hi = *reinterpret_cast<const h4*>(row + 16);
      const h8 av = h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      o[dt] = mfma(av, bp, o[dt]);
    }
  };
  auto to_h8 = [](const f32x4& x, const f32x4& y) {
    return h8{(_Float16)x[0], (_Float16)x[1], (_Float16)x[2], (_Float16)x[3],
              (_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
  };
  for (int qt = qt0 + wave; qt < qt1; qt += 4) {
    h8 bq[kQs];
#pragma unroll
    for (int h = 0; h < kQs; ++h) bq[h] = *reinterpret_cast<const h8*>(a.q + base + (size_t)(16 * qt + n) * D + 32 * h + 8 * gq);
    // S^T tile kt, scaled by kScale; keys 361.. are -3e38
    auto score = [&](int kt) {
      f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < kQs; ++h) {
        const h8 ak = *reinterpret_cast<const h8*>(ks + (16 * kt + n) * kKs + 32 * h + 8 * gq);
        r = mfma(ak, bq[h], r);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = 16 * kt + 4 * gq + i;
        r[i] = key < kTfmL ? r[i] * kScale : -3.0e38f;
      }
      return r;
    };
    f32x4 o[kDt];
#pragma unroll
    for (int dt = 0; dt < kDt; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float sum = 0.f;
    if constexpr (D == 32) {
      f32x4 s[kKt];
      float m = -3.0e38f;
#pragma unroll
      for (int kt = 0; kt < kKt; ++kt) {
        const h8 ak = *reinterpret_cast<const h8*>(ks + (16 * kt + n) * kKs + 8 * gq);
        s[kt] = mfma(ak, bq[0], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = 16 * kt + 4 * gq + i;
          s[kt][i] = key < kTfmL ? s[kt][i] * kScale : -3.0e38f;
          m = fmaxf(m, s[kt][i]);
        }
      }
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
#pragma unroll
      for (int kt = 0; kt < kKt; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s[kt][i] = exp2f(s[kt][i] - m);
          sum += s[kt][i];
        }
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
#pragma unroll
      for (int j = 0; j < kKt / 2; ++j) {
        const h8 bp = h8{(_Float16)s[2 * j][0], (_Float16)s[2 * j][1], (_Float16)s[2 * j][2], (_Float16)s[2 * j][3],
                         (_Float16)s[2 * j + 1][0], (_Float16)s[2 * j + 1][1], (_Float16)s[2 * j + 1][2],
                         (_Float16)s[2 * j + 1][3]};
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const _Float16* row = vt + (16 * dt + n) * kVt + 32 * j + 4 * gq;
          const h4 lo = *reinterpret_cast<const h4*>(row), hi = *reinterpret_cast<const h4*>(row + 16);
          const h8 av = h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[dt] = mfma(av, bp, o[dt]);
        }
      }
    } else {
      constexpr int kBt = 4;   // key tiles per block
      float m = -3.0e38f;
#pragma unroll 1
      for (int b = 0; b < kKt / kBt; ++b) {
        f32x4 s[kBt];
        float mb = m;
#pragma unroll
        for (int t = 0; t < kBt; ++t) {
          s[t] = score(kBt * b + t);
#pragma unroll
          for (int i = 0; i < 4; ++i) mb = fmaxf(mb, s[t][i]);
        }
        mb = fmaxf(mb, __shfl_xor(mb, 16));
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float alpha = exp2f(m - mb);
        m = mb;
        sum *= alpha;
#pragma unroll
        for (int dt = 0; dt < kDt; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int t = 0; t < kBt; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            s[t][i] = exp2f(s[t][i] - m);
            sum += s[t][i];
          }
#pragma unroll
        for (int j = 0; j < kBt / 2; ++j) pv_step(kBt / 2 * b + j, to_h8(s[2 * j], s[2 * j + 1]), o);
      }
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
    }
    const int query = 16 * qt + n;
    if (query < kTfmL) {
      const float inv = 1.0f / sum;
      const size_t orow = ((size_t)p * kTfmL + query) * (size_t)(nh * D) + head * D;
#pragma unroll
      for (int dt = 0; dt < kDt; ++dt) {
        const h4 r = h4{(_Float16)(o[dt][0] * inv), (_Float16)(o[dt][1] * inv), (_Float16)(o[dt][2] * inv),
                        (_Float16)(o[dt][3] * inv)};
        *reinterpret_cast<h4*>(a.o + orow + 16 * dt + 4 * gq) = r;
      }
    }
  }
}

// Both x1 forms of k_tfm_ffn: C <= 96, x1 = x + o . Wo as fp32 rows in LDS; C >= 128, x1 in the registers of the lanes
// that computed it, its rows passing through hs's space for RMSNorm_out.
template <int C, int NT>
__global__ __launch_bounds__(256) void k_tfm_ffn_split(TfmFfnArgs a) {
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
  if (threadIdx.x < 4 * kTok) {
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
  if (threadIdx.x < 4 * kTok) rms_rows<C>([&](int r, int c) { return x1[r * kX1 + c]; }, a.rms_scale, xs);
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
}

}  // namespace

static int token_tiles(int npos, int tokens) { return (int)(((long)npos * kTfmL + tokens - 1) / tokens); }

// every supported model width C (multiples of 32, 64..384) as a compile-time constant
template <class F>
static hipError_t dispatch_c(int C, F&& f) {
  switch (C) {
#define P3_TFM_C(c) case c: return f(std::integral_constant<int, c>{});
    P3_TFM_C(64) P3_TFM_C(96) P3_TFM_C(128) P3_TFM_C(160) P3_TFM_C(192) P3_TFM_C(224)
    P3_TFM_C(256) P3_TFM_C(288) P3_TFM_C(320) P3_TFM_C(352) P3_TFM_C(384)
#undef P3_TFM_C
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_tfm_qkv_split(int C, int D, const TfmQkvArgs& a, int tokens, hipStream_t s) {
  if (!tfm_split_valid(1, tokens) || D < 1 || !tfm_supported(C, C / D)) return hipErrorInvalidValue;
  if (tokens == 64) return launch_tfm_qkv(C, D, a, s);
  const dim3 grid(token_tiles(a.npos, tokens));
  return dispatch_c(C, [&](auto c) {
    constexpr int kC = decltype(c)::value;
    if (D == 32) {
      if (tokens == 16) hipLaunchKernelGGL((k_tfm_qkv_split<kC, 32, 1>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_tfm_qkv_split<kC, 32, 2>), grid, dim3(256), 0, s, a);
    } else if constexpr (kC % 64 == 0) {
      if (tokens == 16) hipLaunchKernelGGL((k_tfm_qkv_split<kC, 64, 1>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_tfm_qkv_split<kC, 64, 2>), grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
  });
}

hipError_t launch_tfm_attn_split(int D, const TfmAttnArgs& a, int parts, hipStream_t s) {
  if (!tfm_split_valid(parts, 64)) return hipErrorInvalidValue;
  if (parts == 1) return launch_tfm_attn(D, a, s);
  const dim3 grid(a.npos * a.heads * parts);
  if (D == 32) hipLaunchKernelGGL(k_tfm_attn_split<32>, grid, dim3(256), 0, s, a, parts);
  else if (D == 64) hipLaunchKernelGGL(k_tfm_attn_split<64>, grid, dim3(256), 0, s, a, parts);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_tfm_ffn_split(int C, const TfmFfnArgs& a, int tokens, hipStream_t s) {
  if (!tfm_split_valid(1, tokens)) return hipErrorInvalidValue;
  if (tokens == 64) return launch_tfm_ffn(C, a, s);
  const dim3 grid(token_tiles(a.npos, tokens));
  return dispatch_c(C, [&](auto c) {
    constexpr int kC = decltype(c)::value;
    if (tokens == 16) hipLaunchKernelGGL((k_tfm_ffn_split<kC, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_tfm_ffn_split<kC, 2>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

}  // namespace p3
