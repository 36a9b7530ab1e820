// transformer.hip — the transformer trunk (python/model_transformer.py TransformerBlock, config b14d96h3_transformer)
// on v_mfma_f32_16x16x32_f16.  Three launches per block:
//   k_tfm_qkv   64 tokens per workgroup: RMSNorm_in, x^ . [Wq | Wk | Wv], spiral RoPE on q and k  -> q, k, v fp16
//   k_tfm_attn  one workgroup per (position, head): K and V in LDS, full-row softmax over the 361 keys  -> o fp16
//   k_tfm_ffn   64 tokens per workgroup: o . Wo + x, RMSNorm_out, silu(x^ . Wgate) * (x^ . Wup), . Wdown + residual
// The residual stream keeps the conv trunk's layout and width, [pos][128 / 8][361][8] fp16 (kernels.h): the model's
// 96 channels are channels 0..95, channels 96..127 are the zero padding the stem leaves and no kernel here writes.
// Tokens are s = 19 row + col.  qkv and ffn see the batch as one [npos * 361][96] matrix: a token tile may span two
// positions.  Accumulation, RMSNorm, RoPE, softmax and SiLU are fp32; what goes between kernels, and every MFMA
// operand, is fp16.
#include "transformer.h"

namespace p3 {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTok = 64;          // tokens per workgroup of k_tfm_qkv / k_tfm_ffn
constexpr int kXs = kTfmC + 8;    // LDS row of a [token][96] fp16 tile (16-byte aligned, rows spread over the banks)
constexpr int kHs = kTfmF + 8;    // ... of a [token][192] one
constexpr int kCPad = 128;        // channels of the residual stream

__device__ inline f32x4 mfma(const h8& a, const h8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// address of channel c of token g (= pos * 361 + s) in the residual stream
__device__ inline size_t x_index(int g, int c) {
  const int p = g / kTfmL, s = g - p * kTfmL;
  return (((size_t)p * (kCPad / 8) + (c >> 3)) * kTfmL + s) * 8 + (c & 7);
}

// D^T tile = W^T . T^T for output-channel tile ct and the four 16-token tiles of the workgroup:
// acc[tt][i] = sum_k W[k][16 ct + 4 g + i] * T[16 tt + (lane & 15)][k], g = lane >> 4.
// W is packed as MFMA A fragments [ct][k32 step][64 lanes][8] (engine.cpp pack_afrag); T is an LDS tile with rows of
// `ld` halves.
template <int NST>
__device__ inline void gemm_tile(const h8* __restrict__ wpack, int ct, const _Float16* t, int ld, f32x4 acc[4]) {
  const int lane = threadIdx.x & 63;
  for (int tt = 0; tt < 4; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < NST; ++st) {
    const h8 a = wpack[((size_t)ct * NST + st) * 64 + lane];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const h8 b = *reinterpret_cast<const h8*>(t + (16 * tt + (lane & 15)) * ld + 32 * st + 8 * (lane >> 4));
      acc[tt] = mfma(a, b, acc[tt]);
    }
  }
}

// RMSNorm of the kTok x 96 fp32 rows `src(r, c)` into the fp16 LDS tile dst (4 threads per token, 24 channels each).
// eps = 1e-6: the keras.layers.RMSNormalization default, which the reference does not override (not verified
// against Keras itself; at these magnitudes its effect is far below the engine's tolerance).
template <class Src>
__device__ inline void rms_rows(Src src, const float* __restrict__ scale, _Float16* dst) {
  const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
  float v[24];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 24; ++j) {
    v[j] = src(r, 24 * q + j);
    ss += v[j] * v[j];
  }
  ss += __shfl_xor(ss, 1);
  ss += __shfl_xor(ss, 2);
  const float inv = rsqrtf(ss * (1.0f / kTfmC) + 1e-6f);
#pragma unroll
  for (int j = 0; j < 24; ++j) dst[r * kXs + 24 * q + j] = (_Float16)(v[j] * inv * scale[24 * q + j]);
}

__global__ __launch_bounds__(256) void k_tfm_qkv(TfmQkvArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 xs[kTok * kXs];
  const int T = a.npos * kTfmL, g0 = blockIdx.x * kTok;
  {
    const int r = threadIdx.x >> 2, q = threadIdx.x & 3, g = g0 + r;
    float v[24];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      h8 h = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (g < T) h = *reinterpret_cast<const h8*>(a.x + x_index(g, 24 * q + 8 * j));
#pragma unroll
      for (int e = 0; e < 8; ++e) v[8 * j + e] = (float)h[e];
    }
    rms_rows([&](int, int c) { return v[c - 24 * q]; }, a.rms_scale, xs);
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4;
  const h8* w = reinterpret_cast<const h8*>(a.wqkv);
  for (int ct = wave; ct < 3 * kTfmC / 16; ct += 4) {
    f32x4 acc[4];
    gemm_tile<kTfmC / 32>(w, ct, xs, kXs, acc);
    const int oc = 16 * ct + 4 * gq;               // first of the lane's four output channels
    const int which = oc / kTfmC, hc = oc % kTfmC;  // 0 q, 1 k, 2 v; channel within the 96
    const int head = hc / kTfmD, d = hc % kTfmD;    // d is a multiple of 4: two RoPE pairs (d, d+1), (d+2, d+3)
    _Float16* dst = which == 0 ? a.q : (which == 1 ? a.k : a.v);
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int g = g0 + 16 * tt + (lane & 15);
      if (g >= T) continue;
      const int p = g / kTfmL, s = g - p * kTfmL;
      f32x4 y = acc[tt];
      if (which < 2) {   // RoPE.call: x'[2j] = x[2j] cos + x[2j+1] sin, x'[2j+1] = x[2j] sin - x[2j+1] cos (a reflection)
        const float* cs = a.rope_cos + s * kTfmD + d;
        const float* sn = a.rope_sin + s * kTfmD + d;
        f32x4 z;
        z[0] = y[0] * cs[0] + y[1] * sn[0];
        z[1] = y[0] * sn[1] - y[1] * cs[1];
        z[2] = y[2] * cs[2] + y[3] * sn[2];
        z[3] = y[2] * sn[3] - y[3] * cs[3];
        y = z;
      }
      const h4 o = h4{(_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
      *reinterpret_cast<h4*>(dst + (((size_t)p * kTfmHeads + head) * kTfmLPad + s) * kTfmD + d) = o;
    }
  }
}

// One (position, head) per workgroup, 16 queries per wave step.  S^T = K . Q^T puts a query in each lane column and
// 4 keys of every 16-key tile in the lane (the whole 384-key row of a query in the 4 lanes lane & 15): the softmax
// reduces in registers and across lanes 16 and 32 apart.  O^T = V^T . P^T takes P straight from those registers:
// k32 step j covers key tiles 2j and 2j + 1, k index 8 g + e standing for key 16 (2j + e / 4) + 4 g + e % 4.
__global__ __launch_bounds__(256) void k_tfm_attn(TfmAttnArgs a) {
  constexpr int kKs = kTfmD + 8, kVt = kTfmLPad + 8;
  __shared__ __attribute__((aligned(16))) _Float16 ks[kTfmLPad * kKs];
  __shared__ __attribute__((aligned(16))) _Float16 vt[kTfmD * kVt];
  const int p = blockIdx.x / kTfmHeads, head = blockIdx.x % kTfmHeads;
  const size_t base = ((size_t)p * kTfmHeads + head) * kTfmLPad * kTfmD;
  for (int i = threadIdx.x; i < kTfmLPad * kTfmD / 8; i += 256) {
    const int key = i / (kTfmD / 8), d0 = 8 * (i % (kTfmD / 8));
    *reinterpret_cast<h8*>(ks + key * kKs + d0) = *reinterpret_cast<const h8*>(a.k + base + key * kTfmD + d0);
    const h8 v = *reinterpret_cast<const h8*>(a.v + base + key * kTfmD + d0);
#pragma unroll
    for (int e = 0; e < 8; ++e) vt[(d0 + e) * kVt + key] = v[e];
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4, n = lane & 15;
  const float kScale = 1.4426950408889634f / 5.656854249492381f;   // log2(e) / sqrt(head_dim)
  constexpr int kKt = kTfmLPad / 16;                                // 24 key tiles
  for (int qt = wave; qt * 16 < kTfmL; qt += 4) {
    const h8 bq = *reinterpret_cast<const h8*>(a.q + base + (16 * qt + n) * kTfmD + 8 * gq);
    f32x4 s[kKt];
    float m = -3.0e38f;
#pragma unroll
    for (int kt = 0; kt < kKt; ++kt) {
      const h8 ak = *reinterpret_cast<const h8*>(ks + (16 * kt + n) * kKs + 8 * gq);
      s[kt] = mfma(ak, bq, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = 16 * kt + 4 * gq + i;
        s[kt][i] = key < kTfmL ? s[kt][i] * kScale : -3.0e38f;
        m = fmaxf(m, s[kt][i]);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < kKt; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[kt][i] = exp2f(s[kt][i] - m);
        sum += s[kt][i];
      }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
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
    const int query = 16 * qt + n;
    if (query < kTfmL) {
      const float inv = 1.0f / sum;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const h4 r = h4{(_Float16)(o[dt][0] * inv), (_Float16)(o[dt][1] * inv), (_Float16)(o[dt][2] * inv),
                        (_Float16)(o[dt][3] * inv)};
        *reinterpret_cast<h4*>(a.o + ((size_t)p * kTfmL + query) * kTfmC + head * kTfmD + 16 * dt + 4 * gq) = r;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_tfm_ffn(TfmFfnArgs a) {
  constexpr int kX1 = kTfmC + 1;
  __shared__ __attribute__((aligned(16))) _Float16 xs[kTok * kXs];   // o, then RMSNorm_out(x1)
  __shared__ __attribute__((aligned(16))) _Float16 hs[kTok * kHs];   // silu(gate) * up
  __shared__ float x1[kTok * kX1];                                   // x + o . Wo, fp32
  const int T = a.npos * kTfmL, g0 = blockIdx.x * kTok;
  {
    const int r = threadIdx.x >> 2, q = threadIdx.x & 3, g = g0 + r;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      h8 h = h8{0, 0, 0, 0, 0, 0, 0, 0};
      if (g < T) h = *reinterpret_cast<const h8*>(a.o + (size_t)g * kTfmC + 24 * q + 8 * j);
      *reinterpret_cast<h8*>(xs + r * kXs + 24 * q + 8 * j) = h;
    }
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4, n = lane & 15;
  for (int ct = wave; ct < kTfmC / 16; ct += 4) {
    f32x4 acc[4];
    gemm_tile<kTfmC / 32>(reinterpret_cast<const h8*>(a.wo), ct, xs, kXs, acc);
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int r = 16 * tt + n, g = g0 + r, c = 16 * ct + 4 * gq;
      h4 res = h4{0, 0, 0, 0};
      if (g < T) res = *reinterpret_cast<const h4*>(a.x + x_index(g, c));
#pragma unroll
      for (int i = 0; i < 4; ++i) x1[r * kX1 + c + i] = acc[tt][i] + (float)res[i];
    }
  }
  __syncthreads();
  rms_rows([&](int r, int c) { return x1[r * kX1 + c]; }, a.rms_scale, xs);
  __syncthreads();
  for (int c2 = wave; c2 < kTfmF / 16; c2 += 4) {   // gate tile c2 and up tile c2 (packed as tiles 12 + c2)
    f32x4 gt[4], up[4];
    gemm_tile<kTfmC / 32>(reinterpret_cast<const h8*>(a.wgu), c2, xs, kXs, gt);
    gemm_tile<kTfmC / 32>(reinterpret_cast<const h8*>(a.wgu), kTfmF / 16 + c2, xs, kXs, up);
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
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
  for (int ct = wave; ct < kTfmC / 16; ct += 4) {
    f32x4 acc[4];
    gemm_tile<kTfmF / 32>(reinterpret_cast<const h8*>(a.wdown), ct, hs, kHs, acc);
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int r = 16 * tt + n, g = g0 + r, c = 16 * ct + 4 * gq;
      if (g >= T) continue;
      h4 y;
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = (_Float16)(acc[tt][i] + x1[r * kX1 + c + i]);
      *reinterpret_cast<h4*>(a.x + x_index(g, c)) = y;
    }
  }
}

}  // namespace

static int token_tiles(int npos) { return (npos * kTfmL + kTok - 1) / kTok; }

hipError_t launch_tfm_qkv(const TfmQkvArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_tfm_qkv, dim3(token_tiles(a.npos)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_tfm_attn(const TfmAttnArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_tfm_attn, dim3(a.npos * kTfmHeads), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_tfm_ffn(const TfmFfnArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_tfm_ffn, dim3(token_tiles(a.npos)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace p3
