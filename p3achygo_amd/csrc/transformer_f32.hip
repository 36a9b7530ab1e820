// transformer_f32.hip — gfx950 kernels of the fp32 plan of the transformer trunks (transformer_f32.h,
// P3HIP_FLAG_FP32_TFM): the three launches per block of transformer.hip with every value in fp32 and every product on
// v_mfma_f32_16x16x4_f32.
//   k_tfm_qkv_f32<C>   32 tokens per workgroup: RMSNorm_in, x^ . [Wq | Wk | Wv], spiral RoPE on q and k  -> q, k, v
//   k_tfm_attn_f32<D>  64 queries of one (position, head) per workgroup, a 16-query tile per wave; the keys pass through
//                      LDS in three blocks of 128 with an online softmax  -> o
//   k_tfm_ffn_f32<C>   32 tokens per workgroup: o . Wo + x, RMSNorm_out, silu(x^ . Wgate) * (x^ . Wup), . Wdown + residual
// The fragment order is the fp16 kernels': where v_mfma_f32_16x16x32_f16 takes eight halves of a lane, k = 8 (lane >> 4)
// + e of a step of 32, eight v_mfma_f32_16x16x4_f32 take the eight floats one after the other (MFMA e multiplies the
// k of index e of every lane group; A and B agree, and the order inside a sum is the only thing that differs).  The C / D
// map is the same: a lane holds rows 4 (lane >> 4) .. + 3 of column lane & 15.
//
// qkv and ffn see the batch as one [npos * 361][C] matrix, a token tile may span two positions; every token's sums run
// in an order that depends on nothing but its channels, so a position's results do not depend on its slot or the batch.
// A sum over more than 128 products is taken in chunks of 128 (one MFMA chain each) whose results are added up: the
// rounding error of an fp32 chain grows with its length (conv_f32.hip).
#include "transformer_f32.h"

#include <type_traits>

namespace p3 {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTok = 32;          // tokens per workgroup of k_tfm_qkv_f32 / k_tfm_ffn_f32
constexpr int kChunk = 4;         // steps of 32 products per MFMA chain

__device__ inline f32x4 mfma(float a, float b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// address of channel c of token g (= pos * 361 + s) in the residual stream of width Cs
template <int Cs>
__device__ inline size_t x_index(int g, int c) {
  const int p = g / kTfmL, s = g - p * kTfmL;
  return (((size_t)p * (Cs / 8) + (c >> 3)) * kTfmL + s) * 8 + (c & 7);
}

// D^T tile = W^T . T^T for output-channel tile ct and the two 16-token tiles of the workgroup:
// acc[tt][i] = sum_k W[k][16 ct + 4 g + i] * T[16 tt + (lane & 15)][k], g = lane >> 4.
// W is the image of pack_tfm_f32, T an LDS tile with rows of `ld` floats.  NST steps of 32 products.
template <int NST>
__device__ inline void gemm_tile(const float* __restrict__ wpack, int ct, const float* t, int ld, f32x4 acc[2]) {
  const int lane = threadIdx.x & 63, n = lane & 15, gq = lane >> 4;
  const f32x4* w = reinterpret_cast<const f32x4*>(wpack) + ((size_t)ct * NST * 64 + lane) * 2;
  acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c0 = 0; c0 < NST; c0 += kChunk) {
    f32x4 part[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      const int st = c0 + j;
      if (NST % kChunk != 0 && st >= NST) break;
      const f32x4 a0 = w[(size_t)st * 128], a1 = w[(size_t)st * 128 + 1];
      f32x4 b[2][2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const float* row = t + (16 * tt + n) * ld + 32 * st + 8 * gq;
        b[tt][0] = *reinterpret_cast<const f32x4*>(row);
        b[tt][1] = *reinterpret_cast<const f32x4*>(row + 4);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) part[tt] = mfma(a0[e], b[tt][0][e], part[tt]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) part[tt] = mfma(a1[e], b[tt][1][e], part[tt]);
    }
    acc[0] += part[0];
    acc[1] += part[1];
  }
}

// RMSNorm of the kTok rows of C floats `src(r, c)` (c a multiple of 4, four channels at a time) into the LDS tile dst of
// rows ld: 8 threads per token, C / 8 channels each.  eps = 1e-6 as in transformer.hip rms_rows.
template <int C, class Src>
__device__ inline void rms_rows(Src src, const float* __restrict__ scale, float* dst, int ld) {
  constexpr int P = C / 8;
  const int r = threadIdx.x >> 3, q = threadIdx.x & 7;
  f32x4 v[P / 4];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < P / 4; ++j) {
    v[j] = src(r, P * q + 4 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += v[j][e] * v[j][e];
  }
  ss += __shfl_xor(ss, 1);
  ss += __shfl_xor(ss, 2);
  ss += __shfl_xor(ss, 4);
  const float inv = rsqrtf(ss * (1.0f / C) + 1e-6f);
#pragma unroll
  for (int j = 0; j < P / 4; ++j) {
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + P * q + 4 * j);
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = v[j][e] * inv * sc[e];
    *reinterpret_cast<f32x4*>(dst + r * ld + P * q + 4 * j) = y;
  }
}

template <int C>
__global__ __launch_bounds__(256) void k_tfm_qkv_f32(TfmQkvF32Args a) {
  constexpr int kXs = C + 4, Cs = tfm_stream_width(C);
  __shared__ __attribute__((aligned(16))) float xs[kTok * kXs];
  const int T = a.npos * kTfmL, g0 = blockIdx.x * kTok;
  const int D = a.D, NH = C / D;
  rms_rows<C>([&](int r, int c) {
    const int g = g0 + r;
    return g < T ? *reinterpret_cast<const f32x4*>(a.x + x_index<Cs>(g, c)) : f32x4{0.f, 0.f, 0.f, 0.f};
  }, a.rms_scale, xs, kXs);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4;
  for (int ct = wave; ct < 3 * C / 16; ct += 4) {
    f32x4 acc[2];
    gemm_tile<C / 32>(a.wqkv, ct, xs, kXs, acc);
    const int oc = 16 * ct + 4 * gq;             // first of the lane's four output channels
    const int which = oc / C, hc = oc % C;        // 0 q, 1 k, 2 v; channel within the C
    const int head = hc / D, d = hc % D;          // d is a multiple of 4: two RoPE pairs (d, d+1), (d+2, d+3)
    float* dst = which == 0 ? a.q : (which == 1 ? a.k : a.v);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int g = g0 + 16 * tt + (lane & 15);
      if (g >= T) continue;
      const int p = g / kTfmL, s = g - p * kTfmL;
      f32x4 y = acc[tt];
      if (which < 2) {   // RoPE.call: x'[2j] = x[2j] cos + x[2j+1] sin, x'[2j+1] = x[2j] sin - x[2j+1] cos (a reflection)
        const f32x4 cs = *reinterpret_cast<const f32x4*>(a.rope_cos + s * D + d);
        const f32x4 sn = *reinterpret_cast<const f32x4*>(a.rope_sin + s * D + d);
        f32x4 z;
        z[0] = y[0] * cs[0] + y[1] * sn[0];
        z[1] = y[0] * sn[1] - y[1] * cs[1];
        z[2] = y[2] * cs[2] + y[3] * sn[2];
        z[3] = y[2] * sn[3] - y[3] * cs[3];
        y = z;
      }
      *reinterpret_cast<f32x4*>(dst + (((size_t)p * NH + head) * kTfmLPad + s) * D + d) = y;
    }
  }
}

// A workgroup takes 64 queries of one (position, head), a 16-query tile per wave (the last of the six workgroups of a
// head has one live wave: queries 352..360).  K and V of a head in fp32 are 2 x 384 x D x 4 bytes, 192 KiB at D = 64, so
// the keys pass through LDS in blocks of kKb = 128: K as [key][D + 4], V transposed as [D][kKb + 4], 67 KiB at D = 64.
// S^T = K . Q^T puts a query in each lane column and 4 keys of every 16-key tile in the lane; O^T = V^T . P^T takes P
// from those registers: MFMA i of key tile t multiplies key 16 t + 4 g + i of lane group g.  The softmax is online over
// the blocks: a block's numerators exp(s - m) use the running maximum m up to and including the block, and o and the sum
// are rescaled by exp(m_old - m).  Keys 361.. are masked (every block holds unmasked keys, so m is finite after the
// first).
constexpr int kKb = 128, kQChunks = 6;

template <int D>
__global__ __launch_bounds__(256) void k_tfm_attn_f32(TfmAttnF32Args a) {
  constexpr int kKs = D + 4, kVt = kKb + 4;
  constexpr int kBt = kKb / 16;        // key tiles per block
  constexpr int kQs = D / 32;          // steps of 32 of q . k
  constexpr int kDt = D / 16;          // 16-channel tiles of o
  __shared__ __attribute__((aligned(16))) float ks[kKb * kKs];
  __shared__ __attribute__((aligned(16))) float vt[D * kVt];
  const int nh = a.heads;
  const int ph = blockIdx.x / kQChunks, chunk = blockIdx.x % kQChunks;   // (position, head); its 64-query chunk
  const int p = ph / nh, head = ph % nh;
  const size_t base = (size_t)ph * kTfmLPad * D;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4, n = lane & 15;
  const int qt = 4 * chunk + wave;
  const bool live = 16 * qt < kTfmL;
  // Scores are scaled by 1 / sqrt(head_dim) (exact at D = 64) and kept in natural units; log2(e) multiplies the
  // difference s - m, which is small where a numerator matters, so its rounding is too.
  const float kScale = D == 32 ? 1.0f / 5.656854249492381f : 0.125f;
  constexpr float kLog2e = 1.4426950408889634f;
  f32x4 bq[kQs][2];
#pragma unroll
  for (int h = 0; h < kQs; ++h) {
    bq[h][0] = bq[h][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) {   // rows up to 367 < 384
      const float* row = a.q + base + (size_t)(16 * qt + n) * D + 32 * h + 8 * gq;
      bq[h][0] = *reinterpret_cast<const f32x4*>(row);
      bq[h][1] = *reinterpret_cast<const f32x4*>(row + 4);
    }
  }
  f32x4 o[kDt];
#pragma unroll
  for (int dt = 0; dt < kDt; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sum = 0.f, m = -3.0e38f;
#pragma unroll 1
  for (int b = 0; b < kTfmLPad / kKb; ++b) {
    if (b) __syncthreads();   // every wave is done with the block before
    for (int i = threadIdx.x; i < kKb * D / 4; i += 256) {
      const int key = i / (D / 4), d0 = 4 * (i % (D / 4));
      const size_t src = base + (size_t)(kKb * b + key) * D + d0;
      *reinterpret_cast<f32x4*>(ks + key * kKs + d0) = *reinterpret_cast<const f32x4*>(a.k + src);
      const f32x4 v = *reinterpret_cast<const f32x4*>(a.v + src);
#pragma unroll
      for (int e = 0; e < 4; ++e) vt[(d0 + e) * kVt + key] = v[e];
    }
    __syncthreads();
    if (!live) continue;
    f32x4 s[kBt];
    float mb = m;
#pragma unroll
    for (int t = 0; t < kBt; ++t) {
      f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < kQs; ++h) {
        const float* row = ks + (16 * t + n) * kKs + 32 * h + 8 * gq;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(row), a1 = *reinterpret_cast<const f32x4*>(row + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) r = mfma(a0[e], bq[h][0][e], r);
#pragma unroll
        for (int e = 0; e < 4; ++e) r = mfma(a1[e], bq[h][1][e], r);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kKb * b + 16 * t + 4 * gq + i;
        r[i] = key < kTfmL ? r[i] * kScale : -3.0e38f;
        mb = fmaxf(mb, r[i]);
      }
      s[t] = r;
    }
    mb = fmaxf(mb, __shfl_xor(mb, 16));
    mb = fmaxf(mb, __shfl_xor(mb, 32));
    const float alpha = exp2f((m - mb) * kLog2e);
    m = mb;
    // the block's own sums from zero (one MFMA chain of 128 products per element), then o = alpha o + its part
    float bsum = 0.f;
    f32x4 ob[kDt];
#pragma unroll
    for (int dt = 0; dt < kDt; ++dt) ob[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < kBt; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[t][i] = exp2f((s[t][i] - m) * kLog2e);
        bsum += s[t][i];
      }
#pragma unroll
    for (int t = 0; t < kBt; ++t)
#pragma unroll
      for (int dt = 0; dt < kDt; ++dt) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(vt + (16 * dt + n) * kVt + 16 * t + 4 * gq);
#pragma unroll
        for (int i = 0; i < 4; ++i) ob[dt] = mfma(av[i], s[t][i], ob[dt]);
      }
    sum = sum * alpha + bsum;
#pragma unroll
    for (int dt = 0; dt < kDt; ++dt) o[dt] = o[dt] * alpha + ob[dt];
  }
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  const int query = 16 * qt + n;
  if (live && query < kTfmL) {
    const float inv = 1.0f / sum;
    const size_t orow = ((size_t)p * kTfmL + query) * (size_t)(nh * D) + (size_t)head * D;
#pragma unroll
    for (int dt = 0; dt < kDt; ++dt) *reinterpret_cast<f32x4*>(a.o + orow + 16 * dt + 4 * gq) = o[dt] * inv;
  }
}

// x1 = x + o . Wo stays in the registers of the lanes that computed it (the Wo and Wdown tiles of a wave are the same
// (ct, token tile) pairs); its rows pass through hs's space for RMSNorm_out, before hs is written.  LDS is
// xs + hs = 32 (C + 4) 4 + 32 (2 C + 4) 4 bytes, 145 KiB at C = 384.
template <int C>
__global__ __launch_bounds__(256) void k_tfm_ffn_f32(TfmFfnF32Args a) {
  constexpr int F = 2 * C, kXs = C + 4, kHs = F + 4, kX1 = C + 4, P = C / 8, Cs = tfm_stream_width(C);
  constexpr int kCt = C / 16, kWt = (kCt + 3) / 4;   // output-channel tiles; per wave at most
  __shared__ __attribute__((aligned(16))) float xs[kTok * kXs];   // o, then RMSNorm_out(x1)
  __shared__ __attribute__((aligned(16))) float hs[kTok * kHs];   // x1 rows, then silu(gate) * up
  float* x1 = hs;
  f32x4 x1r[kWt][2];
  const int T = a.npos * kTfmL, g0 = blockIdx.x * kTok;
  {
    const int r = threadIdx.x >> 3, q = threadIdx.x & 7, g = g0 + r;
#pragma unroll
    for (int j = 0; j < P / 4; ++j) {
      f32x4 h = f32x4{0.f, 0.f, 0.f, 0.f};
      if (g < T) h = *reinterpret_cast<const f32x4*>(a.o + (size_t)g * C + P * q + 4 * j);
      *reinterpret_cast<f32x4*>(xs + r * kXs + P * q + 4 * j) = h;
    }
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4, n = lane & 15;
#pragma unroll
  for (int w = 0; w < kWt; ++w) {
    const int ct = wave + 4 * w;
    if (ct >= kCt) break;
    f32x4 acc[2];
    gemm_tile<C / 32>(a.wo, ct, xs, kXs, acc);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int r = 16 * tt + n, g = g0 + r, c = 16 * ct + 4 * gq;
      f32x4 res = f32x4{0.f, 0.f, 0.f, 0.f};
      if (g < T) res = *reinterpret_cast<const f32x4*>(a.x + x_index<Cs>(g, c));
      x1r[w][tt] = acc[tt] + res;
      *reinterpret_cast<f32x4*>(x1 + r * kX1 + c) = x1r[w][tt];
    }
  }
  __syncthreads();
  rms_rows<C>([&](int r, int c) { return *reinterpret_cast<const f32x4*>(x1 + r * kX1 + c); }, a.rms_scale, xs, kXs);
  __syncthreads();
  for (int c2 = wave; c2 < F / 16; c2 += 4) {   // gate tile c2 and up tile c2 (packed as tiles F / 16 + c2)
    f32x4 gt[2], up[2];
    gemm_tile<C / 32>(a.wgu, c2, xs, kXs, gt);
    gemm_tile<C / 32>(a.wgu, F / 16 + c2, xs, kXs, up);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      f32x4 hv;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t = gt[tt][i];
        hv[i] = t / (1.0f + __expf(-t)) * up[tt][i];
      }
      *reinterpret_cast<f32x4*>(hs + (16 * tt + n) * kHs + 16 * c2 + 4 * gq) = hv;
    }
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kWt; ++w) {
    const int ct = wave + 4 * w;
    if (ct >= kCt) break;
    f32x4 acc[2];
    gemm_tile<F / 32>(a.wdown, ct, hs, kHs, acc);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int r = 16 * tt + n, g = g0 + r, c = 16 * ct + 4 * gq;
      if (g >= T) continue;
      *reinterpret_cast<f32x4*>(a.x + x_index<Cs>(g, c)) = acc[tt] + x1r[w][tt];
    }
  }
}

}  // namespace

static int token_tiles(int npos) { return (npos * kTfmL + kTok - 1) / kTok; }

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

hipError_t launch_tfm_qkv_f32(const TfmQkvF32Args& a, hipStream_t s) {
  if (a.D < 1 || a.npos < 1 || !tfm_supported(a.C, a.C / a.D)) return hipErrorInvalidValue;
  return dispatch_c(a.C, [&](auto c) {
    hipLaunchKernelGGL((k_tfm_qkv_f32<decltype(c)::value>), dim3(token_tiles(a.npos)), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}
hipError_t launch_tfm_attn_f32(int D, const TfmAttnF32Args& a, hipStream_t s) {
  if (a.npos < 1 || a.heads < 1) return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.npos * a.heads * kQChunks);
  if (D == 32) hipLaunchKernelGGL(k_tfm_attn_f32<32>, grid, dim3(256), 0, s, a);
  else if (D == 64) hipLaunchKernelGGL(k_tfm_attn_f32<64>, grid, dim3(256), 0, s, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t launch_tfm_ffn_f32(const TfmFfnF32Args& a, hipStream_t s) {
  if (a.npos < 1) return hipErrorInvalidValue;
  return dispatch_c(a.C, [&](auto c) {
    hipLaunchKernelGGL((k_tfm_ffn_f32<decltype(c)::value>), dim3(token_tiles(a.npos)), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}
const char* tfm_attn_f32_kernel_name() { return "k_tfm_attn_f32"; }

}  // namespace p3
