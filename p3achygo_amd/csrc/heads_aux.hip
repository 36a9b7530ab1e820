// heads_aux.hip — k_heads_aux: the fifteen outputs of the model that k_heads / k_headsx leave out (heads_aux.h), from the
// head convs' fp32 output hp.  PolicyHead.call model.py:791-810 (out_moves channel 1, soft_moves, their pass logits),
// ValueHead.call :893-904 and :950-973 (the eleven remaining columns of oq_out, mcts_dist), the softmax of :1267.
//
// fp32 VALU throughout, one 256-thread workgroup per position at a time.  A position reads its p channels once and its
// g and v channels once (139 KB) and writes one 3,360 B record; every weight is staged in LDS once per workgroup.
#include <hip/hip_runtime.h>

#include "conv_core.h"
#include "heads_aux.h"
#include "launch_util.h"

namespace p3 {
namespace {

constexpr int kH = 32;          // head channels
constexpr int kAuxWg = 256;

// LDS plan (float offsets), every region a multiple of four floats so that the record is 16-byte aligned
struct AuxLds {
  int gd_w, oq_embed_w, mcts_w, oq_aux_w, pass_aux_w, soft_pass_w, moves_aux_w, soft_moves_w, gbn_scale, gbn_shift, gd_b,
      oq_embed_b, mcts_b, oq_aux_b, gp, vp, gbias, emb, rec, total;
  __host__ __device__ explicit AuxLds(int V) {
    int o = 0;
    auto take = [&](int n) { const int at = o; o += (n + 3) & ~3; return at; };
    gd_w = take(2 * kH * kH);
    oq_embed_w = take(2 * kH * V);
    mcts_w = take(V * kAuxBins);
    oq_aux_w = take(V * kAuxGoCols);
    pass_aux_w = take(2 * kH);
    soft_pass_w = take(2 * kH);
    moves_aux_w = take(kH);
    soft_moves_w = take(kH);
    gbn_scale = take(kH);
    gbn_shift = take(kH);
    gd_b = take(kH);
    oq_embed_b = take(V);
    mcts_b = take(kAuxBins);
    oq_aux_b = take(kAuxGoCols);
    gp = take(2 * kH);
    vp = take(2 * kH);
    gbias = take(kH);
    emb = take(V);
    rec = take(kAuxStride);
    total = o;
  }
};

__global__ void __launch_bounds__(kAuxWg) k_heads_aux(HeadsAuxArgs a) {
  extern __shared__ __attribute__((aligned(16))) float al[];
  const int V = a.V;
  const AuxLds L(V);
  const int t = threadIdx.x, wid = t >> 6, lane = t & 63;
  auto stage = [&](int off, const float* __restrict__ src, int n) {
    for (int i = t; i < n; i += kAuxWg) al[off + i] = src[i];
  };
  stage(L.gd_w, a.gd_w, 2 * kH * kH);
  stage(L.oq_embed_w, a.oq_embed_w, 2 * kH * V);
  stage(L.mcts_w, a.mcts_w, V * kAuxBins);
  stage(L.oq_aux_w, a.oq_aux_w, V * kAuxGoCols);
  stage(L.pass_aux_w, a.pass_aux_w, 2 * kH);
  stage(L.soft_pass_w, a.soft_pass_w, 2 * kH);
  stage(L.moves_aux_w, a.moves_aux_w, kH);
  stage(L.soft_moves_w, a.soft_moves_w, kH);
  stage(L.gbn_scale, a.gbn_scale, kH);
  stage(L.gbn_shift, a.gbn_shift, kH);
  stage(L.gd_b, a.gd_b, kH);
  stage(L.oq_embed_b, a.oq_embed_b, V);
  stage(L.mcts_b, a.mcts_b, kAuxBins);
  stage(L.oq_aux_b, a.oq_aux_b, kAuxGoCols);
  const float pass_aux_b = a.pass_aux_b[0], soft_pass_b = a.soft_pass_b[0];
  float* __restrict__ rec = al + L.rec;
  if (t < kAuxStride - kAuxFloats) rec[kAuxFloats + t] = 0.0f;   // the row's padding
  __syncthreads();

  for (int pos = blockIdx.x; pos < a.npos; pos += gridDim.x) {
    // head activations as channel quads (HeadsArgs::hp): quads 0 .. 7 = p, 8 .. 15 = g, 16 .. 23 = v
    const f32x4* __restrict__ hp4 = (const f32x4*)(a.hp + (size_t)pos * 3 * kH * kNLoc);
    // ---- pooled g (after bn + mish) and pooled v (raw): one wave per channel quad, as k_heads -------------------
    for (int qd = wid; qd < 2 * kH / 4; qd += 4) {
      const int c = 4 * qd;
      const f32x4* src = hp4 + (size_t)(kH / 4 + qd) * kNLoc;
      f32x4 v[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int i = lane + 64 * k;
        v[k] = src[i < kNLoc ? i : kNLoc - 1];
      }
      const bool is_g = c < kH;
      const int ch = is_g ? c : c - kH;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float bsc = is_g ? al[L.gbn_scale + ch + e] : 1.0f, bsh = is_g ? al[L.gbn_shift + ch + e] : 0.0f;
        float s = 0.0f, m = -3.0e38f;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          float x = v[k][e];
          if (is_g) x = mish_f(x * bsc + bsh);
          if (lane + 64 * k < kNLoc) {
            s += x;
            m = fmaxf(m, x);
          }
        }
        s = wave_sum(s);
        m = wave_max(m);
        if (lane == 0) {
          float* dst = al + (is_g ? L.gp : L.vp);
          dst[ch + e] = s * (1.0f / kNLoc);
          dst[kH + ch + e] = m;
        }
      }
    }
    __syncthreads();
    // ---- the pooled bias, emb = mish(oq_embed(vp)), the two pass logits ------------------------------------------
    if (t < kH) {
      float s = al[L.gd_b + t];
#pragma unroll 8
      for (int k = 0; k < 2 * kH; ++k) s += al[L.gp + k] * al[L.gd_w + k * kH + t];
      al[L.gbias + t] = s;
    } else if (t >= 64 && t < 64 + V) {
      const int o = t - 64;
      float s = al[L.oq_embed_b + o];
#pragma unroll 8
      for (int k = 0; k < 2 * kH; ++k) s += al[L.vp + k] * al[L.oq_embed_w + k * V + o];
      al[L.emb + o] = mish_f(s);
    } else if (t == 192 || t == 193) {
      const int w = t == 192 ? L.pass_aux_w : L.soft_pass_w;
      float s = t == 192 ? pass_aux_b : soft_pass_b;
#pragma unroll 8
      for (int k = 0; k < 2 * kH; ++k) s += al[L.gp + k] * al[w + k];
      rec[(t == 192 ? kAuxOffPiAux : kAuxOffPiSoft) + 361] = s - 3.0f;
    }
    __syncthreads();
    // ---- go's eleven columns with their activations; the 51 bin logits ---------------------------------------------
    if (t < kAuxGoCols) {
      float s = 0.0f;   // the bias last: it may dwarf the products (the far tail of the sigmoid)
#pragma unroll 8
      for (int k = 0; k < V; ++k) s += al[L.emb + k] * al[L.oq_aux_w + k * kAuxGoCols + t];
      s += al[L.oq_aux_b + t];
      // columns 2, 3, 4 | 6, 7 | 8, 9, 10 | 11, 12, 13 of go lie in record order from kAuxOffQ on
      float r = s;
      if (t < 3) r = tanhf(s);
      else if (t < 5) r = 4.0f / (1.0f + __expf(-s));   // exp(-s) = inf below -88.7 gives 4 / inf = 0, never inf / inf
      else if (t >= 8) r = fabsf(s);
      rec[kAuxOffQ + t] = r;
    } else if (t >= 64 && t < 64 + kAuxBins) {
      const int o = t - 64;
      float s = 0.0f;
#pragma unroll 8
      for (int k = 0; k < V; ++k) s += al[L.emb + k] * al[L.mcts_w + k * kAuxBins + o];
      s += al[L.mcts_b + o];
      rec[kAuxOffMctsLogits + o] = s;
    }
    // ---- the two 1x1 maps over the activated p ------------------------------------------------------------------
    for (int i = t; i < kNLoc; i += kAuxWg) {
      float pa = 0.0f, ps = 0.0f;
#pragma unroll
      for (int c0 = 0; c0 < kH; c0 += 8) {
        const f32x4 p0 = hp4[(size_t)(c0 / 4) * kNLoc + i], p1 = hp4[(size_t)(c0 / 4 + 1) * kNLoc + i];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float p = mish_f((c < 4 ? p0[c & 3] : p1[c & 3]) + al[L.gbias + c0 + c]);
          pa += p * al[L.moves_aux_w + c0 + c];
          ps += p * al[L.soft_moves_w + c0 + c];
        }
      }
      rec[kAuxOffPiAux + i] = pa;
      rec[kAuxOffPiSoft + i] = ps;
    }
    __syncthreads();
    // ---- softmax of the bins: one wave, the row maximum subtracted ------------------------------------------------
    if (wid == 0) {
      const bool on = lane < kAuxBins;
      const float l = on ? rec[kAuxOffMctsLogits + lane] : -3.0e38f;
      const float m = wave_max(l);
      const float e = on ? __expf(l - m) : 0.0f;
      const float sum = wave_sum(e);
      if (on) rec[kAuxOffMctsProbs + lane] = e * (1.0f / sum);
    }
    __syncthreads();
    // ---- the record, 16 bytes per lane -----------------------------------------------------------------------------
    if (t < kAuxStride / 4) ((f32x4*)(a.aux + (size_t)pos * kAuxStride))[t] = ((const f32x4*)rec)[t];
    __syncthreads();   // rec and the pooled values are rewritten by the next position
  }
}

}  // namespace

hipError_t launch_heads_aux(const HeadsAuxArgs& a, int n_cu, hipStream_t s) {
  if (a.npos < 1 || (a.V != 32 && a.V != 48 && a.V != 64 && a.V != 80)) return hipErrorInvalidValue;
  const size_t lds = (size_t)AuxLds(80).total * 4;   // the attribute is set once: for the widest V
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_heads_aux, lds); e != hipSuccess) return e;
  const int grid = a.npos < 2 * n_cu ? a.npos : 2 * n_cu;   // 55 KB of LDS at V = 80: two workgroups per CU
  hipLaunchKernelGGL(k_heads_aux, dim3(grid), dim3(kAuxWg), (size_t)AuxLds(a.V).total * 4, s, a);
  return hipGetLastError();
}

}  // namespace p3
