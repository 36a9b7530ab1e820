// edge_split.hip — k_init_split<CP>, k_bdense_split and k_heads_pool / k_heads_points / k_heads_softmax: the split stem,
// broadcast dense and heads of the low-latency plans (edge_split.h), for gfx950.
//
// The first two are the bodies of layer_kernels.h (init_body, bdense_body / bdense_passes) with the loop over a position's output
// passes taken out of the workgroup: a workgroup keeps ONE pass (the stem's cp, the dense's jp) for all its items, so its
// weight ring walks that pass's part of the stream circularly and never has to change streams between items, and deals
// itself the (position [, half [, channel tile]]) items of that pass round.  What a lane computes for an output value is
// what it computes there, from one text: stem_planes.inc, stem_epilogue.inc, bdense_transpose.inc and bdense_epilogue.inc
// are included here and in those bodies, around the same conv_segment instantiation.  Of the heads,
// heads_score_bin.inc is shared with k_heads; the pooling quad and the per-point loop are k_heads' text written a second
// time, because k_heads' code objects change when it takes its operands through the names a shared text needs
// (DESIGN.md §17).  The wave reductions are conv_core.h's.
#include "edge_split.h"

#include <hip/hip_runtime.h>

#include "launch_util.h"
#include "layer_kernels.h"

namespace p3 {

namespace {

struct InitSplitArgs { InitArgs a; int C; };
struct BDenseSplitArgs { BDenseArgs a; int C, nct; };   // nct: channel tiles an item is cut into, 1 or 4

constexpr int kEdgeMaxC = 512;
constexpr int kDensePassSteps = 6;   // macro-steps of one pass jp of the dense stream: 24 k16 steps (plan.cpp pack_dense)
constexpr int kStemPassSteps = 7;    // ... of one output pass of the stem's stream: 28 taps of 16 channels

// LDS of k_bdense_split: Tt, the ring, the dense bias [384] and the folded bn1 [2][kEdgeMaxC]; one workgroup per CU
constexpr size_t kBDenseSplitLds = kTtBytes + ring_bytes(128) + (384 + 2 * kEdgeMaxC) * 4;
static_assert(kBDenseSplitLds <= 160 * 1024, "k_bdense_split: LDS of one CU");

}  // namespace

// =======================================================================================
// The stem.  Workgroup b owns output pass b % NCP and the positions b / NCP, b / NCP + gridDim.x / NCP, ..
// (gridDim.x is a multiple of NCP).
// =======================================================================================
template <int CP>
__global__ void __launch_bounds__(kWG, 2) k_init_split(InitSplitArgs aa) {
  const InitArgs& a = aa.a;
  const int C = aa.C;
  using G = Geo<1, 16, 5>;
  using T = Tiling<G, CP>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr uint32_t kRingOff = G::ACT_BYTES;
  act_zero<G>(smem);
  const int NCP = C / CP;
  const int cp = blockIdx.x % NCP;
  const int nms = a.nms_total / NCP;   // the stream is pass-major: [cp][28 taps][16 channels]
  Ring<T::RS> ring;
  ring_init(ring, smem, (const char*)a.wstream + (size_t)cp * nms * T::RS, nms, kRingOff);
  lds_barrier();
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lg = wid / T::CG;
  const int lr = lane & 31, h = lane >> 5;

  for (int pos = blockIdx.x / NCP; pos < a.npos; pos += gridDim.x / NCP) {
    // ---- feature planes -> LDS, game-state scalars -> gsv[8] ----------------------------
#include "stem_planes.inc"

    // game-state dense of this pass's channels: thread tc computes (gs . Wg + b)[cp CP + tc] into LDS behind the ring
    // (init_body's sum, term by term); the first ring acquire of the K loop below is the barrier that publishes it
    float* bias_lds = (float*)(smem + kRingOff + ring_bytes(CP));
    const int tc = launder(threadIdx.x);
    if (tc < CP) {
      const int c = cp * CP + tc;
      float b = a.game_b[c];
#pragma unroll
      for (int k = 0; k < 8; ++k) b += a.game_w[k * C + c] * gsv[k];
      bias_lds[tc] = b;
    }

    f32x16 acc[2][T::NT];
    acc_zero<G, CP>(acc);
    conv_segment<G, CP, 5, 28>(ring, smem, acc);
    // epilogue: + (gs . Wg + b)[c]  -> x
    constexpr int bias_cp = 0;
#include "stem_epilogue.inc"
    lds_barrier();   // the next position rewrites the planes and the bias
  }
  ring_drain();
}

// =======================================================================================
// The broadcast dense.  Workgroup b owns dense pass jp = b % 3 and the items b / 3, b / 3 + gridDim.x / 3, .. of
// (position, half [, channel tile]); gridDim.x is a multiple of 3.  An item with a channel tile stages that tile's four
// channel blocks only: the rows of Tt are the channels, a row of the product needs its own row of Tt alone, so what the
// other rows hold (an earlier item's channels) changes nothing that is stored.
// =======================================================================================
namespace {

// one pass of bdense_passes: the 128 dense columns of pass jp for the channels in Tt; `active`: this wave's channel
// tile is the item's (and real)
template <class W>
__device__ __forceinline__ void bdense_one_pass(W wc, Ring<16384>& ring, char* smem, const float* p_bias, const float* p_scale,
                                                const float* p_shift, _Float16* __restrict__ u, int pos, int half, int jp,
                                                bool active) {
  const int C = wc.get();
  constexpr int CH = kTtChannels;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int jg = wid & 1;        // which 64 of the 128 j rows in this pass
  const int ct = wid >> 1;       // channel tile (32 channels) 0..3
  const int lr = lane & 31, h = lane >> 5;
  f32x16 acc2[2][1];
  acc_zero<GeoTt, 128>(acc2);
  conv_segment<GeoTt, 128, 1, 1, true>(ring, smem, acc2);
  if (!active) return;
#include "bdense_epilogue.inc"
}

}  // namespace

__global__ void __launch_bounds__(kWG, 2) k_bdense_split(BDenseSplitArgs aa) {
  const BDenseArgs& a = aa.a;
  const RuntimeW wc{aa.C};
  const int C = aa.C, nct = aa.nct;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int CH = kTtChannels;
  constexpr uint32_t kRingOff = kTtBytes;
  for (int i = threadIdx.x * 16; i < (int)kTtBytes; i += kWG * 16) *(f32x4*)(smem + i) = f32x4{0, 0, 0, 0};
  const int jp = blockIdx.x % 3;
  const int nms = a.nms_total / 3;   // the stream is pass-major: [jp][24 k16 steps]
  Ring<16384> ring;
  ring_init(ring, smem, (const char*)a.wstream + (size_t)jp * nms * 16384, nms, kRingOff);
  float* p_bias = (float*)(smem + kRingOff + ring_bytes(128));
  float* p_scale = p_bias + 384;
  float* p_shift = p_scale + C;
  bdense_stage_params(wc, p_bias, a.bias, a.scale, a.shift);
  lds_barrier();

  using GS = Geo<1, 128, 1>;
  const int NHALF = (C + CH - 1) / CH;
  const long items = (long)a.npos * NHALF * nct;
  const long stride = gridDim.x / 3;
  const int combo = threadIdx.x >> 5, l32 = threadIdx.x & 31;   // combo = channel block of the pass
  struct Item { int pos, half, ct, nch; };
  // item index -> (position, half, channel tile or -1); past the end: the last item again (loaded, never stored)
  auto item_of = [&](long it) {
    if (it >= items) it = items - 1;
    Item r;
    r.ct = nct == 4 ? (int)(it & 3) : -1;
    const long ph = it / nct;
    r.pos = (int)(ph / NHALF);
    r.half = (int)(ph - (long)r.pos * NHALF);
    r.nch = (C - r.half * CH) < CH ? (C - r.half * CH) : CH;
    return r;
  };
  // this thread's channel block is one the item stages
  auto mine = [&](const Item& it) { return combo * 8 < it.nch && (it.ct < 0 || (combo >> 2) == it.ct); };
  // Every thread issues its kXLoads loads, as bdense_body (the ring's vmcnt bookkeeping counts them): a thread whose
  // block the item does not stage re-reads the half's first block, which always exists, and ignores it
  XRegs<GS> xr;
  auto pair_load = [&](const Item& it) {
    static_assert(kXLoads == 12, "six pairs");
    const int cblk = it.half * (CH / 8) + (mine(it) ? combo : 0);
    const _Float16* src = a.t + ((size_t)it.pos * (C / 8) + cblk) * (kNLoc * 8);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      int l0 = 2 * (l32 + 32 * i), l1 = l0 + 1;
      if (l0 >= kNLoc) l0 = kNLoc - 1;   // tail lanes re-read a valid point (not stored)
      if (l1 >= kNLoc) l1 = kNLoc - 1;
      xr.v[2 * i] = *(const h8*)(src + l0 * 8);
      xr.v[2 * i + 1] = *(const h8*)(src + l1 * 8);
    }
  };
  pair_load(item_of(blockIdx.x / 3));
  for (long idx = blockIdx.x / 3; idx < items; idx += stride) {
    const Item it = item_of(idx);
    lds_barrier();
    // ---- transpose-stage t[pos][cblk][loc][8] -> Tt[c][i], as bdense_body ---------------
    if (mine(it)) {
#include "bdense_transpose.inc"
    }
    pair_load(item_of(idx + stride));
    ring_note_xloads(ring);
    const int wct = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);   // this wave's channel tile
    bdense_one_pass(wc, ring, smem, p_bias, p_scale, p_shift, a.u, it.pos, it.half, jp,
                    wct * 32 < it.nch && (it.ct < 0 || wct == it.ct));
  }
  lds_barrier();
  ring_drain();
}

// =======================================================================================
// The heads: k_heads (kernels.hip) in three launches, cut where a value needs another workgroup's.
//   k_heads_pool     one wave per channel quad of g and v, four quads per workgroup: the pooled values -> `pooled`
//   k_heads_points   `parts` workgroups per position.  The first parts / 4 take ranges of the 361 board points: gbias from
//                    the pooled g, then the policy and optimistic-policy logits and the ownership of their points (the
//                    first one the two pass logits as well).  The others take ranges of the 800 score bins: base, gpre and
//                    gamma from the pooled v, then their bins' logits (the first one the outcome logits, err2 and gamma
//                    as well).  Logits go to the output row.
//   k_heads_softmax  one workgroup per (position, softmax) with k_heads' thread mapping, i = t; i += 256, wave_max /
//                    wave_sum and the four-wave combine in its written order: the same max and sum; the value softmax
// Every expression is k_heads', in its order of operations; the weights come from global memory where k_heads staged
// them in LDS, which changes no value.
// =======================================================================================
namespace {

struct HeadsSplitArgs { HeadsArgs a; float* pooled; int parts; };
constexpr int kHeadsH = 32, kHeadsMaxV = 80;
static_assert(kHeadsPoolFloats == 4 * kHeadsH, "pooled values of a position: mean and max of g, mean and max of v");

}  // namespace

__global__ void __launch_bounds__(256) k_heads_pool(HeadsSplitArgs aa) {
  const HeadsArgs& a = aa.a;
  constexpr int H = kHeadsH;
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pos = blockIdx.x >> 2, qd = (blockIdx.x & 3) * 4 + wid;   // quad of the g / v channels
  const f32x4* __restrict__ hp4 = (const f32x4*)(a.hp + (size_t)pos * 3 * H * kNLoc);
  const int c = 4 * qd;                          // g channels are c < H, v channels c >= H
  const f32x4* src = hp4 + (size_t)(H / 4 + qd) * kNLoc;
  f32x4 v[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int i = lane + 64 * k;
    v[k] = src[i < kNLoc ? i : kNLoc - 1];
  }
  const bool is_g = c < H;
  const int ch = is_g ? c : c - H;
  float* dst = aa.pooled + (size_t)pos * kHeadsPoolFloats + (is_g ? 0 : 2 * H);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float bsc = is_g ? a.gbn_scale[ch + e] : 1.0f, bsh = is_g ? a.gbn_shift[ch + e] : 0.0f;
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
      dst[ch + e] = s * (1.0f / kNLoc);
      dst[H + ch + e] = m;
    }
  }
}

__global__ void __launch_bounds__(256) k_heads_points(HeadsSplitArgs aa) {
  const HeadsArgs& a = aa.a;
  constexpr int H = kHeadsH;
  const int V = a.V, parts = aa.parts, np = parts / 4, nb = parts - np;
  const int t = threadIdx.x;
  const int pos = blockIdx.x / parts, r = blockIdx.x - pos * parts;
  __shared__ float pl[2 * H], gbias[H], w_moves[2 * H], w_opt[H], w_own[H];
  __shared__ float emb[kHeadsMaxV], gpre[kHeadsMaxV], base[kHeadsMaxV], w_sp[kHeadsMaxV], w_so[kHeadsMaxV], misc[4];
  const f32x4* __restrict__ hp4 = (const f32x4*)(a.hp + (size_t)pos * 3 * H * kNLoc);
  float* __restrict__ out = a.out + (size_t)pos * kOutStride;
  float* __restrict__ res = a.res ? a.res + (size_t)pos * kResultFloats : nullptr;
  const float* pooled = aa.pooled + (size_t)pos * kHeadsPoolFloats;
  if (r < np) {
    // ---- board points: pl = gp -----------------------------------------------------------------------
    if (t < 2 * H) { pl[t] = pooled[t]; w_moves[t] = a.moves_w[t]; }
    if (t < H) { w_opt[t] = a.opt_moves_w[t]; w_own[t] = a.own_w[t]; }
    __syncthreads();
    if (t < H) {
      float s = a.gd_b[t];
#pragma unroll 8
      for (int k = 0; k < 2 * H; ++k) s += pl[k] * a.gd_w[k * H + t];
      gbias[t] = s;
    } else if (t == 192 && r == 0) {
      float s0 = a.pass_b[0], so = a.opt_pass_b[0];
#pragma unroll 8
      for (int k = 0; k < 2 * H; ++k) {
        s0 += pl[k] * a.pass_w[k * 2];
        so += pl[k] * a.opt_pass_w[k];
      }
      out[kOffMoveLogits + 361] = s0 - 3.0f;
      out[kOffOptLogits + 361] = so - 3.0f;
      if (res) res[kOffMoveLogits + 361] = s0 - 3.0f;
    }
    __syncthreads();
    const int per = (kNLoc + np - 1) / np, lo = r * per, hi = lo + per < kNLoc ? lo + per : kNLoc;
    for (int i = lo + t; i < hi; i += 256) {
      float pi = 0.0f, po = 0.0f, ow = 0.0f;
      const int z = launder(0);   // keeps the LDS weight reads inside the location loop
#pragma unroll
      for (int c0 = 0; c0 < H; c0 += 8) {   // four 16-byte loads in flight per round
        float pv[8], vv[8];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const f32x4 p4 = hp4[(size_t)(c0 / 4 + u) * kNLoc + i];
          const f32x4 v4 = hp4[(size_t)(2 * H / 4 + c0 / 4 + u) * kNLoc + i];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            pv[4 * u + e] = p4[e];
            vv[4 * u + e] = v4[e];
          }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float p = mish_f(pv[c] + gbias[z + c0 + c]);
          pi += p * w_moves[z + (c0 + c) * 2];
          po += p * w_opt[z + c0 + c];
          ow += vv[c] * w_own[z + c0 + c];
        }
      }
      out[kOffMoveLogits + i] = pi;
      out[kOffOptLogits + i] = po;
      if (res) res[kOffMoveLogits + i] = pi;
      out[kOffOwnership + i] = tanhf(ow);
    }
    return;
  }
  // ---- score bins: pl = vp ---------------------------------------------------------------------------
  const int rb = r - np;
  if (t < 2 * H) pl[t] = pooled[2 * H + t];
  if (t < V) { w_sp[t] = a.score_pre_w[(2 * H) * V + t]; w_so[t] = a.score_out_w[t]; }
  __syncthreads();
  if (t < V) {
    const int o = t;
    float s = a.oq_embed_b[o], gm = a.gamma_pre_b[o], b = a.score_pre_b[o];
#pragma unroll 8
    for (int k = 0; k < 2 * H; ++k) {
      const float x = pl[k];
      s += x * a.oq_embed_w[k * V + o];
      gm += x * a.gamma_pre_w[k * V + o];
      b += x * a.score_pre_w[k * V + o];
    }
    emb[o] = mish_f(s);
    gpre[o] = mish_f(gm);
    base[o] = b;
  }
  __syncthreads();
  if (t < 14 && rb == 0) {
    float s = a.oq_out_b[t];
#pragma unroll 8
    for (int k = 0; k < V; ++k) s += emb[k] * a.oq_out_w[k * 14 + t];
    if (t < 2) out[kOffOutcomeLogits + t] = s;
    if (t == 5) {
      out[kOffErr2] = 4.0f / (1.0f + __expf(-s));
      if (res) res[kOffErr2] = out[kOffErr2];
    }
  } else if (t == 64) {
    float s = a.gamma_out_b[0];
#pragma unroll 8
    for (int k = 0; k < V; ++k) s += gpre[k] * a.gamma_out_w[k];
    if (rb == 0) out[kOffGamma] = s;
    const float sp = s > 20.0f ? s : log1pf(__expf(s));
    misc[2] = fminf(sp, 10.0f);
  }
  __syncthreads();
  {
    const float gam = misc[2], score_out_b = a.score_out_b[0];
    const int per = (800 + nb - 1) / nb, lo = rb * per, hi = lo + per < 800 ? lo + per : 800;
    for (int sidx = lo + t; sidx < hi; sidx += 256) {
#include "heads_score_bin.inc"
      out[kOffScoreLogits + sidx] = gam * s;
    }
  }
}

__global__ void __launch_bounds__(256) k_heads_softmax(HeadsSplitArgs aa) {
  const HeadsArgs& a = aa.a;
  const int t = threadIdx.x, wid = t >> 6, lane = t & 63;
  const int pos = blockIdx.x / 3, r = blockIdx.x - pos * 3;   // r: policy, optimistic policy, score
  __shared__ float red[4];
  float* __restrict__ out = a.out + (size_t)pos * kOutStride;
  float* __restrict__ res = a.res ? a.res + (size_t)pos * kResultFloats : nullptr;
  const int n = r == 2 ? 800 : 362;
  const int src = r == 0 ? kOffMoveLogits : r == 1 ? kOffOptLogits : kOffScoreLogits;
  const int dst = r == 0 ? kOffMoveProbs : r == 1 ? kOffOptProbs : kOffScoreProbs;
  float lg[4];   // this thread's logits, then their exponentials: i = t + 256 k
  float m = -3.0e38f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = t + 256 * k;
    if (i < n) {
      lg[k] = out[src + i];
      m = fmaxf(m, lg[k]);
    }
  }
  m = wave_max(m);
  if (lane == 0) red[wid] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();   // red is rewritten below
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = t + 256 * k;
    if (i < n) {
      lg[k] = __expf(lg[k] - m);
      s += lg[k];
    }
  }
  s = wave_sum(s);
  if (lane == 0) red[wid] = s;
  __syncthreads();
  const float inv = 1.0f / (red[0] + red[1] + red[2] + red[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = t + 256 * k;
    if (i < n) {
      out[dst + i] = lg[k] * inv;
      if (res) res[dst + i] = lg[k] * inv;
    }
  }
  if (r == 2 && t == 0) {
    const float v0 = out[kOffOutcomeLogits], v1 = out[kOffOutcomeLogits + 1];
    const float mm = fmaxf(v0, v1);
    const float e0 = __expf(v0 - mm), e1 = __expf(v1 - mm);
    out[kOffValueProbs] = e0 / (e0 + e1);
    out[kOffValueProbs + 1] = e1 / (e0 + e1);
    if (res) {
      res[kOffValueProbs] = e0 / (e0 + e1);
      res[kOffValueProbs + 1] = e1 / (e0 + e1);
    }
  }
}

// =======================================================================================
// Host-side launchers
// =======================================================================================
namespace {

// the items dealt round over whole units of `unit` workgroups (one per pass), at most n_cu of them
int unit_grid(long items, int unit, int n_cu) {
  long cap = (long)(n_cu / unit) * unit;
  if (cap < unit) cap = unit;
  return (int)(items < cap ? items : cap);
}

template <int CP>
hipError_t launch_init_split_cp(const InitSplitArgs& a, int n_cu, hipStream_t s) {
  using G = Geo<1, 16, 5>;
  constexpr size_t lds = G::ACT_BYTES + ring_bytes(CP) + CP * 4;   // + the game-state bias of the pass
  static_assert(2 * lds <= 160 * 1024, "k_init_split: two workgroups per CU");
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_init_split<CP>, lds); e != hipSuccess) return e;
  const int ncp = a.C / CP;
  hipLaunchKernelGGL((k_init_split<CP>), dim3(unit_grid((long)a.a.npos * ncp, ncp, n_cu)), dim3(kWG), lds, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_init_split(int C, const InitArgs& a, int parts, int n_cu, hipStream_t s) {
  if (!edge_width_ok(C) || a.npos < 1 || n_cu < 1 || parts < 2 || parts != edge_stem_passes(C) ||
      a.nms_total != parts * kStemPassSteps)
    return hipErrorInvalidValue;
  const InitSplitArgs b{a, C};
  return edge_stem_pass(C) == 128 ? launch_init_split_cp<128>(b, n_cu, s) : launch_init_split_cp<64>(b, n_cu, s);
}

hipError_t launch_bdense_split(int C, const BDenseArgs& a, int parts, int n_cu, hipStream_t s) {
  if (!edge_width_ok(C) || a.npos < 1 || n_cu < 1 || (parts != 3 && parts != 12) || a.nms_total != 3 * kDensePassSteps)
    return hipErrorInvalidValue;
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_bdense_split, kBDenseSplitLds); e != hipSuccess) return e;
  const BDenseSplitArgs b{a, C, parts / 3};
  const long items = (long)a.npos * ((C + kTtChannels - 1) / kTtChannels) * parts;
  hipLaunchKernelGGL(k_bdense_split, dim3(unit_grid(items, 3, n_cu)), dim3(kWG), kBDenseSplitLds, s, b);
  return hipGetLastError();
}

hipError_t launch_heads_split(const HeadsArgs& a, float* pooled, int parts, hipStream_t s) {
  if (a.npos < 1 || !pooled || (parts != 4 && parts != 8) || a.V < 1 || a.V > kHeadsMaxV) return hipErrorInvalidValue;
  const HeadsSplitArgs b{a, pooled, parts};
  hipLaunchKernelGGL(k_heads_pool, dim3(a.npos * 4), dim3(256), 0, s, b);
  hipLaunchKernelGGL(k_heads_points, dim3(a.npos * parts), dim3(256), 0, s, b);
  hipLaunchKernelGGL(k_heads_softmax, dim3(a.npos * 3), dim3(256), 0, s, b);
  return hipGetLastError();
}

}  // namespace p3
