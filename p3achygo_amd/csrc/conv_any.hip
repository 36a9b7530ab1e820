// conv_any.hip — gfx950 kernels of the layer-wise conv trunk at any width from 64 to 512 channels (conv_any.h).
//
// They are the kernels of kernels.hip with the channel counts turned from template arguments into launch arguments:
// the K-slice loop count, the output pass count and the layout strides are runtime values, in units of 64 channels.
// What stays a template argument is what changes the instruction stream (kernel size, prologue / epilogue flags,
// slice and pass width).  One kernel per flag set serves every width; with the same slices in the same order the
// results are bit for bit those of the templated kernels (P3HIP_CONV_ANY=1 runs the C = 384 and classic C = 192
// trunks through these; tests/test_conv_widths_gpu.py compares).
//
// Layouts, ring and tiling: conv_core.h, as in kernels.hip.  Activation offsets are 64-bit per position
// (stage_load, residual_addr), the 32-bit lane offsets stay inside one workgroup's positions.
#include "conv_any.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>

#include "conv_core.h"

namespace p3 {

namespace {

struct InitAnyArgs { InitArgs a; int C; };
struct Conv1x1AnyArgs { Conv1x1Args a; int cin, cout; };
struct LConvAnyArgs { LConvArgs a; int nip, ncp; };   // input slices / output passes of 64 channels
struct BDenseAnyArgs { BDenseArgs a; int C; };

struct FeatOff {  // byte offsets inside p3hip_features (include/p3hip.h)
  static constexpr int color = 4, komi = 8, board = 12, last = 376, atari = 416, two = 777,
                       three = 1138, ladder = 1499, size = 1860;
};

}  // namespace

// =======================================================================================
// Initial 5x5 conv + game-state dense (k_init of kernels.hip), C a launch argument.
// =======================================================================================
template <int CP>
__global__ void __launch_bounds__(kWG, 2) k_init_any(InitAnyArgs aa) {
  const InitArgs& a = aa.a;
  const int C = aa.C;
  using G = Geo<1, 16, 5>;
  using T = Tiling<G, CP>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr uint32_t kRingOff = G::ACT_BYTES;
  act_zero<G>(smem);
  Ring<T::RS> ring;
  ring_init(ring, smem, a.wstream, a.nms_total, kRingOff);
  lds_barrier();
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lg = wid / T::CG;
  const int lr = lane & 31, h = lane >> 5;

  for (int pos = blockIdx.x; pos < a.npos; pos += gridDim.x) {
    const unsigned char* f = (const unsigned char*)a.feats + (size_t)pos * FeatOff::size;
    const int color = (signed char)f[FeatOff::color];
    for (int loc = threadIdx.x; loc < kNLoc; loc += kWG) {
      h8 lo = {0, 0, 0, 0, 0, 0, 0, 0}, hi = {0, 0, 0, 0, 0, 0, 0, 0};
      auto our = [&](int off) {
        return (_Float16)((signed char)f[off + loc] == color ? 1.0f : 0.0f);
      };
      auto opp = [&](int off) {
        return (_Float16)((signed char)f[off + loc] == -color ? 1.0f : 0.0f);
      };
      lo[0] = our(FeatOff::board); lo[1] = opp(FeatOff::board);
      lo[7] = our(FeatOff::atari); hi[0] = opp(FeatOff::atari);
      hi[1] = our(FeatOff::two); hi[2] = opp(FeatOff::two);
      hi[3] = our(FeatOff::three); hi[4] = opp(FeatOff::three);
      hi[5] = our(FeatOff::ladder); hi[6] = opp(FeatOff::ladder);
      const int y = (loc * 3450) >> 16, xx = loc - y * kBL;
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const int* lm = (const int*)(f + FeatOff::last + m * 8);
        if (lm[0] == y && lm[1] == xx) lo[2 + m] = (_Float16)1.0f;  // pass {19,0}/noop never match
      }
      const int s = G::PADTOP + y * G::S + xx;
      *(h8*)(smem + s * G::SLOTB) = lo;
      *(h8*)(smem + s * G::SLOTB + 16) = hi;
    }
    float gsv[8];
    gsv[0] = color == 1 ? 1.0f : 0.0f;
    gsv[1] = color == 1 ? 0.0f : 1.0f;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      const int* lm = (const int*)(f + FeatOff::last + m * 8);
      gsv[2 + m] = (lm[0] == 19 && lm[1] == 0) ? 1.0f : 0.0f;
    }
    gsv[7] = (color == 1 ? -1.0f : 1.0f) * (*(const float*)(f + FeatOff::komi)) / 15.0f;

    // game-state dense: thread c computes (gs . Wg + b)[c] into LDS behind the ring (kConvAnyMaxC floats = one
    // channel per thread of the workgroup); the first ring acquire below is the barrier that publishes it
    static_assert(kConvAnyMaxC <= kWG, "one thread per channel");
    float* bias_lds = (float*)(smem + kRingOff + ring_bytes(CP));
    // (laundered: with C a runtime value the eight weight addresses would be hoisted out of the position loop and spilled)
    const int tc = launder((int)threadIdx.x);
    if (tc < C) {
      float b = a.game_b[tc];
#pragma unroll
      for (int k = 0; k < 8; ++k) b += a.game_w[k * C + tc] * gsv[k];
      bias_lds[tc] = b;
    }

#pragma unroll 1
    for (int cp = 0; cp < C / CP; ++cp) {
      f32x16 acc[2][T::NT];
      acc_zero<G, CP>(acc);
      conv_segment<G, CP, 5, 28>(ring, smem, acc);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int c = cp * CP + acc_chan<G, CP>(mt, g4);
          const f32x4 bias = *(const f32x4*)(bias_lds + c);
#pragma unroll
          for (int j = 0; j < T::NT; ++j) {
            const int t = lg + j * T::LG;
            if (t >= G::NT_TOTAL) continue;
            const int r = t * 32 + lr;
            int loc;
            if (!row_valid<G::S>(r, loc)) continue;
            h4 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = (_Float16)(acc[mt][j][g4 * 4 + i] + bias[i]);
            *(h4*)(a.x + ((size_t)pos * (C / 8) + (c >> 3)) * (kNLoc * 8) + loc * 8 + h * 4) = o;
          }
        }
    }
    lds_barrier();
  }
  ring_drain();
}

// =======================================================================================
// 1x1 conv over the channel-blocked stream (k_conv1x1 of kernels.hip): CB-channel K slices, CP-channel output
// passes split across workgroups; cin a multiple of CB, cout <= NCP * CP.
//   PRE / EPI as there: EPI 0 out = mish(acc) fp16, 1 x += acc, 2 head activations fp32 channel quads
// =======================================================================================
template <int CB, int CP, bool PRE, int EPI>
__global__ void __launch_bounds__(kWG, 2) k_conv1x1_any(Conv1x1AnyArgs aa) {
  const Conv1x1Args& a = aa.a;
  const int CIN = aa.cin, COUT = aa.cout;
  constexpr int NPOS = 128 / CB;
  using G = Geo<NPOS, CB, 1>;
  using T = Tiling<G, CP>;
  const int NCP = (COUT + CP - 1) / CP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr uint32_t kRingOff = G::ACT_BYTES;
  act_zero<G>(smem);
  // workgroup b owns pass cp = (b / 8) % NCP of the position groups pg0, pg0 + gridDim / NCP, ...: the NCP workgroups
  // of one position group are 8 block ids apart, on one XCD (conv_split_grid)
  const int cp = (blockIdx.x >> 3) % NCP;
  const int pg0 = (blockIdx.x / (8 * NCP)) * 8 + (blockIdx.x & 7);
  const int pg_stride = gridDim.x / NCP;
  Ring<T::RS> ring;
  ring_init(ring, smem, (const char*)a.wstream + (size_t)cp * (a.nms_total / NCP) * T::RS, a.nms_total / NCP, kRingOff);
  lds_barrier();
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lg = wid / T::CG;
  const int lr = lane & 31;

  const int NIP = CIN / CB;
  XRegs<G> xr;
  stage_load<G>(xr, a.in, CIN, pg0 * NPOS, a.npos, 0);
  int pending_stores = 0;
  for (int pos0 = pg0 * NPOS; pos0 < a.npos; pos0 += pg_stride * NPOS) {
    f32x16 acc[2][T::NT];
    acc_zero<G, CP>(acc);
#pragma unroll 1
    for (int ip = 0; ip < NIP; ++ip) {
      if (PRE) stage_math<G>(xr, ip * G::NCH, a.scale, a.shift);
      lds_barrier();
      stage_store<G, false>(smem, xr, ip * G::NCH, nullptr, nullptr);
      int nip = ip + 1, npos0 = pos0;
      if (nip == NIP) {
        nip = 0;
        npos0 = pos0 + pg_stride * NPOS;   // past the end: clamped to a valid position
      }
      stage_load<G>(xr, a.in, CIN, npos0, a.npos, nip * G::NCH);
      ring_note_inflight(ring, pending_stores + kXLoads);
      pending_stores = 0;
      conv_segment<G, CP, 1, 1>(ring, smem, acc);
    }
    static_assert(EPI == 2 || T::NT == 3, "vmcnt bookkeeping: 12 sixteen-byte stores per pass");
    pending_stores = (EPI == 2) ? 0 : 12;
    if (EPI == 1) {
      epilogue_to_global<G, CP, true>(acc, a.out16, COUT, pos0, a.npos, cp * CP);
    } else if (EPI == 0) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int j = 0; j < T::NT; ++j)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[mt][j][i] = mish_f(acc[mt][j][i]);
      epilogue_to_global<G, CP, false>(acc, a.out16, COUT, pos0, a.npos, cp * CP);
    } else {
      const int h = lane >> 5;
#pragma unroll
      for (int j = 0; j < T::NT; ++j) {
        const int t = lg + j * T::LG;
        if (t >= G::NT_TOTAL) continue;
        const int p = t / G::NT_POS, tt = t - p * G::NT_POS;
        const int loc = tt * 32 + lr;  // S == 19: row == loc
        if (loc >= kNLoc || pos0 + p >= a.npos) continue;
        // hp[pos][c / 4][loc][4] fp32, one 16-byte store per accumulator quad (cout a multiple of 4)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const int wid_cg = wid % T::CG;
            const int c0 = cp * CP + wid_cg * 64 + mt * 32 + 8 * g4 + 4 * h;   // first channel of the quad
            if (c0 < COUT)
              *(f32x4*)(a.out32 + (((size_t)(pos0 + p) * (COUT / 4) + (c0 >> 2)) * kNLoc + loc) * 4) =
                  f32x4{acc[mt][j][4 * g4], acc[mt][j][4 * g4 + 1], acc[mt][j][4 * g4 + 2], acc[mt][j][4 * g4 + 3]};
          }
      }
    }
  }
  lds_barrier();
  ring_drain();
}

// =======================================================================================
// Layer conv (k_lconv of kernels.hip in its shipped 4-wave form): one position per 256-thread workgroup, two
// workgroups per CU taking turns at the higher wave priority; `nip` 64-channel K slices with the fp32 accumulators
// in registers across them, `ncp` 64-channel output passes split across the workgroups of one XCD.
//   pre / act / res / dual: LConvArgs
// =======================================================================================
template <int KW, bool PRE, bool ACT, bool RES, bool DUAL>
__global__ void __launch_bounds__(256, 2) k_lconv_any(LConvAnyArgs aa) {
  static_assert(!(ACT && DUAL), "act stores the activated tensor only, dual stores both");
  const LConvArgs& a = aa.a;
  constexpr int NW = 4, CB = 64, NPOS = 1, CP = 64;
  using G = Geo<NPOS, CB, KW, NW, KW == 3 ? 2 : kKMS>;
  using T = Tiling<G, CP>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  act_zero<G>(smem);
  const int NIP = aa.nip, NCP = aa.ncp;
  const int CIN = NIP * CB, COUT = NCP * CP;
  const int cp = (blockIdx.x >> 3) % NCP;
  const int pg0 = (blockIdx.x / (8 * NCP)) * 8 + (blockIdx.x & 7);
  const int pg_stride = gridDim.x / NCP;
  Ring<T::RS, G::NW, G::RD> ring;
  ring_init(ring, smem, (const char*)a.wstream + (size_t)cp * (a.nms_total / NCP) * T::RS, a.nms_total / NCP, G::ACT_BYTES);
  lds_barrier();
  XRegs<G> xr;   // software-pipelined staging
  stage_load<G>(xr, a.in, CIN, pg0 * NPOS, a.npos, 0);
  int pending_stores = 0;
  int turn = 0;
  for (int pos0 = pg0 * NPOS; pos0 < a.npos; pos0 += pg_stride * NPOS, ++turn) {
    if (a.pair_split > 0) {
      if (((int)blockIdx.x >= a.pair_split) != (bool)(turn & 1)) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    f32x16 acc[2][T::NT];
    acc_zero<G, CP>(acc);
#pragma unroll 1
    for (int ip = 0; ip < NIP; ++ip) {
      if (PRE) stage_math<G>(xr, ip * G::NCH, a.scale_in, a.shift_in);
      lds_barrier();
      stage_store<G, false>(smem, xr, ip * G::NCH, nullptr, nullptr);
      int nip = ip + 1, npos0 = pos0;
      if (nip == NIP) {
        nip = 0;
        npos0 = pos0 + pg_stride * NPOS;
      }
      stage_load<G>(xr, a.in, CIN, npos0, a.npos, nip * G::NCH);
      ring_note_inflight(ring, pending_stores + kXLoads);
      pending_stores = 0;
      conv_segment<G, CP, KW, KW * KW>(ring, smem, acc);
    }
    // BN + mish of the output in place, one channel quad of parameters at a time
    auto activate = [&]() {
      const int c0 = cp * CP + cg_of<G, CP>() * 64 + (launder(threadIdx.x & 63) >> 5) * 4;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const f32x4 sc = *(const f32x4*)(a.scale_out + c0 + 8 * k), sh = *(const f32x4*)(a.shift_out + c0 + 8 * k);
#pragma unroll
        for (int j = 0; j < T::NT; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            acc[k >> 2][j][(k & 3) * 4 + i] = mish_f(acc[k >> 2][j][(k & 3) * 4 + i] * sc[i] + sh[i]);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    static_assert(T::NT == 3, "vmcnt bookkeeping: 12 sixteen-byte stores per output");
    if (DUAL) {
      ResRegs<G, CP, T::NT> rr;
      residual_addr<G, CP, T::NT>(rr, COUT, pos0, a.npos, cp * CP);
      if (RES) {
        residual_load<G, CP, T::NT>(rr, a.out);
        residual_add<G, CP, T::NT>(acc, rr);
      }
      epilogue_store<G, CP, false, T::NT>(acc, rr, a.out);    // raw y
      activate();
      epilogue_store<G, CP, false, T::NT>(acc, rr, a.out2);   // the consumer's input, activated once here
      pending_stores = 24;
    } else {
      pending_stores = 12;
      if (ACT) activate();
      epilogue_to_global<G, CP, RES>(acc, a.out, COUT, pos0, a.npos, cp * CP);
    }
  }
  lds_barrier();
  ring_drain();
}

// =======================================================================================
// Broadcast dense (k_bdense of kernels.hip): u[c][j] = mish(bn1(sum_i t[c][i] W[i][j] + b[j])), 128 channels per
// pass transposed into LDS, three passes of 128 dense columns through the ring.  C a launch argument.
// =======================================================================================
namespace {
constexpr int kTtStride = 784;  // bytes per channel row in LDS: 384 fp16 + 16 B pad
constexpr int kTtChannels = 128;
constexpr uint32_t kTtBytes = kTtChannels * kTtStride;
struct GeoTt {
  static constexpr int NW = 8, KMS = kKMS, RD = kRingDepth;
  static constexpr int NPOS = 1, CB = 384, NCH = 48, SLOTB = kTtStride, PAD = 0, S = 1, NROWS = 128,
                       NT_POS = 4, PADTOP = 0, PSLOTS = 128, ACT_BYTES = 128 * kTtStride, NT_TOTAL = 4;
};
// LDS of k_bdense_any: Tt, the ring, the dense bias [384] and the folded bn1 [2][kConvAnyMaxC]; one workgroup per CU
constexpr size_t kBDenseAnyLds = kTtBytes + ring_bytes(128) + (384 + 2 * kConvAnyMaxC) * 4;
static_assert(kBDenseAnyLds <= 160 * 1024, "k_bdense_any: LDS of one CU");
}  // namespace

__global__ void __launch_bounds__(kWG, 2) k_bdense_any(BDenseAnyArgs aa) {
  const BDenseArgs& a = aa.a;
  const int C = aa.C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int CH = kTtChannels;
  constexpr uint32_t kRingOff = kTtBytes;
  for (int i = threadIdx.x * 16; i < (int)kTtBytes; i += kWG * 16) *(f32x4*)(smem + i) = f32x4{0, 0, 0, 0};
  Ring<16384> ring;
  ring_init(ring, smem, a.wstream, a.nms_total, kRingOff);
  float* p_bias = (float*)(smem + kRingOff + ring_bytes(128));
  float* p_scale = p_bias + 384;
  float* p_shift = p_scale + C;
  for (int i = threadIdx.x; i < 384; i += kWG) p_bias[i] = i < kNLoc ? a.bias[i] : 0.0f;
  for (int i = threadIdx.x; i < C; i += kWG) { p_scale[i] = a.scale[i]; p_shift[i] = a.shift[i]; }
  lds_barrier();

  using GS = Geo<1, 128, 1>;
  const int NHALF = (C + CH - 1) / CH;
  XRegs<GS> xr;
  auto pair_load = [&](int pos_, int cblk) {
    static_assert(kXLoads == 12, "six pairs");
    int pp = pos_ < a.npos ? pos_ : a.npos - 1;
    const _Float16* src = a.t + ((size_t)pp * (C / 8) + cblk + (threadIdx.x >> 5)) * (kNLoc * 8);
    const int l32 = threadIdx.x & 31;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      int l0 = 2 * (l32 + 32 * i), l1 = l0 + 1;
      if (l0 >= kNLoc) l0 = kNLoc - 1;   // tail lanes re-read a valid item (not stored)
      if (l1 >= kNLoc) l1 = kNLoc - 1;
      xr.v[2 * i] = *(const h8*)(src + l0 * 8);
      xr.v[2 * i + 1] = *(const h8*)(src + l1 * 8);
    }
  };
  // channel blocks past C (last pass of a C that is not a multiple of 128) are clamped to the pass's first block
  auto pass_cblk = [&](int half) {
    return half * (CH / 8) + ((int)(threadIdx.x >> 5) * 8 < C - half * CH ? 0 : -(int)(threadIdx.x >> 5));
  };
  pair_load(blockIdx.x, pass_cblk(0));
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int jg = wid & 1;        // which 64 of the 128 j rows in this pass
  const int ct = wid >> 1;       // channel tile (32 channels) 0..3
  const int lr = lane & 31, h = lane >> 5;
  for (int pos = blockIdx.x; pos < a.npos; pos += gridDim.x) {
#pragma unroll 1
    for (int half = 0; half < NHALF; ++half) {
      const int nch = (C - half * CH) < CH ? (C - half * CH) : CH;
      lds_barrier();
      {
        const int combo = threadIdx.x >> 5, l32 = threadIdx.x & 31;   // combo = channel block of this pass
        if (combo * 8 < nch) {
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            const int loc = 2 * (l32 + 32 * i);
            if (loc >= kNLoc) continue;
            const h8 v0 = xr.v[2 * i];
            h8 v1 = xr.v[2 * i + 1];
            if (loc + 1 >= kNLoc) v1 = h8{0, 0, 0, 0, 0, 0, 0, 0};   // board point 361 is padding (K = 384)
#pragma unroll
            for (int e = 0; e < 8; ++e) *(h2*)(smem + (combo * 8 + e) * kTtStride + loc * 2) = h2{v0[e], v1[e]};
          }
        }
      }
      {
        int nhalf = half + 1, npos = pos;
        if (nhalf == NHALF) { nhalf = 0; npos = pos + gridDim.x; }
        pair_load(npos, pass_cblk(nhalf));
        ring_note_xloads(ring);
      }
      const bool ct_active = ct * 32 < nch;
#pragma unroll 1
      for (int jp = 0; jp < 3; ++jp) {
        f32x16 acc2[2][1];
        acc_zero<GeoTt, 128>(acc2);
        conv_segment<GeoTt, 128, 1, 1, true>(ring, smem, acc2);
        if (!ct_active) continue;
        const f32x16 acc[2] = {acc2[0][0], acc2[1][0]};
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const int j = jp * 128 + jg * 64 + mt * 32 + lr;
          if (j >= kNLoc) continue;
          const float bj = p_bias[j];
#pragma unroll
          for (int gp = 0; gp < 2; ++gp) {
            h4 o[2];
            {
              const int g4 = 2 * gp;
              const int c = half * CH + ct * 32 + g4 * 8 + h * 4;
              const f32x4 sc0 = scale_log2e(*(const f32x4*)(p_scale + c)), sh0 = scale_log2e(*(const f32x4*)(p_shift + c));
              const f32x4 sc1 = scale_log2e(*(const f32x4*)(p_scale + c + 8)), sh1 = scale_log2e(*(const f32x4*)(p_shift + c + 8));
              const f32x4 v0 = {acc[mt][g4 * 4] + bj, acc[mt][g4 * 4 + 1] + bj, acc[mt][g4 * 4 + 2] + bj, acc[mt][g4 * 4 + 3] + bj};
              const f32x4 v1 = {acc[mt][g4 * 4 + 4] + bj, acc[mt][g4 * 4 + 5] + bj, acc[mt][g4 * 4 + 6] + bj, acc[mt][g4 * 4 + 7] + bj};
              bn_mish8_l2(v0, v1, sc0, sh0, sc1, sh1, o[0], o[1]);
            }
            half_swap32(o[0], o[1]);
            const h8 piece = {o[0][0], o[0][1], o[0][2], o[0][3], o[1][0], o[1][1], o[1][2], o[1][3]};
            const int cb = (half * CH + ct * 32) / 8 + 2 * gp + h;   // this lane's channel block
            *(h8*)(a.u + ((size_t)pos * (C / 8) + cb) * (kNLoc * 8) + j * 8) = piece;
          }
        }
      }
    }
  }
  lds_barrier();
  ring_drain();
}

// =======================================================================================
// Host-side launchers
// =======================================================================================
namespace {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device), as in kernels.hip
struct AttrOnce { std::atomic<bool> done[32]; };
template <class K>
hipError_t ensure_lds(AttrOnce& once, K kernel, size_t lds) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32)
    return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (once.done[dev].load(std::memory_order_acquire)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) once.done[dev].store(true, std::memory_order_release);
  return e;
}

// a multiple of 8 * ncp, at most n_cu, enough for every (position group, pass) pair
int conv_split_grid(int npos, int npos_per_wg, int ncp, int n_cu) {
  const int unit = 8 * ncp;
  const int groups = (npos + npos_per_wg - 1) / npos_per_wg;
  int want = ((groups + 7) / 8) * unit;
  int cap = (n_cu / unit) * unit;
  if (cap < unit) cap = unit;
  return want < cap ? want : cap;
}

bool width_ok(int c) { return c >= 64 && c <= kConvAnyMaxC && c % 64 == 0; }

template <int CP>
hipError_t launch_init_cp(const InitAnyArgs& a, int grid, hipStream_t s) {
  using G = Geo<1, 16, 5>;
  constexpr size_t lds = G::ACT_BYTES + ring_bytes(CP) + kConvAnyMaxC * 4;   // + the game-state bias vector
  static_assert(2 * lds <= 160 * 1024, "k_init_any: two workgroups per CU");
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_init_any<CP>, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((k_init_any<CP>), dim3(grid), dim3(kWG), lds, s, a);
  return hipGetLastError();
}

template <int CB, int CP, bool PRE, int EPI>
hipError_t launch_conv1x1_t(const Conv1x1AnyArgs& a, int n_cu, hipStream_t s) {
  using G = Geo<128 / CB, CB, 1>;
  const int grid = conv_split_grid(a.a.npos, 128 / CB, (a.cout + CP - 1) / CP, n_cu);
  constexpr size_t lds = G::ACT_BYTES + ring_bytes(CP);
  static_assert(lds <= 160 * 1024, "k_conv1x1_any: LDS of one CU");
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_conv1x1_any<CB, CP, PRE, EPI>, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((k_conv1x1_any<CB, CP, PRE, EPI>), dim3(grid), dim3(kWG), lds, s, a);
  return hipGetLastError();
}

template <int KW, bool PRE, bool ACT, bool RES, bool DUAL>
hipError_t launch_lconv_t(const LConvArgs& a, int cin, int cout, int n_cu, hipStream_t s) {
  using G = Geo<1, 64, KW, 4, KW == 3 ? 2 : kKMS>;
  const int grid = conv_split_grid(a.npos, 1, cout / 64, 2 * n_cu);   // two workgroups per CU
  constexpr size_t lds = G::ACT_BYTES + ring_bytes(64, G::KMS);
  static_assert(2 * lds <= 160 * 1024, "k_lconv_any: two workgroups per CU");
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_lconv_any<KW, PRE, ACT, RES, DUAL>, lds); e != hipSuccess) return e;
  LConvAnyArgs b{a, cin / 64, cout / 64};
  b.a.nms_total = a.nms_total * (kKMS / G::KMS);   // the host counts macro-steps of kKMS k16-steps
  static const bool turns = getenv("P3HIP_NO_PAIR_TURNS") == nullptr;
  b.a.pair_split = (turns && grid > n_cu) ? n_cu : 0;
  hipLaunchKernelGGL((k_lconv_any<KW, PRE, ACT, RES, DUAL>), dim3(grid), dim3(256), lds, s, b);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_init_any(int C, const InitArgs& a, int grid, hipStream_t s) {
  if (!width_ok(C)) return hipErrorInvalidValue;
  const InitAnyArgs b{a, C};
  return conv_any_init_pass(C) == 128 ? launch_init_cp<128>(b, grid, s) : launch_init_cp<64>(b, grid, s);
}

hipError_t launch_conv1x1_any(int C, int which, const Conv1x1Args& a, int n_cu, hipStream_t s) {
  if (!width_ok(C) || which < 0 || which > 2) return hipErrorInvalidValue;
  const Conv1x1AnyArgs b{a, C, which == 2 ? 96 : C};
  if (conv_any_slice(C) == 128) {
    if (which == 0) return launch_conv1x1_t<128, 128, true, 0>(b, n_cu, s);
    if (which == 1) return launch_conv1x1_t<128, 128, false, 1>(b, n_cu, s);
    return launch_conv1x1_t<128, 64, false, 2>(b, n_cu, s);
  }
  if (which == 0) return launch_conv1x1_t<64, 64, true, 0>(b, n_cu, s);
  if (which == 1) return launch_conv1x1_t<64, 64, false, 1>(b, n_cu, s);
  return launch_conv1x1_t<64, 64, false, 2>(b, n_cu, s);
}

// the flag sets of the layer-wise plan (engine.cpp build_plan); f = pre, act, res, dual
hipError_t launch_lconv_any(int kw, int cin, int cout, const LConvArgs& a, int n_cu, hipStream_t s) {
  if (!width_ok(cin) || !width_ok(cout)) return hipErrorInvalidValue;
  const int f = (a.pre ? 8 : 0) | (a.act ? 4 : 0) | (a.res ? 2 : 0) | (a.dual ? 1 : 0);
#define P3_LCONV_ANY(KW, PRE, ACT, RES, DUAL) \
  if (kw == KW && f == ((PRE ? 8 : 0) | (ACT ? 4 : 0) | (RES ? 2 : 0) | (DUAL ? 1 : 0))) \
    return launch_lconv_t<KW, PRE, ACT, RES, DUAL>(a, cin, cout, n_cu, s);
  P3_LCONV_ANY(1, true, true, false, false)     // btl reduce from the raw stream
  P3_LCONV_ANY(1, false, true, false, false)    // btl reduce from the activated copy
  P3_LCONV_ANY(1, true, false, false, true)     // nbt reduce (t raw + act1(t))
  P3_LCONV_ANY(1, false, false, false, true)
  P3_LCONV_ANY(3, false, true, false, false)    // inner conv, activated output
  P3_LCONV_ANY(3, true, true, false, false)     // classic conv0 from the raw stream
  P3_LCONV_ANY(3, false, false, true, false)    // classic conv1 (+x), last block
  P3_LCONV_ANY(3, false, false, true, true)     // nbt conv2 / conv4, classic conv1 (+x, + next act)
  P3_LCONV_ANY(1, false, false, true, false)    // expand + x
  P3_LCONV_ANY(1, false, false, true, true)     // expand + x, + the next block's activated input
#undef P3_LCONV_ANY
  return hipErrorInvalidValue;
}

const char* lconv_any_kernel_name(int kw) { return kw == 3 ? "k_lconv_any<3>" : "k_lconv_any<1>"; }

hipError_t launch_bdense_any(int C, const BDenseArgs& a, int grid, hipStream_t s) {
  if (!width_ok(C)) return hipErrorInvalidValue;
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_bdense_any, kBDenseAnyLds); e != hipSuccess) return e;
  const BDenseAnyArgs b{a, C};
  hipLaunchKernelGGL(k_bdense_any, dim3(grid), dim3(kWG), kBDenseAnyLds, s, b);
  return hipGetLastError();
}

}  // namespace p3
