// layer_kernels.h — the bodies of the layer-wise conv kernels, written once for fixed and runtime widths.
//
// k_init, k_conv1x1, k_lconv and k_bdense (kernels.hip: channel counts are template arguments) and k_init_any,
// k_conv1x1_any, k_lconv_any and k_bdense_any (conv_any.hip: channel counts are launch arguments) are entry points of
// a few lines over the bodies below.  A body takes each width as a policy object, FixedW<N> or RuntimeW: with FixedW
// the loop counts, pass counts and layout strides fold to the constants the templated kernels always had, with
// RuntimeW they are registers.  What changes the instruction stream stays a template argument of the body (kernel
// size, prologue / epilogue flags, slice and pass width, waves per workgroup).  Both forms run the same slices in the
// same order, so their results are equal bit for bit (tests/test_conv_widths_gpu.py compares).  Where the two forms
// differ on purpose the body says so under `if constexpr (W::fixed)`.
//
// Four passages of init_body, bdense_body and bdense_passes are also the split kernels' (edge_split.hip: one output pass
// per workgroup) and are written once as text that both include in place: stem_planes.inc, stem_epilogue.inc,
// bdense_transpose.inc, bdense_epilogue.inc; each names at its head what must be in scope.  Text, not functions, so that
// the bodies reach the compiler token for token as before; bdense_passes is inlined into k_block's
// fused tail, whose register allocation tests/test_kernel_resources_cpu.py guards.
//
// Layouts, ring and tiling: conv_core.h.  Activation offsets are 64-bit per position (stage_load, residual_addr), the
// 32-bit lane offsets stay inside one workgroup's positions.
#pragma once
#include "conv_core.h"
#include "kernels.h"

namespace p3 {

// a channel count (or a count of 64-channel slices) known at compile time / passed with the launch
template <int N>
struct FixedW {
  static constexpr bool fixed = true;
  __host__ __device__ static constexpr int get() { return N; }
};
struct RuntimeW {
  static constexpr bool fixed = false;
  int n;
  __host__ __device__ int get() const { return n; }
};

struct FeatOff {  // byte offsets inside p3hip_features (include/p3hip.h)
  static constexpr int color = 4, komi = 8, board = 12, last = 376, atari = 416, two = 777,
                       three = 1138, ladder = 1499, size = 1860;
};

// ---- broadcast dense, shared by k_bdense, k_bdense_any and the fused tail of k_block ------------------
constexpr int kTtStride = 784;  // bytes per channel row in LDS: 384 fp16 + 16 B pad
constexpr int kTtChannels = 128;                          // channels resident per pass
constexpr uint32_t kTtBytes = kTtChannels * kTtStride;    // 100,352

// Tt seen as a conv act buffer: one slot per channel (128 per pass), K = 384 board points.
struct GeoTt {
  static constexpr int NW = 8, KMS = kKMS, RD = kRingDepth;
  static constexpr int NPOS = 1, CB = 384, NCH = 48, SLOTB = kTtStride, PAD = 0, S = 1, NROWS = 128,
                       NT_POS = 4, PADTOP = 0, PSLOTS = 128, ACT_BYTES = 128 * kTtStride, NT_TOTAL = 4;
};

// u[c][j] = mish(bn1(sum_i Tt[c][i] W[i][j] + b[j])) for the 128 channels in Tt (channel half `half` of position
// `pos`), three passes of 128 dense columns j streamed through the ring, -> HBM in the piece layout.
// p_bias [384], p_scale / p_shift [C]: LDS.  nch = channels of this pass that are real.
template <class W>
__device__ __forceinline__ void bdense_passes(W wc, Ring<16384>& ring, char* smem, const float* p_bias, const float* p_scale,
                                              const float* p_shift, _Float16* __restrict__ u, int pos, int half, int nch) {
  const int C = wc.get();
  constexpr int CH = kTtChannels;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int jg = wid & 1;        // which 64 of the 128 j rows in this pass
  const int ct = wid >> 1;       // channel tile (32 channels) 0..3
  const int lr = lane & 31, h = lane >> 5;
  const bool ct_active = ct * 32 < nch;
#pragma unroll 1
  for (int jp = 0; jp < 3; ++jp) {
    // D[c][j] = sum_i Tt[c][i] * W[i][j]: the conv K loop with its operands swapped —
    // "act buffer" = Tt (slot = channel, 48 chunks of 8 board points), "weights" = the
    // 128 dense columns of this pass streamed through the ring; fragments are prefetched
    // two k16 steps ahead exactly as in the conv kernels.
    f32x16 acc2[2][1];
    acc_zero<GeoTt, 128>(acc2);
    conv_segment<GeoTt, 128, 1, 1, true>(ring, smem, acc2);
    if (!ct_active) continue;
    // epilogue: rows = channel (regs), cols = j (lanes)
#include "bdense_epilogue.inc"
  }
}

// dense bias per board point and folded bn1 per channel into LDS at `dst` ([384] + [C] + [C] floats)
template <class W>
__device__ __forceinline__ void bdense_stage_params(W wc, float* dst, const float* __restrict__ bias,
                                                    const float* __restrict__ scale, const float* __restrict__ shift) {
  const int C = wc.get();
  for (int i = threadIdx.x; i < 384; i += kWG) dst[i] = i < kNLoc ? bias[i] : 0.0f;
  for (int i = threadIdx.x; i < C; i += kWG) { dst[384 + i] = scale[i]; dst[384 + C + i] = shift[i]; }
}

// =======================================================================================
// Initial 5x5 conv over the 15 binary input planes + game-state dense, model.py:1230-1237.
// Input planes are expanded on the fly from the packed GoFeatures bytes (restating
// LoadPlanes/LoadFeatures, cc/nn/engine/go_features.cc:10-61): nothing but the 1.9 KB POD
// crosses PCIe.  Channel 15 is a zero pad.  CP: channels per output pass, C a multiple of it.
// =======================================================================================
template <int CP, class W>
__device__ __forceinline__ void init_body(InitArgs a, W wc) {
  const int C = wc.get();
  using G = Geo<1, 16, 5>;
  if constexpr (W::fixed) static_assert(W::get() % CP == 0, "output passes");
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
    // ---- feature planes -> LDS, game-state scalars -> gsv[8] ----------------------------
#include "stem_planes.inc"

    // game-state dense once per position: thread c computes (gs . Wg + b)[c] into LDS (the
    // area behind the weight ring, one float per channel: C <= kWG); the first ring acquire of
    // the K loop below is the barrier that publishes it.  (Each lane used to fetch its 32
    // channels' 8 x 4 weights from L2 in the epilogue of every output pass.)
    float* bias_lds = (float*)(smem + kRingOff + ring_bytes(CP));
    int tc = threadIdx.x;
    // (laundered: with C a runtime value the eight weight addresses would be hoisted out of the position loop and spilled)
    if constexpr (!W::fixed) tc = launder(tc);
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
      // epilogue: + (gs . Wg + b)[c]  -> x
      const int bias_cp = cp;
#include "stem_epilogue.inc"
    }
    lds_barrier();
    // clear the 5 last-move/stone planes for the next position: every valid slot is
    // rewritten in full by the staging loop above, so nothing to do.
  }
  ring_drain();
}

// =======================================================================================
// Generic 1x1 conv kernel over the channel-blocked stream: CB-channel K slices, CP-channel output
// passes; cin a multiple of CB, cout <= NCP * CP.
//   PRE  : apply mish(bn(.)) while staging (ConvPreActivation prologue)
//   EPI 0: out = mish(acc)               -> y (fp16)   [broadcast conv_first + BroadcastPreAct act,
//                                                       model.py:556-560,590-596]
//   EPI 1: x  += acc                      (residual)   [broadcast conv_last, model.py:600-606]
//   EPI 2: hp  = acc (fp32 [pos][COUT][361])            [policy conv_p/conv_g, value conv;
//                                                       model.py:783-786,889]
// =======================================================================================
template <int CB, int CP, bool PRE, int EPI, class WI, class WO>
__device__ __forceinline__ void conv1x1_body(Conv1x1Args a, WI wi, WO wo) {
  const int CIN = wi.get(), COUT = wo.get();
  constexpr int NPOS = 128 / CB;
  using G = Geo<NPOS, CB, 1>;
  using T = Tiling<G, CP>;
  const int NCP = (COUT + CP - 1) / CP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr uint32_t kRingOff = G::ACT_BYTES;
  act_zero<G>(smem);
  // Output passes are split ACROSS workgroups: workgroup b owns pass cp = (b / 8) % NCP of the
  // position groups pg0, pg0 + gridDim/NCP, ...  The NCP workgroups of one position group are
  // 8 block ids apart, i.e. on the same XCD and dispatched together, so the input slices they
  // all stage come from HBM once and from that XCD's L2 afterwards (each workgroup restaging
  // every pass itself re-read them from HBM: the working set of an XCD's 32 workgroups is
  // larger than its L2).  gridDim.x is a multiple of 8 * NCP (conv_split_grid).
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

  // Staging is software-pipelined: the slice after the current one (next K slice or next
  // position) is fetched into registers while the current segment's MFMAs run, its BN+mish
  // is applied in registers before the barrier that frees the act buffer.
  const int NIP = CIN / CB;
  XRegs<G> xr;
  stage_load<G>(xr, a.in, CIN, pg0 * NPOS, a.npos, 0);
  int pending_stores = 0;   // vector-memory ops of the previous epilogue that may still be in flight
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
        // head activations go out as the accumulator quads they are: hp[pos][c / 4][loc][4] fp32, one 16-byte
        // store per quad (a wave instruction covers two contiguous 512-byte runs); k_heads reads quads
        // (cout a multiple of 4: the runtime form's only cout here is 96)
        if constexpr (WO::fixed) static_assert(WO::get() % 4 == 0, "channel quads");
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
// Layer-wise conv kernel for trunks whose bottleneck does not fit the fused block kernel's
// LDS plan (C = 384, C_b = 192: one position of 192 channels on the padded grid is 168 KB).
// Each conv of a block is its own launch; activations round-trip HBM in fp16.  Input channels
// are staged in `wi` 64-channel slices (K split, accumulators stay in registers across slices),
// outputs are produced in `wo` 64-channel passes split across the workgroups of one XCD.
//   pre : stage mish(bn_in(.))          (ConvPreActivation prologue, model.py:203-292)
//   act : store mish(bn_out(acc))       (the NEXT layer's prologue applied by the producer,
//                                        so inner layers stage without VALU work)
//   res : out += acc                    (residual, in place)
//   dual: store the raw and the activated tensor
// =======================================================================================
// NW = 4 (the shipped form; NW = 8 = two positions per 512-thread workgroup, one per CU, P3HIP_LCONV_WG8): a
// 256-thread workgroup per position — 1x1: 52 KB of activations + 24 KB of ring, 3x3: 60.6 KB + 12 KB (K = 32 ring
// steps) — so that TWO workgroups share a CU and one's loads, stores and BN + mish run under the other's K loop;
// they take turns at the higher wave priority, one position group each (see BlockArgs::pair_turns).
//   Q   : how the activated tensor (act, or dual's second output) is stored.  FpOut: as fp16, the fp16 plans.  A policy
//         with `on` set (lconv_conv3.hip Q8Out, P3HIP_FLAG_INT8_CONV3) stores it quantized, from the fp32 values, in
//         the int8 layout the INT8 3x3 conv reads; dual's raw output stays fp16
struct FpOut { static constexpr bool on = false; };
template <int KW, bool PRE, bool ACT, bool RES, bool DUAL, int NW, class Q = FpOut, class WI, class WO>
__device__ __forceinline__ void lconv_body(LConvArgs a, WI wi, WO wo, Q q = Q{}) {
  static_assert(!(ACT && DUAL), "act stores the activated tensor only, dual stores both");
  static_assert(!Q::on || (NW == 4 && (ACT || DUAL) && !(ACT && RES)), "a quantized output is an activated one");
  constexpr int CB = 64, NPOS = NW == 8 ? 2 : 1, CP = 64;
  // 3x3 layers in the 4-wave form: K = 32 ring steps (60.6 KB of activations + 12 KB of ring), as in k_block
  using G = Geo<NPOS, CB, KW, NW, (NW == 4 && KW == 3) ? 2 : kKMS>;
  using T = Tiling<G, CP>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  act_zero<G>(smem);
  const int NIP = wi.get(), NCP = wo.get();
  const int CIN = NIP * CB, COUT = NCP * CP;
  // output passes split across workgroups, as in conv1x1_body
  const int cp = (blockIdx.x >> 3) % NCP;
  const int pg0 = (blockIdx.x / (8 * NCP)) * 8 + (blockIdx.x & 7);
  const int pg_stride = gridDim.x / NCP;
  Ring<T::RS, G::NW, G::RD> ring;
  ring_init(ring, smem, (const char*)a.wstream + (size_t)cp * (a.nms_total / NCP) * T::RS, a.nms_total / NCP, G::ACT_BYTES);
  lds_barrier();
  XRegs<G> xr;   // software-pipelined staging, as in conv1x1_body
  stage_load<G>(xr, a.in, CIN, pg0 * NPOS, a.npos, 0);
  int pending_stores = 0;
  int turn = 0;
  for (int pos0 = pg0 * NPOS; pos0 < a.npos; pos0 += pg_stride * NPOS, ++turn) {
    if (NW == 4 && a.pair_split > 0) {
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
    // BN + mish of the output in place; parameters are fetched one channel quad at a time so
    // the prefetched slice stays in registers
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
      if constexpr (Q::on) {
        q.template store<G, CP, T::NT>(acc, a.out2, COUT, pos0, cp * CP);   // 24 four-byte stores
        pending_stores = 36;
      } else {
        epilogue_store<G, CP, false, T::NT>(acc, rr, a.out2);   // the consumer's input, activated once here
        pending_stores = 24;
      }
    } else if constexpr (Q::on) {
      activate();
      q.template store<G, CP, T::NT>(acc, a.out, COUT, pos0, cp * CP);
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
// Broadcast dense: per channel c, u[c][j] = sum_i t[c][i] W[i][j] + b[j]  (Dense(361) over
// the flattened board, weights shared by all channels; BroadcastPreAct.call, model.py:
// 556-567; `t` already carries the mish).  Then the following ConvPreActivation prologue
// mish(bn1(u)) is applied here so that conv_last runs with PRE = false.
//   MFMA orientation: D[c][j] = sum_i Tt[c][i] * Wt[j][i]  (A = activations transposed in
//   LDS to [c][i], B = dense matrix rows streamed through the ring).
// =======================================================================================
template <class W>
__device__ __forceinline__ void bdense_body(BDenseArgs a, W wc) {
  const int C = wc.get();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int CH = kTtChannels;
  constexpr uint32_t kRingOff = kTtBytes;
  for (int i = threadIdx.x * 16; i < (int)kTtBytes; i += kWG * 16) *(f32x4*)(smem + i) = f32x4{0, 0, 0, 0};
  Ring<16384> ring;
  ring_init(ring, smem, a.wstream, a.nms_total, kRingOff);
  // epilogue parameters (dense bias per board point, folded BN per channel) live in LDS behind
  // the ring: fetched once per workgroup instead of from L2 after every K loop
  float* p_bias = (float*)(smem + kRingOff + ring_bytes(128));
  float* p_scale = p_bias + 384;
  float* p_shift = p_scale + C;
  bdense_stage_params(wc, p_bias, a.bias, a.scale, a.shift);
  lds_barrier();

  // Staging is software-pipelined like the conv kernels': the 12 16-byte loads of the next
  // 128-channel pass (next half or next position) are issued before the current pass's K loop
  // and scattered (transposed) into LDS after the barrier that ends it.
  // Thread (combo = channel block of the pass, l32) owns the six PAIRS of adjacent board points
  // 2*(l32 + 32*i), +1: two adjacent 16-byte loads per pair (still kXLoads = 12 per thread, the
  // ring's vmcnt bookkeeping is unchanged) and one ds_write_b32 per channel and pair when the
  // slice is transposed into Tt[c][i] — half the LDS store instructions of a per-point scatter.
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
  // channel blocks past C (last pass of a C that is not a multiple of 128, or the only pass of C = 64) are clamped to
  // the pass's first block and ignored
  auto pass_cblk = [&](int half) {
    return half * (CH / 8) + ((int)(threadIdx.x >> 5) * 8 < C - half * CH ? 0 : -(int)(threadIdx.x >> 5));
  };
  // (a fixed C is at least one whole pass, so every channel block of the first pass exists and pass_cblk(0) is 0; the
  // compiler does not fold it, and computing it made b15c192_classic's forward pass 0.15 % slower)
  if constexpr (W::fixed) static_assert(W::get() >= CH, "the first pass is whole");
  pair_load(blockIdx.x, W::fixed ? 0 : pass_cblk(0));
  for (int pos = blockIdx.x; pos < a.npos; pos += gridDim.x) {
#pragma unroll 1
    for (int half = 0; half < NHALF; ++half) {
      // channels of this pass (the last pass of C = 192 has 64: its upper channel tiles idle
      // but still take part in the ring's barriers)
      const int nch = (C - half * CH) < CH ? (C - half * CH) : CH;
      lds_barrier();
      // ---- transpose-stage t[pos][cblk][loc][8] -> Tt[c][i] --------------------------
      {
        const int combo = threadIdx.x >> 5, l32 = threadIdx.x & 31;   // combo = channel block of this pass
        if (combo * 8 < nch) {
#include "bdense_transpose.inc"
        }
      }
      {
        int nhalf = half + 1, npos = pos;
        if (nhalf == NHALF) { nhalf = 0; npos = pos + gridDim.x; }
        pair_load(npos, pass_cblk(nhalf));
        ring_note_xloads(ring);
      }
      bdense_passes(wc, ring, smem, p_bias, p_scale, p_shift, a.u, pos, half, nch);
    }
  }
  lds_barrier();
  ring_drain();
}

}  // namespace p3
