// engine.cpp — the p3hip C ABI (include/p3hip.h): weight loading / repacking, pinned
// staging, slot compaction, launch sequence.  Compiled with hipcc into libp3hip.so.
//
// Replaces TrtEngineImpl (cc/nn/engine/trt_engine.cc:85-351) behind nn::Engine
// (cc/nn/engine/engine.h:22-43).  Differences by design:
//   * the GoFeatures POD itself (1,860 B) is what crosses PCIe; planes are expanded on
//     the device (go_features.cc:10-61 restated in k_init) instead of 21,692 B of fp32;
//   * only slots loaded since the previous run are uploaded and evaluated, compacted
//     into a dense batch (the TRT engine always runs the full static batch);
//   * only the consumed outputs (7,556 B / position) come back every run; ownership and
//     raw logits stay on the device until asked for.
#include <hip/hip_runtime.h>
#include <chrono>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <unordered_set>
#include <string>
#include <vector>

#include "../../include/p3hip.h"
#include "kernels.h"
#include "block_i8.h"
#include "conv_any.h"
#include "conv_f32.h"
#include "lconv_i8.h"
#include "slot_state.h"
#include "symmetry.h"
#include "transformer.h"
#include "transformer_f32.h"

namespace {

constexpr float kBnEps = 1e-3f;  // model.py:231
constexpr int kNLoc = 361;
constexpr size_t kFeatBytes = sizeof(p3hip_features);
static_assert(sizeof(p3hip_features) == 1860, "p3hip_features layout");
static_assert(sizeof(p3hip_result) == 4 * 1892, "p3hip_result layout");

thread_local std::string g_create_error;

struct Tensor {
  std::vector<int> dims;
  const float* data;
  size_t size() const {
    size_t n = 1;
    for (int d : dims) n *= d;
    return n;
  }
};

struct WeightFile {
  int version = 0, nblocks = 0, C = 0, Cb = 0, H = 0, V = 0, bint = 0, inner = 0, btype = 0;
  // Transformer trunks (btype 3): model_C is the file's C (the model width d); C becomes the residual stream's width
  // p3::tfm_stream_width(d), the smallest of 128, 256 and 384 that holds d, and where that is wider than d the tensors
  // of the stem and the heads are zero-padded to it (pad_transformer_io), so that k_init and the heads of that width
  // serve the trunk unchanged.  model_C == C for every other architecture.
  int model_C = 0;
  // Conv trunks of the set P3HIP_CONV_SET whose C or C_b is not a multiple of 64: C and Cb become the next multiples of
  // 64 and every tensor is zero-padded to them (pad_conv); model_C / model_Cb keep the file's widths.  model_Cb == Cb
  // for every other architecture.
  int model_Cb = 0;
  std::vector<std::vector<float>> padded;
  std::vector<float> data;
  std::map<std::string, Tensor> tensors;

  bool load(const char* path, std::string& err) {
    FILE* f = fopen(path, "rb");
    if (!f) { err = std::string("cannot open ") + path; return false; }
    char magic[4];
    int hdr[10];
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "P3W1", 4) != 0 || fread(hdr, 4, 10, f) != 10) {
      err = "not a .p3w file"; fclose(f); return false;
    }
    version = hdr[0]; nblocks = hdr[1]; C = hdr[2]; Cb = hdr[3]; H = hdr[4]; V = hdr[5];
    bint = hdr[6]; inner = hdr[7]; btype = hdr[8];
    int nt = hdr[9];
    if (nt < 1 || nt > 8192 || nblocks < 1 || nblocks > 256 || (btype == 3 ? bint != 0 : bint < 1)) {
      err = "implausible .p3w header"; fclose(f); return false;
    }
    struct Ent { char name[48]; int ndim; int dims[4]; long long off; };
    std::vector<Ent> ents(nt);
    long long total = 0;
    for (auto& e : ents) {
      if (fread(e.name, 1, 48, f) != 48 || fread(&e.ndim, 4, 1, f) != 1 ||
          fread(e.dims, 4, 4, f) != 4 || fread(&e.off, 8, 1, f) != 1) {
        err = "truncated tensor table"; fclose(f); return false;
      }
      long long sz = 1;
      bool ok = e.ndim >= 0 && e.ndim <= 4 && e.off >= 0 && e.off < (1ll << 31);
      for (int d = 0; ok && d < e.ndim; ++d) {
        ok = e.dims[d] > 0 && e.dims[d] < (1 << 24);
        sz *= e.dims[d];
        ok = ok && sz < (1ll << 31);
      }
      if (!ok) { err = "corrupt tensor table"; fclose(f); return false; }
      if (e.off + sz > total) total = e.off + sz;
    }
    long pos = ftell(f);
    pos += (64 - pos % 64) % 64;
    fseek(f, pos, SEEK_SET);
    data.resize(total);
    if (fread(data.data(), 4, total, f) != (size_t)total) { err = "truncated data"; fclose(f); return false; }
    fclose(f);
    for (auto& e : ents) {
      Tensor t;
      t.dims.assign(e.dims, e.dims + e.ndim);
      t.data = data.data() + e.off;
      tensors[std::string(e.name, strnlen(e.name, sizeof e.name))] = t;
    }
    model_C = C;
    model_Cb = Cb;
    if (conv_set(C, Cb, btype, inner, bint) && H == 32) {
      const int Cp = (C + 63) / 64 * 64, Cbp = btype == 2 ? Cb : (Cb + 63) / 64 * 64;
      if (Cp != C || Cbp != Cb) pad_conv(Cp, Cbp);
    }
    if (btype == 3 && p3::tfm_supported(C, Cb) && p3::tfm_stream_width(C) != C) pad_transformer_io(p3::tfm_stream_width(C));
    return true;
  }
  // The conv trunks of include/p3hip.h P3HIP_CONV_SET (the file's own widths)
  static bool conv_set(int C, int Cb, int btype, int inner, int bint) {
    if (C % 32 != 0 || C < 64 || C > 512 || bint < 2) return false;
    if (btype == 2) return inner == 2;                                   // classic: two 3x3 convs, C_b is ignored
    if (btype != 1 && !(btype == 0 && inner >= 1 && inner <= 3)) return false;
    return Cb % 16 == 0 && Cb >= 32 && Cb <= C;
  }
  // Every tensor with a C or C_b axis zero-padded to Cp / Cbp channels: conv rows and columns, the stem's weights and
  // bias, and BN gamma = beta = mean = var = 0, which folds to scale = shift = 0.  mish(0) = 0, so a padded channel of
  // x, t and u is exactly 0 everywhere (the broadcast dense adds its bias to it; the zero bn1 that follows removes it).
  void pad_conv(int Cp, int Cbp) {
    auto pad = [&](const std::string& n, const std::vector<int>& od, const std::vector<int>& nd) {
      auto it = tensors.find(n);
      size_t on = 1, nn = 1;
      for (int d : od) on *= d;
      for (int d : nd) nn *= d;
      if (it == tensors.end() || it->second.size() != on) return;   // build_plan reports it as missing
      std::vector<float> w(nn, 0.0f);
      std::vector<int> idx(od.size(), 0);
      for (size_t i = 0; i < on; ++i) {
        size_t o = 0;
        for (size_t k = 0; k < od.size(); ++k) o = o * nd[k] + idx[k];
        w[o] = it->second.data[i];
        for (int k = (int)od.size() - 1; k >= 0; --k) {
          if (++idx[k] < od[k]) break;
          idx[k] = 0;
        }
      }
      padded.push_back(std::move(w));
      Tensor t;
      t.dims = nd;
      t.data = padded.back().data();
      it->second = t;
    };
    auto bn = [&](const std::string& n, int c, int cp) {
      for (const char* f : {".gamma", ".beta", ".mean", ".var"}) pad(n + f, {c}, {cp});
    };
    auto conv = [&](const std::string& n, int k, int ci, int co, int cip, int cop) {
      pad(n + ".w", {k, k, ci, co}, {k, k, cip, cop});
    };
    pad("init_conv.w", {5, 5, 15, C}, {5, 5, 15, Cp});
    pad("init_game.w", {8, C}, {8, Cp});
    pad("init_game.b", {C}, {Cp});
    for (int i = 0; i < nblocks; ++i) {
      const std::string p = "blocks." + std::to_string(i);
      if (is_broadcast(i) || btype == 2) {
        const int k = btype == 2 && !is_broadcast(i) ? 3 : 1;
        for (int j = 0; j < 2; ++j) {
          bn(p + ".bn" + std::to_string(j), C, Cp);
          conv(p + ".conv" + std::to_string(j), k, C, C, Cp, Cp);
        }
      } else {
        const int last = btype == 0 ? inner + 1 : 5;
        bn(p + ".bn0", C, Cp);
        conv(p + ".conv0", 1, C, Cb, Cp, Cbp);
        for (int j = 1; j < last; ++j) {
          bn(p + ".bn" + std::to_string(j), Cb, Cbp);
          conv(p + ".conv" + std::to_string(j), 3, Cb, Cb, Cbp, Cbp);
        }
        bn(p + ".bn" + std::to_string(last), Cb, Cbp);
        conv(p + ".conv" + std::to_string(last), 1, Cb, C, Cbp, Cp);
      }
    }
    for (const char* n : {"policy.conv_p", "policy.conv_g", "value.conv"}) conv(n, 1, C, 32, Cp, 32);
    C = Cp;
    Cb = Cbp;
  }
  // [..][C] -> [..][Cp] (init conv, game dense) and [C][32] -> [Cp][32] (the head convs), zeros in the new channels
  void pad_transformer_io(int Cp) {
    auto pad = [&](const std::string& n, size_t rows, bool out_channels) {
      auto it = tensors.find(n);
      const size_t want = out_channels ? rows * C : (size_t)C * 32;
      if (it == tensors.end() || it->second.size() != want) return;   // build_plan reports it as missing
      std::vector<float> w(out_channels ? rows * Cp : (size_t)Cp * 32, 0.0f);
      for (size_t i = 0; i < want; ++i) {
        const size_t r = out_channels ? i / C : 0, c = out_channels ? i % C : i;
        w[out_channels ? r * Cp + c : c] = it->second.data[i];
      }
      padded.push_back(std::move(w));
      Tensor t;
      t.dims = it->second.dims;
      t.dims.back() = out_channels ? Cp : t.dims.back();
      if (!out_channels) t.dims[t.dims.size() - 2] = Cp;
      t.data = padded.back().data();
      it->second = t;
    };
    pad("init_conv.w", 25 * 15, true);
    pad("init_game.w", 8, true);
    pad("init_game.b", 1, true);
    for (const char* n : {"policy.conv_p.w", "policy.conv_g.w", "value.conv.w"}) pad(n, 0, false);
    C = Cp;
  }
  // A missing or mis-shaped tensor (truncated / foreign file) is recorded and answered with a
  // zero tensor of the expected size; build_plan checks `missing` once at the end and
  // p3hip_create fails with the list — the library never aborts the host process.
  mutable std::string missing;
  mutable std::vector<std::vector<float>> zeros;
  mutable std::map<std::string, Tensor> stand_ins;
  const Tensor& get(const std::string& n, size_t expect = 0) const {
    auto it = tensors.find(n);
    if (it != tensors.end() && (expect == 0 || it->second.size() == expect)) return it->second;
    if (missing.size() < 400) missing += (missing.empty() ? "" : ", ") + n + (it == tensors.end() ? "" : " (wrong size)");
    auto st = stand_ins.find(n);
    if (st != stand_ins.end()) return st->second;
    zeros.emplace_back(expect ? expect : 1, 0.0f);
    Tensor t;
    t.dims = {(int)zeros.back().size()};
    t.data = zeros.back().data();
    return stand_ins[n] = t;
  }
  bool is_broadcast(int i) const { return bint > 0 && i % bint == bint - 1; }  // model.py:1002
};

// ---- device arena -----------------------------------------------------------------
struct Arena {
  std::vector<unsigned char> host;
  bool bad_stream = false;
  size_t add(const void* p, size_t bytes) {
    size_t off = (host.size() + 255) & ~size_t(255);
    host.resize(off + bytes);
    memcpy(host.data() + off, p, bytes);
    return off;
  }
};

// k16 blocks [h(2)][CP couts][8] fp16 in (tap major, channel-pair minor) order; see
// conv_segment in conv_core.h.  W is HWIO flattened as [taps][cin_total][cout_total].
void pack_segment(std::vector<_Float16>& dst, const float* W, int taps, int ntaps_pad,
                  int cin_total, int cout_total, int cin0, int CB, int cout0, int CP) {
  for (int tap = 0; tap < ntaps_pad; ++tap)
    for (int q = 0; q < CB / 16; ++q)
      for (int h = 0; h < 2; ++h)
        for (int co = 0; co < CP; ++co)
          for (int e = 0; e < 8; ++e) {
            int ci = cin0 + q * 16 + h * 8 + e, c = cout0 + co;
            float v = 0.0f;
            if (tap < taps && ci < cin_total && c < cout_total)
              v = W[((size_t)tap * cin_total + ci) * cout_total + c];
            dst.push_back((_Float16)v);
          }
}

// 3x3 weights of the fused block kernel: k16 blocks in (kernel row, k32 index, kernel column)
// order — the three taps of a kernel row share their activation fragments (conv16.h
// conv_segment16_3x3), so a step advances the column before the channel slice.
void pack_segment_3x3(std::vector<_Float16>& dst, const float* W, int cin_total, int cout_total, int CB, int CP) {
  for (int ky = 0; ky < 3; ++ky)
    for (int q32 = 0; q32 < CB / 32; ++q32)
      for (int kx = 0; kx < 3; ++kx)
        for (int q = 2 * q32; q < 2 * q32 + 2; ++q)
          for (int h = 0; h < 2; ++h)
            for (int co = 0; co < CP; ++co)
              for (int e = 0; e < 8; ++e) {
                const int ci = q * 16 + h * 8 + e, tap = ky * 3 + kx;
                float v = 0.0f;
                if (ci < cin_total && co < cout_total) v = W[((size_t)tap * cin_total + ci) * cout_total + co];
                dst.push_back((_Float16)v);
              }
}

// k_blockw's weight granule (csrc/asm/blockw_gen.py): 64 output channels x 32 input channels of one tap as four
// MFMA 32x32x16 A fragments, [k16 half j][cout tile c][h][n][8] = W[tap][k0 + 16 j + 8 h + e][cout0 + 32 c + n]: lane
// (n, h) of fragment (j, c) reads its 16 bytes at (2 j + c) * 1024 + lane * 16.  scale (may be null): the folded BN scale
// of the layer that FOLLOWS the conv, times log2(e), per output channel — multiplied in before the one fp16 rounding.
void pack_granule(std::vector<_Float16>& dst, const float* W, int cin_total, int cout_total, int tap, int k0, int cout0,
                  const float* scale) {
  for (int j = 0; j < 2; ++j)
    for (int c = 0; c < 2; ++c)
      for (int h = 0; h < 2; ++h)
        for (int n = 0; n < 32; ++n)
          for (int el = 0; el < 8; ++el) {
            const int co = cout0 + 32 * c + n;
            float v = W[((size_t)tap * cin_total + k0 + 16 * j + 8 * h + el) * cout_total + co];
            if (scale) v *= scale[co];
            dst.push_back((_Float16)v);
          }
}

struct FoldedBN { size_t scale_off, shift_off; };

// A Keras (in, out) matrix W[K][N] as MFMA 16x16x32 A fragments [N / 16][K / 32][64 lanes][8] (transformer.h).
// `col0` / `ld`: the matrix is columns col0 .. col0 + N of a row-major [K][ld] tensor.
void pack_afrag(std::vector<_Float16>& dst, const float* W, int K, int N, int ld, int col0) {
  for (int ct = 0; ct < N / 16; ++ct)
    for (int st = 0; st < K / 32; ++st)
      for (int lane = 0; lane < 64; ++lane)
        for (int el = 0; el < 8; ++el)
          dst.push_back((_Float16)W[(size_t)(32 * st + 8 * (lane >> 4) + el) * ld + col0 + 16 * ct + (lane & 15)]);
}

// The spiral RoPE tables of python/model_transformer.py spiral_rope_cos_sin_table(num_rotations = 4, embed_dim = D,
// grid_len = 19), ROPE_THETA = 100, restated: [361 tokens][D] each, token s = 19 row + col (meshgrid indexing "ij":
// the first coordinate is the row).  Channel i belongs to rotation partition k = i / per (direction k pi / 4), per = D / 4,
// and takes the frequency theta^(-t / nth), nth = D / 4, t = min(nth - 1, 2 (k % 2) + 4 ((i % per) / 4) + (i % per) / 2 % 2):
// both channels of a pair share it.  At D = 32: per = nth = 8.
// Any head width D that is a multiple of 8 (the engine uses 32 and 64): per = nth = D / 4.
void spiral_rope_table(int D, double* cos_out, double* sin_out) {
  const int K = 4, per = D / K, nth = D / 4;
  const double kPi = 3.14159265358979323846;
  std::vector<double> theta(D);
  for (int i = 0; i < D; ++i) {
    const int k = i / per, r = (i % per) / 2;
    int t = 2 * (k % (K / 2)) + (r / 2) * K + (r % 2);
    if (t > nth - 1) t = nth - 1;
    theta[i] = std::pow(100.0, -(double)t / nth);
  }
  for (int s = 0; s < kNLoc; ++s)
    for (int i = 0; i < D; ++i) {
      const double ang = (i / per) * (kPi / K);
      const double proj = (s / 19) * std::cos(ang) + (s % 19) * std::sin(ang);
      cos_out[s * D + i] = std::cos(theta[i] * proj);
      sin_out[s * D + i] = std::sin(theta[i] * proj);
    }
}

// One conv launch of a layer-wise block (kind 4).  Regions: 0 = x; 1, 2 = the two C_b-channel
// halves of the scratch buffer t; 3, 4 = those of u (3 also names u as a whole C-channel buffer).
struct LayerPlan {
  int kw, cin, cout;
  bool pre, act, res, dual;   // see p3::LConvArgs
  FoldedBN pre_bn, out_bn;    // prologue / epilogue BN (epilogue: of act or of dual's second output)
  int in_buf, out_buf, out2_buf;
  size_t stream_off = 0;
  int nms = 0;
  // P3HIP_FLAG_INT8: the quantized weights (lconv_i8.h pack_lconv_i8), their per-output-channel scales, and the index of
  // this layer's input among the engine's quantized tensors (its output, when quantized, is the next one: its consumer)
  size_t q_off = 0, qs_off = 0;
  int qidx = -1;
  size_t w32_off = 0;   // P3HIP_FLAG_FP32: the fp32 weight image (conv_f32.h pack_conv_f32)
};

// One transformer block (kind 5): arena offsets of its tensors, the GEMM weights as MFMA A fragments (transformer.h)
struct TfmPlan { size_t rms_in = 0, rms_out = 0, wqkv = 0, wo = 0, wgu = 0, wdown = 0; };

struct BlockPlan {
  int kind;  // 0 btl, 1 nbt, 3 broadcast, 4 layer-wise (btl/nbt at widths the fused kernel lacks), 5 transformer
  TfmPlan tfm;
  std::vector<LayerPlan> layers;
  size_t stream_off = 0;
  int nms = 0;
  size_t stream_bytes = 0;   // fused blocks: the launch picks the macro-step size (kernels.h block_macro_step_bytes)
  FoldedBN bn[p3::kMaxBlockLayers];
  // broadcast extras
  size_t stream2_off = 0, stream3_off = 0;
  int nms2 = 0, nms3 = 0;
  size_t dense_bias_off = 0;
  size_t w32_first = 0, w32_dense = 0, w32_last = 0;   // P3HIP_FLAG_FP32: conv_first, the dense, conv_last in fp32
  // Broadcast 1x1 convs taken into the neighbouring block launches (k_block's BC form).
  //   on a broadcast block: its conv_first runs at the tail of the launch before it / its conv_last
  //   at the head of the launch after it;
  //   on a fused block: the run's first block carries the head conv (head_of = that broadcast block,
  //   its stream lies right before stream_off), the run's last block the tail conv (right after).
  bool first_fused = false, last_fused = false;
  bool dense_fused = false;   // C = 256: the dense runs in that tail as well (no k_bdense launch, t never stored)
  int head_of = -1, tail_of = -1;
  size_t head_bytes = 0, tail_bytes = 0;
};

// One forward pass: everything it reads or writes that changes from call to call.
struct Pass {
  const unsigned char* feats = nullptr;   // the records k_init reads (a symmetry pass: the records k_sym_expand reads)
  int npos = 0;
  float* out = nullptr;   // the rows the heads write: d_out, or d_cout for the copies of a symmetry pass
  float* res = nullptr;   // d_res: the result records a second time, dense (HeadsArgs::res); null: not written
  int* timed = nullptr;   // p3hip_time_trunk_kernel: launches timed so far, event pairs e->blk_ev[2 i, 2 i + 1]
};

}  // namespace

struct p3hip_engine {
  std::string path, err;
  int batch = 0, device = 0;
  uint32_t flags = 0;
  WeightFile wf;
  int n_cu = 256;
  bool c128_wg8 = false;   // P3HIP_C128_WG8: C = 128 blocks as one 8-wave workgroup per CU (A/B timing)
  bool runs_contiguous = false;   // build_plan laid every run's streams back to back (joined launches possible)
  bool bcast_fuse = true;  // P3HIP_NO_BFUSE clears it: broadcast 1x1 convs as their own launches (A/B, tests)
  int stop_block = -1;     // P3HIP_DEBUG_STOP_BLOCK at create: the forward pass ends in front of plan block n (debugging, tests)
  int last_npos = 0;       // positions of the last forward pass enqueued or replayed (p3hip_debug_tfm)
  bool fuse = true, join = true;   // P3HIP_NO_FUSE clears both: one k_block launch per block; P3HIP_NO_JOIN join: one per run
  int stagger = -1;        // P3HIP_STAGGER: block launches' start-up stagger in cycles (-1: block_args decides)
  bool pair_turns = true;  // P3HIP_NO_PAIR_TURNS clears it: C = 128 workgroup pairs leave the wave priorities alone
  bool direct_results = true;   // P3HIP_NO_DIRECT_RESULTS clears it: p3hip_run copies the results strided from d_out
  bool time_run = false;   // P3HIP_TIME_RUN: p3hip_run times its stages (a measurement aid)
  // k_blockw (csrc/asm/blockw_gen.py): the runs of C = 256 btl blocks by the hand-scheduled one-wave-per-SIMD kernel
  bool blockw = false;
  bool blockw_diag = false;   // P3HIP_BLOCKW_DIAG: the _diag twin, which writes d_bw_stamps
  struct BlockwRun { size_t first; int nblk; size_t stream_off, prm_off; };
  std::vector<BlockwRun> bw_runs;
  hipModule_t bw_mod = nullptr;
  hipFunction_t bw_fn = nullptr;
  unsigned long long* d_bw_stamps = nullptr;   // P3HIP_BLOCKW_DIAG: s_memtime stamps of the _diag kernel
  hipStream_t stream = nullptr;
  // P3HIP_FLAG_LAUNCH_GRAPH: the forward pass over the full static batch, captured once (trt_engine.cc:260-303)
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  bool graph_failed = false, graph_warm = false;
  Pass graph_pass;   // the pass the graph was captured for (kernel arguments are baked in): its feats and res are the key
  // p3hip_time_trunk_kernel: event pairs around the timed launches of a forward pass
  std::vector<hipEvent_t> blk_ev;

  unsigned char* d_arena = nullptr;
  std::vector<BlockPlan> blocks;
  size_t init_stream_off = 0; int init_nms = 0;
  size_t game_w_off = 0, game_b_off = 0;
  size_t heads_stream_off = 0; int heads_nms = 0;
  size_t heads_conv_a_off = 0, heads_image_off = 0;
  bool tfm = false;                     // transformer trunk (blocks of kind 5)
  int tfm_heads = 0, tfm_D = 0;         // its head count and head width (model width wf.model_C = heads x D)
  size_t rope_cos_off = 0, rope_sin_off = 0;
  // P3HIP_FLAG_INT8: the layer-wise blocks' convs run on int8 inputs with per-tensor activation
  // scales.  amax: running per-tensor maxima of the calibration runs (float bits, atomicMax); scale: the s_a = max / 127
  // the int8 kernels read at launch time, so that a replayed graph sees new scales.
  // P3HIP_FLAG_INT8_FUSED (section 9, "Fused INT8 blocks"): int8 is set as well; the C = 256 / C_b = 128 btl blocks are
  // planned layer by layer (the fp16 plan the calibration runs) and run as one k_block_i8 launch each (csrc/block_i8.hip)
  // P3HIP_FLAG_INT8_C128 (section 9, "Fused INT8 blocks at C = 128"): int8, i8f and i8c128 are set; the same plan on the
  // C = 128 / C_b = 64 btl blocks (csrc/block_i8_c128.hip), calibrated through k_lconv_any
  bool int8 = false, i8f = false, i8c128 = false, calibrating = false, have_scales = false;
  int n_q = 0;
  unsigned* d_amax = nullptr;
  float* d_ascale = nullptr;
  std::vector<float> h_scale;
  // P3HIP_FLAG_SYMMETRY_AVG: every slot is evaluated as k copies, one per symmetry of the mask,
  // and the rows averaged back into d_out.  rows: the row capacity of the per-row device buffers (8 x batch with the
  // flag, batch without).  The upload lands in d_sfeats, k_sym_expand writes the copies to d_feats, the heads write the
  // copies' rows to d_cout, k_sym_reduce averages them into d_out (and d_res).
  bool sym = false;
  uint32_t sym_mask = 0xFF;
  int sym_k = 8;
  int sym_syms[p3::kNumSyms] = {0, 1, 2, 3, 4, 5, 6, 7};
  int rows = 0;
  unsigned char* d_sfeats = nullptr;
  float* d_cout = nullptr;
  // The layer-wise conv trunk through the kernels of conv_any.hip (widths as launch arguments): every trunk of
  // P3HIP_CONV_SET that the templated kernels do not serve, and with P3HIP_CONV_ANY=1 in the environment at create the
  // templated layer-wise shapes too (C = 384 / C_b = 192 btl and nbt, classic C = 192), bit for bit the same results
  bool conv_any = false, conv_any_env = false;
  // P3HIP_FLAG_FP32: every conv trunk layer by layer through the kernels of conv_f32.hip; weights and the activation
  // buffers d_x, d_t, d_u are fp32 (the buffers keep their fp16 pointer types and are 4 bytes per element), the heads
  // run k_heads on the hp the fp32 head convs write.  No fp16 value exists in the pass.
  // P3HIP_FLAG_FP32_TFM: the same for a transformer trunk, its blocks through the kernels of transformer_f32.hip; d_qkv
  // is fp32 too.
  bool f32 = false;
  size_t init_w32_off = 0, heads_w32_off = 0;
  bool heads_fused = false;   // k_headsx: the head convs inside the heads kernel (C <= 256; P3HIP_NO_HFUSE clears it)
  std::map<std::string, size_t> head_off;

  // buffers
  unsigned char* h_feats = nullptr;       // pinned [batch] slots as loaded
  unsigned char* h_feats_compact = nullptr;  // pinned, dense
  unsigned char* d_feats = nullptr;
  _Float16 *d_x = nullptr, *d_t = nullptr, *d_u = nullptr;
  _Float16* d_qkv = nullptr;   // transformer trunks: q, k, v [3][rows][head][384][D] (rows 361.. zeroed once)
#ifdef P3_DIAG
  unsigned long long* d_stamps = nullptr;   // diagnostic build: k_block phase stamps of one launch (P3DIAG_LAUNCH)
  unsigned long long* d_spans = nullptr;    // and every workgroup's entry / per-position / exit times of that launch
  int launch_index = 0;
#endif
  _Float16* d_s = nullptr;   // nbt trunks: the block kernel's inner-stream scratch (t and u carry the broadcast blocks' tensors)
  float* d_hp = nullptr;
  float* d_out = nullptr;
  float* h_out = nullptr;  // pinned [batch][kResultFloats]
  float* d_res = nullptr;  // [batch][kResultFloats] dense: the heads kernel writes the result records a second time there
                           // (Pass::res), so that the D2H copy is ONE contiguous transfer instead of a strided one
  double t_h2d = 0, t_fwd = 0, t_d2h = 0;   // P3HIP_TIME_RUN
  long t_runs = 0;
  bool feats_identity = false;   // gather_loaded: every slot was dirty, row == slot: the upload comes straight from h_feats
  p3::SlotStates slots;   // dirty flags + slot -> dense row of the last run (slot_state.h)
  int last_n = 0;
  std::vector<unsigned char> slot_sym, row_sym;   // symmetry given with a keyed load, by slot / by row of the last run

  // on-device NN cache (p3hip_cache_enable): the table, the per-slot keys as loaded, and the per-run lists
  struct DeviceCache {
    bool on = false;
    unsigned mask = 0, run = 0;
    unsigned long long* d_tkeys = nullptr;
    unsigned* d_tmeta = nullptr;
    float* d_tvals = nullptr;
    p3::CacheKey* h_slot_keys = nullptr;   // [batch] by slot (plain memory, written by load_slot_keyed)
    p3::CacheKey *h_keys = nullptr, *d_keys = nullptr;   // [batch] by row of the run (pinned / device)
    int *h_hit = nullptr, *d_hit = nullptr, *h_victim = nullptr, *d_victim = nullptr;
    int *h_lists = nullptr, *d_lists = nullptr;          // [5][batch]: miss rows, hit entries, insert rows, insert src, insert entries
    unsigned *h_sym = nullptr, *d_sym = nullptr;         // [batch] symmetry of the result in out row r
    unsigned char* d_feats2 = nullptr;                   // features of the misses, dense
    std::vector<int> out_row;                            // row of the run -> row of d_out / h_out
    std::vector<unsigned char> was_hit;                  // by row of the run
    unsigned long long lookups = 0, hits = 0, inserts = 0;
  } cache;
  // row of d_out / h_out that holds `slot`'s result (-1: not evaluated by the last run)
  int out_row_of(int slot) const {
    const int row = slots.row(slot);
    return (row >= 0 && cache.on) ? cache.out_row[row] : row;
  }

  bool check(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
  }
  template <class T>
  const T* dev(size_t off) const { return reinterpret_cast<const T*>(d_arena + off); }
  // HIP's current device is per host thread, and the ABI is called from whatever thread the
  // host likes (the infer thread, one GPU thread per game group, a rank's main thread): every
  // entry point that touches HIP binds the engine's device first.
  bool bind() { return check(hipSetDevice(device), "hipSetDevice"); }
};

namespace {

FoldedBN fold_bn(Arena& ar, const WeightFile& wf, const std::string& prefix, size_t n) {
  const Tensor& g = wf.get(prefix + ".gamma", n);
  const Tensor& b = wf.get(prefix + ".beta", n);
  const Tensor& m = wf.get(prefix + ".mean", n);
  const Tensor& v = wf.get(prefix + ".var", n);
  std::vector<float> sc(n), sh(n);
  for (size_t i = 0; i < n; ++i) {
    sc[i] = g.data[i] / std::sqrt(v.data[i] + kBnEps);
    sh[i] = b.data[i] - m.data[i] * sc[i];
  }
  FoldedBN f;
  f.scale_off = ar.add(sc.data(), n * 4);
  f.shift_off = ar.add(sh.data(), n * 4);
  return f;
}

// A stream is a whole number of macro-steps of 4 k16 blocks = cout_pass * 128 bytes
// (conv_core.h ring_slot_bytes).
// A stream that is not a whole number of macro-steps is a packing bug: it is reported through
// Arena::bad_stream and fails p3hip_create (never abort() inside the library).
size_t add_stream(Arena& ar, const std::vector<_Float16>& s, int& nms, int cout_pass) {
  const size_t ms = (size_t)cout_pass * 128;
  if (s.size() * 2 % ms != 0) ar.bad_stream = true;
  nms = (int)(s.size() * 2 / ms);
  return ar.add(s.data(), s.size() * 2);
}

bool build_plan(p3hip_engine* e, Arena& ar) {
  const WeightFile& wf = e->wf;
  const int C = wf.C, Cb = wf.Cb;
  const bool i8f = e->i8f;
  const bool f32 = e->f32;
  // P3HIP_FLAG_FP32 serves the conv trunks, P3HIP_FLAG_FP32_TFM the transformers; both together: whatever the trunk
  const bool f32_conv = (e->flags & P3HIP_FLAG_FP32) != 0, f32_tfm = (e->flags & P3HIP_FLAG_FP32_TFM) != 0;
  if (f32 && wf.btype == 3 && !f32_tfm) {
    e->err = "P3HIP_FLAG_FP32 serves the conv trunks only (" P3HIP_CONV_SET "); the transformer trunks run in fp16, or in "
             "fp32 with P3HIP_FLAG_FP32_TFM";
    return false;
  }
  if (f32 && wf.btype != 3 && !f32_conv) {
    e->err = "P3HIP_FLAG_FP32_TFM serves the transformer trunks only (" P3HIP_TRANSFORMER_SET "); the conv trunks have "
             "P3HIP_FLAG_FP32";
    return false;
  }
  if (f32 && e->int8) {
    e->err = std::string(f32_conv ? (f32_tfm ? "P3HIP_FLAG_FP32 | P3HIP_FLAG_FP32_TFM" : "P3HIP_FLAG_FP32") : "P3HIP_FLAG_FP32_TFM") +
             " cannot be combined with P3HIP_FLAG_INT8, P3HIP_FLAG_INT8_FUSED or P3HIP_FLAG_INT8_C128: an "
             "engine runs one precision plan";
    return false;
  }
  // a conv file whose widths were padded (WeightFile::pad_conv) never takes the plan of the shape it was padded to
  const bool exact = wf.btype == 3 || (wf.model_C == C && wf.model_Cb == Cb);
  const bool fused = !i8f && !f32 && exact && ((C == 256 && Cb == 128) || (C == 128 && Cb == 64));
  const bool classic = wf.btype == 2 && wf.inner == 2;                 // two 3x3 convs C -> C
  const bool classic192 = classic && exact && C == 192;                // b15c192_classic
  const bool bottleneck_ok = wf.btype == 1 || (wf.btype == 0 && wf.inner >= 1 && wf.inner <= 3);
  // P3HIP_FLAG_INT8_FUSED: the btl trunks of the fused block kernel's C = 256 width; P3HIP_FLAG_INT8_C128: those of its
  // C = 128 width; each alone among the three INT8 flags
  const bool i8c = e->i8c128;
  const uint32_t i8_flags = e->flags & (P3HIP_FLAG_INT8 | P3HIP_FLAG_INT8_FUSED | P3HIP_FLAG_INT8_C128);
  const bool i8_alone = (i8_flags & (i8_flags - 1)) == 0;
  const bool i8f_ok = i8f && i8_alone && exact && (i8c ? (C == 128 && Cb == 64) : (C == 256 && Cb == 128)) && wf.btype == 0 &&
                      wf.inner >= 1 && wf.inner <= 3;
  const bool fused_shape = exact && ((C == 256 && Cb == 128) || (C == 128 && Cb == 64)) && bottleneck_ok;
  const bool lw_shape = (exact && C == 384 && Cb == 192 && bottleneck_ok) || classic192;   // the templated k_lconv's shapes
  // every other conv trunk of P3HIP_CONV_SET: layer-wise through conv_any.hip, C and Cb padded to multiples of 64
  const bool any = !fused_shape && !lw_shape &&
                   WeightFile::conv_set(wf.model_C, wf.model_Cb, wf.btype, wf.inner, wf.bint) && C % 64 == 0 &&
                   (wf.btype == 2 || Cb % 64 == 0);
  // (P3HIP_FLAG_FP32 runs the fused shapes layer by layer too)
  const bool layerwise = lw_shape || i8f_ok || any || (f32 && fused_shape);
  const bool v_ok = wf.V == 32 || wf.V == 48 || wf.V == 64 || wf.V == 80;
  // transformer trunk: the file's C is the model width d and Cb the head count (include/p3hip.h: d a multiple of 32,
  // 64 <= d <= 384, head width d / heads 32 or 64); the stream is padded to C = p3::tfm_stream_width(d), and V is what
  // the heads of that width serve (the fused heads at C = 128 / 256: {32, 48, 64}; the C = 384 heads: v_ok)
  const bool tfm = wf.btype == 3 && p3::tfm_supported(wf.model_C, Cb) && C == p3::tfm_stream_width(wf.model_C) &&
                   (C == 384 || p3::heads_fusable(C, wf.V));
  // (a trunk the fp16 engine serves and INT8_FUSED does not is refused below, with INT8_FUSED's own message)
  const bool arch_ok = (fused && bottleneck_ok) || layerwise || tfm ||
                       (i8f && fused_shape);
  if (!arch_ok || wf.H != 32 || !v_ok) {
    e->err = "unsupported architecture for the HIP engine (need a conv trunk (" P3HIP_CONV_SET "), or a transformer "
             "trunk (" P3HIP_TRANSFORMER_SET "); H=32, V in {32,48,64,80} (transformer: V in {32,48,64}, and 80 at "
             "d > 256))";
    return false;
  }
  // (INT8_C128 answers every trunk it does not serve with its own message, the runtime-width conv trunks included)
  if (i8c && !i8f_ok) {
    e->err = "INT8_C128 is available only for C = 128 / C_b = 64 trunks of btl blocks with 1, 2 or 3 inner layers "
             "(b12c128btl3, b10c128btl3, small and their kin, broadcast blocks at any interval), and not together with "
             "another INT8 flag; nbt trunks, the other widths (P3HIP_FLAG_INT8_FUSED serves C = 256 / C_b = 128 btl trunks, "
             "P3HIP_FLAG_INT8 the layer-wise trunks) and the transformer are not served";
    return false;
  }
  if (any && e->int8) {
    e->err = std::string(e->i8f ? "INT8_FUSED" : "INT8") + " is not available for this conv trunk: "
             "P3HIP_FLAG_INT8 serves C = 384 / C_b = 192 btl or nbt blocks and C = 192 classic blocks, P3HIP_FLAG_INT8_FUSED "
             "serves C = 256 / C_b = 128 btl blocks with 1, 2 or 3 inner layers, P3HIP_FLAG_INT8_C128 serves C = 128 / "
             "C_b = 64 btl blocks with 1, 2 or 3 inner layers; the other widths run in fp16 only";
    return false;
  }
  e->conv_any = !f32 && (any || (e->conv_any_env && lw_shape && !e->int8));
  e->tfm = tfm;
  if (tfm) {
    e->tfm_heads = Cb;
    e->tfm_D = wf.model_C / Cb;
  }
  if (i8f && !i8f_ok) {
    e->err = "INT8_FUSED is available only for C = 256 / C_b = 128 trunks of btl blocks with 1, 2 or 3 inner layers "
             "(b12c256btl3 and its kin, broadcast blocks at any interval), and not together with P3HIP_FLAG_INT8; nbt and "
             "C = 128 trunks, the layer-wise trunks (P3HIP_FLAG_INT8 serves those) and the transformer are not served";
    return false;
  }
  if (e->int8 && !layerwise) {
    e->err = "INT8 is available only for layer-wise trunks (C = 384 / C_b = 192 btl or nbt blocks, C = 192 classic "
             "blocks); this trunk runs fused block kernels or the transformer";
    return false;
  }
  // slice width of the per-position kernels that stage C channels (k_conv1x1 family)
  // (layer-wise: p3::conv_any_slice(C) = 64 at classic C = 192 and at INT8_C128's C = 128, 128 at C = 384 and at
  // INT8_FUSED's C = 256)
  const int CB = layerwise ? p3::conv_any_slice(C) : (tfm ? 128 : Cb);
  const int CPI = layerwise ? p3::conv_any_init_pass(C) : 128;   // output pass width of the init conv
  // init conv
  {
    std::vector<_Float16> s;
    const Tensor& w = wf.get("init_conv.w", (size_t)25 * 15 * C);  // [5][5][15][C]
    if (f32) {
      std::vector<float> s32;
      p3::pack_conv_f32(s32, w.data, 25, 15, C, 16, C);
      e->init_w32_off = ar.add(s32.data(), s32.size() * 4);
    } else {
      for (int cp = 0; cp < C / CPI; ++cp)
        pack_segment(s, w.data, 25, 28, 15, C, 0, 16, cp * CPI, CPI);
      e->init_stream_off = add_stream(ar, s, e->init_nms, CPI);
    }
    e->game_w_off = ar.add(wf.get("init_game.w", (size_t)8 * C).data, 8 * C * 4);
    e->game_b_off = ar.add(wf.get("init_game.b", (size_t)C).data, C * 4);
  }
  // k_blockw serves C = 256 / C_b = 128 btl trunks; the broadcast blocks then run as their own launches
  {
    static const bool want_blockw = getenv("P3HIP_BLOCKW") != nullptr && atoi(getenv("P3HIP_BLOCKW")) != 0;
    e->blockw = want_blockw && !i8f && C == 256 && Cb == 128 && wf.btype == 0 && wf.inner >= 1 && wf.inner <= 3;
    if (e->blockw) e->bcast_fuse = false;
  }
  bool have_xa = false;   // layer-wise path: u holds mish(bn0(x)) of the next block
  // The weight streams of consecutive fused blocks go into the arena back to back, after the
  // run's other tensors: one k_block launch walks the streams of all its blocks as ONE circular
  // stream (position-major order, kernels.hip), so a run must be contiguous.
  // With the broadcast 1x1 convs fused in, a run's stream is [conv_last of the broadcast block before
  // it] [its blocks] [conv_first of the broadcast block after it].
  std::vector<std::pair<size_t, std::vector<_Float16>>> run_streams;   // (block index, stream)
  std::vector<_Float16> head_stream, tail_stream;   // of the run being collected
  int head_of = -1, tail_of = -1;
  // The runs' streams are laid out after the loop, all runs back to back ([head r][blocks r][tail r][head r + 1] ...):
  // with everything of the broadcast blocks between them fused, one k_block launch walks them all (joined_launch).
  std::vector<std::function<void()>> layout;
  auto flush_run = [&]() {
    if (!run_streams.empty()) {
      auto rs_all = std::make_shared<std::vector<std::pair<size_t, std::vector<_Float16>>>>(std::move(run_streams));
      auto hs = std::make_shared<std::vector<_Float16>>(std::move(head_stream));
      auto ts = std::make_shared<std::vector<_Float16>>(std::move(tail_stream));
      const int h_of = head_of, t_of = tail_of;
      layout.push_back([&ar, e, rs_all, hs, ts, h_of, t_of, Cb]() {
        int nms_unused = 0;
        if (h_of >= 0) {
          add_stream(ar, *hs, nms_unused, Cb);
          BlockPlan& b = e->blocks[rs_all->front().first];
          b.head_of = h_of;
          b.head_bytes = hs->size() * 2;
          e->blocks[h_of].last_fused = true;
        }
        for (auto& rs : *rs_all) {
          BlockPlan& b = e->blocks[rs.first];
          b.stream_off = add_stream(ar, rs.second, b.nms, Cb);
          b.stream_bytes = rs.second.size() * 2;
        }
        if (t_of >= 0) {
          add_stream(ar, *ts, nms_unused, Cb);
          BlockPlan& b = e->blocks[rs_all->back().first];
          b.tail_of = t_of;
          b.tail_bytes = ts->size() * 2;
        }
      });
    }
    run_streams.clear();
    head_stream.clear();
    tail_stream.clear();
    head_of = tail_of = -1;
  };
  if (tfm) {
    std::vector<double> cd(kNLoc * e->tfm_D), sd(kNLoc * e->tfm_D);
    spiral_rope_table(e->tfm_D, cd.data(), sd.data());
    const std::vector<float> cf(cd.begin(), cd.end()), sf(sd.begin(), sd.end());
    e->rope_cos_off = ar.add(cf.data(), cf.size() * 4);
    e->rope_sin_off = ar.add(sf.data(), sf.size() * 4);
  }
  for (int i = 0; tfm && i < wf.nblocks; ++i) {
    const std::string p = "blocks." + std::to_string(i);
    const int c = wf.model_C, f = 2 * c;
    auto T = [&](const char* n, size_t sz) { return wf.get(p + "." + n, sz).data; };
    BlockPlan bp;
    bp.kind = 5;
    bp.tfm.rms_in = ar.add(T("rms_in.scale", c), c * 4);
    bp.tfm.rms_out = ar.add(T("rms_out.scale", c), c * 4);
    if (f32) {   // P3HIP_FLAG_FP32_TFM: the same fragments in fp32 (transformer_f32.h pack_tfm_f32), no fp16 image
      std::vector<float> w32;
      for (const char* n : {"q.w", "k.w", "v.w"}) p3::pack_tfm_f32(w32, T(n, (size_t)c * c), c, c, c, 0);
      bp.tfm.wqkv = ar.add(w32.data(), w32.size() * 4);
      w32.clear();
      p3::pack_tfm_f32(w32, T("o.w", (size_t)c * c), c, c, c, 0);
      bp.tfm.wo = ar.add(w32.data(), w32.size() * 4);
      w32.clear();
      p3::pack_tfm_f32(w32, T("ffn_gate.w", (size_t)c * f), c, f, f, 0);
      p3::pack_tfm_f32(w32, T("ffn_up.w", (size_t)c * f), c, f, f, 0);
      bp.tfm.wgu = ar.add(w32.data(), w32.size() * 4);
      w32.clear();
      p3::pack_tfm_f32(w32, T("ffn_down.w", (size_t)f * c), f, c, c, 0);
      bp.tfm.wdown = ar.add(w32.data(), w32.size() * 4);
      e->blocks.push_back(bp);
      continue;
    }
    std::vector<_Float16> w;
    for (const char* n : {"q.w", "k.w", "v.w"}) pack_afrag(w, T(n, (size_t)c * c), c, c, c, 0);
    bp.tfm.wqkv = ar.add(w.data(), w.size() * 2);
    w.clear();
    pack_afrag(w, T("o.w", (size_t)c * c), c, c, c, 0);
    bp.tfm.wo = ar.add(w.data(), w.size() * 2);
    w.clear();
    pack_afrag(w, T("ffn_gate.w", (size_t)c * f), c, f, f, 0);
    pack_afrag(w, T("ffn_up.w", (size_t)c * f), c, f, f, 0);
    bp.tfm.wgu = ar.add(w.data(), w.size() * 2);
    w.clear();
    pack_afrag(w, T("ffn_down.w", (size_t)f * c), f, c, c, 0);
    bp.tfm.wdown = ar.add(w.data(), w.size() * 2);
    e->blocks.push_back(bp);
  }
  for (int i = 0; !tfm && i < wf.nblocks; ++i) {
    BlockPlan bp;
    if (layerwise) flush_run();
    const std::string p = "blocks." + std::to_string(i);
    // conv j of this block, checked against the [k][k][cin][cout] size the packer will read
    auto W = [&](int j, int kw, int cin, int cout) {
      return wf.get(p + ".conv" + std::to_string(j) + ".w", (size_t)kw * kw * cin * cout).data;
    };
    if (wf.is_broadcast(i)) {
      bp.kind = 3;
      have_xa = false;
      bp.bn[0] = fold_bn(ar, wf, p + ".bn0", C);
      bp.bn[1] = fold_bn(ar, wf, p + ".bn1", C);
      const int CPb = (CB == 128) ? 128 : 64;
      std::vector<_Float16> s0, s1, s2;
      if (f32) {
        std::vector<float> w32;
        p3::pack_conv_f32(w32, W(0, 1, C, C), 1, C, C, C, C);
        bp.w32_first = ar.add(w32.data(), w32.size() * 4);
        w32.clear();
        p3::pack_dense_f32(w32, wf.get(p + ".dense.w", (size_t)kNLoc * kNLoc).data);
        bp.w32_dense = ar.add(w32.data(), w32.size() * 4);
        w32.clear();
        p3::pack_conv_f32(w32, W(1, 1, C, C), 1, C, C, C, C);
        bp.w32_last = ar.add(w32.data(), w32.size() * 4);
        bp.dense_bias_off = ar.add(wf.get(p + ".dense.b", (size_t)kNLoc).data, kNLoc * 4);
        e->blocks.push_back(bp);
        continue;
      }
      for (int cp = 0; cp < C / CPb; ++cp)
        for (int ip = 0; ip < C / CB; ++ip) {
          pack_segment(s0, W(0, 1, C, C), 1, 1, C, C, ip * CB, CB, cp * CPb, CPb);
          pack_segment(s2, W(1, 1, C, C), 1, 1, C, C, ip * CB, CB, cp * CPb, CPb);
        }
      const Tensor& dw = wf.get(p + ".dense.w", (size_t)kNLoc * kNLoc);  // [361 i][361 j]
      for (int jp = 0; jp < 3; ++jp)
        for (int q = 0; q < 24; ++q)
          for (int h = 0; h < 2; ++h)
            for (int jj = 0; jj < 128; ++jj)
              for (int el = 0; el < 8; ++el) {
                int ii = q * 16 + h * 8 + el, j = jp * 128 + jj;
                float v = (ii < kNLoc && j < kNLoc) ? dw.data[(size_t)ii * kNLoc + j] : 0.0f;
                s1.push_back((_Float16)v);
              }
      // The run before this block takes conv_first as its tail, the run after it conv_last as its
      // head (the stand-alone streams below serve P3HIP_NO_BFUSE and broadcast blocks without a
      // fused neighbour).
      const bool fused_neighbours = fused && e->bcast_fuse;
      // fused copies: output pass 1 takes its K slices in the order (1, 0) — slice 1 is the one
      // still in the act buffer when pass 0 ends (kernels.hip k_block, BC form)
      std::vector<_Float16> f0, f2;
      if (fused_neighbours)
        for (int cp = 0; cp < 2; ++cp)
          for (int k = 0; k < 2; ++k) {
            const int ip = cp == 0 ? k : 1 - k;
            pack_segment(f0, W(0, 1, C, C), 1, 1, C, C, ip * Cb, Cb, cp * Cb, Cb);
            pack_segment(f2, W(1, 1, C, C), 1, 1, C, C, ip * Cb, Cb, cp * Cb, Cb);
          }
      if (fused_neighbours && !run_streams.empty()) {
        tail_stream = f0;
        tail_of = i;
        bp.first_fused = true;
        // C = 256: the dense rides in that tail too (k_block, tail_dense).  Its stream there:
        // [conv_first pass 0 (K slices 0, 1)] [dense] [conv_first pass 1 (K slices 0, 1)] [dense], the dense matrix
        // with its K index = the act buffer's padded board row r = 20 y + x (zero rows for x = 19 and r >= 379)
        static const bool no_dfuse = getenv("P3HIP_NO_DFUSE") != nullptr;
        if (C == 256 && Cb == 128 && wf.btype == 0 && !no_dfuse) {   // btl blocks only (k_block's tail_dense)
          bp.dense_fused = true;
          std::vector<_Float16> dpad;
          for (int jp = 0; jp < 3; ++jp)
            for (int q = 0; q < 24; ++q)
              for (int h = 0; h < 2; ++h)
                for (int jj = 0; jj < 128; ++jj)
                  for (int el = 0; el < 8; ++el) {
                    const int r = q * 16 + h * 8 + el, y = r / 20, x = r % 20, j = jp * 128 + jj;
                    const bool on_board = x < 19 && y < 19;
                    float v = (on_board && j < kNLoc) ? dw.data[(size_t)(y * 19 + x) * kNLoc + j] : 0.0f;
                    dpad.push_back((_Float16)v);
                  }
          tail_stream.clear();
          for (int cp = 0; cp < 2; ++cp) {
            for (int ip = 0; ip < 2; ++ip) pack_segment(tail_stream, W(0, 1, C, C), 1, 1, C, C, ip * Cb, Cb, cp * Cb, Cb);
            tail_stream.insert(tail_stream.end(), dpad.begin(), dpad.end());
          }
        }
      }
      flush_run();
      if (fused_neighbours && i + 1 < wf.nblocks && !wf.is_broadcast(i + 1)) {
        head_stream = f2;
        head_of = i;   // last_fused is set when the run is laid out
      }
      bp.stream_off = add_stream(ar, s0, bp.nms, CPb);
      bp.stream2_off = add_stream(ar, s1, bp.nms2, 128);
      bp.stream3_off = add_stream(ar, s2, bp.nms3, CPb);
      bp.dense_bias_off = ar.add(wf.get(p + ".dense.b", (size_t)kNLoc).data, kNLoc * 4);
    } else if (layerwise) {
      bp.kind = 4;
      const int nconv = classic ? 2 : ((wf.btype == 0) ? wf.inner + 2 : 6);
      for (int j = 0; j < nconv; ++j) bp.bn[j] = fold_bn(ar, wf, p + ".bn" + std::to_string(j), (classic || j == 0) ? C : Cb);
      // The consumer's prologue (BN + mish of its input) is applied ONCE by the producer: a
      // layer either stores its output already activated for the next conv (act), or stores it
      // raw and a second, activated copy (dual).  Only the first layer after the init conv or
      // a broadcast block still activates its input while staging (pre) — every workgroup of
      // an output pass would otherwise redo that VALU work.  `xa` = activated copy of x, in u.
      FoldedBN next_bn0{};
      // (an INT8_FUSED block depends on the stored x alone: every block's first conv activates it, pre)
      const bool next_layerwise = !i8f && i + 1 < wf.nblocks && !wf.is_broadcast(i + 1);
      if (next_layerwise) next_bn0 = fold_bn(ar, wf, "blocks." + std::to_string(i + 1) + ".bn0", C);
      const FoldedBN none{};
      auto add_layer = [&](int j, int kw, int cin, int cout, bool pre, const FoldedBN& pre_bn, bool act, bool res,
                           bool dual, const FoldedBN& out_bn, int in_buf, int out_buf, int out2_buf) {
        LayerPlan lp{kw, cin, cout, pre, act, res, dual, pre_bn, out_bn, in_buf, out_buf, out2_buf};
        std::vector<_Float16> s;
        if (f32) {
          std::vector<float> w32;
          p3::pack_conv_f32(w32, W(j, kw, cin, cout), kw * kw, cin, cout, cin, cout);
          lp.w32_off = ar.add(w32.data(), w32.size() * 4);
        } else {
          for (int cp = 0; cp < cout / 64; ++cp)
            for (int ip = 0; ip < cin / 64; ++ip) pack_segment(s, W(j, kw, cin, cout), kw * kw, kw * kw, cin, cout, ip * 64, 64, cp * 64, 64);
          lp.stream_off = add_stream(ar, s, lp.nms, 64);
        }
        if (e->int8) {
          std::vector<int8_t> q;
          std::vector<float> sw;
          p3::pack_lconv_i8(q, sw, W(j, kw, cin, cout), kw * kw, cin, cout);
          lp.q_off = ar.add(q.data(), q.size());
          lp.qs_off = ar.add(sw.data(), sw.size() * 4);
          lp.qidx = e->n_q++;
        }
        bp.layers.push_back(lp);
      };
      const bool from_xa = have_xa;          // first layer input: activated copy in u, or raw x with pre
      const int in0 = from_xa ? 3 : 0;
      if (classic) {         // x + conv3(act1(conv3(act0(x)))), model.py:330-368
        add_layer(0, 3, C, C, !from_xa, bp.bn[0], true, false, false, bp.bn[1], in0, 1, -1);
        add_layer(1, 3, C, C, false, none, false, true, next_layerwise, next_bn0, 1, 0, 3);
      } else if (wf.btype == 0) {   // btl
        add_layer(0, 1, C, Cb, !from_xa, bp.bn[0], true, false, false, bp.bn[1], in0, 1, -1);
        int cur = 1;
        for (int j = 1; j <= wf.inner; ++j) {
          add_layer(j, 3, Cb, Cb, false, none, true, false, false, bp.bn[j + 1], cur, 3 - cur, -1);
          cur = 3 - cur;
        }
        add_layer(wf.inner + 1, 1, Cb, C, false, none, false, true, next_layerwise, next_bn0, cur, 0, 3);
      } else {               // nbt: the inner residual stream t stays raw in region 1
        add_layer(0, 1, C, Cb, !from_xa, bp.bn[0], false, false, true, bp.bn[1], in0, 1, 2);   // t, act1(t)
        add_layer(1, 3, Cb, Cb, false, none, true, false, false, bp.bn[2], 2, 3, -1);
        add_layer(2, 3, Cb, Cb, false, none, false, true, true, bp.bn[3], 3, 1, 2);             // t' = t + ., act3(t')
        add_layer(3, 3, Cb, Cb, false, none, true, false, false, bp.bn[4], 2, 3, -1);
        add_layer(4, 3, Cb, Cb, false, none, false, true, true, bp.bn[5], 3, 1, 2);             // t'', act5(t'')
        add_layer(5, 1, Cb, C, false, none, false, true, next_layerwise, next_bn0, 2, 0, 3);
      }
      have_xa = next_layerwise;
    } else {
      bp.kind = wf.btype;
      const int nconv = (wf.btype == 0) ? wf.inner + 2 : 6;
      for (int j = 0; j < nconv; ++j) bp.bn[j] = fold_bn(ar, wf, p + ".bn" + std::to_string(j), j == 0 ? C : Cb);
      std::vector<_Float16> s;
      for (int ip = 0; ip < C / CB; ++ip) pack_segment(s, W(0, 1, C, Cb), 1, 1, C, Cb, ip * CB, CB, 0, CB);
      for (int j = 1; j < nconv - 1; ++j) pack_segment_3x3(s, W(j, 3, Cb, Cb), Cb, Cb, CB, CB);
      for (int cp = 0; cp < C / CB; ++cp) pack_segment(s, W(nconv - 1, 1, Cb, C), 1, 1, Cb, C, 0, CB, cp * CB, CB);
      run_streams.emplace_back(e->blocks.size(), std::move(s));
    }
    e->blocks.push_back(bp);
  }
  flush_run();
  for (auto& f : layout) f();
  e->runs_contiguous = true;
  if (e->blockw) {
    // Per run of consecutive btl blocks: the weight stream in the order k_blockw consumes it and the parameter table.
    // The BN in front of a conv's consumer rides in the conv: its folded scale times log2(e) is multiplied into the fp16
    // weights, its shift times log2(e) is the accumulators' initial value (the kernel's exp2-based mish takes
    // log2(e) * y, as bn_mish8_l2 does).
    //   block stream: reduce: x halves (quarters 0, 1 / 2, 3); in a half set A's four k32 granules, then set B's
    //                 layer j: phases (A, lo) (B, lo) (A, hi) (B, hi), each (ky, q32, kx) over its 64 input channels
    //                 expand: output quarters 0..3, k32 steps 0..3 (unscaled: the residual add follows)
    //   block table:  bn0 scale[256] shift[256] (times log2 e) | conv j = 0 .. L: shift[128] of bn j + 1 (times log2 e)
    const int L = wf.inner;
    const float kLog2e = 1.4426950408889634f;
    for (size_t bi = 0; bi < e->blocks.size();) {
      if (e->blocks[bi].kind != 0) { ++bi; continue; }
      size_t n = 1;
      while (bi + n < e->blocks.size() && e->blocks[bi + n].kind == 0) ++n;
      std::vector<_Float16> ws;
      std::vector<float> prm;
      for (size_t b = bi; b < bi + n; ++b) {
        // block index in the weight file = plan index (one BlockPlan per trunk block)
        const std::string p = "blocks." + std::to_string(b);
        auto W = [&](int j, int kw, int cin, int cout) {
          return wf.get(p + ".conv" + std::to_string(j) + ".w", (size_t)kw * kw * cin * cout).data;
        };
        const BlockPlan& bp = e->blocks[b];
        auto bn_row = [&](int j, bool shift) {
          const float* v = reinterpret_cast<const float*>(ar.host.data() + (shift ? bp.bn[j].shift_off : bp.bn[j].scale_off));
          std::vector<float> r((size_t)(j == 0 ? C : Cb));
          for (size_t c = 0; c < r.size(); ++c) r[c] = v[c] * kLog2e;
          return r;
        };
        const float* w0 = W(0, 1, C, Cb);
        const std::vector<float> s1 = bn_row(1, false);
        for (int half = 0; half < 2; ++half)
          for (int s0 = 0; s0 < 128; s0 += 64)
            for (int st = 0; st < 4; ++st) pack_granule(ws, w0, C, Cb, 0, 128 * half + 32 * st, s0, s1.data());
        for (int j = 1; j <= L; ++j) {
          const float* wj = W(j, 3, Cb, Cb);
          const std::vector<float> sj = bn_row(j + 1, false);
          for (int ph = 0; ph < 4; ++ph) {
            const int s0 = (ph & 1) * 64, half = ph >> 1;
            for (int ky = 0; ky < 3; ++ky)
              for (int q = 0; q < 2; ++q)
                for (int kx = 0; kx < 3; ++kx) pack_granule(ws, wj, Cb, Cb, ky * 3 + kx, 64 * half + 32 * q, s0, sj.data());
          }
        }
        const float* we = W(L + 1, 1, Cb, C);
        for (int qo = 0; qo < 4; ++qo)
          for (int c = 0; c < 4; ++c) pack_granule(ws, we, Cb, C, 0, 32 * c, 64 * qo, nullptr);
        for (int sh = 0; sh < 2; ++sh) {
          const std::vector<float> r = bn_row(0, sh == 1);
          prm.insert(prm.end(), r.begin(), r.end());
        }
        for (int j = 1; j <= L + 1; ++j) {
          const std::vector<float> r = bn_row(j, true);
          prm.insert(prm.end(), r.begin(), r.end());
        }
      }
      p3hip_engine::BlockwRun run;
      run.first = bi;
      run.nblk = (int)n;
      run.stream_off = ar.add(ws.data(), ws.size() * 2);
      run.prm_off = ar.add(prm.data(), prm.size() * 4);
      if (ws.size() * 2 != n * (size_t)(32 + 72 * L) * 4096 || prm.size() != n * (size_t)(512 + 128 * (L + 1))) ar.bad_stream = true;
      e->bw_runs.push_back(run);
      bi += n;
    }
  }
  // heads: conv_p | conv_g | value.conv  -> [C][96]
  {
    std::vector<float> w((size_t)C * 96);
    const float* wp = wf.get("policy.conv_p.w", (size_t)C * 32).data;
    const float* wg = wf.get("policy.conv_g.w", (size_t)C * 32).data;
    const float* wv = wf.get("value.conv.w", (size_t)C * 32).data;
    for (int c = 0; c < C; ++c)
      for (int o = 0; o < 32; ++o) {
        w[(size_t)c * 96 + o] = wp[c * 32 + o];
        w[(size_t)c * 96 + 32 + o] = wg[c * 32 + o];
        w[(size_t)c * 96 + 64 + o] = wv[c * 32 + o];
      }
    std::vector<_Float16> s;
    if (f32) {
      std::vector<float> w32;
      p3::pack_conv_f32(w32, w.data(), 1, C, 96, C, 128);
      e->heads_w32_off = ar.add(w32.data(), w32.size() * 4);
    } else {
      for (int cp = 0; cp < 2; ++cp)
        for (int ip = 0; ip < C / CB; ++ip) pack_segment(s, w.data(), 1, 1, C, 96, ip * CB, CB, cp * 64, 64);
      e->heads_stream_off = add_stream(ar, s, e->heads_nms, 64);
    }
    // the same weights as MFMA 16x16x32 A fragments for k_headsx (the convs inside the heads kernel):
    // [cout tile ct][k32 step][lane (n = lane & 15, q = lane >> 4)][8] = w[cin = 32 step + 8 q + e][cout = 16 ct + n]
    if (!f32 && p3::heads_fusable(C, wf.V)) {
      std::vector<_Float16> af;
      for (int ct = 0; ct < 6; ++ct)
        for (int st = 0; st < C / 32; ++st)
          for (int lane = 0; lane < 64; ++lane)
            for (int el = 0; el < 8; ++el)
              af.push_back((_Float16)w[(size_t)(st * 32 + 8 * (lane >> 4) + el) * 96 + ct * 16 + (lane & 15)]);
      e->heads_conv_a_off = ar.add(af.data(), af.size() * 2);
      e->heads_fused = getenv("P3HIP_NO_HFUSE") == nullptr && !e->conv_any;
    }
    FoldedBN g = fold_bn(ar, wf, "policy.gpool_bn", 32);
    e->head_off["gbn_scale"] = g.scale_off;
    e->head_off["gbn_shift"] = g.shift_off;
    const size_t H = 32, V = (size_t)wf.V;
    const struct { const char* name; size_t n; } heads[] = {   // sizes k_heads reads (kernels.h HeadsArgs)
        {"policy.gpool_dense.w", 2 * H * H}, {"policy.gpool_dense.b", H}, {"policy.out_moves.w", 2 * H},
        {"policy.out_pass.w", 4 * H}, {"policy.out_pass.b", 2}, {"policy.opt_moves.w", H},
        {"policy.opt_pass.w", 2 * H}, {"policy.opt_pass.b", 1}, {"value.oq_embed.w", 2 * H * V},
        {"value.oq_embed.b", V}, {"value.oq_out.w", V * 14}, {"value.oq_out.b", 14}, {"value.own.w", H},
        {"value.gamma_pre.w", 2 * H * V}, {"value.gamma_pre.b", V}, {"value.gamma_out.w", V},
        {"value.gamma_out.b", 1}, {"value.score_pre.w", (2 * H + 1) * V}, {"value.score_pre.b", V},
        {"value.score_out.w", V}, {"value.score_out.b", 1}};
    for (const auto& h : heads) {
      const Tensor& t = wf.get(h.name, h.n);
      e->head_off[h.name] = ar.add(t.data, t.size() * 4);
    }
    // k_headsx takes the same tensors as one image in its LDS order (kernels.h heads_image_floats)
    if (!f32 && p3::heads_fusable(C, wf.V) && wf.missing.empty()) {
      std::vector<float> img;
      auto put = [&](const char* name, size_t n, size_t pad = 0) {
        const Tensor& t = wf.get(name, n);
        img.insert(img.end(), t.data, t.data + n);
        img.insert(img.end(), pad, 0.0f);
      };
      put("policy.gpool_dense.w", 2 * H * H); put("value.oq_embed.w", 2 * H * V); put("value.gamma_pre.w", 2 * H * V);
      put("value.score_pre.w", (2 * H + 1) * V); put("value.oq_out.w", V * 14); put("value.gamma_out.w", V);
      put("value.score_out.w", V); put("policy.out_pass.w", 4 * H); put("policy.opt_pass.w", 2 * H);
      put("policy.out_moves.w", 2 * H); put("policy.opt_moves.w", H); put("value.own.w", H);
      {
        const float* gs = reinterpret_cast<const float*>(ar.host.data() + g.scale_off);
        const float* gh = reinterpret_cast<const float*>(ar.host.data() + g.shift_off);
        std::vector<float> tmp(gs, gs + H);
        img.insert(img.end(), tmp.begin(), tmp.end());
        tmp.assign(gh, gh + H);
        img.insert(img.end(), tmp.begin(), tmp.end());
      }
      put("policy.gpool_dense.b", H); put("value.oq_embed.b", V); put("value.gamma_pre.b", V); put("value.score_pre.b", V);
      put("value.oq_out.b", 14, 2);
      if ((int)img.size() != p3::heads_image_floats(32, wf.V)) {
        e->err = "internal error: heads image size";
        return false;
      }
      e->heads_image_off = ar.add(img.data(), img.size() * 4);
    }
  }
  if (!wf.missing.empty()) {
    e->err = "weight file lacks tensors of the architecture its header names: " + wf.missing;
    return false;
  }
  if (ar.bad_stream) {
    e->err = "internal error: a packed weight stream is not a whole number of ring macro-steps";
    return false;
  }
  return true;
}

int grid_for(const p3hip_engine* e, int npos, int npos_per_wg) {
  int wgs = (npos + npos_per_wg - 1) / npos_per_wg;
  return wgs < e->n_cu ? wgs : e->n_cu;
}

// Arguments of one k_block launch over the consecutive fused blocks [first, first + count).
p3::BlockArgs block_args(p3hip_engine* e, size_t first, int count, int npos) {
  p3::BlockArgs a{};
  a.x = e->d_x;
  a.t = e->d_s ? e->d_s : e->d_t;
  a.npos = npos;
  a.nblk = count;
  a.nruns = 1;
  // the streams of consecutive fused blocks lie back to back in the arena (build_plan), the fused
  // broadcast convs' right before the run's first and right after its last block
  const BlockPlan& fb = e->blocks[first];
  const BlockPlan& lb = e->blocks[first + count - 1];
  const size_t ms_bytes = (size_t)p3::block_macro_step_bytes(e->wf.C, e->c128_wg8);
  a.wstream = e->d_arena + fb.stream_off;
  if (fb.head_of >= 0) {
    a.head = 1;
    a.zin = a.zin2 = e->d_u;
    a.wstream = e->d_arena + fb.stream_off - fb.head_bytes;
    a.nms_total += (int)(fb.head_bytes / ms_bytes);
  }
  if (lb.tail_of >= 0) {
    const BlockPlan& bb = e->blocks[lb.tail_of];
    a.tail = 1;
    a.tout = e->d_t;
    a.tail_scale[0] = e->dev<float>(bb.bn[0].scale_off);
    a.tail_shift[0] = e->dev<float>(bb.bn[0].shift_off);
    if (bb.dense_fused) {
      a.tail_dense = 1;
      a.uout = a.uout2 = e->d_u;
      a.dense_bias[0] = e->dev<float>(bb.dense_bias_off);
      a.dense_scale[0] = e->dev<float>(bb.bn[1].scale_off);
      a.dense_shift[0] = e->dev<float>(bb.bn[1].shift_off);
    }
    a.nms_total += (int)(lb.tail_bytes / ms_bytes);
  }
  {
    // Workgroups run their positions in lockstep, so the HBM-bound phases of a launch (the fused
    // broadcast convs above all) hit the memory system from every CU at once.  A start-up stagger of
    // 10,000 cycles per step (seven steps across the CU slots of an XCD) measured -2 % on the forward
    // pass at four positions per workgroup (gpurun_out/stagger_ab.log); it costs its own length once
    // per launch, so short launches go without.  P3HIP_STAGGER overrides (0 = off).
    const bool long_launch = npos >= 3 * e->n_cu * (e->wf.C == 256 || e->c128_wg8 ? 1 : 2);
    // (engines sharing the GPU with others: the spread costs its own length and another stream's kernels fill a
    // launch's tail anyway — 0.3-0.6 % of the self-play rate, gpurun_out/stagger_selfplay.log)
    const bool shared = (e->flags & P3HIP_FLAG_SHARED_DEVICE) != 0;
    a.stagger = e->stagger >= 0 ? e->stagger : ((a.head || a.tail) && long_launch && !shared ? 10000 : 0);
    // two 4-wave workgroups per CU and at least two positions each: they take turns at the higher wave
    // priority (kernels.h; b12c128btl3 forward -3.5 %, b8c128nbt -2.5 % at 1024 positions, nothing at 512 and
    // below; profiles/r02_c128_pair_turns.txt).  P3HIP_NO_PAIR_TURNS=1 leaves the priorities alone.
    a.pair_turns = e->pair_turns && e->wf.C == 128 && !e->c128_wg8 && npos >= 4 * e->n_cu;
  }
  for (int b = 0; b < count; ++b) {
    const BlockPlan& bp = e->blocks[first + b];
    a.nms_total += (int)(bp.stream_bytes / ms_bytes);
    for (int j = 0; j < p3::kMaxBlockLayers; ++j) {
      a.blk[b].scale[j] = e->dev<float>(bp.bn[j].scale_off);
      a.blk[b].shift[j] = e->dev<float>(bp.bn[j].shift_off);
    }
  }
  return a;
}

// Joined launch (C = 256 btl): the runs of fused blocks from `first` on, with the broadcast blocks between them inside
// ONE k_block launch — possible when every such broadcast block has both its 1x1 convs AND its dense fused into the
// neighbouring runs (then their streams lie back to back in the arena, build_plan).  Returns the number of plan
// blocks covered (0: not joinable) and fills `a`.
int joined_launch(p3hip_engine* e, size_t first, int npos, p3::BlockArgs* out) {
  if (!e->join || !e->runs_contiguous) return 0;
  std::vector<std::pair<size_t, int>> runs;   // (first block, count)
  size_t bi = first;
  int nb = 0;
  while (bi < e->blocks.size() && (int)runs.size() < p3::kMaxRuns) {
    const int kind = e->blocks[bi].kind;
    if (kind != 0) break;
    int n = 1;
    while (bi + n < e->blocks.size() && e->blocks[bi + n].kind == kind) ++n;
    if (n > p3::kMaxFuse || nb + n > p3::kMaxLaunchBlocks) break;
    runs.emplace_back(bi, n);
    nb += n;
    bi += n;
    // a broadcast block with everything fused, followed by another run?
    if (bi + 1 < e->blocks.size() && e->blocks[bi].kind == 3 && e->blocks[bi].first_fused && e->blocks[bi].last_fused &&
        e->blocks[bi].dense_fused && e->blocks[bi + 1].kind == 0) ++bi;
    else break;
  }
  if (runs.size() < 2) return 0;
  // the loop may have stepped over a broadcast block without taking the run behind it (kMaxRuns, block limit)
  const size_t last_run_end = runs.back().first + runs.back().second;
  p3::BlockArgs a = block_args(e, runs[0].first, runs[0].second, npos);   // head of run 0 (if any), stagger, stream start
  a.nruns = (int)runs.size();
  a.nms_total = 0;
  a.tail = 0;
  a.tail_dense = 1;
  // u alternates between two buffers inside the launch (t's buffer is free: the dense is fused) when the launch
  // neither starts with a head fed from outside nor ends with a tail read from outside; otherwise one buffer
  const bool closed = !a.head && !(e->blocks[runs.back().first + runs.back().second - 1].tail_of >= 0);
  _Float16* other = closed ? e->d_t : e->d_u;
  a.zin2 = e->d_u;   // head of an even run: what the odd run before it wrote
  a.uout = other;    // tail of an even run
  a.zin = other;     // head of an odd run
  a.uout2 = e->d_u;  // tail of an odd run
  const size_t ms_bytes = (size_t)p3::block_macro_step_bytes(e->wf.C, e->c128_wg8);
  int k = 0;
  for (size_t r = 0; r < runs.size(); ++r) {
    a.run_nblk[r] = runs[r].second;
    const BlockPlan& fb = e->blocks[runs[r].first];
    const BlockPlan& lb = e->blocks[runs[r].first + runs[r].second - 1];
    if (fb.head_of >= 0) a.nms_total += (int)(fb.head_bytes / ms_bytes);
    for (int b = 0; b < runs[r].second; ++b, ++k) {
      const BlockPlan& bp = e->blocks[runs[r].first + b];
      a.nms_total += (int)(bp.stream_bytes / ms_bytes);
      for (int j = 0; j < p3::kMaxBlockLayers; ++j) {
        a.blk[k].scale[j] = e->dev<float>(bp.bn[j].scale_off);
        a.blk[k].shift[j] = e->dev<float>(bp.bn[j].shift_off);
      }
    }
    if (r + 1 < runs.size() || lb.tail_of >= 0) {
      const BlockPlan& bb = e->blocks[lb.tail_of];
      a.nms_total += (int)(lb.tail_bytes / ms_bytes);
      a.tail_scale[r] = e->dev<float>(bb.bn[0].scale_off);
      a.tail_shift[r] = e->dev<float>(bb.bn[0].shift_off);
      a.dense_bias[r] = e->dev<float>(bb.dense_bias_off);
      a.dense_scale[r] = e->dev<float>(bb.bn[1].scale_off);
      a.dense_shift[r] = e->dev<float>(bb.bn[1].shift_off);
      if (r + 1 == runs.size()) a.tail = 1;   // the last run has a tail too (a broadcast block follows it)
    }
  }
  // every run's streams must lie back to back: [head r][blocks r][tail r][head r+1] ...
  for (size_t r = 0; r + 1 < runs.size(); ++r) {
    const BlockPlan& lb = e->blocks[runs[r].first + runs[r].second - 1];
    const BlockPlan& nf = e->blocks[runs[r + 1].first];
    if (lb.stream_off + lb.stream_bytes + lb.tail_bytes + nf.head_bytes != nf.stream_off) return 0;
  }
  *out = a;
  return (int)(last_run_end - first);
}

// Number of blocks the launch starting at block `first` covers: consecutive blocks of the fused
// kernel's kind, at most kMaxFuse (1 when P3HIP_NO_FUSE is set: one launch per block).
int fused_run(const p3hip_engine* e, size_t first) {
  const int kind = e->blocks[first].kind;
  if (kind != 0 && kind != 1) return 0;
  int n = 1;
  while (e->fuse && n < p3::kMaxFuse && first + n < e->blocks.size() && e->blocks[first + n].kind == kind) ++n;
  return n;
}

// k_blockw: the code object assembled from csrc/asm/blockw_gen.py's output rides in the library as a blob
// (blockw_blob.S); one module per engine (modules are per device).  Kernel arguments: csrc/asm/blockw_gen.py.
extern "C" const unsigned char p3_blockw_hsaco[];
extern "C" const unsigned char p3_blockw_hsaco_end[];
struct BlockwArgs {
  const void* x; const void* ws; const void* prm;
  int npos, nblk, nwg, pad;
  void* stamps;
  unsigned long long pad2[2];
};
static_assert(sizeof(BlockwArgs) == 64, "kernarg layout of k_blockw");

bool load_blockw(p3hip_engine* e) {
  if (e->bw_fn) return true;
  if (!e->check(hipModuleLoadData(&e->bw_mod, p3_blockw_hsaco), "hipModuleLoadData k_blockw")) return false;
  const std::string name = "k_blockw_L" + std::to_string(e->wf.inner) + (e->blockw_diag ? "_diag" : "");
  if (!e->check(hipModuleGetFunction(&e->bw_fn, e->bw_mod, name.c_str()), "hipModuleGetFunction k_blockw")) return false;
  if (e->blockw_diag) {
    constexpr size_t bytes = 8 * 16 * 4 * 24 * 8;   // [workgroup 0..7][block][wave][stamp]
    if (!e->check(hipMalloc((void**)&e->d_bw_stamps, bytes), "hipMalloc stamps") ||
        !e->check(hipMemsetAsync(e->d_bw_stamps, 0, bytes, e->stream), "hipMemset stamps")) return false;
  }
  return true;
}

bool launch_blockw(p3hip_engine* e, const p3hip_engine::BlockwRun& run, int npos) {
  if (!load_blockw(e)) return false;
  BlockwArgs a{};
  a.x = e->d_x;
  a.ws = e->d_arena + run.stream_off;
  a.prm = e->d_arena + run.prm_off;
  a.npos = npos;
  a.nblk = run.nblk;
  a.nwg = npos < e->n_cu ? npos : e->n_cu;
  a.stamps = e->d_bw_stamps;
  size_t size = sizeof a;
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  return e->check(hipModuleLaunchKernel(e->bw_fn, a.nwg, 1, 1, 256, 1, 1, 0, e->stream, nullptr, cfg), "launch k_blockw");
}

// Enqueues `launch`; `timed` (p3hip_time_trunk_kernel, null otherwise) counts the launches put between an event pair of
// e->blk_ev, while events last.
template <class Launch>
bool timed_launch(p3hip_engine* e, int* timed, Launch&& launch) {
  const bool on = timed && 2 * *timed + 1 < (int)e->blk_ev.size();
  if (on) hipEventRecord(e->blk_ev[2 * *timed], e->stream);
  if (!launch()) return false;
  if (on) hipEventRecord(e->blk_ev[2 * (*timed)++ + 1], e->stream);
  return true;
}

// Enqueues the whole forward pass `p`.
bool enqueue_forward(p3hip_engine* e, const Pass& p) {
  const WeightFile& wf = e->wf;
  const int C = wf.C, npos = p.npos;
  hipStream_t s = e->stream;
  const bool any = e->conv_any;
  auto conv1x1 = [&](int which, const p3::Conv1x1Args& a) {
    return any ? p3::launch_conv1x1_any(C, which, a, e->n_cu, s) : p3::launch_conv1x1(C, which, a, e->n_cu, s);
  };
  if (e->f32) {
    const p3::InitF32Args a{p.feats, (float*)e->d_x, npos, C, e->dev<float>(e->init_w32_off), e->dev<float>(e->game_w_off),
                            e->dev<float>(e->game_b_off)};
    if (!e->check(p3::launch_init_f32(a, e->n_cu, s), "launch k_init_f32")) return false;
  } else {
    p3::InitArgs a{};
    a.feats = p.feats; a.x = e->d_x; a.npos = npos;
    a.wstream = e->d_arena + e->init_stream_off; a.nms_total = e->init_nms;
    a.game_w = e->dev<float>(e->game_w_off); a.game_b = e->dev<float>(e->game_b_off);
    if (!e->check(e->conv_any ? p3::launch_init_any(C, a, grid_for(e, npos, 1), s)
                              : p3::launch_init(C, a, grid_for(e, npos, 1), s), "launch k_init")) return false;
  }
#ifdef P3_DIAG
  e->launch_index = 0;
#endif
  // debugging aid (tools/gpu_blockw_ab.py xdiff, tests/test_trunk_blocks_gpu.py): stop the forward pass in front of
  // plan block e->stop_block (P3HIP_DEBUG_STOP_BLOCK when the engine was created); a value equal to the block count
  // stops it after the last block, in front of the heads (which take d_t, the transformer's o, as scratch)
  const int stop_block = e->stop_block;
  e->last_npos = npos;
  for (size_t bi = 0; bi < e->blocks.size(); ++bi) {
    if (stop_block >= 0 && (int)bi >= stop_block) return true;
    const BlockPlan& bp = e->blocks[bi];
    if (bp.kind == 5 && e->f32) {
      const int d = wf.model_C;
      const size_t per = (size_t)e->rows * p3::kTfmLPad * d;   // one of q, k, v: [rows][head][384][D] floats
      float *x = (float*)e->d_x, *q = (float*)e->d_qkv, *k = q + per, *v = k + per, *o = (float*)e->d_t;
      const p3::TfmQkvF32Args a{x, q, k, v, npos, d, e->tfm_D, e->dev<float>(bp.tfm.rms_in), e->dev<float>(bp.tfm.wqkv),
                                e->dev<float>(e->rope_cos_off), e->dev<float>(e->rope_sin_off)};
      if (!e->check(p3::launch_tfm_qkv_f32(a, s), "launch k_tfm_qkv_f32")) return false;
      const p3::TfmAttnF32Args b{q, k, v, o, npos, e->tfm_heads};
      if (!timed_launch(e, p.timed, [&] { return e->check(p3::launch_tfm_attn_f32(e->tfm_D, b, s), "launch k_tfm_attn_f32"); }))
        return false;
      const p3::TfmFfnF32Args f{o, x, npos, d, e->dev<float>(bp.tfm.wo), e->dev<float>(bp.tfm.rms_out),
                                e->dev<float>(bp.tfm.wgu), e->dev<float>(bp.tfm.wdown)};
      if (!e->check(p3::launch_tfm_ffn_f32(f, s), "launch k_tfm_ffn_f32")) return false;
    } else if (bp.kind == 5) {
      const int d = wf.model_C;
      const size_t per = (size_t)e->rows * p3::kTfmLPad * d;   // one of q, k, v: [rows][head][384][D]
      _Float16 *q = e->d_qkv, *k = q + per, *v = k + per, *o = e->d_t;
      p3::TfmQkvArgs a{e->d_x, q, k, v, npos, e->dev<float>(bp.tfm.rms_in), e->d_arena + bp.tfm.wqkv,
                       e->dev<float>(e->rope_cos_off), e->dev<float>(e->rope_sin_off)};
      if (!e->check(p3::launch_tfm_qkv(d, e->tfm_D, a, s), "launch k_tfm_qkv")) return false;
      const p3::TfmAttnArgs b{q, k, v, o, npos, e->tfm_heads};
      if (!timed_launch(e, p.timed, [&] { return e->check(p3::launch_tfm_attn(e->tfm_D, b, s), "launch k_tfm_attn"); }))
        return false;
      const p3::TfmFfnArgs f{o, e->d_x, npos, e->d_arena + bp.tfm.wo, e->dev<float>(bp.tfm.rms_out),
                             e->d_arena + bp.tfm.wgu, e->d_arena + bp.tfm.wdown};
      if (!e->check(p3::launch_tfm_ffn(d, f, s), "launch k_tfm_ffn")) return false;
    } else if (bp.kind == 3 && e->f32) {
      float *x = (float*)e->d_x, *t = (float*)e->d_t, *u = (float*)e->d_u;
      p3::LConvF32Args c0{};   // t = mish(conv_first(mish(bn0(x))))
      c0.in = x; c0.out = t; c0.npos = npos; c0.cin = c0.cout = C; c0.w = e->dev<float>(bp.w32_first);
      c0.pre = 1; c0.act = 2;
      c0.scale_in = e->dev<float>(bp.bn[0].scale_off); c0.shift_in = e->dev<float>(bp.bn[0].shift_off);
      if (!e->check(p3::launch_lconv_f32(1, c0, e->n_cu, s), "launch conv_first (fp32)")) return false;
      const p3::BDenseF32Args d{t, u, npos, C, e->dev<float>(bp.w32_dense), e->dev<float>(bp.dense_bias_off),
                                e->dev<float>(bp.bn[1].scale_off), e->dev<float>(bp.bn[1].shift_off)};
      if (!e->check(p3::launch_bdense_f32(d, e->n_cu, s), "launch k_bdense_f32")) return false;
      p3::LConvF32Args c1{};   // x += conv_last(u)
      c1.in = u; c1.out = x; c1.npos = npos; c1.cin = c1.cout = C; c1.w = e->dev<float>(bp.w32_last);
      c1.res = 1;
      if (!e->check(p3::launch_lconv_f32(1, c1, e->n_cu, s), "launch conv_last (fp32)")) return false;
    } else if (bp.kind == 4 && e->f32) {
      const size_t half = (size_t)e->rows * wf.Cb * kNLoc;   // elements of one C_b-channel tensor
      float* bufs[5] = {(float*)e->d_x, (float*)e->d_t, (float*)e->d_t + half, (float*)e->d_u, (float*)e->d_u + half};
      for (const LayerPlan& lp : bp.layers) {
        p3::LConvF32Args a{};
        a.in = bufs[lp.in_buf]; a.out = bufs[lp.out_buf]; a.out2 = lp.out2_buf >= 0 ? bufs[lp.out2_buf] : nullptr;
        a.npos = npos; a.cin = lp.cin; a.cout = lp.cout; a.w = e->dev<float>(lp.w32_off);
        a.pre = lp.pre; a.act = lp.act; a.res = lp.res; a.dual = lp.dual;
        if (a.pre) { a.scale_in = e->dev<float>(lp.pre_bn.scale_off); a.shift_in = e->dev<float>(lp.pre_bn.shift_off); }
        if (a.act || a.dual) { a.scale_out = e->dev<float>(lp.out_bn.scale_off); a.shift_out = e->dev<float>(lp.out_bn.shift_off); }
        auto launch = [&] { return e->check(p3::launch_lconv_f32(lp.kw, a, e->n_cu, s), "launch k_lconv_f32"); };
        if (!timed_launch(e, lp.kw == 3 ? p.timed : nullptr, launch)) return false;
      }
    } else if (bp.kind == 3) {
      p3::Conv1x1Args c0{};
      c0.in = e->d_x; c0.out16 = e->d_t; c0.npos = npos;
      c0.wstream = e->d_arena + bp.stream_off; c0.nms_total = bp.nms;
      c0.scale = e->dev<float>(bp.bn[0].scale_off); c0.shift = e->dev<float>(bp.bn[0].shift_off);
      if (!bp.first_fused && !e->check(conv1x1(0, c0), "launch conv_first")) return false;
      p3::BDenseArgs d{};
      d.t = e->d_t; d.u = e->d_u; d.npos = npos;
      d.wstream = e->d_arena + bp.stream2_off; d.nms_total = bp.nms2;
      d.bias = e->dev<float>(bp.dense_bias_off);
      d.scale = e->dev<float>(bp.bn[1].scale_off); d.shift = e->dev<float>(bp.bn[1].shift_off);
      if (!(bp.first_fused && bp.dense_fused) &&
          !e->check(any ? p3::launch_bdense_any(C, d, grid_for(e, npos, 1), s)
                        : p3::launch_bdense(C, d, grid_for(e, npos, 1), s), "launch bdense")) return false;
      p3::Conv1x1Args c1{};
      c1.in = e->d_u; c1.out16 = e->d_x; c1.npos = npos;
      c1.wstream = e->d_arena + bp.stream3_off; c1.nms_total = bp.nms3;
      if (!bp.last_fused && !e->check(conv1x1(1, c1), "launch conv_last")) return false;
    } else if (bp.kind == 4) {
      const size_t half = (size_t)e->rows * wf.Cb * kNLoc;   // elements of one C_b-channel tensor
      _Float16* bufs[5] = {e->d_x, e->d_t, e->d_t + half, e->d_u, e->d_u + half};
      // the fields p3::LConvArgs and p3::LConvI8Args share
      auto fill = [&](auto& a, const LayerPlan& lp) {
        a.in = bufs[lp.in_buf]; a.out = bufs[lp.out_buf]; a.npos = npos;
        a.out2 = lp.out2_buf >= 0 ? reinterpret_cast<decltype(a.out2)>(bufs[lp.out2_buf]) : nullptr;
        a.pre = lp.pre; a.act = lp.act; a.res = lp.res; a.dual = lp.dual;
        if (a.pre) { a.scale_in = e->dev<float>(lp.pre_bn.scale_off); a.shift_in = e->dev<float>(lp.pre_bn.shift_off); }
        if (a.act || a.dual) { a.scale_out = e->dev<float>(lp.out_bn.scale_off); a.shift_out = e->dev<float>(lp.out_bn.shift_off); }
      };
      if (e->i8f && !e->calibrating) {
        // one launch runs the block's convs with the activations in LDS; the layers carry its tensors
        p3::BlockI8Args a{};
        a.x = e->d_x; a.npos = npos; a.inner = wf.inner;
        a.act_scale = e->d_ascale; a.q0 = bp.layers[0].qidx;
        for (size_t j = 0; j < bp.layers.size(); ++j) {
          const LayerPlan& lp = bp.layers[j];
          a.w[j] = e->dev<int8_t>(lp.q_off); a.w_scale[j] = e->dev<float>(lp.qs_off);
          // bn_j is the prologue of conv 0 and the epilogue of conv j - 1
          const FoldedBN& bn = j == 0 ? lp.pre_bn : bp.layers[j - 1].out_bn;
          a.scale[j] = e->dev<float>(bn.scale_off); a.shift[j] = e->dev<float>(bn.shift_off);
        }
        auto launch = [&] {
          return e->check(e->i8c128 ? p3::launch_block_i8_c128(a, e->n_cu, s) : p3::launch_block_i8(a, e->n_cu, s), "launch k_block_i8");
        };
        if (!timed_launch(e, p.timed, launch)) return false;
        continue;
      }
      if (e->int8 && !e->calibrating) {
        // the int8 plan (its callers check int8_ready): the same regions, an int8 tensor where the fp16 plan stores an activated one
        for (const LayerPlan& lp : bp.layers) {
          p3::LConvI8Args a{};
          fill(a, lp);
          a.w = e->dev<int8_t>(lp.q_off); a.w_scale = e->dev<float>(lp.qs_off);
          a.act_scale = e->d_ascale; a.in_scale = lp.qidx; a.out_scale = lp.qidx + 1;
          auto launch = [&] { return e->check(p3::launch_lconv_i8(lp.kw, lp.cin, lp.cout, a, s), "launch k_lconv_i8"); };
          if (!timed_launch(e, lp.kw == 3 ? p.timed : nullptr, launch)) return false;
        }
        continue;
      }
      for (const LayerPlan& lp : bp.layers) {
        if (e->calibrating) {
          // MinMax calibration: the absmax of this conv's quantized input, the activated tensor (pre: mish(bn0(x)),
          // which the fp16 plan never stores) folded into the running maximum
          p3::AbsmaxArgs m{};
          m.in = bufs[lp.in_buf]; m.npos = npos; m.C = lp.cin; m.amax = e->d_amax + lp.qidx;
          if (lp.pre) { m.scale = e->dev<float>(lp.pre_bn.scale_off); m.shift = e->dev<float>(lp.pre_bn.shift_off); }
          if (!e->check(p3::launch_absmax(m, e->n_cu, s), "launch k_absmax")) return false;
        }
        p3::LConvArgs a{};
        fill(a, lp);
        a.wstream = e->d_arena + lp.stream_off; a.nms_total = lp.nms;
        // (INT8_C128 calibrates through the runtime-width kernel: k_lconv has no C = 128 / C_b = 64 instantiations)
        const bool lany = any || e->i8c128;
        auto launch = [&] {
          return e->check(lany ? p3::launch_lconv_any(lp.kw, lp.cin, lp.cout, a, e->n_cu, s)
                               : p3::launch_lconv(lp.kw, lp.cin, lp.cout, a, e->n_cu, s), lany ? "launch k_lconv_any" : "launch k_lconv");
        };
        if (!timed_launch(e, lp.kw == 3 ? p.timed : nullptr, launch)) return false;
      }
    } else if (e->blockw && bp.kind == 0) {
      const p3hip_engine::BlockwRun* run = nullptr;
      for (const auto& r : e->bw_runs) if (r.first == bi) run = &r;
      if (!run) { e->err = "internal error: no k_blockw run starts at this block"; return false; }
      if (!timed_launch(e, p.timed, [&] { return launch_blockw(e, *run, npos); })) return false;
      bi += run->nblk - 1;
    } else {
      int run = fused_run(e, bi);
      p3::BlockArgs a;
      const int joined = joined_launch(e, bi, npos, &a);
      if (joined > 0) run = joined;
      else a = block_args(e, bi, run, npos);
#ifdef P3_DIAG
      {
        static const int which = getenv("P3DIAG_LAUNCH") ? atoi(getenv("P3DIAG_LAUNCH")) : 1;
        constexpr size_t bytes = (size_t)p3::kStampWgs * 8 * p3::kStampSections * p3::kStampSlots * 8;
        if (!e->d_stamps && hipMalloc((void**)&e->d_stamps, bytes) == hipSuccess) hipMemset(e->d_stamps, 0, bytes);
        constexpr size_t span_bytes = (size_t)p3::kSpanWgs * p3::kSpanSlots * 8;
        if (!e->d_spans && hipMalloc((void**)&e->d_spans, span_bytes) == hipSuccess) hipMemset(e->d_spans, 0, span_bytes);
        // joined launches: ONE block launch per forward pass (index 0); P3DIAG_RUN picks the run whose phases are stamped
        static const int which_run = getenv("P3DIAG_RUN") ? atoi(getenv("P3DIAG_RUN")) : 1;
        const int idx = (a.nruns > 1) ? 0 : which;
        a.stamp_run = (a.nruns > 1) ? which_run : 0;
        a.spans = (e->launch_index == idx) ? e->d_spans : nullptr;
        a.stamps = (e->launch_index++ == idx) ? e->d_stamps : nullptr;
      }
#endif
      auto launch = [&] { return e->check(p3::launch_block(C, bp.kind, wf.inner, e->c128_wg8, a, e->n_cu, s), "launch k_block"); };
      if (!timed_launch(e, p.timed, launch)) return false;
      bi += run - 1;
    }
  }
  if (stop_block == (int)e->blocks.size()) return true;
  {
    p3::Conv1x1Args c{};
    c.in = e->d_x; c.out32 = e->d_hp; c.npos = npos;
    c.wstream = e->d_arena + e->heads_stream_off; c.nms_total = e->heads_nms;
    if (e->f32) {
      p3::LConvF32Args hc{};   // the three head convs C -> 96 in fp32, hp in k_heads' layout
      hc.in = (const float*)e->d_x; hc.out = e->d_hp; hc.npos = npos; hc.cin = C; hc.cout = 128; hc.hp = 1;
      hc.w = e->dev<float>(e->heads_w32_off);
      if (!e->check(p3::launch_lconv_f32(1, hc, e->n_cu, s), "launch head convs (fp32)")) return false;
    } else if (!e->heads_fused && !e->check(conv1x1(2, c), "launch head convs")) return false;
    p3::HeadsArgs h{};
    h.x = e->d_x;
    h.conv_a = e->d_arena + e->heads_conv_a_off;
    h.image = e->dev<float>(e->heads_image_off);
    h.hp = e->d_hp; h.out = p.out; h.npos = npos; h.V = wf.V;
    h.res = p.res;
    auto F = [&](const char* n) { return e->dev<float>(e->head_off.at(n)); };
    h.gbn_scale = F("gbn_scale"); h.gbn_shift = F("gbn_shift");
    h.gd_w = F("policy.gpool_dense.w"); h.gd_b = F("policy.gpool_dense.b");
    h.moves_w = F("policy.out_moves.w");
    h.pass_w = F("policy.out_pass.w"); h.pass_b = F("policy.out_pass.b");
    h.opt_moves_w = F("policy.opt_moves.w");
    h.opt_pass_w = F("policy.opt_pass.w"); h.opt_pass_b = F("policy.opt_pass.b");
    h.oq_embed_w = F("value.oq_embed.w"); h.oq_embed_b = F("value.oq_embed.b");
    h.oq_out_w = F("value.oq_out.w"); h.oq_out_b = F("value.oq_out.b");
    h.own_w = F("value.own.w");
    h.gamma_pre_w = F("value.gamma_pre.w"); h.gamma_pre_b = F("value.gamma_pre.b");
    h.gamma_out_w = F("value.gamma_out.w"); h.gamma_out_b = F("value.gamma_out.b");
    h.score_pre_w = F("value.score_pre.w"); h.score_pre_b = F("value.score_pre.b");
    h.score_out_w = F("value.score_out.w"); h.score_out_b = F("value.score_out.b");
    if (e->heads_fused) {
      if (!e->check(p3::launch_headsx(C, h, e->n_cu, s), "launch k_headsx")) return false;
    } else if (!e->check(p3::launch_heads(h, npos, s), "launch k_heads")) return false;
  }
  return true;
}

// k_sym_expand: the `n` records at `src` -> their k copies in d_feats
bool expand_sym(p3hip_engine* e, const unsigned char* src, int n) {
  p3::SymExpandArgs x{};
  x.in = src; x.out = e->d_feats; x.n = n; x.k = e->sym_k;
  for (int j = 0; j < p3::kNumSyms; ++j) x.syms[j] = e->sym_syms[j];
  return e->check(p3::launch_sym_expand(x, e->stream), "launch k_sym_expand");
}

// P3HIP_FLAG_SYMMETRY_AVG: the `p.npos` slots' records in p.feats -> k copies each in d_feats -> the forward pass over
// n k rows (the heads write d_cout, never d_res) -> the averaged rows in p.out, and the result records in p.res.
bool enqueue_sym(p3hip_engine* e, const Pass& p) {
  if (!expand_sym(e, p.feats, p.npos) || !enqueue_forward(e, Pass{e->d_feats, p.npos * e->sym_k, e->d_cout})) return false;
  p3::SymReduceArgs r{};
  r.rows = e->d_cout; r.out = p.out; r.res = p.res; r.n = p.npos; r.k = e->sym_k;
  for (int j = 0; j < p3::kNumSyms; ++j) r.syms[j] = e->sym_syms[j];
  return e->check(p3::launch_sym_reduce(r, e->stream), "launch k_sym_reduce");
}

// The forward pass of a run (with P3HIP_FLAG_SYMMETRY_AVG: expand, forward and reduce): one captured graph for the full
// static batch when the engine was created with P3HIP_FLAG_LAUNCH_GRAPH (the reference's TensorRT engine replays a
// captured graph, trt_engine.cc:260-303), the kernel-by-kernel launches otherwise and for every other position count.
// The first full-batch run goes out kernel by kernel (the launchers set their kernels' LDS attributes on first use,
// which a capture must not see), the second is captured, the rest replay.  A capture that fails falls back to the
// launches for good.  Calibration runs (the fp16 plan + absmax) go kernel by kernel.
bool run_pass(p3hip_engine* e, const Pass& p) {
  e->last_npos = p.npos * (e->sym ? e->sym_k : 1);
  auto enqueue = [&] { return e->sym ? enqueue_sym(e, p) : enqueue_forward(e, p); };
  if (!(e->flags & P3HIP_FLAG_LAUNCH_GRAPH) || p.npos != e->batch || e->graph_failed || e->calibrating) return enqueue();
  // The capture bakes every kernel argument in: the feature buffer the pass reads (run_cached's passes read the cache's
  // gathered copy) and whether it writes d_res.  The graph serves the pass it was captured for; any other goes out
  // kernel by kernel.
  if (e->graph_exec) {
    if (p.feats != e->graph_pass.feats || p.res != e->graph_pass.res) return enqueue();
    return e->check(hipGraphLaunch(e->graph_exec, e->stream), "hipGraphLaunch");
  }
  if (!e->graph_warm) {
    e->graph_warm = true;
    return enqueue();
  }
  if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    e->graph_failed = true;
    (void)hipGetLastError();
    return enqueue();
  }
  const bool ok = enqueue();
  hipGraph_t g = nullptr;
  const hipError_t ce = hipStreamEndCapture(e->stream, &g);
  if (!ok || ce != hipSuccess || !g || hipGraphInstantiate(&e->graph_exec, g, nullptr, nullptr, 0) != hipSuccess) {
    if (g) hipGraphDestroy(g);
    e->graph_exec = nullptr;
    e->graph_failed = true;
    (void)hipGetLastError();
    return enqueue();   // nothing was executed by the capture
  }
  e->graph = g;
  e->graph_pass = p;
  return e->check(hipGraphLaunch(e->graph_exec, e->stream), "hipGraphLaunch");
}

void drop_graph(p3hip_engine* e) {
  if (e->graph_exec) hipGraphExecDestroy(e->graph_exec);
  if (e->graph) hipGraphDestroy(e->graph);
  e->graph_exec = nullptr;
  e->graph = nullptr;
}

// where p3hip_run / p3hip_upload put the slots' records: the forward pass's input, or the expand's
unsigned char* upload_buffer(p3hip_engine* e) { return e->sym ? e->d_sfeats : e->d_feats; }

// H2D of the `n` records gather_loaded put in the dense upload
bool upload(p3hip_engine* e, int n) {
  return e->check(hipMemcpyAsync(upload_buffer(e), e->feats_identity ? e->h_feats : e->h_feats_compact,
                                 (size_t)n * kFeatBytes, hipMemcpyHostToDevice, e->stream), "H2D features");
}

// D2H of the result records of rows 0 .. n - 1 into h_out: one contiguous copy from `res` (d_res), or strided from d_out
bool download(p3hip_engine* e, int n, const float* res) {
  const size_t rec = p3::kResultFloats * 4;
  return e->check(res ? hipMemcpyAsync(e->h_out, res, n * rec, hipMemcpyDeviceToHost, e->stream)
                      : hipMemcpy2DAsync(e->h_out, rec, e->d_out, p3::kOutStride * 4, rec, n, hipMemcpyDeviceToHost, e->stream),
                  "D2H results");
}

// Frees the NN cache's buffers and leaves it off (p3hip_destroy; a p3hip_cache_enable that failed part-way)
void free_cache(p3hip_engine::DeviceCache& c) {
  hipFree(c.d_tkeys); hipFree(c.d_tmeta); hipFree(c.d_tvals); hipFree(c.d_keys); hipFree(c.d_hit); hipFree(c.d_victim);
  hipFree(c.d_lists); hipFree(c.d_sym); hipFree(c.d_feats2);
  if (c.h_keys) hipHostFree(c.h_keys);
  if (c.h_hit) hipHostFree(c.h_hit);
  if (c.h_victim) hipHostFree(c.h_victim);
  if (c.h_lists) hipHostFree(c.h_lists);
  if (c.h_sym) hipHostFree(c.h_sym);
  delete[] c.h_slot_keys;
  c = p3hip_engine::DeviceCache{};
}

}  // namespace

extern "C" {

const char* p3hip_create_error(void) { return g_create_error.c_str(); }
int p3hip_graph_state(const p3hip_engine* e) { return e->graph_failed ? -1 : (e->graph_exec ? 1 : 0); }

p3hip_engine* p3hip_create(const char* weights_path, int batch_size, int version,
                           int device_ordinal, uint32_t flags) {
  g_create_error.clear();
  if (version != 1) { g_create_error = "only model version 1 (15 planes + 8 scalars) is supported"; return nullptr; }
  if (batch_size < 1 || batch_size > (1 << 16)) { g_create_error = "bad batch size"; return nullptr; }
  const bool sym = (flags & P3HIP_FLAG_SYMMETRY_AVG) != 0;
  if (sym && (size_t)p3::kNumSyms * batch_size > (1u << 16)) {
    g_create_error = "P3HIP_FLAG_SYMMETRY_AVG evaluates 8 copies of every slot: 8 x batch size " +
                     std::to_string(batch_size) + " exceeds the engine's row limit of 65536 (batch size at most 8192)";
    return nullptr;
  }
  p3hip_engine* e = new p3hip_engine();
  e->path = weights_path;
  e->batch = batch_size;
  e->device = device_ordinal;
  e->flags = flags;
  e->c128_wg8 = getenv("P3HIP_C128_WG8") != nullptr;
  e->bcast_fuse = getenv("P3HIP_NO_BFUSE") == nullptr;
  e->stop_block = getenv("P3HIP_DEBUG_STOP_BLOCK") ? atoi(getenv("P3HIP_DEBUG_STOP_BLOCK")) : -1;
  e->fuse = getenv("P3HIP_NO_FUSE") == nullptr;
  e->join = e->fuse && getenv("P3HIP_NO_JOIN") == nullptr;
  e->stagger = getenv("P3HIP_STAGGER") ? atoi(getenv("P3HIP_STAGGER")) : -1;
  e->pair_turns = getenv("P3HIP_NO_PAIR_TURNS") == nullptr;
  e->direct_results = getenv("P3HIP_NO_DIRECT_RESULTS") == nullptr;
  e->time_run = getenv("P3HIP_TIME_RUN") != nullptr;
  e->blockw_diag = getenv("P3HIP_BLOCKW_DIAG") != nullptr;
  e->conv_any_env = getenv("P3HIP_CONV_ANY") != nullptr && atoi(getenv("P3HIP_CONV_ANY")) != 0;
  e->int8 = (flags & (P3HIP_FLAG_INT8 | P3HIP_FLAG_INT8_FUSED | P3HIP_FLAG_INT8_C128)) != 0;
  e->i8f = (flags & (P3HIP_FLAG_INT8_FUSED | P3HIP_FLAG_INT8_C128)) != 0;
  e->i8c128 = (flags & P3HIP_FLAG_INT8_C128) != 0;
  e->f32 = (flags & (P3HIP_FLAG_FP32 | P3HIP_FLAG_FP32_TFM)) != 0;
  e->sym = sym;
  e->rows = sym ? p3::kNumSyms * batch_size : batch_size;
  auto fail = [&](const std::string& m) {
    g_create_error = m;
    p3hip_destroy(e);
    return (p3hip_engine*)nullptr;
  };
  if (!e->wf.load(weights_path, e->err)) return fail(e->err);
  // host-side plan first (weight repacking; no HIP call): a bad file fails here, GPU or not
  Arena ar;
  if (!build_plan(e, ar)) return fail(e->err);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_ordinal)
    return fail("no HIP device " + std::to_string(device_ordinal) + " (the HIP engine has no CPU fallback)");
  if (!e->check(hipSetDevice(device_ordinal), "hipSetDevice")) return fail(e->err);
  hipDeviceProp_t prop;
  if (!e->check(hipGetDeviceProperties(&prop, device_ordinal), "hipGetDeviceProperties")) return fail(e->err);
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(std::string("device is ") + prop.gcnArchName + ", this engine is built for gfx950 only");
  e->n_cu = prop.multiProcessorCount;
  const int C = e->wf.C;
  const size_t B = batch_size;
  const size_t R = e->rows;   // the per-row device buffers: 8 x batch copies with P3HIP_FLAG_SYMMETRY_AVG
  // t holds a C-channel tensor (broadcast blocks, classic blocks, the transformer's o) or, in a layer-wise btl / nbt block,
  // two C_b-channel ones side by side (enqueue_forward, regions 1 and 2): 2 C_b > C where C_b > C / 2 (P3HIP_CONV_SET
  // allows C_b up to C, and padding C_b to a multiple of 64 can pass C / 2 as well)
  const size_t Ct = (e->wf.btype == 0 || e->wf.btype == 1) ? std::max<size_t>(C, 2 * (size_t)e->wf.Cb) : (size_t)C;
  const size_t eb = e->f32 ? 4 : 2;   // bytes per activation element
  const size_t qkv_bytes = 3 * R * p3::kTfmLPad * (size_t)e->wf.model_C * eb;   // heads x head width = model width
  bool ok = e->check(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking), "hipStreamCreate") &&
            e->check(hipMalloc((void**)&e->d_arena, ar.host.size()), "hipMalloc arena") &&
            // on the engine's own stream: it is non-blocking (no implicit ordering with the null stream a plain
            // hipMemcpy / hipMemset runs on), and the first run must find the weights there
            e->check(hipMemcpyAsync(e->d_arena, ar.host.data(), ar.host.size(), hipMemcpyHostToDevice, e->stream), "upload weights") &&
            e->check(hipHostMalloc((void**)&e->h_feats, B * kFeatBytes, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&e->h_feats_compact, B * kFeatBytes, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&e->h_out, B * p3::kResultFloats * 4, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipMalloc((void**)&e->d_res, B * p3::kResultFloats * 4), "hipMalloc results") &&
            e->check(hipMalloc((void**)&e->d_feats, R * kFeatBytes), "hipMalloc feats") &&
            e->check(hipMalloc((void**)&e->d_x, R * C * kNLoc * eb), "hipMalloc x") &&
            e->check(hipMalloc((void**)&e->d_t, R * Ct * kNLoc * eb), "hipMalloc t") &&
            e->check(hipMalloc((void**)&e->d_u, R * C * kNLoc * eb), "hipMalloc u") &&
            // (d_s is the fused nbt kernel's scratch; the fp32 plan runs layer by layer and has none)
            (e->wf.btype != 1 || e->f32 || e->check(hipMalloc((void**)&e->d_s, R * e->wf.Cb * kNLoc * 2), "hipMalloc s")) &&
            (!e->tfm || e->check(hipMalloc((void**)&e->d_qkv, qkv_bytes), "hipMalloc qkv")) &&
            e->check(hipMalloc((void**)&e->d_hp, R * 96 * kNLoc * 4), "hipMalloc hp") &&
            e->check(hipMalloc((void**)&e->d_out, B * p3::kOutStride * 4), "hipMalloc out") &&
            (!sym || (e->check(hipMalloc((void**)&e->d_sfeats, B * kFeatBytes), "hipMalloc symmetry upload") &&
                      e->check(hipMalloc((void**)&e->d_cout, R * p3::kOutStride * 4), "hipMalloc copy rows"))) &&
            (!e->int8 || (e->check(hipMalloc((void**)&e->d_amax, (size_t)e->n_q * 4), "hipMalloc amax") &&
                          e->check(hipMalloc((void**)&e->d_ascale, (size_t)e->n_q * 4), "hipMalloc scales") &&
                          e->check(hipMemsetAsync(e->d_amax, 0, (size_t)e->n_q * 4, e->stream), "hipMemset amax") &&
                          e->check(hipMemsetAsync(e->d_ascale, 0, (size_t)e->n_q * 4, e->stream), "hipMemset scales")));
  if (!ok) return fail(e->err);
  e->h_scale.assign(e->n_q, 0.0f);
  memset(e->h_feats, 0, B * kFeatBytes);
  if (!e->check(hipMemsetAsync(e->d_feats, 0, R * kFeatBytes, e->stream), "hipMemset feats") ||
      (sym && !e->check(hipMemsetAsync(e->d_sfeats, 0, B * kFeatBytes, e->stream), "hipMemset symmetry upload")) ||
      (sym && !e->check(hipMemsetAsync(e->d_cout, 0, R * p3::kOutStride * 4, e->stream), "hipMemset copy rows")) ||
      (e->tfm && !e->check(hipMemsetAsync(e->d_qkv, 0, qkv_bytes, e->stream), "hipMemset qkv")) ||
      !e->check(hipMemsetAsync(e->d_out, 0, B * p3::kOutStride * 4, e->stream), "hipMemset out") ||
      !e->check(hipStreamSynchronize(e->stream), "upload sync")) return fail(e->err);
  e->slots = p3::SlotStates((int)B);
  e->slot_sym.assign(B, 0);
  e->row_sym.assign(B, 0);
  return e;
}

void p3hip_destroy(p3hip_engine* e) {
  if (!e) return;
  if (e->stream || e->d_arena) (void)hipSetDevice(e->device);
  if (e->stream) hipStreamSynchronize(e->stream);
  hipFree(e->d_arena); hipFree(e->d_feats); hipFree(e->d_x); hipFree(e->d_t); hipFree(e->d_u); hipFree(e->d_s);
  hipFree(e->d_hp); hipFree(e->d_out); hipFree(e->d_res); hipFree(e->d_qkv);
  hipFree(e->d_sfeats); hipFree(e->d_cout);
  hipFree(e->d_bw_stamps);
  hipFree(e->d_amax); hipFree(e->d_ascale);
  if (e->bw_mod) hipModuleUnload(e->bw_mod);
  free_cache(e->cache);
  if (e->h_feats) hipHostFree(e->h_feats);
  if (e->h_feats_compact) hipHostFree(e->h_feats_compact);
  if (e->h_out) hipHostFree(e->h_out);
  for (hipEvent_t ev : e->blk_ev) hipEventDestroy(ev);
  drop_graph(e);
  if (e->stream) hipStreamDestroy(e->stream);
  delete e;
}

int p3hip_kind(const p3hip_engine*) { return P3HIP_KIND_HIP; }
const char* p3hip_path(const p3hip_engine* e) { return e->path.c_str(); }
int p3hip_batch_size(const p3hip_engine* e) { return e->batch; }
const char* p3hip_last_error(const p3hip_engine* e) { return e->err.c_str(); }

int p3hip_load_slot(p3hip_engine* e, int slot, const p3hip_features* f) {
  if (slot < 0 || slot >= e->batch) return 1;
  memcpy(e->h_feats + (size_t)slot * kFeatBytes, f, kFeatBytes);
  e->slot_sym[slot] = 0;
  if (e->cache.on) e->cache.h_slot_keys[slot] = p3::CacheKey{0, 0, 0};   // no key: evaluated, never cached
  e->slots.loaded(slot);
  return 0;
}

int p3hip_load_slot_keyed(p3hip_engine* e, int slot, const p3hip_features* f, uint64_t key_lo, uint64_t key_hi, int symmetry) {
  if (slot < 0 || slot >= e->batch) return 1;
  if (symmetry < 0 || symmetry > 7) return 1;
  memcpy(e->h_feats + (size_t)slot * kFeatBytes, f, kFeatBytes);
  e->slot_sym[slot] = (unsigned char)symmetry;
  if (e->cache.on) e->cache.h_slot_keys[slot] = p3::CacheKey{key_lo, key_hi, (unsigned long long)symmetry};
  e->slots.loaded(slot);
  return 0;
}

int p3hip_cache_enable(p3hip_engine* e, int log2_entries) {
  if (!e->bind()) return 1;
  if (e->cache.on) { e->err = "cache already enabled"; return 1; }
  if (log2_entries < 4 || log2_entries > 26) { e->err = "cache size: 2^4 .. 2^26 entries"; return 1; }
  auto& c = e->cache;
  const size_t cap = (size_t)1 << log2_entries, B = (size_t)e->batch;
  bool ok = e->check(hipMalloc((void**)&c.d_tkeys, cap * 16), "hipMalloc cache keys") &&
            e->check(hipMalloc((void**)&c.d_tmeta, cap * 4), "hipMalloc cache meta") &&
            e->check(hipMalloc((void**)&c.d_tvals, cap * p3::kOutStride * 4), "hipMalloc cache records") &&
            e->check(hipMalloc((void**)&c.d_keys, B * sizeof(p3::CacheKey)), "hipMalloc") &&
            e->check(hipMalloc((void**)&c.d_hit, B * 4), "hipMalloc") && e->check(hipMalloc((void**)&c.d_victim, B * 4), "hipMalloc") &&
            e->check(hipMalloc((void**)&c.d_lists, 5 * B * 4), "hipMalloc") && e->check(hipMalloc((void**)&c.d_sym, B * 4), "hipMalloc") &&
            e->check(hipMalloc((void**)&c.d_feats2, B * kFeatBytes), "hipMalloc") &&
            e->check(hipHostMalloc((void**)&c.h_keys, B * sizeof(p3::CacheKey), hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&c.h_hit, B * 4, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&c.h_victim, B * 4, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&c.h_lists, 5 * B * 4, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&c.h_sym, B * 4, hipHostMallocDefault), "hipHostMalloc") &&
            // (the engine's stream, as in p3hip_create: the table must be empty before the first probe kernel)
            e->check(hipMemsetAsync(c.d_tkeys, 0, cap * 16, e->stream), "hipMemset") &&
            e->check(hipMemsetAsync(c.d_tmeta, 0, cap * 4, e->stream), "hipMemset") &&
            e->check(hipStreamSynchronize(e->stream), "cache table sync");
  if (!ok) {
    // free what was allocated (an over-large table fails at the records): a later, smaller enable starts clean
    const std::string why = e->err;
    free_cache(c);
    (void)hipGetLastError();   // the failed allocation's sticky error
    e->err = why;
    return 1;
  }
  c.h_slot_keys = new p3::CacheKey[B]();
  c.out_row.assign(B, -1);
  c.was_hit.assign(B, 0);
  c.mask = (unsigned)(cap - 1);
  c.run = 0;
  c.on = true;
  return 0;
}

int p3hip_cache_stats(const p3hip_engine* e, uint64_t out[4]) {
  out[0] = e->cache.lookups; out[1] = e->cache.hits; out[2] = e->cache.inserts; out[3] = e->cache.on ? (uint64_t)e->cache.mask + 1 : 0;
  return e->cache.on ? 0 : 1;
}

// Compacts every dirty slot (loaded and not yet fetched, slot_state.h) into the dense upload.
static int gather_loaded(p3hip_engine* e) {
  const bool all = (e->flags & P3HIP_FLAG_RUN_ALL_SLOTS) != 0;
  // When every slot of the static batch is evaluated (the common case: NNInterface fills the whole batch, the self-play
  // scheduler always does) the dense upload IS h_feats: no second host copy of 1.9 MB per run.
  std::vector<std::pair<int, int>> moved;
  bool identity = true;
  const int n = e->slots.gather(all, [&](int s, int row) {
    if (s != row) identity = false;
    moved.emplace_back(s, row);
    e->row_sym[row] = e->slot_sym[s];
    if (e->cache.on) {
      e->cache.h_keys[row] = e->cache.h_slot_keys[s];
      e->cache.out_row[row] = row;   // p3hip_run re-maps (misses first, then hits)
      e->cache.was_hit[row] = 0;
      e->cache.h_sym[row] = (unsigned)e->cache.h_slot_keys[s].sym;
    }
  });
  e->feats_identity = identity && n == e->batch && !e->cache.on;
  if (!e->feats_identity)
    for (const auto& m : moved)
      memcpy(e->h_feats_compact + (size_t)m.second * kFeatBytes, e->h_feats + (size_t)m.first * kFeatBytes, kFeatBytes);
  e->last_n = n;
  return n;
}

// An INT8 engine runs only once it has activation scales (the reference refuses --use_int8 without a calibration set);
// every entry point that enqueues a forward pass checks it
static bool int8_ready(p3hip_engine* e) {
  if (!e->int8 || e->calibrating || e->have_scales) return true;
  e->err = "INT8 engine has no activation scales: run p3hip_int8_calibrate on calibration batches or load a saved "
           "calibration with p3hip_int8_set_scales first";
  return false;
}

int p3hip_int8_calibrate(p3hip_engine* e) {
  if (!e->int8) { e->err = "p3hip_int8_calibrate: the engine was not created with P3HIP_FLAG_INT8"; return 1; }
  if (!e->bind()) return 1;
  e->calibrating = true;
  e->last_n = 0;
  const int rc = p3hip_run(e);
  e->calibrating = false;
  if (rc != 0) return rc;
  if (e->last_n <= 0) { e->err = "p3hip_int8_calibrate: no loaded positions to calibrate on"; return 1; }
  std::vector<unsigned> bits(e->n_q);
  if (!e->check(hipMemcpyAsync(bits.data(), e->d_amax, (size_t)e->n_q * 4, hipMemcpyDeviceToHost, e->stream), "D2H amax") ||
      !e->check(hipStreamSynchronize(e->stream), "sync")) return 1;
  for (int i = 0; i < e->n_q; ++i) {
    float m;
    memcpy(&m, &bits[i], 4);
    e->h_scale[i] = m / 127.0f;
  }
  if (!e->check(hipMemcpyAsync(e->d_ascale, e->h_scale.data(), (size_t)e->n_q * 4, hipMemcpyHostToDevice, e->stream), "H2D scales") ||
      !e->check(hipStreamSynchronize(e->stream), "sync")) return 1;
  e->have_scales = true;
  return 0;
}

int p3hip_int8_scales(const p3hip_engine* e, float* out, int n) {
  if (!e->int8) return -1;
  for (int i = 0; i < n && i < e->n_q; ++i) out[i] = e->h_scale[i];
  return e->n_q;
}

int p3hip_int8_set_scales(p3hip_engine* e, const float* scales, int n) {
  if (!e->int8) { e->err = "p3hip_int8_set_scales: the engine was not created with P3HIP_FLAG_INT8"; return 1; }
  if (n != e->n_q) {
    e->err = "p3hip_int8_set_scales: " + std::to_string(n) + " scales given, the engine has " + std::to_string(e->n_q) +
             " quantized tensors";
    return 1;
  }
  for (int i = 0; i < n; ++i)
    if (!(scales[i] >= 0.0f) || !std::isfinite(scales[i])) { e->err = "p3hip_int8_set_scales: bad scale"; return 1; }
  if (!e->bind()) return 1;
  // the running maxima restart from the loaded calibration: a later p3hip_int8_calibrate widens it
  std::vector<float> amax(n);
  for (int i = 0; i < n; ++i) { e->h_scale[i] = scales[i]; amax[i] = scales[i] * 127.0f; }
  if (!e->check(hipMemcpyAsync(e->d_ascale, e->h_scale.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream), "H2D scales") ||
      !e->check(hipMemcpyAsync(e->d_amax, amax.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream), "H2D amax") ||
      !e->check(hipStreamSynchronize(e->stream), "sync")) return 1;
  e->have_scales = true;
  return 0;
}

int p3hip_upload(p3hip_engine* e) {
  if (!e->bind()) return 1;
  int n = gather_loaded(e);
  if (n == 0) return 0;
  return upload(e, n) && e->check(hipStreamSynchronize(e->stream), "sync") ? 0 : 1;
}

int p3hip_forward_resident(p3hip_engine* e, int n_positions) {
  if (n_positions < 1 || n_positions > e->batch || !e->bind() || !int8_ready(e)) return 1;
  return run_pass(e, Pass{upload_buffer(e), n_positions, e->d_out}) ? 0 : 1;
}

int p3hip_sync(p3hip_engine* e) { return e->bind() && e->check(hipStreamSynchronize(e->stream), "sync") ? 0 : 1; }

// p3hip_run with the cache on: probe, evaluate the misses only, fill the hits from the table, store the misses.
// d_out / h_out rows: the misses first (in row order), then the hits (in row order); cache.out_row maps.
static int run_cached(p3hip_engine* e, int n) {
  auto& c = e->cache;
  hipStream_t s = e->stream;
  const size_t B = (size_t)e->batch;
  ++c.run;
  if (!upload(e, n) ||   // (the cache's runs are never feats_identity: the upload comes from h_feats_compact)
      !e->check(hipMemcpyAsync(c.d_keys, c.h_keys, (size_t)n * sizeof(p3::CacheKey), hipMemcpyHostToDevice, s), "H2D keys")) return 1;
  p3::CacheArgs a{};
  a.keys = c.d_keys; a.n = n; a.tkeys = c.d_tkeys; a.tmeta = c.d_tmeta; a.tvals = c.d_tvals; a.mask = c.mask; a.run = c.run;
  a.hit = c.d_hit; a.victim = c.d_victim; a.out = e->d_out; a.out_sym = c.d_sym;
  if (!e->check(p3::launch_cache_probe(a, s), "launch k_cache_probe") ||
      !e->check(hipMemcpyAsync(c.h_hit, c.d_hit, (size_t)n * 4, hipMemcpyDeviceToHost, s), "D2H hits") ||
      !e->check(hipMemcpyAsync(c.h_victim, c.d_victim, (size_t)n * 4, hipMemcpyDeviceToHost, s), "D2H victims") ||
      !e->check(hipStreamSynchronize(s), "sync")) return 1;
  int* miss_rows = c.h_lists;
  int* hit_idx = c.h_lists + B;
  int* ins_rows = c.h_lists + 2 * B;
  int* ins_src = c.h_lists + 3 * B;
  int* ins_idx = c.h_lists + 4 * B;
  int nm = 0, nh = 0, ni = 0;
  for (int r = 0; r < n; ++r) nm += c.h_hit[r] < 0;
  int mi = 0, hi = 0;
  // entries this run reads (hits) or has already given to an insert: one writer per entry, no reader evicted
  std::unordered_set<int> claimed;
  for (int r = 0; r < n; ++r) if (c.h_hit[r] >= 0) claimed.insert(c.h_hit[r]);
  for (int r = 0; r < n; ++r) {
    const bool keyed = (c.h_keys[r].lo | c.h_keys[r].hi) != 0;
    c.lookups += keyed;
    if (c.h_hit[r] >= 0) {
      c.was_hit[r] = 1;
      c.out_row[r] = nm + hi;
      hit_idx[hi++] = c.h_hit[r];
      ++c.hits;
    } else {
      c.was_hit[r] = 0;
      c.out_row[r] = mi;
      c.h_sym[mi] = (unsigned)c.h_keys[r].sym;
      miss_rows[mi] = r;
      const int v = c.h_victim[r];
      if (keyed && v >= 0 && claimed.insert(v).second) {
        ins_rows[ni] = r; ins_src[ni] = mi; ins_idx[ni] = v; ++ni;
      }
      ++mi;
    }
  }
  nh = hi;
  if (!e->check(hipMemcpyAsync(c.d_lists, c.h_lists, 5 * B * 4, hipMemcpyHostToDevice, s), "H2D lists")) return 1;
  if (nm > 0) {
    a.rows = c.d_lists; a.m = nm; a.feats_in = upload_buffer(e); a.feats_out = c.d_feats2;
    // the misses are evaluated into their d_out rows 0 .. nm - 1 (symmetry averaging: expanded, evaluated and reduced)
    if (!e->check(p3::launch_cache_gather(a, s), "launch k_cache_gather") || !run_pass(e, Pass{c.d_feats2, nm, e->d_out}))
      return 1;
  }
  if (nh > 0) {
    a.idx = c.d_lists + B; a.m = nh; a.out_row0 = nm;
    if (!e->check(p3::launch_cache_fill(a, s), "launch k_cache_fill")) return 1;
  }
  if (ni > 0) {
    a.rows = c.d_lists + 2 * B; a.src = c.d_lists + 3 * B; a.idx = c.d_lists + 4 * B; a.m = ni;
    if (!e->check(p3::launch_cache_insert(a, s), "launch k_cache_insert")) return 1;
    c.inserts += ni;
  }
  if (!download(e, n, nullptr)) return 1;
  if (nh > 0 && !e->check(hipMemcpyAsync(c.h_sym + nm, c.d_sym + nm, (size_t)nh * 4, hipMemcpyDeviceToHost, s), "D2H symmetries")) return 1;
  return e->check(hipStreamSynchronize(s), "sync") ? 0 : 1;
}

int p3hip_run(p3hip_engine* e) {
  if (!e->bind() || !int8_ready(e)) return 1;
  int n = gather_loaded(e);
  if (n == 0) return 0;
  if (e->cache.on && !e->calibrating) return run_cached(e, n);   // calibration evaluates every slot, stores nothing
  if (!upload(e, n)) return 1;
  // The heads kernel writes the result records (the first kResultFloats of an output row) a second time into a dense
  // device buffer (HeadsArgs::res), so the copy TrtEngineImpl::RunInference queues behind its graph (trt_engine.cc:283-297)
  // is one contiguous 7.7 MB transfer at the link's rate; the strided copy of rounds 1-3 (1024 rows of 7,556 B out of a
  // 13,664 B pitch) took 0.45 ms, and 4-byte stores straight into host memory from the kernel took as long (round 4,
  // gpurun_out/r4d/breakdown.log).  P3HIP_NO_DIRECT_RESULTS=1: the strided copy (A/B, tests).
  // P3HIP_TIME_RUN=1 (tools/gpu_run_breakdown.py): the stream is drained after every stage and the stages' wall times are
  // summed into the engine's error string on request — a measurement aid, never set in production
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto t_start = now();
  if (e->time_run) {
    hipStreamSynchronize(e->stream);
    e->t_h2d += std::chrono::duration<double>(now() - t_start).count();
    t_start = now();
  }
  const Pass p{upload_buffer(e), n, e->d_out, e->direct_results ? e->d_res : nullptr};   // symmetry: k_sym_reduce fills d_res
  const bool ok = run_pass(e, p);
  if (e->time_run) {
    hipStreamSynchronize(e->stream);
    e->t_fwd += std::chrono::duration<double>(now() - t_start).count();
    t_start = now();
  }
  if (!ok || !download(e, n, p.res)) return 1;
  const bool sync_ok = e->check(hipStreamSynchronize(e->stream), "sync");
  if (e->time_run) {
    e->t_d2h += std::chrono::duration<double>(now() - t_start).count();
    ++e->t_runs;
    char buf[200];
    snprintf(buf, sizeof buf, "timing: runs %ld  h2d %.1f us  forward %.1f us  d2h %.1f us", e->t_runs, e->t_h2d / e->t_runs * 1e6,
             e->t_fwd / e->t_runs * 1e6, e->t_d2h / e->t_runs * 1e6);
    e->err = buf;
  }
  return sync_ok ? 0 : 1;
}

int p3hip_get_slot(p3hip_engine* e, int slot, p3hip_result* out) {
  if (slot < 0 || slot >= e->batch) return 1;
  int row = e->out_row_of(slot);
  if (row < 0) return 2;
  const float* r = e->h_out + (size_t)row * p3::kResultFloats;
  memcpy(out->move_logits, r + p3::kOffMoveLogits, 362 * 4);
  memcpy(out->move_probs, r + p3::kOffMoveProbs, 362 * 4);
  memcpy(out->value_probs, r + p3::kOffValueProbs, 2 * 4);
  memcpy(out->score_probs, r + p3::kOffScoreProbs, 800 * 4);
  memcpy(out->opt_move_probs, r + p3::kOffOptProbs, 362 * 4);
  out->err2_outcome = r[p3::kOffErr2];
  e->slots.fetched(slot);
  return 0;
}

int p3hip_get_slot_keyed(p3hip_engine* e, int slot, p3hip_result* out, int* symmetry, int* from_cache) {
  if (slot < 0 || slot >= e->batch) return 1;
  const int row = e->slots.row(slot), orow = e->out_row_of(slot);
  if (row < 0) return 2;
  if (symmetry) *symmetry = e->cache.on ? (int)e->cache.h_sym[orow] : (int)e->row_sym[row];
  if (from_cache) *from_cache = e->cache.on ? e->cache.was_hit[row] : 0;
  return p3hip_get_slot(e, slot, out);
}

int p3hip_get_ownership(p3hip_engine* e, int slot, float out[P3HIP_NUM_LOCS]) {
  if (slot < 0 || slot >= e->batch) return 1;
  int row = e->out_row_of(slot);
  if (row < 0) return 2;
  if (!e->bind()) return 1;
  if (!e->check(hipMemcpy(out, e->d_out + (size_t)row * p3::kOutStride + p3::kOffOwnership,
                          kNLoc * 4, hipMemcpyDeviceToHost), "D2H ownership")) return 1;
  e->slots.fetched(slot);
  return 0;
}

int p3hip_get_raw(p3hip_engine* e, int slot, float* out) {
  if (slot < 0 || slot >= e->batch) return 1;
  int row = e->out_row_of(slot);
  if (row < 0) return 2;
  std::vector<float> rec(p3::kOutStride);
  if (!e->bind()) return 1;
  if (!e->check(hipMemcpy(rec.data(), e->d_out + (size_t)row * p3::kOutStride, p3::kOutStride * 4,
                          hipMemcpyDeviceToHost), "D2H raw")) return 1;
  memcpy(out, rec.data() + p3::kOffMoveLogits, 362 * 4);
  memcpy(out + 362, rec.data() + p3::kOffOptLogits, 362 * 4);
  memcpy(out + 724, rec.data() + p3::kOffOutcomeLogits, 2 * 4);
  memcpy(out + 726, rec.data() + p3::kOffScoreLogits, 800 * 4);
  memcpy(out + 1526, rec.data() + p3::kOffOwnership, 361 * 4);
  out[1887] = rec[p3::kOffErr2];
  out[1888] = rec[p3::kOffGamma];
  return 0;
}

void p3hip_flops_per_position(const p3hip_engine* e, double* total, double* conv3x3) {
  const WeightFile& w = e->wf;
  const double C = w.model_C, Cb = w.model_Cb, H = w.H, V = w.V, L = kNLoc;
  double mac = L * 25 * 15 * C + 8 * C, mac3 = 0;
  for (int i = 0; i < w.nblocks; ++i) {
    if (e->tfm) mac += L * 4 * C * C + 2 * L * L * C + L * 3 * C * 2 * C;   // q k v o, q.k^T and p.v, SwiGLU
    else if (w.is_broadcast(i)) mac += L * 2 * C * C + C * L * L;
    else if (w.btype == 0) { mac += L * 2 * C * Cb; mac3 += L * w.inner * 9 * Cb * Cb; }
    else if (w.btype == 1) { mac += L * 2 * C * Cb; mac3 += L * 4 * 9 * Cb * Cb; }
    else { mac3 += L * w.inner * 9 * C * C; }
  }
  mac += L * 3 * C * H + L * H * 5 + 2 * H * H + 2 * H * 4 + 2 * H * V * 2 + V * (14 + 51 + 1) +
         (2 * H + 1) * V + 800 * V;
  if (total) *total = 2.0 * (mac + mac3);
  if (conv3x3) *conv3x3 = 2.0 * mac3;
}

double p3hip_time_trunk_kernel(p3hip_engine* e, int n_positions, int iters,
                               double* flops_per_launch, const char** kernel_name) {
  const WeightFile& wf = e->wf;
  const BlockPlan* bp = nullptr;
  int nfused = 0, n3x3 = 0, c3 = 0, nlw = 0;
  for (const BlockPlan& b : e->blocks) {
    if (b.kind == 0 || b.kind == 1) { if (!bp) bp = &b; ++nfused; }   // fused block kernel
    if (b.kind == 4) {
      ++nlw;
      for (const LayerPlan& lp : b.layers)
        if (lp.kw == 3) { ++n3x3; c3 = lp.cin; }
    }
  }
  if (n_positions < 1 || n_positions > e->batch || iters < 1 || !e->bind() || !int8_ready(e)) return -1.0;
  // The timed kernel (enqueue_forward records an event pair around each of its launches) and its launches per forward
  // pass: the attention kernel k_tfm_attn of transformer trunks, the fused block kernel, or else the 3x3 layer conv
  // k_lconv<3, ..> of layer-wise trunks (C = 384, classic)
  // (P3HIP_FLAG_INT8_FUSED, P3HIP_FLAG_INT8_C128: k_block_i8, one launch per btl block)
  const int per_pass = e->tfm ? wf.nblocks : (bp ? nfused : (e->i8f ? nlw : n3x3));
  if (per_pass == 0) return -1.0;
  if (e->sym) {
    // symmetry averaging: the trunk runs over the k copies of the resident slots (p3hip_upload put them in d_sfeats)
    if (!expand_sym(e, e->d_sfeats, n_positions)) return -1.0;
    n_positions *= e->sym_k;
  }
  while ((int)e->blk_ev.size() < 2 * per_pass) {
    hipEvent_t ev;
    if (!e->check(hipEventCreate(&ev), "hipEventCreate")) return -1.0;
    e->blk_ev.push_back(ev);
  }
  // Time the kernel where it runs: whole forward passes over the resident batch, with a HIP event pair (on the engine's
  // stream) around each timed launch.  The average over all launches is what rocprofv3 --kernel-trace --stats reports
  // for the same run.
  Pass p{e->d_feats, n_positions, e->sym ? e->d_cout : e->d_out};
  if (!enqueue_forward(e, p)) return -1.0;   // warm-up
  double total_ms = 0.0;
  long launches = 0;
  for (int i = 0; i < iters; ++i) {
    int timed = 0;
    p.timed = &timed;
    if (!enqueue_forward(e, p) || !e->check(hipStreamSynchronize(e->stream), "sync")) return -1.0;
    for (int b = 0; b < timed; ++b, ++launches) {
      float ms = 0;
      hipEventElapsedTime(&ms, e->blk_ev[2 * b], e->blk_ev[2 * b + 1]);
      total_ms += ms;
    }
  }
  double flops = 0.0;
  const char* name = nullptr;
  if (e->tfm) {
    // q.k^T and p.v over the 361 x 361 tokens of every head (algorithmic, not the padded 384 keys)
    flops = 2.0 * n_positions * 2.0 * kNLoc * kNLoc * wf.model_C;
    name = e->f32 ? p3::tfm_attn_f32_kernel_name() : "k_tfm_attn";
  } else if (e->i8f) {
    // every conv of one btl block, as for the fp16 block launch below
    flops = 2.0 * n_positions * kNLoc * (wf.inner * 9.0 * wf.Cb * wf.Cb + 2.0 * wf.C * wf.Cb);
    name = e->i8c128 ? p3::block_i8_c128_kernel_name() : p3::block_i8_kernel_name();
  } else if (!bp) {
    // (conv_any: the file's own width, not the padded one the kernel runs)
    const double w3 = (e->conv_any || e->f32) ? (wf.btype == 2 ? wf.model_C : wf.model_Cb) : c3;
    flops = 2.0 * n_positions * kNLoc * 9.0 * w3 * w3;
    name = e->f32 ? p3::lconv_f32_kernel_name(3) : e->int8 ? p3::lconv_i8_kernel_name(3, c3, c3)
                   : (e->conv_any ? p3::lconv_any_kernel_name(3) : (c3 == 192 ? "k_lconv<3,192,192>" : "k_lconv<3,64,64>"));
  } else {
    const double n3 = (wf.btype == 0) ? wf.inner : 4;
    // every conv the block kernel executes: the inner 3x3s plus the 1x1 reduce and expand
    // a launch covers `nfused / launches-per-forward` blocks on average
    const double blocks_per_launch = launches ? (double)nfused * iters / launches : 1.0;
    // plus the broadcast blocks' C -> C convs that ride in the block launches
    int nbconv = 0;
    for (const BlockPlan& b : e->blocks) nbconv += (b.head_of >= 0) + (b.tail_of >= 0);
    const double bconv_per_launch = launches ? (double)nbconv * iters / launches : 0.0;
    // ... and their dense where it rides in the tail (algorithmic 361 x 361 per channel, not the padded K = 384)
    int ndense = 0;
    for (const BlockPlan& b : e->blocks) ndense += b.kind == 3 && b.first_fused && b.dense_fused;
    const double dense_per_launch = launches ? (double)ndense * iters / launches : 0.0;
    flops = 2.0 * n_positions * kNLoc *
            (blocks_per_launch * (n3 * 9.0 * wf.Cb * wf.Cb + 2.0 * wf.C * wf.Cb) + bconv_per_launch * (double)wf.C * wf.C +
             dense_per_launch * (double)wf.C * kNLoc);
    name = e->blockw ? (wf.inner == 3 ? "k_blockw_L3" : wf.inner == 2 ? "k_blockw_L2" : "k_blockw_L1")
                     : p3::block_kernel_name(wf.C, bp->kind, wf.inner);
  }
  if (flops_per_launch) *flops_per_launch = flops;
  if (kernel_name) *kernel_name = name;
  return launches ? total_ms / launches : -1.0;
}

// debugging aid: the residual stream x of the last forward pass, n_positions x C x 361 fp16 in the device layout
// [pos][C / 8][361][8], as floats
int p3hip_debug_x(p3hip_engine* e, float* out, int n_positions) {
  if (e->sym) { e->err = "p3hip_debug_x: not available on a P3HIP_FLAG_SYMMETRY_AVG engine"; return 1; }
  if (!e->bind() || n_positions < 1 || n_positions > e->batch) return 1;
  const size_t n = (size_t)n_positions * e->wf.C * kNLoc;
  if (e->f32) {   // the fp32 stream has the same order: the stored values themselves
    hipStreamSynchronize(e->stream);
    return hipMemcpy(out, e->d_x, n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
  }
  std::vector<_Float16> h(n);
  hipStreamSynchronize(e->stream);
  if (hipMemcpy(h.data(), e->d_x, n * 2, hipMemcpyDeviceToHost) != hipSuccess) return 2;
  for (size_t i = 0; i < n; ++i) out[i] = (float)h[i];
  return 0;
}

// test hook: what the last transformer block that ran left in HBM, as floats.  which 0, 1, 2: q, k, v of d_qkv,
// [pos][head][384][D] with the 23 padding rows; 3: o of d_t, [pos][361][d].  Only reads; no launch, no allocation on the
// device.  The heads take d_t as scratch, so o is that of the last block only on an engine stopped in front of them
// (P3HIP_DEBUG_STOP_BLOCK = the block count, or any earlier block).
int p3hip_debug_tfm(p3hip_engine* e, int which, float* out, int n_positions) {
  if (!e->tfm || e->sym) { e->err = "p3hip_debug_tfm: only on a transformer engine without P3HIP_FLAG_SYMMETRY_AVG"; return 1; }
  if (which < 0 || which > 3) { e->err = "p3hip_debug_tfm: which must be 0 (q), 1 (k), 2 (v) or 3 (o)"; return 1; }
  if (n_positions < 1 || n_positions > e->last_npos) { e->err = "p3hip_debug_tfm: more positions than the last run had"; return 1; }
  if (!e->bind()) return 1;
  const size_t d = (size_t)e->wf.model_C;
  const size_t per = (size_t)e->rows * p3::kTfmLPad * d;
  const size_t n = (size_t)n_positions * (which < 3 ? p3::kTfmLPad : kNLoc) * d;
  hipStreamSynchronize(e->stream);
  if (e->f32) {   // the fp32 buffers have the same orders: the stored values themselves
    const float* src32 = which < 3 ? (const float*)e->d_qkv + which * per : (const float*)e->d_t;
    return hipMemcpy(out, src32, n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
  }
  const _Float16* src = which < 3 ? e->d_qkv + which * per : e->d_t;
  std::vector<_Float16> h(n);
  if (hipMemcpy(h.data(), src, n * 2, hipMemcpyDeviceToHost) != hipSuccess) return 2;
  for (size_t i = 0; i < n; ++i) out[i] = (float)h[i];
  return 0;
}

void p3hip_rope_table(double* cos_out, double* sin_out) { spiral_rope_table(32, cos_out, sin_out); }

int p3hip_rope_table_dim(int head_dim, double* cos_out, double* sin_out) {
  if (head_dim != 32 && head_dim != 64) return 1;
  spiral_rope_table(head_dim, cos_out, sin_out);
  return 0;
}

void p3hip_symmetry_maps(uint16_t fwd[8][361], uint16_t inv[8][361]) { p3::sym_maps(fwd, inv); }

int p3hip_set_symmetries(p3hip_engine* e, uint32_t mask) {
  if (!e->sym) { e->err = "p3hip_set_symmetries: the engine was not created with P3HIP_FLAG_SYMMETRY_AVG"; return 1; }
  if (mask < 1 || mask > 255) { e->err = "p3hip_set_symmetries: the mask must be 1 .. 255 (bit s = symmetry s)"; return 1; }
  if (mask == e->sym_mask) return 0;
  if (!e->bind()) return 1;
  // the captured graph holds the old list in its kernel arguments: drop it.  The next full run goes out kernel by
  // kernel (a new k means new row counts, whose launchers may meet kernels for the first time), the one after is captured
  if ((e->graph_exec || e->graph) && !e->check(hipStreamSynchronize(e->stream), "sync")) return 1;
  drop_graph(e);
  e->graph_warm = false;
  e->sym_mask = mask;
  e->sym_k = p3::sym_list(mask, e->sym_syms);
  return 0;
}

int p3hip_blockw_stamps(p3hip_engine* e, unsigned long long* out, int n) {
  if (!e->bind() || !e->d_bw_stamps) return 1;
  constexpr int total = 8 * 16 * 4 * 24;
  hipStreamSynchronize(e->stream);
  return hipMemcpy(out, e->d_bw_stamps, (size_t)(n < total ? n : total) * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
}

#ifdef P3_DIAG
// diagnostic build only: the phase stamps of the last forward pass's launch P3DIAG_LAUNCH
int p3hip_debug_block_stamps(p3hip_engine* e, unsigned long long* out, int n) {
  if (!e->bind() || !e->d_stamps) return 1;
  constexpr int total = p3::kStampWgs * 8 * p3::kStampSections * p3::kStampSlots;
  hipStreamSynchronize(e->stream);
  return hipMemcpy(out, e->d_stamps, (size_t)(n < total ? n : total) * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
}
int p3hip_debug_block_spans(p3hip_engine* e, unsigned long long* out, int n) {
  if (!e->bind() || !e->d_spans) return 1;
  constexpr int total = p3::kSpanWgs * p3::kSpanSlots;
  hipStreamSynchronize(e->stream);
  return hipMemcpy(out, e->d_spans, (size_t)(n < total ? n : total) * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
}
#endif

}  // extern "C"
