// plan.cpp — choose_plan (which trunk path an engine runs, and every refusal) and build_plan (the weights of that path
// repacked into the arena image, one packer per block family).  No HIP runtime call.
#include "plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../include/p3hip.h"
#include "conv_any.h"
#include "conv_f32.h"
#include "conv_split.h"
#include "conv_wino.h"
#include "edge_split.h"
#include "graph_table.h"
#include "lconv_i8.h"
#include "transformer.h"
#include "transformer_f32.h"
#include "transformer_split.h"

namespace eng {

Options Options::from_env() {
  auto set = [](const char* n) { return getenv(n) != nullptr; };
  auto num = [](const char* n, int dflt) { return getenv(n) ? atoi(getenv(n)) : dflt; };
  Options o;
  o.c128_wg8 = set("P3HIP_C128_WG8");
  o.bcast_fuse = !set("P3HIP_NO_BFUSE");
  o.dense_fuse = !set("P3HIP_NO_DFUSE");
  o.heads_fuse = !set("P3HIP_NO_HFUSE");
  o.stop_block = num("P3HIP_DEBUG_STOP_BLOCK", -1);
  o.fuse = !set("P3HIP_NO_FUSE");
  o.join = o.fuse && !set("P3HIP_NO_JOIN");
  o.stagger = num("P3HIP_STAGGER", -1);
  o.pair_turns = !set("P3HIP_NO_PAIR_TURNS");
  o.direct_results = !set("P3HIP_NO_DIRECT_RESULTS");
  o.time_run = set("P3HIP_TIME_RUN");
  o.blockw = num("P3HIP_BLOCKW", 0) != 0;
  o.blockw_diag = set("P3HIP_BLOCKW_DIAG");
  o.conv_any = num("P3HIP_CONV_ANY", 0) != 0;
  if (const char* sp = getenv("P3HIP_SPLIT")) {
    char tail = 0;
    if (sscanf(sp, "%d,%d%c", &o.split_s, &o.split_t, &tail) != 2 || !p3::sconv_split_valid(o.split_s, o.split_t)) {
      o.split_s = o.split_t = 0;
      o.split_bad = true;
    }
  }
  if (const char* sp = getenv("P3HIP_TFM_SPLIT")) {
    char tail = 0;
    if (sscanf(sp, "%d,%d%c", &o.tfm_split_s, &o.tfm_split_t, &tail) != 2 || !p3::tfm_split_valid(o.tfm_split_s, o.tfm_split_t)) {
      o.tfm_split_s = o.tfm_split_t = 0;
      o.tfm_split_bad = true;
    }
  }
  if (const char* sp = getenv("P3HIP_EDGE_SPLIT")) {
    char tail = 0;
    if (strcmp(sp, "0") == 0) {
      o.edge_s = o.edge_d = o.edge_h = 1;
    } else if (sscanf(sp, "%d,%d,%d%c", &o.edge_s, &o.edge_d, &o.edge_h, &tail) != 3 || o.edge_s < 1 || o.edge_s > 8 ||
               !p3::edge_split_valid(64, 1, o.edge_d, o.edge_h)) {   // (s against the file's width: choose_plan)
      o.edge_s = o.edge_d = o.edge_h = 0;
      o.edge_bad = true;
    }
  }
  o.graph_cache = gt::capacity_from(getenv("P3HIP_GRAPH_CACHE"));
  if (o.graph_cache == 0) {
    o.graph_cache = gt::kDefaultCapacity;
    o.graph_cache_bad = true;
  }
  o.graph_min_seen = std::min(std::max(num("P3HIP_GRAPH_MIN_SEEN", gt::kMinSeen), gt::kMinSeen), 64);
  o.graph_max_rows = std::max(num("P3HIP_GRAPH_MAX_ROWS", gt::kDefaultMaxRows), 0);
  return o;
}

const char* path_name(Path p) {
  switch (p) {
    case Path::Refused: return "Refused";
    case Path::Fused: return "Fused";
    case Path::Blockw: return "Blockw";
    case Path::Layerwise: return "Layerwise";
    case Path::ConvAny: return "ConvAny";
    case Path::Int8: return "Int8";
    case Path::Int8Fused256: return "Int8Fused256";
    case Path::Int8Fused128: return "Int8Fused128";
    case Path::Int8Any: return "Int8Any";
    case Path::Int8Conv3: return "Int8Conv3";
    case Path::Winograd3: return "Winograd3";
    case Path::F32Conv: return "F32Conv";
    case Path::Split: return "Split";
    case Path::Tfm: return "Tfm";
    case Path::TfmF32: return "TfmF32";
    case Path::TfmSplit: return "TfmSplit";
  }
  return "?";
}

namespace {

// What kind of trunk a file holds, as far as the plans tell trunks apart
enum class Trunk {
  None,          // nothing the engine serves
  BlockShape,    // a k_block shape: btl or nbt at C = 256 / C_b = 128 or 128 / 64
  LconvShape,    // a templated k_lconv shape: C = 384 / C_b = 192 btl or nbt, classic C = 192 (b15c192_classic)
  OtherConv,     // every other conv trunk of P3HIP_CONV_SET, C and C_b padded to multiples of 64
  Transformer,   // a transformer of P3HIP_TRANSFORMER_SET whose heads the engine has
};

// The classification of a file, computed once, and the few other facts the refusals ask about
struct TrunkClass {
  Trunk trunk = Trunk::None;
  bool tfm_file = false;   // the header says transformer, served or not
  bool btl123 = false;     // btl blocks with 1, 2 or 3 inner layers
  bool in_set = false;     // a conv trunk of P3HIP_CONV_SET (a k_block or k_lconv shape with a broadcast block at every
                           // position is none, and runs all the same)
  bool hv_ok = false;      // H = 32 and V in {32, 48, 64, 80}
  bool classic = false;    // classic blocks: 3x3 convs only
};

TrunkClass classify(const WeightFile& wf) {
  const int C = wf.C, Cb = wf.Cb;
  TrunkClass t;
  t.tfm_file = wf.btype == 3;
  t.btl123 = wf.btype == 0 && wf.inner >= 1 && wf.inner <= 3;
  t.classic = wf.btype == 2;
  t.in_set = WeightFile::conv_set(wf.model_C, wf.model_Cb, wf.btype, wf.inner, wf.bint) && C % 64 == 0 &&
             (wf.btype == 2 || Cb % 64 == 0);
  t.hv_ok = wf.H == 32 && (wf.V == 32 || wf.V == 48 || wf.V == 64 || wf.V == 80);
  // a conv file whose widths were padded (WeightFile::pad_conv) never takes the plan of the shape it was padded to
  const bool exact = wf.model_C == C && wf.model_Cb == Cb;
  const bool bottleneck = wf.btype == 1 || t.btl123;
  if (exact && bottleneck && ((C == 256 && Cb == 128) || (C == 128 && Cb == 64))) t.trunk = Trunk::BlockShape;
  else if (exact && ((bottleneck && C == 384 && Cb == 192) || (wf.btype == 2 && wf.inner == 2 && C == 192))) t.trunk = Trunk::LconvShape;
  else if (t.in_set) t.trunk = Trunk::OtherConv;
  // transformer: the file's C is the model width d and Cb the head count (include/p3hip.h: d a multiple of 32,
  // 64 <= d <= 384, head width d / heads 32 or 64); the stream is padded to C = p3::tfm_stream_width(d), and V is what
  // the heads of that width serve (the fused heads at C = 128 / 256: {32, 48, 64}; the C = 384 heads: hv_ok's)
  else if (t.tfm_file && p3::tfm_supported(wf.model_C, Cb) && C == p3::tfm_stream_width(wf.model_C) &&
           (C == 384 || p3::heads_fusable(C, wf.V))) t.trunk = Trunk::Transformer;
  return t;
}

// What the precision flags ask for: one plan
struct Request {
  enum Kind { Fp16, Int8, Int8Fused, Int8C128, Int8Any, Int8Conv3, Winograd, Fp32, LowLatency, LowLatencyTfm } kind = Fp16;
  bool int8_any = false;   // P3HIP_FLAG_INT8_ANY was given (kind is the plan it chose)
  bool int8_conv3 = false;   // P3HIP_FLAG_INT8_CONV3 was given (a classic trunk: kind is Int8 or Int8Any, its whole plan)
  bool alone = true;       // Int8Fused, Int8C128: no other of the three INT8 flags beside it
  bool f32_conv = false, f32_tfm = false;   // Fp32: P3HIP_FLAG_FP32 serves the conv trunks, P3HIP_FLAG_FP32_TFM the
                                            // transformers; both together: whatever the trunk
  bool ll_tfm = false;     // LowLatency: P3HIP_FLAG_LOW_LATENCY_TFM stands beside P3HIP_FLAG_LOW_LATENCY (whatever the
                           // trunk); LowLatencyTfm is that flag alone, which serves the transformers only
  std::string clash;       // the flags cannot be combined: the refusal's text
};

// P3HIP_FLAG_INT8_ANY: a trunk one of the three other INT8 flags serves takes that flag's plan, bit-identical to the flag
// alone, and every other conv trunk the path of its own.  P3HIP_CONV_ANY=1 sends the templated layer-wise shapes there too.
Request::Kind int8_any_choice(const TrunkClass& t, int C, bool conv_any) {
  if (t.trunk == Trunk::LconvShape && !conv_any) return Request::Int8;
  if (t.trunk == Trunk::BlockShape && t.btl123) return C == 256 ? Request::Int8Fused : Request::Int8C128;
  return Request::Int8Any;
}

// The flags read once.  P3HIP_FLAG_LOW_LATENCY, then P3HIP_FLAG_LOW_LATENCY_TFM, then P3HIP_FLAG_INT8_ANY, then the fp32
// flags name the plan, and whatever else stands beside them is a clash; of the three other INT8 flags together INT8_C128 speaks, then INT8_FUSED.
Request read_request(uint32_t flags, const TrunkClass& t, int C, const Options& opt) {
  const uint32_t i8_three = flags & (P3HIP_FLAG_INT8 | P3HIP_FLAG_INT8_FUSED | P3HIP_FLAG_INT8_C128);
  const bool fp32_flag = (flags & (P3HIP_FLAG_FP32 | P3HIP_FLAG_FP32_TFM)) != 0;
  Request r;
  r.f32_conv = (flags & P3HIP_FLAG_FP32) != 0;
  r.f32_tfm = (flags & P3HIP_FLAG_FP32_TFM) != 0;
  if (flags & P3HIP_FLAG_WINOGRAD) {
    // (as P3HIP_FLAG_INT8_CONV3 below: the flag added last answers every set it stands in)
    r.kind = Request::Winograd;
    if (i8_three || (flags & (P3HIP_FLAG_INT8_ANY | P3HIP_FLAG_INT8_CONV3)))
      r.clash = "P3HIP_FLAG_WINOGRAD cannot be combined with P3HIP_FLAG_INT8, P3HIP_FLAG_INT8_FUSED, P3HIP_FLAG_INT8_C128, "
                "P3HIP_FLAG_INT8_ANY or P3HIP_FLAG_INT8_CONV3: its kernel runs in fp16";
    else if (fp32_flag)
      r.clash = "P3HIP_FLAG_WINOGRAD cannot be combined with P3HIP_FLAG_FP32 or P3HIP_FLAG_FP32_TFM: an engine runs one "
                "precision plan";
    else if (flags & (P3HIP_FLAG_LOW_LATENCY | P3HIP_FLAG_LOW_LATENCY_TFM))
      r.clash = "P3HIP_FLAG_WINOGRAD cannot be combined with P3HIP_FLAG_LOW_LATENCY or P3HIP_FLAG_LOW_LATENCY_TFM: it has no "
                "low-latency form";
  } else if (flags & P3HIP_FLAG_INT8_CONV3) {
    // (a flag set with this flag in it is this flag's to answer: it was added last, and the answers of every set without
    // it stay what they were)
    r.int8_conv3 = true;
    r.kind = !t.classic ? Request::Int8Conv3 : (t.trunk == Trunk::LconvShape && !opt.conv_any) ? Request::Int8 : Request::Int8Any;
    if (i8_three || (flags & P3HIP_FLAG_INT8_ANY))
      r.clash = "P3HIP_FLAG_INT8_CONV3 cannot be combined with P3HIP_FLAG_INT8, P3HIP_FLAG_INT8_FUSED, P3HIP_FLAG_INT8_C128 or "
                "P3HIP_FLAG_INT8_ANY: an engine runs one INT8 plan";
    else if (fp32_flag)
      r.clash = "P3HIP_FLAG_INT8_CONV3 cannot be combined with P3HIP_FLAG_FP32 or P3HIP_FLAG_FP32_TFM: an engine runs one "
                "precision plan";
    else if (flags & (P3HIP_FLAG_LOW_LATENCY | P3HIP_FLAG_LOW_LATENCY_TFM))
      r.clash = "P3HIP_FLAG_INT8_CONV3 cannot be combined with P3HIP_FLAG_LOW_LATENCY or P3HIP_FLAG_LOW_LATENCY_TFM: their "
                "kernels run in fp16";
  } else if (flags & P3HIP_FLAG_LOW_LATENCY) {
    r.kind = Request::LowLatency;
    r.ll_tfm = (flags & P3HIP_FLAG_LOW_LATENCY_TFM) != 0;
    if (i8_three || (flags & P3HIP_FLAG_INT8_ANY))
      r.clash = "P3HIP_FLAG_LOW_LATENCY cannot be combined with P3HIP_FLAG_INT8, P3HIP_FLAG_INT8_FUSED, P3HIP_FLAG_INT8_C128 or "
                "P3HIP_FLAG_INT8_ANY: its kernel runs in fp16";
    else if (fp32_flag)
      r.clash = "P3HIP_FLAG_LOW_LATENCY cannot be combined with P3HIP_FLAG_FP32 or P3HIP_FLAG_FP32_TFM: its kernel runs in fp16";
  } else if (flags & P3HIP_FLAG_LOW_LATENCY_TFM) {
    r.kind = Request::LowLatencyTfm;
    if (i8_three || (flags & P3HIP_FLAG_INT8_ANY))
      r.clash = "P3HIP_FLAG_LOW_LATENCY_TFM cannot be combined with P3HIP_FLAG_INT8, P3HIP_FLAG_INT8_FUSED, P3HIP_FLAG_INT8_C128 "
                "or P3HIP_FLAG_INT8_ANY: its kernels run in fp16";
    else if (fp32_flag)
      r.clash = "P3HIP_FLAG_LOW_LATENCY_TFM cannot be combined with P3HIP_FLAG_FP32 or P3HIP_FLAG_FP32_TFM: its kernels run in "
                "fp16";
  } else if (flags & P3HIP_FLAG_INT8_ANY) {
    r.kind = int8_any_choice(t, C, opt.conv_any);
    r.int8_any = true;
    if (i8_three)
      r.clash = "P3HIP_FLAG_INT8_ANY cannot be combined with P3HIP_FLAG_INT8, P3HIP_FLAG_INT8_FUSED or P3HIP_FLAG_INT8_C128: it "
                "chooses among their plans itself";
    else if (fp32_flag)
      r.clash = "P3HIP_FLAG_INT8_ANY cannot be combined with P3HIP_FLAG_FP32 or P3HIP_FLAG_FP32_TFM: an engine runs one "
                "precision plan";
  } else if (fp32_flag) {
    r.kind = Request::Fp32;
    if (i8_three)
      r.clash = std::string(r.f32_conv ? (r.f32_tfm ? "P3HIP_FLAG_FP32 | P3HIP_FLAG_FP32_TFM" : "P3HIP_FLAG_FP32") : "P3HIP_FLAG_FP32_TFM") +
                " cannot be combined with P3HIP_FLAG_INT8, P3HIP_FLAG_INT8_FUSED or P3HIP_FLAG_INT8_C128: an "
                "engine runs one precision plan";
  } else if (i8_three) {
    r.kind = (i8_three & P3HIP_FLAG_INT8_C128) ? Request::Int8C128 : (i8_three & P3HIP_FLAG_INT8_FUSED) ? Request::Int8Fused : Request::Int8;
    r.alone = (i8_three & (i8_three - 1)) == 0;
  }
  return r;
}

// The path of a request the refusals let through
Path path_of(const Request& r, const TrunkClass& t, const WeightFile& wf, const Options& opt) {
  if (t.trunk == Trunk::Transformer) {
    if (r.kind == Request::LowLatencyTfm || (r.kind == Request::LowLatency && r.ll_tfm)) return Path::TfmSplit;
    return r.kind == Request::Fp32 ? Path::TfmF32 : Path::Tfm;
  }
  switch (r.kind) {
    case Request::Fp32: return Path::F32Conv;
    case Request::LowLatency: return Path::Split;
    case Request::Int8Any: return Path::Int8Any;
    case Request::Int8Conv3: return Path::Int8Conv3;
    case Request::Winograd: return Path::Winograd3;
    case Request::Int8Fused: return Path::Int8Fused256;
    case Request::Int8C128: return Path::Int8Fused128;
    case Request::Int8: return Path::Int8;
    case Request::LowLatencyTfm:   // (refused on every conv trunk)
    case Request::Fp16: break;
  }
  if (t.trunk == Trunk::OtherConv || (t.trunk == Trunk::LconvShape && opt.conv_any)) return Path::ConvAny;
  if (t.trunk == Trunk::LconvShape) return Path::Layerwise;
  // k_blockw serves C = 256 / C_b = 128 btl trunks
  return (opt.blockw && wf.C == 256 && wf.btype == 0) ? Path::Blockw : Path::Fused;
}

}  // namespace

PlanChoice choose_plan(const WeightFile& wf, uint32_t flags, const Options& opt, std::string& err) {
  const int C = wf.C, Cb = wf.Cb;
  PlanChoice c;
  const TrunkClass t = classify(wf);
  const Request r = read_request(flags, t, C, opt);
  const Request::Kind k = r.kind;
  const Trunk tr = t.trunk;
  // Every refusal, in the order of precedence: the first that applies answers.  (A flag that names the plan first says
  // which trunks it serves, then what cannot stand beside it; a request has one kind, so the first four never compete.)
  const struct { bool applies; std::string text; } refusals[] = {
      // (the text is from before the transformers had a low-latency plan: P3HIP_FLAG_LOW_LATENCY_TFM's)
      {k == Request::LowLatency && t.tfm_file && !r.ll_tfm,
       "P3HIP_FLAG_LOW_LATENCY serves the conv trunks (" P3HIP_CONV_SET "); the transformer trunks (" P3HIP_TRANSFORMER_SET
       ") have no low-latency plan"},
      {k == Request::LowLatencyTfm && !t.tfm_file,
       "P3HIP_FLAG_LOW_LATENCY_TFM serves the transformer trunks only (" P3HIP_TRANSFORMER_SET "); the conv trunks have "
       "P3HIP_FLAG_LOW_LATENCY"},
      {k == Request::Winograd && t.tfm_file,
       "P3HIP_FLAG_WINOGRAD serves the conv trunks (" P3HIP_CONV_SET ") whose fp16 plan runs layer by layer; the "
       "transformer trunks (" P3HIP_TRANSFORMER_SET ") have no 3x3 convs"},
      {r.int8_conv3 && t.tfm_file,
       "P3HIP_FLAG_INT8_CONV3 serves the conv trunks (" P3HIP_CONV_SET ") whose fp16 plan runs layer by layer; the "
       "transformer trunks (" P3HIP_TRANSFORMER_SET ") have no INT8 plan"},
      {r.int8_any && t.tfm_file,
       "P3HIP_FLAG_INT8_ANY serves the conv trunks (" P3HIP_CONV_SET "); the transformer trunks (" P3HIP_TRANSFORMER_SET
       ") have no INT8 plan"},
      {k == Request::Fp32 && t.tfm_file && !r.f32_tfm,
       "P3HIP_FLAG_FP32 serves the conv trunks only (" P3HIP_CONV_SET "); the transformer trunks run in fp16, or in "
       "fp32 with P3HIP_FLAG_FP32_TFM"},
      {k == Request::Fp32 && !t.tfm_file && !r.f32_conv,
       "P3HIP_FLAG_FP32_TFM serves the transformer trunks only (" P3HIP_TRANSFORMER_SET "); the conv trunks have "
       "P3HIP_FLAG_FP32"},
      {!r.clash.empty(), r.clash},
      {(flags & P3HIP_FLAG_LAUNCH_GRAPH_ANY) && opt.graph_cache_bad,
       "P3HIP_FLAG_LAUNCH_GRAPH_ANY: P3HIP_GRAPH_CACHE must be a whole number of graphs from 1 to 1024 (default 64)"},
      {k == Request::LowLatency && !t.tfm_file && opt.split_bad,
       "P3HIP_FLAG_LOW_LATENCY: P3HIP_SPLIT must be \"S,T\" with S row strips of 1, 2 or 4 and output tiles of T = 16, 32 "
       "or 64 channels"},
      {(k == Request::LowLatencyTfm || (k == Request::LowLatency && t.tfm_file)) && opt.tfm_split_bad,
       "P3HIP_FLAG_LOW_LATENCY_TFM: P3HIP_TFM_SPLIT must be \"S,T\" with S query parts of 1, 2, 3 or 6 and T = 16, 32 or 64 "
       "tokens per workgroup"},
      {(k == Request::LowLatency || k == Request::LowLatencyTfm) &&
           (opt.edge_bad || (opt.edge_s && !p3::edge_split_valid(C, opt.edge_s, opt.edge_d, opt.edge_h))),
       "P3HIP_FLAG_LOW_LATENCY / P3HIP_FLAG_LOW_LATENCY_TFM: P3HIP_EDGE_SPLIT must be \"0\" or \"s,d,h\" with s = 1 or the "
       "stem's output passes (the stream's channels / 128, or / 64 where they are no multiple of 128), d = 1, 3 or 12 parts "
       "of the broadcast dense and h = 1, 4 or 8 parts of the heads"},
      // (INT8_ANY's own path runs the nbt k_block shapes layer by layer, as conv trunks of the set)
      {tr == Trunk::None || (k == Request::Int8Any && tr == Trunk::BlockShape && !t.in_set) || !t.hv_ok,
       "unsupported architecture for the HIP engine (need a conv trunk (" P3HIP_CONV_SET "), or a transformer "
       "trunk (" P3HIP_TRANSFORMER_SET "); H=32, V in {32,48,64,80} (transformer: V in {32,48,64}, and 80 at "
       "d > 256))"},
      {k == Request::Winograd && tr == Trunk::BlockShape,
       "P3HIP_FLAG_WINOGRAD serves the trunks whose fp16 plan runs layer by layer; the C = 256 / C_b = 128 and C = 128 / "
       "C_b = 64 btl and nbt trunks run the fused block kernel, and a layer-wise Winograd plan for them is not built"},
      {r.int8_conv3 && tr == Trunk::BlockShape,
       "P3HIP_FLAG_INT8_CONV3 serves the trunks whose fp16 plan runs layer by layer; the C = 256 / C_b = 128 and C = 128 / "
       "C_b = 64 btl and nbt trunks run the fused block kernel, which no layer-wise plan approaches: P3HIP_FLAG_INT8_FUSED, "
       "P3HIP_FLAG_INT8_C128 and P3HIP_FLAG_INT8_ANY serve them"},
      // (INT8_C128 answers every trunk it does not serve with its own message, the runtime-width conv trunks included)
      {k == Request::Int8C128 && !(r.alone && tr == Trunk::BlockShape && C == 128 && t.btl123),
       "INT8_C128 is available only for C = 128 / C_b = 64 trunks of btl blocks with 1, 2 or 3 inner layers "
       "(b12c128btl3, b10c128btl3, small and their kin, broadcast blocks at any interval), and not together with "
       "another INT8 flag; nbt trunks, the other widths (P3HIP_FLAG_INT8_FUSED serves C = 256 / C_b = 128 btl trunks, "
       "P3HIP_FLAG_INT8 the layer-wise trunks) and the transformer are not served"},
      {(k == Request::Int8 || k == Request::Int8Fused) && tr == Trunk::OtherConv,
       std::string(k == Request::Int8Fused ? "INT8_FUSED" : "INT8") + " is not available for this conv trunk: "
       "P3HIP_FLAG_INT8 serves C = 384 / C_b = 192 btl or nbt blocks and C = 192 classic blocks, P3HIP_FLAG_INT8_FUSED "
       "serves C = 256 / C_b = 128 btl blocks with 1, 2 or 3 inner layers, P3HIP_FLAG_INT8_C128 serves C = 128 / "
       "C_b = 64 btl blocks with 1, 2 or 3 inner layers; the other widths run in fp16 only"},
      {k == Request::Int8Fused && !(r.alone && tr == Trunk::BlockShape && C == 256 && t.btl123),
       "INT8_FUSED is available only for C = 256 / C_b = 128 trunks of btl blocks with 1, 2 or 3 inner layers "
       "(b12c256btl3 and its kin, broadcast blocks at any interval), and not together with P3HIP_FLAG_INT8; nbt and "
       "C = 128 trunks, the layer-wise trunks (P3HIP_FLAG_INT8 serves those) and the transformer are not served"},
      {k == Request::Int8 && tr != Trunk::LconvShape,
       "INT8 is available only for layer-wise trunks (C = 384 / C_b = 192 btl or nbt blocks, C = 192 classic "
       "blocks); this trunk runs fused block kernels or the transformer"},
  };
  for (const auto& refusal : refusals)
    if (refusal.applies) {
      err = refusal.text;
      return c;
    }
  c.path = path_of(r, t, wf, opt);
  c.any_width = (c.path == Path::Int8Conv3 || c.path == Path::Winograd3) && (tr == Trunk::OtherConv || opt.conv_any);
  // (layer-wise: p3::conv_any_slice(C) = 64 at classic C = 192 and at INT8_C128's C = 128, 128 at C = 384 and at
  // INT8_FUSED's C = 256)
  c.CB = is_layerwise(c.path) ? p3::conv_any_slice(C) : (is_tfm(c.path) ? 128 : Cb);
  c.CPI = is_layerwise(c.path) ? p3::conv_any_init_pass(C) : 128;
  c.heads_image = !is_f32(c.path) && p3::heads_fusable(C, wf.V);
  c.heads_fused = c.heads_image && opt.heads_fuse && !runs_conv_any(c);
  if (is_tfm(c.path)) {
    c.tfm_heads = Cb;
    c.tfm_D = wf.model_C / Cb;
  }
  return c;
}

const HeadTensor kHeadTensors[kNumHeadTensors] = {
    {"policy.gpool_dense.w", &p3::HeadsArgs::gd_w, 2 * 32 * 32, 0, 0},
    {"policy.gpool_dense.b", &p3::HeadsArgs::gd_b, 32, 0, 12},
    {"policy.out_moves.w", &p3::HeadsArgs::moves_w, 2 * 32, 0, 9},
    {"policy.out_pass.w", &p3::HeadsArgs::pass_w, 4 * 32, 0, 7},
    {"policy.out_pass.b", &p3::HeadsArgs::pass_b, 2, 0, -1},
    {"policy.opt_moves.w", &p3::HeadsArgs::opt_moves_w, 32, 0, 10},
    {"policy.opt_pass.w", &p3::HeadsArgs::opt_pass_w, 2 * 32, 0, 8},
    {"policy.opt_pass.b", &p3::HeadsArgs::opt_pass_b, 1, 0, -1},
    {"value.oq_embed.w", &p3::HeadsArgs::oq_embed_w, 0, 2 * 32, 1},
    {"value.oq_embed.b", &p3::HeadsArgs::oq_embed_b, 0, 1, 13},
    {"value.oq_out.w", &p3::HeadsArgs::oq_out_w, 0, 14, 4},
    {"value.oq_out.b", &p3::HeadsArgs::oq_out_b, 14, 0, 16},
    {"value.own.w", &p3::HeadsArgs::own_w, 32, 0, 11},
    {"value.gamma_pre.w", &p3::HeadsArgs::gamma_pre_w, 0, 2 * 32, 2},
    {"value.gamma_pre.b", &p3::HeadsArgs::gamma_pre_b, 0, 1, 14},
    {"value.gamma_out.w", &p3::HeadsArgs::gamma_out_w, 0, 1, 5},
    {"value.gamma_out.b", &p3::HeadsArgs::gamma_out_b, 1, 0, -1},
    {"value.score_pre.w", &p3::HeadsArgs::score_pre_w, 0, 2 * 32 + 1, 3},
    {"value.score_pre.b", &p3::HeadsArgs::score_pre_b, 0, 1, 15},
    {"value.score_out.w", &p3::HeadsArgs::score_out_w, 0, 1, 6},
    {"value.score_out.b", &p3::HeadsArgs::score_out_b, 1, 0, -1}};

const AuxTensor kAuxTensors[kNumAuxTensors] = {
    {"policy.soft_moves.w", &p3::HeadsAuxArgs::soft_moves_w, 32, 0, 0, 0, {}},
    {"policy.soft_pass.w", &p3::HeadsAuxArgs::soft_pass_w, 2 * 32, 0, 0, 0, {}},
    {"policy.soft_pass.b", &p3::HeadsAuxArgs::soft_pass_b, 1, 0, 0, 0, {}},
    {"value.mcts_dist.w", &p3::HeadsAuxArgs::mcts_w, 0, p3::kAuxBins, 0, 0, {}},
    {"value.mcts_dist.b", &p3::HeadsAuxArgs::mcts_b, p3::kAuxBins, 0, 0, 0, {}},
    {"policy.out_moves.w", &p3::HeadsAuxArgs::moves_aux_w, 2 * 32, 0, 2, 1, {1}},
    {"policy.out_pass.w", &p3::HeadsAuxArgs::pass_aux_w, 4 * 32, 0, 2, 1, {1}},
    {"policy.out_pass.b", &p3::HeadsAuxArgs::pass_aux_b, 2, 0, 2, 1, {1}},
    {"value.oq_out.w", &p3::HeadsAuxArgs::oq_aux_w, 0, 14, 14, p3::kAuxGoCols, {2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13}},
    {"value.oq_out.b", &p3::HeadsAuxArgs::oq_aux_b, 14, 0, 14, p3::kAuxGoCols, {2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13}}};

namespace {

constexpr float kBnEps = 1e-3f;  // model.py:231

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
// A Keras (in, out) matrix W[K][N] as MFMA 16x16x32 A fragments [N / 16][K / 32][64 lanes][8] (transformer.h).
// `col0` / `ld`: the matrix is columns col0 .. col0 + N of a row-major [K][ld] tensor.
void pack_afrag(std::vector<_Float16>& dst, const float* W, int K, int N, int ld, int col0) {
  for (int ct = 0; ct < N / 16; ++ct)
    for (int st = 0; st < K / 32; ++st)
      for (int lane = 0; lane < 64; ++lane)
        for (int el = 0; el < 8; ++el)
          dst.push_back((_Float16)W[(size_t)(32 * st + 8 * (lane >> 4) + el) * ld + col0 + 16 * ct + (lane & 15)]);
}
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

// The broadcast dense matrix dw [361 i][361 j] as k16 blocks [j pass (3)][q (24)][h][128 j][8], K index r = 16 q + 8 h + e
// a board row of `row_stride` points: 19, r = the point i itself; 20, r = the act buffer's padded board row 20 y + x
// (zero rows for x = 19 and r >= 379), k_block's tail_dense.
void pack_dense(std::vector<_Float16>& dst, const float* dw, int row_stride) {
  for (int jp = 0; jp < 3; ++jp)
    for (int q = 0; q < 24; ++q)
      for (int h = 0; h < 2; ++h)
        for (int jj = 0; jj < 128; ++jj)
          for (int el = 0; el < 8; ++el) {
            const int r = q * 16 + h * 8 + el, y = r / row_stride, x = r % row_stride, j = jp * 128 + jj;
            const bool on_board = x < 19 && y < 19;
            float v = (on_board && j < kNLoc) ? dw[(size_t)(y * 19 + x) * kNLoc + j] : 0.0f;
            dst.push_back((_Float16)v);
          }
}

// conv j of block i, checked against the [k][k][cin][cout] size the packer will read
const float* conv_w(const WeightFile& wf, int i, int j, int kw, int cin, int cout) {
  return wf.get("blocks." + std::to_string(i) + ".conv" + std::to_string(j) + ".w", (size_t)kw * kw * cin * cout).data;
}

// A run of consecutive fused blocks with the broadcast convs that ride at its ends.  The weight streams of a run go
// into the arena back to back, after the run's other tensors: one k_block launch walks the streams of all its blocks
// as ONE circular stream (position-major order, kernels.hip), so a run must be contiguous.  With the broadcast 1x1
// convs fused in, a run's stream is [conv_last of the broadcast block before it] [its blocks] [conv_first of the
// broadcast block after it].
struct Run {
  std::vector<_Float16> head, tail;
  std::vector<std::pair<size_t, std::vector<_Float16>>> blocks;   // (plan index, stream)
  int head_of = -1, tail_of = -1;
};

// What the packers share while build_plan walks the blocks
struct Builder {
  const WeightFile& wf;
  const Options& opt;
  Plan& plan;
  Arena& ar;
  bool have_xa = false;   // layer-wise path: u holds mish(bn0(x)) of the next block
  Run cur;                // the run being collected
  std::vector<Run> runs;  // laid out after the blocks, all runs back to back (lay_out_runs)
  void flush_run() {
    if (!cur.blocks.empty()) runs.push_back(std::move(cur));
    cur = Run{};
  }
};

// Adds the weight image of one conv W ([kw][kw][cin][cout], zero-padded to cin_pad x cout_pad) for the kernel the path
// runs it with, and returns its offset: conv_f32.h's image on the fp32 paths; k_sconv's for a trunk conv (`trunk`: a
// layer conv or a broadcast block's 1x1) of Split; else an fp16 stream of output passes CP wide over K slices CB wide
// (28 taps for the 25 of the init conv), whose macro-steps go to *nms.
size_t add_conv_image(Builder& b, const float* W, int kw, int cin, int cout, int cin_pad, int cout_pad, bool trunk, int CB,
                      int CP, int* nms) {
  const int taps = kw * kw;
  if (is_f32(b.plan.choice.path)) {
    std::vector<float> w32;
    p3::pack_conv_f32(w32, W, taps, cin, cout, cin_pad, cout_pad);
    return b.ar.add(w32.data(), w32.size() * 4);
  }
  std::vector<_Float16> s;
  if (trunk && b.plan.choice.path == Path::Split) {
    p3::pack_sconv(s, W, taps, cin, cout, cin_pad, cout_pad);
    return b.ar.add(s.data(), s.size() * 2);
  }
  for (int cp = 0; cp < cout_pad / CP; ++cp)
    for (int ip = 0; ip < cin_pad / CB; ++ip) pack_segment(s, W, taps, kw == 5 ? 28 : taps, cin, cout, ip * CB, CB, cp * CP, CP);
  return add_stream(b.ar, s, *nms, CP);
}

void pack_stem(Builder& b) {
  const WeightFile& wf = b.wf;
  const int C = wf.C;
  const Tensor& w = wf.get("init_conv.w", (size_t)25 * 15 * C);  // [5][5][15][C]
  b.plan.init_w_off = add_conv_image(b, w.data, 5, 15, C, 16, C, false, 16, b.plan.choice.CPI, &b.plan.init_nms);
  b.plan.game_w_off = b.ar.add(wf.get("init_game.w", (size_t)8 * C).data, 8 * C * 4);
  b.plan.game_b_off = b.ar.add(wf.get("init_game.b", (size_t)C).data, C * 4);
}

void pack_rope(Builder& b) {
  const int D = b.plan.choice.tfm_D;
  std::vector<double> cd(kNLoc * D), sd(kNLoc * D);
  spiral_rope_table(D, cd.data(), sd.data());
  const std::vector<float> cf(cd.begin(), cd.end()), sf(sd.begin(), sd.end());
  b.plan.rope_cos_off = b.ar.add(cf.data(), cf.size() * 4);
  b.plan.rope_sin_off = b.ar.add(sf.data(), sf.size() * 4);
}

// Transformer block i, its GEMM weights as fragments of element type T: pack_afrag (fp16) or, for TfmF32, the same
// fragments in fp32 (transformer_f32.h pack_tfm_f32; no fp16 image then)
template <class T, class Pack>
void pack_tfm_block(Builder& b, int i, Pack pack) {
  const std::string p = "blocks." + std::to_string(i);
  const int c = b.wf.model_C, f = 2 * c;
  auto W = [&](const char* n, size_t sz) { return b.wf.get(p + "." + n, sz).data; };
  BlockPlan bp;
  bp.kind = 5;
  bp.tfm.rms_in = b.ar.add(W("rms_in.scale", c), c * 4);
  bp.tfm.rms_out = b.ar.add(W("rms_out.scale", c), c * 4);
  std::vector<T> w;
  auto flush = [&] {
    const size_t off = b.ar.add(w.data(), w.size() * sizeof(T));
    w.clear();
    return off;
  };
  for (const char* n : {"q.w", "k.w", "v.w"}) pack(w, W(n, (size_t)c * c), c, c, c, 0);
  bp.tfm.wqkv = flush();
  pack(w, W("o.w", (size_t)c * c), c, c, c, 0);
  bp.tfm.wo = flush();
  pack(w, W("ffn_gate.w", (size_t)c * f), c, f, f, 0);
  pack(w, W("ffn_up.w", (size_t)c * f), c, f, f, 0);
  bp.tfm.wgu = flush();
  pack(w, W("ffn_down.w", (size_t)f * c), f, c, c, 0);
  bp.tfm.wdown = flush();
  b.plan.blocks.push_back(bp);
}

// Broadcast block i (kind 3).  On the Fused path the run before it takes conv_first (and at C = 256 btl the dense) as
// its tail, the run after it conv_last as its head; the stand-alone streams serve every other path, P3HIP_NO_BFUSE and
// broadcast blocks without a fused neighbour.
void pack_broadcast_block(Builder& b, int i) {
  const WeightFile& wf = b.wf;
  Arena& ar = b.ar;
  const int C = wf.C, Cb = wf.Cb, CB = b.plan.choice.CB;
  const std::string p = "blocks." + std::to_string(i);
  BlockPlan bp;
  bp.kind = 3;
  b.have_xa = false;
  bp.bn[0] = fold_bn(ar, wf, p + ".bn0", C);
  bp.bn[1] = fold_bn(ar, wf, p + ".bn1", C);
  const Path path = b.plan.choice.path;
  const float *w0 = conv_w(wf, i, 0, 1, C, C), *w1 = conv_w(wf, i, 1, 1, C, C);
  const Tensor& dw = wf.get(p + ".dense.w", (size_t)kNLoc * kNLoc);  // [361 i][361 j]
  // t = mish(conv_first(mish(bn0(x)))), u = the dense over t, x += conv_last(u); in the arena conv_first, the dense,
  // conv_last (Split: the dense behind conv_last) and the dense's bias
  LayerPlan first{1, C, C, true, 2, false, false, bp.bn[0], FoldedBN{}, 0, 1, -1};
  LayerPlan last{1, C, C, false, 0, true, false, FoldedBN{}, FoldedBN{}, 3, 0, -1};
  const int CPb = (CB == 128) ? 128 : 64;
  first.w_off = add_conv_image(b, w0, 1, C, C, C, C, true, CB, CPb, &first.nms);
  if (path == Path::Split) last.w_off = add_conv_image(b, w1, 1, C, C, C, C, true, CB, CPb, &last.nms);
  if (is_f32(path)) {
    std::vector<float> d32;
    p3::pack_dense_f32(d32, dw.data);
    bp.dense_off = ar.add(d32.data(), d32.size() * 4);
  } else {
    std::vector<_Float16> d16;
    pack_dense(d16, dw.data, 19);
    bp.dense_off = add_stream(ar, d16, bp.dense_nms, 128);
  }
  if (path != Path::Split) last.w_off = add_conv_image(b, w1, 1, C, C, C, C, true, CB, CPb, &last.nms);
  bp.dense_bias_off = ar.add(wf.get(p + ".dense.b", (size_t)kNLoc).data, kNLoc * 4);
  bp.layers = {first, last};
  // (k_blockw's trunks run their broadcast blocks as their own launches)
  const bool fused_neighbours = path == Path::Fused && b.opt.bcast_fuse;
  // fused copies: output pass 1 takes its K slices in the order (1, 0) — slice 1 is the one
  // still in the act buffer when pass 0 ends (kernels.hip k_block, BC form)
  std::vector<_Float16> f0, f2;
  if (fused_neighbours)
    for (int cp = 0; cp < 2; ++cp)
      for (int k = 0; k < 2; ++k) {
        const int ip = cp == 0 ? k : 1 - k;
        pack_segment(f0, w0, 1, 1, C, C, ip * Cb, Cb, cp * Cb, Cb);
        pack_segment(f2, w1, 1, 1, C, C, ip * Cb, Cb, cp * Cb, Cb);
      }
  if (fused_neighbours && !b.cur.blocks.empty()) {
    b.cur.tail = f0;
    b.cur.tail_of = i;
    bp.first_fused = true;
    // C = 256: the dense rides in that tail too (k_block, tail_dense).  Its stream there:
    // [conv_first pass 0 (K slices 0, 1)] [dense] [conv_first pass 1 (K slices 0, 1)] [dense], the dense matrix
    // with its K index = the act buffer's padded board row
    if (C == 256 && Cb == 128 && wf.btype == 0 && b.opt.dense_fuse) {   // btl blocks only (k_block's tail_dense)
      bp.dense_fused = true;
      std::vector<_Float16> dpad;
      pack_dense(dpad, dw.data, 20);
      b.cur.tail.clear();
      for (int cp = 0; cp < 2; ++cp) {
        for (int ip = 0; ip < 2; ++ip) pack_segment(b.cur.tail, w0, 1, 1, C, C, ip * Cb, Cb, cp * Cb, Cb);
        b.cur.tail.insert(b.cur.tail.end(), dpad.begin(), dpad.end());
      }
    }
  }
  b.flush_run();
  if (fused_neighbours && i + 1 < wf.nblocks && !wf.is_broadcast(i + 1)) {
    b.cur.head = f2;
    b.cur.head_of = i;   // last_fused is set when the run is laid out
  }
  b.plan.blocks.push_back(bp);
}

// Layer-wise block i (kind 4): one LayerPlan per conv, with the weight image of the path's kernel (add_conv_image), and on
// the INT8 paths the quantized weights as well (the fp16 streams are what the calibration runs)
void pack_layerwise_block(Builder& b, int i) {
  const WeightFile& wf = b.wf;
  Arena& ar = b.ar;
  const Path path = b.plan.choice.path;
  const int C = wf.C, Cb = wf.Cb;
  const bool classic = wf.btype == 2;
  const std::string p = "blocks." + std::to_string(i);
  BlockPlan bp;
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
  const bool next_layerwise = !is_int8_fused(path) && i + 1 < wf.nblocks && !wf.is_broadcast(i + 1);
  if (next_layerwise) next_bn0 = fold_bn(ar, wf, "blocks." + std::to_string(i + 1) + ".bn0", C);
  const FoldedBN none{};
  auto add_layer = [&](int j, int kw, int cin, int cout, bool pre, const FoldedBN& pre_bn, bool act, bool res,
                       bool dual, const FoldedBN& out_bn, int in_buf, int out_buf, int out2_buf) {
    LayerPlan lp{kw, cin, cout, pre, act ? 1 : 0, res, dual, pre_bn, out_bn, in_buf, out_buf, out2_buf};
    const float* W = conv_w(wf, i, j, kw, cin, cout);
    lp.w_off = add_conv_image(b, W, kw, cin, cout, cin, cout, true, 64, 64, &lp.nms);
    if (is_int8(path) && (path != Path::Int8Conv3 || kw == 3)) {
      std::vector<int8_t> q;
      std::vector<float> sw;
      p3::pack_lconv_i8(q, sw, W, kw * kw, cin, cout);
      lp.q_off = ar.add(q.data(), q.size());
      lp.qs_off = ar.add(sw.data(), sw.size() * 4);
      lp.qidx = b.plan.n_q++;
    }
    bp.layers.push_back(lp);
  };
  const bool from_xa = b.have_xa;          // first layer input: activated copy in u, or raw x with pre
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
  // Int8Conv3: the activated output of layer j (act, or dual's second tensor) is the input of layer j + 1 of the block,
  // stored as int8 when that is a 3x3 conv; the last layer's goes to the next block's 1x1 reduce, in fp16
  if (path == Path::Int8Conv3)
    for (size_t j = 0; j + 1 < bp.layers.size(); ++j)
      if (bp.layers[j].act == 1 || bp.layers[j].dual) bp.layers[j].out_qidx = bp.layers[j + 1].qidx;
  b.have_xa = next_layerwise;
  b.plan.blocks.push_back(bp);
}

// Fused block i (kind 0 btl, 1 nbt): its stream joins the run being collected
void pack_fused_block(Builder& b, int i) {
  const WeightFile& wf = b.wf;
  const int C = wf.C, Cb = wf.Cb, CB = b.plan.choice.CB;
  const std::string p = "blocks." + std::to_string(i);
  BlockPlan bp;
  bp.kind = wf.btype;
  const int nconv = (wf.btype == 0) ? wf.inner + 2 : 6;
  for (int j = 0; j < nconv; ++j) bp.bn[j] = fold_bn(b.ar, wf, p + ".bn" + std::to_string(j), j == 0 ? C : Cb);
  std::vector<_Float16> s;
  for (int ip = 0; ip < C / CB; ++ip) pack_segment(s, conv_w(wf, i, 0, 1, C, Cb), 1, 1, C, Cb, ip * CB, CB, 0, CB);
  for (int j = 1; j < nconv - 1; ++j) pack_segment_3x3(s, conv_w(wf, i, j, 3, Cb, Cb), Cb, Cb, CB, CB);
  for (int cp = 0; cp < C / CB; ++cp) pack_segment(s, conv_w(wf, i, nconv - 1, 1, Cb, C), 1, 1, Cb, C, 0, CB, cp * CB, CB);
  b.cur.blocks.emplace_back(b.plan.blocks.size(), std::move(s));
  b.plan.blocks.push_back(bp);
}

// The runs' streams, all runs back to back ([head r][blocks r][tail r][head r + 1] ...): with everything of the
// broadcast blocks between them fused, one k_block launch walks them all (forward.cpp joined_launch).
void lay_out_runs(Builder& b) {
  std::vector<BlockPlan>& blocks = b.plan.blocks;
  const int Cb = b.wf.Cb;
  int nms_unused = 0;
  for (const Run& r : b.runs) {
    if (r.head_of >= 0) {
      add_stream(b.ar, r.head, nms_unused, Cb);
      BlockPlan& fb = blocks[r.blocks.front().first];
      fb.head_of = r.head_of;
      fb.head_bytes = r.head.size() * 2;
      blocks[r.head_of].last_fused = true;
    }
    for (const auto& rs : r.blocks) {
      BlockPlan& bp = blocks[rs.first];
      bp.stream_off = add_stream(b.ar, rs.second, bp.nms, Cb);
      bp.stream_bytes = rs.second.size() * 2;
    }
    if (r.tail_of >= 0) {
      add_stream(b.ar, r.tail, nms_unused, Cb);
      BlockPlan& lb = blocks[r.blocks.back().first];
      lb.tail_of = r.tail_of;
      lb.tail_bytes = r.tail.size() * 2;
    }
  }
}

// k_blockw: per run of consecutive btl blocks, the weight stream in the order the kernel consumes it and the parameter
// table.  The BN in front of a conv's consumer rides in the conv: its folded scale times log2(e) is multiplied into
// the fp16 weights, its shift times log2(e) is the accumulators' initial value (the kernel's exp2-based mish takes
// log2(e) * y, as bn_mish8_l2 does).
//   block stream: reduce: x halves (quarters 0, 1 / 2, 3); in a half set A's four k32 granules, then set B's
//                 layer j: phases (A, lo) (B, lo) (A, hi) (B, hi), each (ky, q32, kx) over its 64 input channels
//                 expand: output quarters 0..3, k32 steps 0..3 (unscaled: the residual add follows)
//   block table:  bn0 scale[256] shift[256] (times log2 e) | conv j = 0 .. L: shift[128] of bn j + 1 (times log2 e)
void pack_blockw_runs(Builder& b) {
  const WeightFile& wf = b.wf;
  Arena& ar = b.ar;
  std::vector<BlockPlan>& blocks = b.plan.blocks;
  const int C = wf.C, Cb = wf.Cb, L = wf.inner;
  const float kLog2e = 1.4426950408889634f;
  for (size_t bi = 0; bi < blocks.size();) {
    if (blocks[bi].kind != 0) { ++bi; continue; }
    size_t n = 1;
    while (bi + n < blocks.size() && blocks[bi + n].kind == 0) ++n;
    std::vector<_Float16> ws;
    std::vector<float> prm;
    for (size_t k = bi; k < bi + n; ++k) {
      // block index in the weight file = plan index (one BlockPlan per trunk block)
      const int i = (int)k;
      const BlockPlan& bp = blocks[k];
      auto bn_row = [&](int j, bool shift) {
        const float* v = reinterpret_cast<const float*>(ar.host.data() + (shift ? bp.bn[j].shift_off : bp.bn[j].scale_off));
        std::vector<float> r((size_t)(j == 0 ? C : Cb));
        for (size_t c = 0; c < r.size(); ++c) r[c] = v[c] * kLog2e;
        return r;
      };
      const float* w0 = conv_w(wf, i, 0, 1, C, Cb);
      const std::vector<float> s1 = bn_row(1, false);
      for (int half = 0; half < 2; ++half)
        for (int s0 = 0; s0 < 128; s0 += 64)
          for (int st = 0; st < 4; ++st) pack_granule(ws, w0, C, Cb, 0, 128 * half + 32 * st, s0, s1.data());
      for (int j = 1; j <= L; ++j) {
        const float* wj = conv_w(wf, i, j, 3, Cb, Cb);
        const std::vector<float> sj = bn_row(j + 1, false);
        for (int ph = 0; ph < 4; ++ph) {
          const int s0 = (ph & 1) * 64, half = ph >> 1;
          for (int ky = 0; ky < 3; ++ky)
            for (int q = 0; q < 2; ++q)
              for (int kx = 0; kx < 3; ++kx) pack_granule(ws, wj, Cb, Cb, ky * 3 + kx, 64 * half + 32 * q, s0, sj.data());
        }
      }
      const float* we = conv_w(wf, i, L + 1, 1, Cb, C);
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
    BlockwRun run;
    run.first = bi;
    run.nblk = (int)n;
    run.stream_off = ar.add(ws.data(), ws.size() * 2);
    run.prm_off = ar.add(prm.data(), prm.size() * 4);
    if (ws.size() * 2 != n * (size_t)(32 + 72 * L) * 4096 || prm.size() != n * (size_t)(512 + 128 * (L + 1))) ar.bad_stream = true;
    blocks[bi].bw_run = (int)b.plan.bw_runs.size();
    b.plan.bw_runs.push_back(run);
    bi += n;
  }
}

// heads: conv_p | conv_g | value.conv -> [C][96], then the small tensors of kHeadTensors
bool pack_heads(Builder& b, std::string& err) {
  const WeightFile& wf = b.wf;
  Arena& ar = b.ar;
  Plan& plan = b.plan;
  const int C = wf.C, CB = plan.choice.CB;
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
  plan.heads_w_off = add_conv_image(b, w.data(), 1, C, 96, C, 128, false, CB, 64, &plan.heads_nms);
  // the same weights as MFMA 16x16x32 A fragments for k_headsx (the convs inside the heads kernel):
  // [cout tile ct][k32 step][lane (n = lane & 15, q = lane >> 4)][8] = w[cin = 32 step + 8 q + e][cout = 16 ct + n]
  if (plan.choice.heads_image) {
    std::vector<_Float16> af;
    pack_afrag(af, w.data(), C, 96, 96, 0);
    plan.heads_conv_a_off = ar.add(af.data(), af.size() * 2);
  }
  plan.heads_gbn = fold_bn(ar, wf, "policy.gpool_bn", 32);
  const float* data[kNumHeadTensors];
  size_t size[kNumHeadTensors];
  for (int k = 0; k < kNumHeadTensors; ++k) {   // sizes k_heads reads (kernels.h HeadsArgs)
    size[k] = (size_t)kHeadTensors[k].n0 + (size_t)kHeadTensors[k].nV * wf.V;
    const Tensor& t = wf.get(kHeadTensors[k].name, size[k]);
    data[k] = t.data;
    plan.head_tensor_off[k] = ar.add(t.data, t.size() * 4);
  }
  // k_headsx takes the same tensors as one image in its LDS order (kernels.h heads_image_floats): the weights, the
  // folded gpool BN, the biases, and two floats of padding behind oq_out.b
  if (plan.choice.heads_image && wf.missing.empty()) {
    std::vector<float> img;
    for (int rank = 0; rank <= 16; ++rank) {
      for (int k = 0; k < kNumHeadTensors; ++k)
        if (kHeadTensors[k].image_rank == rank) img.insert(img.end(), data[k], data[k] + size[k]);
      if (rank == 11)
        for (size_t off : {plan.heads_gbn.scale_off, plan.heads_gbn.shift_off}) {
          const float* bn = reinterpret_cast<const float*>(ar.host.data() + off);
          img.insert(img.end(), bn, bn + 32);
        }
    }
    img.insert(img.end(), 2, 0.0f);
    if ((int)img.size() != p3::heads_image_floats(32, wf.V)) {
      err = "internal error: heads image size";
      return false;
    }
    plan.heads_image_off = ar.add(img.data(), img.size() * 4);
  }
  return true;
}

// P3HIP_FLAG_AUX: the aux tensors of kAuxTensors behind everything else in the arena (an engine without the flag has the
// same image as before), fp32 whatever the plan
void pack_aux(Builder& b) {
  const WeightFile& wf = b.wf;
  for (int k = 0; k < kNumAuxTensors; ++k) {
    const AuxTensor& at = kAuxTensors[k];
    const size_t n = (size_t)at.n0 + (size_t)at.nV * wf.V;
    const Tensor& t = wf.get(at.name, n);
    if (at.cols == 0) {
      b.plan.aux_tensor_off[k] = b.ar.add(t.data, n * 4);
      continue;
    }
    std::vector<float> w;
    for (size_t r = 0; r < n / at.cols; ++r)
      for (int c = 0; c < at.ntake; ++c) w.push_back(t.data[r * at.cols + at.take[c]]);
    b.plan.aux_tensor_off[k] = b.ar.add(w.data(), w.size() * 4);
  }
}

// P3HIP_FLAG_WINOGRAD: k_wconv's image of every 3x3 layer conv, behind everything else in the arena (what lies in front
// is the fp16 plan's image of the same flags, offset for offset), from the file's fp32 weights
void pack_wino(Builder& b) {
  for (size_t i = 0; i < b.plan.blocks.size(); ++i) {   // (plan index = block index in the file)
    BlockPlan& bp = b.plan.blocks[i];
    if (bp.kind != 4) continue;
    for (size_t j = 0; j < bp.layers.size(); ++j) {
      LayerPlan& lp = bp.layers[j];
      if (lp.kw != 3) continue;
      std::vector<_Float16> img;
      p3::pack_wconv(img, conv_w(b.wf, (int)i, (int)j, 3, lp.cin, lp.cout), lp.cin, lp.cout, lp.cin, lp.cout);
      lp.wino_off = b.ar.add(img.data(), img.size() * 2);
    }
  }
}

}  // namespace

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

bool build_plan(const WeightFile& wf, uint32_t flags, const Options& opt, Plan& plan, Arena& ar, std::string& err) {
  plan.choice = choose_plan(wf, flags, opt, err);
  const Path path = plan.choice.path;
  if (path == Path::Refused) return false;
  Builder b{wf, opt, plan, ar};
  pack_stem(b);
  if (is_tfm(path)) pack_rope(b);
  for (int i = 0; i < wf.nblocks; ++i) {
    if (path == Path::Tfm || path == Path::TfmSplit) pack_tfm_block<_Float16>(b, i, pack_afrag);
    else if (path == Path::TfmF32) pack_tfm_block<float>(b, i, p3::pack_tfm_f32);
    else {
      if (is_layerwise(path)) b.flush_run();
      if (wf.is_broadcast(i)) pack_broadcast_block(b, i);
      else if (is_layerwise(path)) pack_layerwise_block(b, i);
      else pack_fused_block(b, i);
    }
  }
  b.flush_run();
  lay_out_runs(b);
  if (path == Path::Blockw) pack_blockw_runs(b);
  if (!pack_heads(b, err)) return false;
  if (flags & P3HIP_FLAG_AUX) pack_aux(b);
  if (path == Path::Winograd3) pack_wino(b);
  if (!wf.missing.empty()) {
    err = "weight file lacks tensors of the architecture its header names: " + wf.missing;
    return false;
  }
  if (ar.bad_stream) {
    err = "internal error: a packed weight stream is not a whole number of ring macro-steps";
    return false;
  }
  return true;
}

}  // namespace eng
