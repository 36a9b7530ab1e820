// weights.h — a .p3w weight file in host memory: its header, its tensors by name, and the zero-padding of the widths
// the kernels do not serve as they are.  No device call.
#pragma once

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "transformer.h"

namespace eng {

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

}  // namespace eng
