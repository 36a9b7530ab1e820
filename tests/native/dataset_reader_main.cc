// dataset_reader_main.cc — runs the chunk reader (p3achygo_amd/host/tf_reader.h) over the fixture chunk and over damaged
// variants of it, for a build with -fsanitize=address,undefined (tests/test_dataset_cpu.py): every outcome must be the
// expected status, and the sanitizers must stay silent.  Usage: dataset_reader_main FIXTURE.tfrecord
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../p3achygo_amd/host/tf_reader.h"

using namespace p3;

namespace {

int g_failures = 0;

void Expect(const char* name, const ReadStatus& st, size_t rows, int code, const char* needle, const char* record, size_t want_rows) {
  const bool ok = st.code == code && rows == want_rows && (!needle || st.msg.find(needle) != std::string::npos) &&
                  (!record || st.msg.find(record) == 0);
  std::printf("%-34s %s  code %d rows %zu  %s\n", name, ok ? "ok  " : "FAIL", st.code, rows, st.msg.c_str());
  if (!ok) ++g_failures;
}

void Case(const char* name, const std::vector<uint8_t>& bytes, int mode, int code, const char* needle, const char* record,
          size_t want_rows) {
  GoDataset ds;
  const ReadStatus st = ds.OpenBytes(bytes.data(), bytes.size(), mode);
  Expect(name, st, ds.size(), code, needle, record, want_rows);
}

void Varint(std::string& o, uint64_t v) {
  while (v >= 0x80) { o.push_back((char)(v | 0x80)); v >>= 7; }
  o.push_back((char)v);
}
std::string Ld(int field, const std::string& p) {
  std::string o;
  Varint(o, (uint64_t)(field << 3 | 2));
  Varint(o, p.size());
  return o + p;
}
std::string BytesFeature(const std::string& b) { return Ld(1, Ld(1, b)); }
std::string FloatFeature(float v, bool packed) {
  std::string f((const char*)&v, 4);
  if (packed) return Ld(2, Ld(1, f));
  std::string list;
  Varint(list, 1 << 3 | 5);
  return Ld(2, list + f);
}
// a record of our own; board_bytes / with_pi make the damaged ones
std::string Example(size_t board_bytes, bool with_pi, bool packed) {
  const std::string grid(361, '\0');
  const int16_t last[5] = {-20, -1, 361, 3, 360};
  std::string fs;
  auto add = [&](const char* key, const std::string& feature) { fs += Ld(1, Ld(1, key) + Ld(2, feature)); };
  add("komi", FloatFeature(7.5f, packed));
  add("bsize", BytesFeature(std::string(1, (char)19)));
  add("board", BytesFeature(std::string(board_bytes, '\1')));
  add("last_moves", BytesFeature(std::string((const char*)last, sizeof last)));
  add("stones_atari", BytesFeature(grid));
  add("stones_two_liberties", BytesFeature(grid));
  add("stones_three_liberties", BytesFeature(grid));
  add("stones_in_ladder", BytesFeature(grid));
  add("color", BytesFeature(std::string(1, (char)-1)));
  if (with_pi) add("pi", BytesFeature(std::string(362 * 4, '\0')));
  add("score_margin", FloatFeature(-2.5f, packed));
  add("q6", FloatFeature(0.25f, packed));
  std::string ex = Ld(1, fs);
  Varint(ex, 9 << 3 | 0);   // an unknown varint field behind the features
  Varint(ex, 77);
  return ex;
}
std::vector<uint8_t> Frame(const std::string& payload) {
  std::vector<uint8_t> o(12);
  const uint64_t n = payload.size();
  std::memcpy(o.data(), &n, 8);
  const uint32_t hc = MaskedCrc32c(o.data(), 8), fc = MaskedCrc32c(payload.data(), payload.size());
  std::memcpy(o.data() + 8, &hc, 4);
  o.insert(o.end(), payload.begin(), payload.end());
  o.insert(o.end(), (const uint8_t*)&fc, (const uint8_t*)&fc + 4);
  return o;
}
std::vector<uint8_t> Deflate(const std::vector<uint8_t>& in) {
  uLongf n = compressBound((uLong)in.size());
  std::vector<uint8_t> out(n);
  if (compress2(out.data(), &n, in.data(), (uLong)in.size(), 2) != Z_OK) n = 0;
  out.resize(n);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s FIXTURE.tfrecord\n", argv[0]); return 2; }
  std::vector<uint8_t> fx;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint8_t buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) fx.insert(fx.end(), buf, buf + n);
    std::fclose(f);
  }
  {   // the fixture from its file, mode by detection and explicit
    GoDataset ds;
    ReadStatus st = ds.Open(argv[1], kModeAuto);
    Expect("fixture (file, auto)", st, ds.size(), kReadOk, nullptr, nullptr, 6);
    if (st.ok() && ds.size() == 6) {
      const float want[6] = {5.5f, -5.5f, 0.5f, 3.5f, -3.5f, 0.0f};
      for (int i = 0; i < 6; ++i) {
        const DatasetRow& r = ds.row(i);
        const bool ok = r.labels.score_margin == want[i] && r.labels.did_win == (want[i] >= 0) && r.features.komi == 6.5f &&
                        r.labels.policy[0] == 1.0f && r.features.last_moves[0].i == 0 && r.features.last_moves[0].j == -1;
        if (!ok) { std::printf("fixture row %d FAIL\n", i); ++g_failures; }
      }
    }
    GoDataset none;
    st = none.Open(std::string(argv[1]) + ".missing", kModeAuto);
    Expect("missing file", st, none.size(), kReadIo, "cannot open", nullptr, 0);
  }
  Case("fixture (bytes, plain)", fx, kModePlain, kReadOk, nullptr, nullptr, 6);
  Case("fixture read as zlib", fx, kModeZlib, kReadZlib, "zlib", "record 0:", 0);
  Case("empty stream", {}, kModeAuto, kReadOk, nullptr, nullptr, 0);
  const size_t rec1 = 16 + 4037, rec2 = 2 * (16 + 4037), rec3 = 3 * (16 + 4037);
  {
    std::vector<uint8_t> d = fx;
    d[rec3 + 12 + 1000] ^= 0x40;
    Case("payload byte flipped", d, kModeAuto, kReadCrc, "CRC of the payload", "record 3:", 0);
  }
  {
    std::vector<uint8_t> d = fx;
    const uint64_t big = 1ull << 40;
    std::memcpy(d.data() + rec2, &big, 8);
    Case("length 2^40, CRC stale", d, kModeAuto, kReadCrc, "CRC of the length", "record 2:", 0);
    const uint32_t hc = MaskedCrc32c(d.data() + rec2, 8);
    std::memcpy(d.data() + rec2 + 8, &hc, 4);
    Case("length 2^40, CRC right", d, kModeAuto, kReadTruncated, "length field says 1099511627776", "record 2:", 0);
  }
  for (size_t cut : {rec1 + 5, rec1 + 12, rec1 + 2000, rec2 - 1}) {
    std::vector<uint8_t> d(fx.begin(), fx.begin() + cut);
    Case("truncated mid-record", d, kModeAuto, kReadTruncated, "truncated", "record 1:", 0);
  }
  const std::vector<uint8_t> zz = Deflate(fx);
  Case("zlib chunk", zz, kModeAuto, kReadOk, nullptr, nullptr, 6);
  Case("zlib chunk read as plain", zz, kModePlain, kReadCrc, nullptr, "record 0:", 0);
  for (size_t cut : {(size_t)1, (size_t)2, zz.size() / 2, zz.size() - 1}) {
    std::vector<uint8_t> d(zz.begin(), zz.begin() + cut);
    Case("zlib chunk truncated", d, cut < 2 ? kModeZlib : kModeAuto, kReadTruncated, "truncated", "record ", 0);
  }
  {
    std::vector<uint8_t> d = zz;
    for (size_t i = d.size() / 2; i < d.size() / 2 + 16; ++i) d[i] ^= 0xff;
    GoDataset ds;
    const ReadStatus st = ds.OpenBytes(d.data(), d.size(), kModeAuto);
    Expect("zlib chunk corrupted", st, ds.size(), st.code == kReadOk ? -1 : st.code, "record ", "record ", 0);   // any error, no rows
  }
  for (bool packed : {true, false}) {
    std::vector<uint8_t> good = Frame(Example(361, true, packed));
    std::vector<uint8_t> two = good;
    two.insert(two.end(), good.begin(), good.end());
    Case(packed ? "own record, packed floats" : "own record, plain floats", two, kModeAuto, kReadOk, nullptr, nullptr, 2);
    GoDataset ds;
    if (ds.OpenBytes(good.data(), good.size()).ok() && ds.size() == 1) {
      const DatasetRow& r = ds.row(0);
      const p3hip_loc want[5] = {{-1, -1}, {0, -1}, {19, 0}, {0, 3}, {18, 18}};
      bool ok = r.features.komi == 7.5f && r.labels.score_margin == -2.5f && r.labels.did_win == 0 && r.features.color == -1;
      for (int m = 0; m < 5; ++m) ok = ok && r.features.last_moves[m].i == want[m].i && r.features.last_moves[m].j == want[m].j;
      if (!ok) { std::printf("own record FAIL\n"); ++g_failures; }
    } else {
      ++g_failures;
    }
  }
  {
    std::vector<uint8_t> d = Frame(Example(361, true, true)), bad = Frame(Example(360, true, true));
    d.insert(d.end(), bad.begin(), bad.end());
    Case("board of 360 bytes", d, kModeAuto, kReadBadLength, "wrong byte length of 'board': 360", "record 1:", 0);
    d = Frame(Example(361, false, true));
    Case("no pi", d, kModeAuto, kReadMissingKey, "missing key 'pi'", "record 0:", 0);
  }
  {   // every prefix of a good payload, framed with right CRCs: the parser alone must refuse it or read it, in bounds
    const std::string ex = Example(361, true, false);
    for (size_t n = 0; n < ex.size(); n += (n < 64 ? 1 : 97)) {
      const std::vector<uint8_t> d = Frame(ex.substr(0, n));
      GoDataset ds;
      const ReadStatus st = ds.OpenBytes(d.data(), d.size());
      if (st.ok() || ds.size() != 0 || st.msg.find("record 0:") != 0) { std::printf("payload prefix %zu FAIL: %s\n", n, st.msg.c_str()); ++g_failures; }
    }
    // and every byte of the wire structure's first 200 set to 0xff
    for (size_t i = 0; i < 200; ++i) {
      std::string m = ex;
      m[i] = (char)0xff;
      const std::vector<uint8_t> d = Frame(m);
      GoDataset ds;
      const ReadStatus st = ds.OpenBytes(d.data(), d.size());
      if (!st.ok() && ds.size() != 0) { std::printf("payload byte %zu FAIL\n", i); ++g_failures; }
    }
  }
  std::printf("%d failures\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}
