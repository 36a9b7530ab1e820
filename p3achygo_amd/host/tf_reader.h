// tf_reader.h — training-chunk reader: the inverse of tf_recorder.h.
//
// Restates what the reference reads chunks with, without protobuf / abseil / TensorFlow:
//   * TFRecord framing (cc/data/tfrecord/record_reader.cc): uint64 length, masked CRC32C of the length,
//     payload, masked CRC32C of the payload; the stream plain or ONE zlib stream (window 15).  Both CRCs of
//     every record are checked.
//   * tf.Example by hand: Example{1: Features{1: map<string, Feature>}}, Feature{1: BytesList | 2: FloatList |
//     3: Int64List}.  Floats packed (wire type 2) or not (wire type 5), unknown fields skipped by wire type, map
//     entries in any order, a repeated key: the last one wins (protobuf's map semantics).
//   * nn::GoDataset rows (cc/nn/engine/go_dataset.cc:32-123): the keys of :60-77 become a p3hip_features and a
//     p3hip_labels; did_win = score_margin >= 0 (:114); bsize must be 19 (:81).  GoDataset reads no other key, and a
//     row needs no other key, so old-schema and new-schema records load alike.
//   * the trainer's targets (python/transforms.py _parse_example / _expand_common, :276-485): the other keys of EX_DESC
//     (own, pi_aux, pi_aux_dist, mcts_value_dist, q6 .. q50_score) become a p3hip_targets beside the row, when the
//     trainer's own parse of the record would succeed (ParseTargets below); a row without targets still loads.  No
//     symmetry is applied and no last moves are masked: the trainer's random ones (:222, :424) are not mirrored.
//
// Where this reader differs from the reference, on purpose:
//   * it never aborts (the reference CHECK-fails on a bad bsize and reads past short strings): every length is checked
//     against what remains, and a bad record fails the whole open with a message that names the record index and what
//     failed.  The reference logs a bad record and leaves a default-constructed row in its place (:48-57);
//   * a short last batch holds only the rows that were read.  The reference resizes every batch to batch_size (:40) and
//     scores the default-constructed rows behind the last record; here rows are a flat list and batching is the
//     caller's.
#pragma once
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/p3hip.h"
#include "crc32c.h"

namespace p3 {

enum ReadCode {
  kReadOk = 0,
  kReadIo = 1,          // the file cannot be opened or read
  kReadCrc = 2,         // a length or payload CRC does not match
  kReadTruncated = 3,   // the stream ends inside a record (or a zlib stream before its end marker)
  kReadParse = 4,       // the payload is not a tf.Example
  kReadMissingKey = 5,  // a key of go_dataset.cc:60-77 is absent (or holds no value of the expected kind)
  kReadBadLength = 6,   // a bytes value has the wrong byte length
  kReadBadValue = 7,    // bsize != 19
  kReadZlib = 8,        // the zlib stream is corrupt
};
struct ReadStatus {
  int code = kReadOk;
  std::string msg;
  bool ok() const { return code == kReadOk; }
};
inline ReadStatus ReadError(int code, long record, const std::string& what) {
  return ReadStatus{code, "record " + std::to_string(record) + ": " + what};
}

enum ReadMode { kModeAuto = 0, kModePlain = 1, kModeZlib = 2 };

// Sequential reader over a TFRecord stream held in memory (a chunk is a few MB).
class RecordReader {
 public:
  // mode kModeAuto: zlib when the first two bytes are a zlib header (RFC 1950: method 8, window <= 15, the pair a
  // multiple of 31) and the first twelve are not a plain record header with a matching length CRC (a plain record of
  // 376 bytes starts 78 01, a valid zlib header too).
  ReadStatus Open(const std::string& path, int mode = kModeAuto) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return ReadStatus{kReadIo, "cannot open " + path};
    std::vector<uint8_t> raw;
    uint8_t buf[1 << 16];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + n);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) return ReadStatus{kReadIo, "cannot read " + path};
    return OpenBytes(raw.data(), raw.size(), mode);
  }
  ReadStatus OpenBytes(const uint8_t* p, size_t n, int mode = kModeAuto) {
    data_.clear();
    pos_ = 0;
    index_ = 0;
    tail_ = ReadStatus{};
    if (mode == kModeAuto) mode = LooksZlib(p, n) ? kModeZlib : kModePlain;
    if (mode != kModeZlib) {
      data_.assign(p, p + n);
      return ReadStatus{};
    }
    // Inflate everything that is there.  A stream that ends early or turns corrupt still yields its leading records;
    // the error is reported by Next() at the record it cuts, so that the message can name it.
    z_stream z;
    std::memset(&z, 0, sizeof z);
    if (inflateInit2(&z, MAX_WBITS) != Z_OK) return ReadStatus{kReadZlib, "inflateInit2 failed"};
    // zlib counts in 32 bits: the input is fed in pieces.  The inflated stream is capped (kMaxInflated): a chunk is a
    // few MB, and a hostile one must not be able to take all memory.
    const size_t kPiece = (size_t)1 << 30;
    size_t fed = 0;
    uint8_t out[1 << 16];
    int rc = Z_OK;
    while (rc == Z_OK) {
      if (z.avail_in == 0 && fed < n) {
        const size_t piece = n - fed < kPiece ? n - fed : kPiece;
        z.next_in = const_cast<Bytef*>(p + fed);
        z.avail_in = (uInt)piece;
        fed += piece;
      }
      z.next_out = out;
      z.avail_out = sizeof out;
      rc = inflate(&z, Z_NO_FLUSH);
      data_.insert(data_.end(), out, out + (sizeof out - z.avail_out));
      if (data_.size() > kMaxInflated) {
        tail_ = ReadStatus{kReadZlib, "the zlib stream inflates to more than " + std::to_string(kMaxInflated >> 20) + " MiB"};
        break;
      }
      if (rc == Z_BUF_ERROR || (rc == Z_OK && z.avail_in == 0 && fed == n && z.avail_out != 0)) {
        tail_ = ReadStatus{kReadTruncated, "truncated stream (the zlib stream ends before its end marker)"};
        break;
      }
    }
    if (rc != Z_OK && rc != Z_STREAM_END && tail_.ok())
      tail_ = ReadStatus{kReadZlib, std::string("corrupt zlib stream (") + (z.msg ? z.msg : "inflate failed") + ")"};
    inflateEnd(&z);
    return ReadStatus{};
  }
  // The next record's payload (valid until the reader is reopened or destroyed).  *eof: the stream ended cleanly.
  ReadStatus Next(const uint8_t** payload, size_t* len, bool* eof) {
    *eof = false;
    const size_t left = data_.size() - pos_;
    if (left == 0) {
      if (!tail_.ok()) return ReadError(tail_.code, index_, tail_.msg);
      *eof = true;
      return ReadStatus{};
    }
    auto cut = [&](const std::string& where) {
      return tail_.ok() || tail_.code == kReadTruncated
                 ? ReadError(kReadTruncated, index_, "truncated stream (ends inside the " + where + ")")
                 : ReadError(tail_.code, index_, tail_.msg);
    };
    if (left < 12) return cut("record header");
    const uint8_t* h = data_.data() + pos_;
    uint64_t n;
    uint32_t hc, fc;
    std::memcpy(&n, h, 8);
    std::memcpy(&hc, h + 8, 4);
    if (hc != MaskedCrc32c(h, 8)) return ReadError(kReadCrc, index_, "CRC of the length field does not match");
    if (n > left - 12 || left - 12 - n < 4)
      return cut("payload: the length field says " + std::to_string(n) + " bytes, " + std::to_string(left - 12) + " remain");
    std::memcpy(&fc, h + 12 + n, 4);
    if (fc != MaskedCrc32c(h + 12, (size_t)n)) return ReadError(kReadCrc, index_, "CRC of the payload does not match");
    *payload = h + 12;
    *len = (size_t)n;
    pos_ += 16 + (size_t)n;
    ++index_;
    return ReadStatus{};
  }
  long index() const { return index_; }   // records returned so far = index of the next one
  static constexpr size_t kMaxInflated = (size_t)1 << 30;   // 1 GiB: some 200,000 positions

 private:
  static bool LooksZlib(const uint8_t* p, size_t n) {
    if (n < 2 || (p[0] & 0x0f) != 8 || (p[0] >> 4) > 7 || ((p[0] << 8) | p[1]) % 31 != 0) return false;
    if (n >= 12) {
      uint32_t hc;
      std::memcpy(&hc, p + 8, 4);
      if (hc == MaskedCrc32c(p, 8)) return false;
    }
    return true;
  }
  std::vector<uint8_t> data_;
  size_t pos_ = 0;
  long index_ = 0;
  ReadStatus tail_;
};

// ---- tf.Example ------------------------------------------------------------------------------------------------
// A bounds-checked cursor over [p, end): no read ever passes `end`.
struct PbCursor {
  const uint8_t* p;
  const uint8_t* end;
  size_t left() const { return (size_t)(end - p); }
  bool Varint(uint64_t* v) {
    uint64_t r = 0;
    for (int shift = 0; shift < 70; shift += 7) {
      if (p == end) return false;
      const uint8_t b = *p++;
      if (shift < 64) r |= (uint64_t)(b & 0x7f) << shift;
      if (!(b & 0x80)) { *v = r; return true; }
    }
    return false;   // more than ten bytes
  }
  bool Tag(int* field, int* wire) {
    uint64_t t;
    if (!Varint(&t) || (t >> 3) == 0 || (t >> 3) > 0x1fffffff) return false;
    *field = (int)(t >> 3);
    *wire = (int)(t & 7);
    return true;
  }
  bool Sub(PbCursor* sub) {   // a length-delimited field's bytes
    uint64_t n;
    if (!Varint(&n) || n > left()) return false;
    *sub = PbCursor{p, p + n};
    p += n;
    return true;
  }
  bool Skip(int wire) {
    uint64_t v;
    PbCursor s;
    switch (wire) {
      case 0: return Varint(&v);
      case 1: if (left() < 8) return false; p += 8; return true;
      case 2: return Sub(&s);
      case 5: if (left() < 4) return false; p += 4; return true;
      default: return false;   // groups (3, 4) and 6, 7: not in a tf.Example
    }
  }
};

// What a Feature holds, as far as a dataset row needs it: the first bytes value, the first float.
struct FeatureView {
  int kind = 0;   // 0 none set, 1 bytes_list, 2 float_list, 3 int64_list
  const uint8_t* bytes = nullptr;
  size_t nbytes = 0;
  int n_values = 0;
  float f0 = 0.0f;
};

inline bool ParseFeature(PbCursor c, FeatureView* out) {
  *out = FeatureView{};
  int field, wire;
  while (c.left() > 0) {
    if (!c.Tag(&field, &wire)) return false;
    if (wire != 2 || field < 1 || field > 3) {
      if (!c.Skip(wire)) return false;
      continue;
    }
    PbCursor list;
    if (!c.Sub(&list)) return false;
    FeatureView v;   // the oneof: the last list on the wire wins
    v.kind = field;
    while (list.left() > 0) {
      int lf, lw;
      if (!list.Tag(&lf, &lw)) return false;
      if (lf != 1) {
        if (!list.Skip(lw)) return false;
        continue;
      }
      if (field == 1 && lw == 2) {
        PbCursor b;
        if (!list.Sub(&b)) return false;
        if (v.n_values++ == 0) { v.bytes = b.p; v.nbytes = b.left(); }
      } else if (field == 2 && lw == 2) {   // packed floats
        PbCursor b;
        if (!list.Sub(&b) || b.left() % 4 != 0) return false;
        if (v.n_values == 0 && b.left() >= 4) std::memcpy(&v.f0, b.p, 4);
        v.n_values += (int)(b.left() / 4);
      } else if (field == 2 && lw == 5) {   // one float, not packed
        if (list.left() < 4) return false;
        if (v.n_values++ == 0) std::memcpy(&v.f0, list.p, 4);
        list.p += 4;
      } else if (field == 3 && (lw == 0 || lw == 2)) {
        if (!list.Skip(lw)) return false;
        ++v.n_values;
      } else {
        return false;   // a value of the wrong wire type
      }
    }
    *out = v;
  }
  return true;
}

// ---- GoDataset rows -----------------------------------------------------------------------------------------------
struct DatasetRow {
  p3hip_features features;
  p3hip_labels labels;
};

// game::AsLoc(int16) (cc/game/loc.h:29-31): C's truncating / and % by 19.  361 is pass {19,0}; the recorder's noop
// {-1,-1} is encoded -1 * 19 + -1 = -20 and decodes to itself.  A -1 (the reference's own test chunk,
// python/test_data/mixed_schema.tfrecord) decodes to {0,-1}, which is neither kNoopLoc nor kPassLoc: the reference's
// LoadPlanes (cc/nn/engine/go_features.cc:27-36) then sets planes[batch][0][-1][channel], one float in front of the
// row — out of bounds for batch 0, channel 2.  Here k_init compares every board point and the pass location with the
// pair, {0,-1} matches neither, and the move sets no plane and no pass scalar.
inline p3hip_loc DecodeLoc16(int16_t enc) { return p3hip_loc{enc / P3HIP_BOARD_LEN, enc % P3HIP_BOARD_LEN}; }

// The trainer's targets of one record, and whether it has them.
struct RowTargets {
  p3hip_targets targets;
  bool has = false;
};
constexpr int kNumTargetKeys = 10;
constexpr int kNumValueBuckets = 51;   // python/constants.py NUM_V_BUCKETS

// GroundTruth of transforms.py:276-485 from the target keys (got, in kTargetKeys' order; bad[k]: the key's Feature was
// malformed), the row's policy, margin and colour.  False, and *out untouched, when the trainer's parse would fail:
// a FixedLenFeature([]) key of EX_DESC (:18-31) that is absent, of the wrong kind or not exactly one value, own not 361
// bytes, pi_aux not one int16 in 0 .. 361, or an optional key (VarLenFeature, :23-24) that holds values of the wrong kind
// or a first value of the wrong length.
inline bool ParseTargets(const FeatureView* got, const bool* bad, const DatasetRow& row, p3hip_targets* out) {
  for (int k = 0; k < kNumTargetKeys; ++k)
    if (bad[k]) return false;
  const FeatureView &own = got[0], &pi_aux = got[1], &dist = got[2], &mcts = got[3];
  if (own.kind != 1 || own.n_values != 1 || own.nbytes != P3HIP_NUM_LOCS) return false;
  if (pi_aux.kind != 1 || pi_aux.n_values != 1 || pi_aux.nbytes != 2) return false;
  for (int k = 4; k < kNumTargetKeys; ++k)
    if (got[k].kind != 2 || got[k].n_values != 1) return false;
  int16_t aux;
  std::memcpy(&aux, pi_aux.bytes, 2);
  if (aux < 0 || aux >= P3HIP_NUM_MOVES) return false;
  // `.values` of a VarLenFeature: empty when the key is absent, unset or an empty list (:312-333)
  const bool has_dist = dist.kind != 0 && !(dist.kind == 1 && dist.n_values == 0);
  const bool has_mcts = mcts.kind != 0 && !(mcts.kind == 1 && mcts.n_values == 0);
  if (has_dist && (dist.kind != 1 || dist.nbytes != P3HIP_NUM_MOVES * 4)) return false;
  if (has_mcts && (mcts.kind != 1 || mcts.nbytes != kNumValueBuckets * 4)) return false;
  p3hip_targets t;
  std::memset(&t, 0, sizeof t);
  std::memcpy(t.policy, row.labels.policy, sizeof t.policy);
  if (has_dist) std::memcpy(t.policy_aux_dist, dist.bytes, sizeof t.policy_aux_dist);
  const bool white = row.features.color != 1;   // :452 `color == BLACK ? own : -own`
  for (int i = 0; i < P3HIP_NUM_LOCS; ++i) {
    const int v = (int8_t)own.bytes[i];
    t.own[i] = (float)(white ? -v : v);
  }
  for (int b = 0; has_mcts && b < kNumValueBuckets; ++b) {
    int32_t c;   // uint32 on the wire, decoded as int32 (:324-331), then cast to float (model.py:1383)
    std::memcpy(&c, mcts.bytes + 4 * b, 4);
    t.mcts_value_dist[b] = (float)c;
  }
  t.score_margin = row.labels.score_margin;
  t.q6 = got[4].f0; t.q16 = got[5].f0; t.q50 = got[6].f0;
  t.q6_score = got[7].f0; t.q16_score = got[8].f0; t.q50_score = got[9].f0;
  t.policy_aux = aux;
  t.has_pi_aux_dist = has_dist ? 1 : 0;
  t.has_mcts_value_dist = has_mcts ? 1 : 0;
  *out = t;
  return true;
}

// Parses one record's payload into `row`, which is written only when the whole record is good; its targets, when asked
// for, into *tg (tg->has false: the record has none, ParseTargets).
inline ReadStatus ParseDatasetRow(const uint8_t* payload, size_t len, long record, DatasetRow* row, RowTargets* tg = nullptr) {
  static const char* const kTargetKeys[kNumTargetKeys] = {"own", "pi_aux", "pi_aux_dist", "mcts_value_dist", "q6", "q16",
                                                          "q50", "q6_score", "q16_score", "q50_score"};
  FeatureView tgot[kNumTargetKeys];
  bool tbad[kNumTargetKeys] = {};
  static const char* const kKeys[11] = {"bsize", "board", "last_moves", "stones_atari", "stones_two_liberties",
                                        "stones_three_liberties", "stones_in_ladder", "color", "pi", "score_margin", "komi"};
  static const size_t kBytes[11] = {1, P3HIP_NUM_LOCS, P3HIP_NUM_LAST_MOVES * 2, P3HIP_NUM_LOCS, P3HIP_NUM_LOCS,
                                    P3HIP_NUM_LOCS, P3HIP_NUM_LOCS, 1, P3HIP_NUM_MOVES * 4, 0, 0};   // 0: a float
  FeatureView got[11];
  auto bad = [&](const char* what) { return ReadError(kReadParse, record, std::string("not a tf.Example (") + what + ")"); };
  PbCursor ex{payload, payload + len};
  int field, wire;
  while (ex.left() > 0) {
    if (!ex.Tag(&field, &wire)) return bad("bad tag");
    if (field != 1 || wire != 2) {
      if (!ex.Skip(wire)) return bad("bad field");
      continue;
    }
    PbCursor feats;
    if (!ex.Sub(&feats)) return bad("Features overruns the record");
    while (feats.left() > 0) {
      if (!feats.Tag(&field, &wire)) return bad("bad tag in Features");
      if (field != 1 || wire != 2) {
        if (!feats.Skip(wire)) return bad("bad field in Features");
        continue;
      }
      PbCursor entry;
      if (!feats.Sub(&entry)) return bad("map entry overruns Features");
      PbCursor key{nullptr, nullptr}, value{nullptr, nullptr};
      while (entry.left() > 0) {
        if (!entry.Tag(&field, &wire)) return bad("bad tag in a map entry");
        if (wire == 2 && field == 1) { if (!entry.Sub(&key)) return bad("key overruns its map entry"); }
        else if (wire == 2 && field == 2) { if (!entry.Sub(&value)) return bad("Feature overruns its map entry"); }
        else if (!entry.Skip(wire)) return bad("bad field in a map entry");
      }
      for (int k = 0; k < 11; ++k) {
        if (key.left() != std::strlen(kKeys[k]) || std::memcmp(key.p, kKeys[k], key.left()) != 0) continue;
        if (!ParseFeature(value, &got[k])) return bad((std::string("Feature '") + kKeys[k] + "' is malformed").c_str());
      }
      for (int k = 0; tg && k < kNumTargetKeys; ++k) {
        if (key.left() != std::strlen(kTargetKeys[k]) || std::memcmp(key.p, kTargetKeys[k], key.left()) != 0) continue;
        tbad[k] = !ParseFeature(value, &tgot[k]);   // a row needs none of these keys: a malformed one costs the targets only
      }
    }
  }
  for (int k = 0; k < 11; ++k) {
    const int want = kBytes[k] ? 1 : 2;
    if (got[k].kind != want || got[k].n_values < 1)
      return ReadError(kReadMissingKey, record, std::string("missing key '") + kKeys[k] + "'" +
                                                    (got[k].kind == 0 ? "" : kBytes[k] ? " (no bytes value)" : " (no float value)"));
    if (kBytes[k] && got[k].nbytes != kBytes[k])
      return ReadError(kReadBadLength, record, std::string("wrong byte length of '") + kKeys[k] + "': " +
                                                   std::to_string(got[k].nbytes) + ", expected " + std::to_string(kBytes[k]));
  }
  if (got[0].bytes[0] != P3HIP_BOARD_LEN)
    return ReadError(kReadBadValue, record, "bsize is " + std::to_string((int)got[0].bytes[0]) + ", only 19 is supported");
  DatasetRow r;
  std::memset(&r, 0, sizeof r);
  r.features.bsize = P3HIP_BOARD_LEN;
  std::memcpy(r.features.board, got[1].bytes, P3HIP_NUM_LOCS);
  for (int m = 0; m < P3HIP_NUM_LAST_MOVES; ++m) {
    int16_t enc;
    std::memcpy(&enc, got[2].bytes + 2 * m, 2);
    r.features.last_moves[m] = DecodeLoc16(enc);
  }
  std::memcpy(r.features.stones_atari, got[3].bytes, P3HIP_NUM_LOCS);
  std::memcpy(r.features.stones_two_liberties, got[4].bytes, P3HIP_NUM_LOCS);
  std::memcpy(r.features.stones_three_liberties, got[5].bytes, P3HIP_NUM_LOCS);
  std::memcpy(r.features.stones_laddered, got[6].bytes, P3HIP_NUM_LOCS);
  r.features.color = (int8_t)got[7].bytes[0];
  std::memcpy(r.labels.policy, got[8].bytes, P3HIP_NUM_MOVES * 4);
  r.labels.score_margin = got[9].f0;
  r.labels.did_win = got[9].f0 >= 0 ? 1 : 0;   // go_dataset.cc:114 (a NaN margin is a loss there too)
  r.features.komi = got[10].f0;
  *row = r;
  if (tg) tg->has = ParseTargets(tgot, tbad, r, &tg->targets);
  return ReadStatus{};
}

// All rows of one chunk.  Open fails as a whole on the first bad record: no partly read dataset is handed out.
class GoDataset {
 public:
  ReadStatus Open(const std::string& path, int mode = kModeAuto) {
    RecordReader rd;
    ReadStatus st = rd.Open(path, mode);
    return st.ok() ? Read(rd) : st;
  }
  ReadStatus OpenBytes(const uint8_t* p, size_t n, int mode = kModeAuto) {
    RecordReader rd;
    ReadStatus st = rd.OpenBytes(p, n, mode);
    return st.ok() ? Read(rd) : st;
  }
  size_t size() const { return rows_.size(); }
  const DatasetRow& row(size_t i) const { return rows_[i]; }
  // the trainer's targets of row i; null when the record has none
  const p3hip_targets* targets(size_t i) const { return target_of_[i] < 0 ? nullptr : &targets_[(size_t)target_of_[i]]; }

 private:
  ReadStatus Read(RecordReader& rd) {
    std::vector<DatasetRow> rows;
    std::vector<p3hip_targets> targets;
    std::vector<long> target_of;
    RowTargets tg;
    for (;;) {
      const uint8_t* payload;
      size_t len;
      bool eof;
      const long record = rd.index();
      ReadStatus st = rd.Next(&payload, &len, &eof);
      if (!st.ok()) return st;
      if (eof) break;
      DatasetRow row;
      st = ParseDatasetRow(payload, len, record, &row, &tg);
      if (!st.ok()) return st;
      rows.push_back(row);
      target_of.push_back(tg.has ? (long)targets.size() : -1);
      if (tg.has) targets.push_back(tg.targets);
    }
    rows_.swap(rows);
    targets_.swap(targets);
    target_of_.swap(target_of);
    return ReadStatus{};
  }
  std::vector<DatasetRow> rows_;
  std::vector<p3hip_targets> targets_;   // of the rows that have them
  std::vector<long> target_of_;          // row -> index into targets_, -1: none
};

}  // namespace p3
