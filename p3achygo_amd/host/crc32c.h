// crc32c.h — the checksum of TFRecord framing, shared by the chunk writer (tf_recorder.h) and reader (tf_reader.h).
#pragma once
#include <cstddef>
#include <cstdint>

namespace p3 {

// ---- CRC32C (Castagnoli, reflected 0x82F63B78), masked as TFRecord wants it --------------
struct Crc32cTable {
  uint32_t v[256];
  Crc32cTable() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
      v[i] = c;
    }
  }
};
inline uint32_t Crc32c(const void* data, size_t n, uint32_t crc = 0) {
  static const Crc32cTable table;   // built once, by whichever thread comes first (the writer and the reader share it)
  crc = ~crc;
  const uint8_t* p = (const uint8_t*)data;
  for (size_t i = 0; i < n; ++i) crc = table.v[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
  return ~crc;
}
inline uint32_t MaskedCrc32c(const void* data, size_t n) {   // crc32.h:38-43
  const uint32_t crc = Crc32c(data, n);
  return ((crc >> 15) | (crc << 17)) + 0xa282ead8u;
}

}  // namespace p3
