// symmetry.hip — the two kernels of symmetry-averaged evaluation (symmetry.h).
//
// Both are small and bound by memory traffic: per slot at k = 8, k_sym_expand reads one 1,860 B record and writes
// eight (15 KB), k_sym_reduce reads eight 13,664 B rows (109 KB) and writes one row plus one result record.  One
// workgroup of 256 threads per slot.  Rows are 16-byte aligned (kOutStride = 3,416 floats), so the reduce moves them
// as float4 wherever four consecutive floats need no rotation; a feature record is 1,860 B (not a multiple of 16), so
// the expand moves dwords, coalesced, through a copy of the record in LDS.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "../../include/p3hip.h"
#include "kernels.h"
#include "symmetry.h"

namespace p3 {

namespace {

constexpr int kRecBytes = (int)sizeof(p3hip_features);
constexpr int kRecWords = kRecBytes / 4;
static_assert(kRecBytes % 4 == 0, "feature records are whole dwords");
constexpr int kGridOff[5] = {(int)offsetof(p3hip_features, board), (int)offsetof(p3hip_features, stones_atari),
                             (int)offsetof(p3hip_features, stones_two_liberties),
                             (int)offsetof(p3hip_features, stones_three_liberties),
                             (int)offsetof(p3hip_features, stones_laddered)};
constexpr int kLastOff = (int)offsetof(p3hip_features, last_moves);
constexpr int kLastBytes = (int)sizeof(p3hip_loc) * P3HIP_NUM_LAST_MOVES;
static_assert(kLastOff % 4 == 0 && sizeof(p3hip_loc) == 8, "last moves are dword pairs");

// the board-indexed segments of an output row (kernels.h): move logits, move probs, opt probs, opt logits, ownership
constexpr int kBoardSeg[5] = {kOffMoveLogits, kOffMoveProbs, kOffOptProbs, kOffOptLogits, kOffOwnership};
static_assert(kOutStride % 4 == 0, "rows are whole float4s");

__constant__ SymMaps d_maps = make_sym_maps();

// where copy (symmetry s) holds the value that lands on row entry e after the inverse rotation
__device__ inline int reduce_src(int e, int s) {
#pragma unroll
  for (int g = 0; g < 5; ++g) {
    const int p = e - kBoardSeg[g];
    if (p >= 0 && p < kSymLocs) return kBoardSeg[g] + d_maps.fwd[s][p];
  }
  return e;
}
__device__ inline bool touches_board(int e0) {   // any of e0 .. e0 + 3 board-indexed?
#pragma unroll
  for (int g = 0; g < 5; ++g)
    if (e0 + 3 >= kBoardSeg[g] && e0 < kBoardSeg[g] + kSymLocs) return true;
  return false;
}

// Stages one 1,860 B record in LDS (both expand kernels)
__device__ inline void stage_record(uint32_t* rec, const unsigned char* in, int tid) {
  const uint32_t* w32 = reinterpret_cast<const uint32_t*>(in);
  for (int w = tid; w < kRecWords; w += 256) rec[w] = w32[w];
  __syncthreads();
}

// One copy: the staged record under symmetry s -> out, as coalesced dwords (both expand kernels)
__device__ inline void expand_copy(const uint32_t* rec, int s, uint32_t* out, int tid) {
  const unsigned char* rb = reinterpret_cast<const unsigned char*>(rec);
  for (int w = tid; w < kRecWords; w += 256) {
    const int o = 4 * w;
    uint32_t v = 0;
    if (o >= kLastOff && o < kLastOff + kLastBytes) {
      // one coordinate of a last move: on-board locations go through the forward map, the rest is copied
      const int m = (o - kLastOff) / 8, first = kLastOff / 4 + 2 * m;
      const int li = (int)rec[first], lj = (int)rec[first + 1];
      v = rec[w];
      if (li >= 0 && li < kSymN && lj >= 0 && lj < kSymN) {
        const int t = d_maps.fwd[s][li * kSymN + lj];
        v = (uint32_t)((o - kLastOff) % 8 == 0 ? t / kSymN : t % kSymN);
      }
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        int src = o + b;
#pragma unroll
        for (int g = 0; g < 5; ++g) {
          const int p = o + b - kGridOff[g];
          if (p >= 0 && p < kSymLocs) src = kGridOff[g] + d_maps.inv[s][p];   // out[fwd[s][i]] = in[i]
        }
        v |= (uint32_t)rb[src] << (8 * b);
      }
    }
    out[w] = v;
  }
}

// One slot: the k rows from `base` on (copy j under symmetry sym_at(j)) rotated back and averaged into `out`, the
// first kResultFloats a second time into `res` (both reduce kernels)
template <class SymAt>
__device__ inline void reduce_rows(const float* base, int k, SymAt sym_at, float* out, float* res, int tid) {
  const float kf = (float)k;
  for (int c = tid; c < kOutStride / 4; c += 256) {
    const int e0 = 4 * c;
    float r[4];
    if (!touches_board(e0)) {
      float4 acc = *reinterpret_cast<const float4*>(base + e0);
      for (int j = 1; j < k; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(base + (size_t)j * kOutStride + e0);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
      r[0] = acc.x / kf; r[1] = acc.y / kf; r[2] = acc.z / kf; r[3] = acc.w / kf;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float acc = base[reduce_src(e0 + q, sym_at(0))];
        for (int j = 1; j < k; ++j) acc += base[(size_t)j * kOutStride + reduce_src(e0 + q, sym_at(j))];
        r[q] = acc / kf;
      }
    }
    *reinterpret_cast<float4*>(out + e0) = make_float4(r[0], r[1], r[2], r[3]);
    if (res)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (e0 + q < kResultFloats) res[e0 + q] = r[q];
  }
}

// The symmetries of a slot's mask in ascending order, one per nibble (uniform over the workgroup); *k: how many
__device__ inline uint32_t pack_syms(uint32_t mask, int* k) {
  uint32_t packed = 0;
  int n = 0;
#pragma unroll
  for (int s = 0; s < kNumSyms; ++s)
    if (mask & (1u << s)) packed |= (uint32_t)s << (4 * n++);
  *k = n;
  return packed;
}

__global__ __launch_bounds__(256) void k_sym_expand(SymExpandArgs a) {
  __shared__ uint32_t rec[kRecWords];
  const int slot = blockIdx.x, tid = threadIdx.x;
  stage_record(rec, a.in + (size_t)slot * kRecBytes, tid);
  for (int j = 0; j < a.k; ++j)
    expand_copy(rec, a.syms[j], reinterpret_cast<uint32_t*>(a.out + ((size_t)slot * a.k + j) * kRecBytes), tid);
}

__global__ __launch_bounds__(256) void k_sym_reduce(SymReduceArgs a) {
  const int slot = blockIdx.x, tid = threadIdx.x, k = a.k;
  reduce_rows(a.rows + (size_t)slot * k * kOutStride, k, [&](int j) { return a.syms[j]; },
              a.out + (size_t)slot * kOutStride, a.res ? a.res + (size_t)slot * kResultFloats : nullptr, tid);
}

// P3HIP_FLAG_SYMMETRY_SLOT: the slot's own mask and first row come from the table uploaded with the features.  A table
// entry that would leave the `cap` rows (none that sym_rows accepted does) writes nothing.
__global__ __launch_bounds__(256) void k_sym_expand_slots(SymExpandSlotsArgs a) {
  __shared__ uint32_t rec[kRecWords];
  const int slot = blockIdx.x, tid = threadIdx.x;
  int k;
  const uint32_t syms = pack_syms(a.mask[slot], &k);
  const int first = a.first[slot];
  if (k < 1 || first < 0 || first + k > a.cap) return;
  stage_record(rec, a.in + (size_t)slot * kRecBytes, tid);
  for (int j = 0; j < k; ++j)
    expand_copy(rec, (int)(syms >> (4 * j)) & 7, reinterpret_cast<uint32_t*>(a.out + ((size_t)first + j) * kRecBytes), tid);
}

__global__ __launch_bounds__(256) void k_sym_reduce_slots(SymReduceSlotsArgs a) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  int k;
  const uint32_t syms = pack_syms(a.mask[slot], &k);
  const int first = a.first[slot];
  if (k < 1 || first < 0 || first + k > a.cap) return;
  reduce_rows(a.rows + (size_t)first * kOutStride, k, [=](int j) { return (int)(syms >> (4 * j)) & 7; },
              a.out + (size_t)slot * kOutStride, a.res ? a.res + (size_t)slot * kResultFloats : nullptr, tid);
}

}  // namespace

hipError_t launch_sym_expand(const SymExpandArgs& a, hipStream_t s) {
  if (a.n < 1 || a.k < 1 || a.k > kNumSyms) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sym_expand, dim3(a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sym_reduce(const SymReduceArgs& a, hipStream_t s) {
  if (a.n < 1 || a.k < 1 || a.k > kNumSyms) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sym_reduce, dim3(a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

int sym_rows(const uint8_t* masks, int n, int rows, int* first, int* total) {
  if (!masks || n < 1) return 1;
  long sum = 0;
  for (int r = 0; r < n; ++r) {
    if (masks[r] == 0) return 1;
    if (first) first[r] = (int)sum;
    sum += __builtin_popcount(masks[r]);
  }
  if (total) *total = (int)sum;
  return sum > rows ? 1 : 0;
}

hipError_t launch_sym_expand_slots(const SymExpandSlotsArgs& a, int total, hipStream_t s) {
  if (a.n < 1 || total < a.n || total > a.cap) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sym_expand_slots, dim3(a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sym_reduce_slots(const SymReduceSlotsArgs& a, int total, hipStream_t s) {
  if (a.n < 1 || total < a.n || total > a.cap) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sym_reduce_slots, dim3(a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

void sym_maps(uint16_t fwd[kNumSyms][kSymLocs], uint16_t inv[kNumSyms][kSymLocs]) {
  static constexpr SymMaps m = make_sym_maps();
  memcpy(fwd, m.fwd, sizeof m.fwd);
  memcpy(inv, m.inv, sizeof m.inv);
}

}  // namespace p3
