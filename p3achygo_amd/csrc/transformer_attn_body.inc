// transformer_attn_body.inc — the body of k_tfm_attn<D> and k_tfm_attn_split<D>, included inside the kernel
// (transformer_core.h says why as text).  In scope: the constant D, TfmAttnArgs a, nh = a.heads, the (position p, head)
// whose K and V the workgroup stages, its first query tile qt0 and the first query q1 past its last tile (a wave takes
// every fourth tile; the bound is in queries because that is the spelling k_tfm_attn's code was built from).
// 16 queries per wave step.  S^T = K . Q^T puts a query in each lane column and 4 keys of every 16-key tile in the lane
// (the whole 384-key row of a query in the 4 lanes lane & 15): the softmax reduces in registers and across lanes 16 and
// 32 apart.  O^T = V^T . P^T takes P straight from those registers: k32 step j covers key tiles 2j and 2j + 1, k index
// 8 g + e standing for key 16 (2j + e / 4) + 4 g + e % 4.
// D = 32: the whole row of scores (96 registers) is held, and the softmax subtracts the row's maximum.
// D = 64: S takes two k32 steps per key tile and O four 16-channel tiles; the row of scores would not fit beside them,
// so the softmax is online over blocks of 64 keys: a block's numerators exp2(s - m) use the running maximum m up to and
// including the block (each is at most 1 before its fp16 rounding), and o and the sum are rescaled by exp2(m_old - m)
// when m grows.  K and V^T fill 103 KiB of LDS: one workgroup per CU.
  constexpr int kKs = D + 8, kVt = kTfmLPad + 8;
  __shared__ __attribute__((aligned(16))) _Float16 ks[kTfmLPad * kKs];
  __shared__ __attribute__((aligned(16))) _Float16 vt[D * kVt];
  const size_t base = ((size_t)p * nh + head) * kTfmLPad * D;
  for (int i = threadIdx.x; i < kTfmLPad * D / 8; i += 256) {
    const int key = i / (D / 8), d0 = 8 * (i % (D / 8));
    *reinterpret_cast<h8*>(ks + key * kKs + d0) = *reinterpret_cast<const h8*>(a.k + base + key * D + d0);
    const h8 v = *reinterpret_cast<const h8*>(a.v + base + key * D + d0);
#pragma unroll
    for (int e = 0; e < 8; ++e) vt[(d0 + e) * kVt + key] = v[e];
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4, n = lane & 15;
  // log2(e) / sqrt(head_dim)
  const float kScale = D == 32 ? 1.4426950408889634f / 5.656854249492381f : 1.4426950408889634f / 8.0f;
  constexpr int kKt = kTfmLPad / 16;   // 24 key tiles
  constexpr int kQs = D / 32;          // k32 steps of q . k
  constexpr int kDt = D / 16;          // 16-channel tiles of o
  // O^T += V^T . P^T over k32 step j (key tiles 2j, 2j + 1) with P's fp16 fragment bp
  auto pv_step = [&](int j, const h8& bp, f32x4* o) {
#pragma unroll
    for (int dt = 0; dt < kDt; ++dt) {
      const _Float16* row = vt + (16 * dt + n) * kVt + 32 * j + 4 * gq;
      const h4 lo = *reinterpret_cast<const h4*>(row), hi = *reinterpret_cast<const h4*>(row + 16);
      const h8 av = h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      o[dt] = mfma(av, bp, o[dt]);
    }
  };
  auto to_h8 = [](const f32x4& x, const f32x4& y) {
    return h8{(_Float16)x[0], (_Float16)x[1], (_Float16)x[2], (_Float16)x[3],
              (_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
  };
  for (int qt = qt0 + wave; 16 * qt < q1; qt += 4) {
    h8 bq[kQs];
#pragma unroll
    for (int h = 0; h < kQs; ++h) bq[h] = *reinterpret_cast<const h8*>(a.q + base + (size_t)(16 * qt + n) * D + 32 * h + 8 * gq);
    // S^T tile kt, scaled by kScale; keys 361.. are -3e38
    auto score = [&](int kt) {
      f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < kQs; ++h) {
        const h8 ak = *reinterpret_cast<const h8*>(ks + (16 * kt + n) * kKs + 32 * h + 8 * gq);
        r = mfma(ak, bq[h], r);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = 16 * kt + 4 * gq + i;
        r[i] = key < kTfmL ? r[i] * kScale : -3.0e38f;
      }
      return r;
    };
    f32x4 o[kDt];
#pragma unroll
    for (int dt = 0; dt < kDt; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float sum = 0.f;
    if constexpr (D == 32) {   // as the kernel was first written, register for register
      f32x4 s[kKt];
      float m = -3.0e38f;
#pragma unroll
      for (int kt = 0; kt < kKt; ++kt) {
        const h8 ak = *reinterpret_cast<const h8*>(ks + (16 * kt + n) * kKs + 8 * gq);
        s[kt] = mfma(ak, bq[0], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = 16 * kt + 4 * gq + i;
          s[kt][i] = key < kTfmL ? s[kt][i] * kScale : -3.0e38f;
          m = fmaxf(m, s[kt][i]);
        }
      }
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
#pragma unroll
      for (int kt = 0; kt < kKt; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s[kt][i] = exp2f(s[kt][i] - m);
          sum += s[kt][i];
        }
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
#pragma unroll
      for (int j = 0; j < kKt / 2; ++j) {
        const h8 bp = h8{(_Float16)s[2 * j][0], (_Float16)s[2 * j][1], (_Float16)s[2 * j][2], (_Float16)s[2 * j][3],
                         (_Float16)s[2 * j + 1][0], (_Float16)s[2 * j + 1][1], (_Float16)s[2 * j + 1][2],
                         (_Float16)s[2 * j + 1][3]};
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const _Float16* row = vt + (16 * dt + n) * kVt + 32 * j + 4 * gq;
          const h4 lo = *reinterpret_cast<const h4*>(row), hi = *reinterpret_cast<const h4*>(row + 16);
          const h8 av = h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[dt] = mfma(av, bp, o[dt]);
        }
      }
    } else {
      constexpr int kBt = 4;   // key tiles per block
      float m = -3.0e38f;
#pragma unroll 1
      for (int b = 0; b < kKt / kBt; ++b) {
        f32x4 s[kBt];
        float mb = m;
#pragma unroll
        for (int t = 0; t < kBt; ++t) {
          s[t] = score(kBt * b + t);
#pragma unroll
          for (int i = 0; i < 4; ++i) mb = fmaxf(mb, s[t][i]);
        }
        mb = fmaxf(mb, __shfl_xor(mb, 16));
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float alpha = exp2f(m - mb);
        m = mb;
        sum *= alpha;
#pragma unroll
        for (int dt = 0; dt < kDt; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int t = 0; t < kBt; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            s[t][i] = exp2f(s[t][i] - m);
            sum += s[t][i];
          }
#pragma unroll
        for (int j = 0; j < kBt / 2; ++j) pv_step(kBt / 2 * b + j, to_h8(s[2 * j], s[2 * j + 1]), o);
      }
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
    }
    const int query = 16 * qt + n;
    if (query < kTfmL) {
      const float inv = 1.0f / sum;
      const size_t orow = ((size_t)p * kTfmL + query) * (size_t)(nh * D) + head * D;
#pragma unroll
      for (int dt = 0; dt < kDt; ++dt) {
        const h4 r = h4{(_Float16)(o[dt][0] * inv), (_Float16)(o[dt][1] * inv), (_Float16)(o[dt][2] * inv),
                        (_Float16)(o[dt][3] * inv)};
        *reinterpret_cast<h4*>(a.o + orow + 16 * dt + 4 * gq) = r;
      }
    }
  }
