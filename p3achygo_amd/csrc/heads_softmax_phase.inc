// heads_softmax_phase.inc — the last phase of k_heads<H, V> and k_headsx<C, H, V> (kernels.hip), included inside the
// position loop as text (DESIGN.md §16 says why not as a function): the raw logits out, the policy, optimistic-policy and
// score softmaxes with their reductions fused, the value softmax, and the barrier that ends the position.
// In scope: L = HeadsLds<H, V>, sc (the group's scratch), t, wid, lane, live, out, res.
// In: sc[L::pi / L::opt] (362 logits each), sc[L::logits] (800), sc[L::misc], sc[L::misc + 1] (outcome logits).
  float m3[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (int i = t; i < 362; i += 256) {
    const float p = sc[L::pi + i], o = sc[L::opt + i];
    if (live) {
      out[kOffMoveLogits + i] = p;
      out[kOffOptLogits + i] = o;
      if (res) res[kOffMoveLogits + i] = p;
    }
    m3[0] = fmaxf(m3[0], p);
    m3[1] = fmaxf(m3[1], o);
  }
  for (int i = t; i < 800; i += 256) {
    const float l = sc[L::logits + i];
    if (live) out[kOffScoreLogits + i] = l;
    m3[2] = fmaxf(m3[2], l);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) m3[r] = wave_max(m3[r]);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) sc[L::red + r * 4 + wid] = m3[r];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 3; ++r)
    m3[r] = fmaxf(fmaxf(sc[L::red + r * 4], sc[L::red + r * 4 + 1]),
                  fmaxf(sc[L::red + r * 4 + 2], sc[L::red + r * 4 + 3]));
  __syncthreads();   // red is rewritten below
  float s3[3] = {0.0f, 0.0f, 0.0f};
  for (int i = t; i < 362; i += 256) {
    const float e0 = __expf(sc[L::pi + i] - m3[0]), e1 = __expf(sc[L::opt + i] - m3[1]);
    sc[L::pi + i] = e0;
    sc[L::opt + i] = e1;
    s3[0] += e0;
    s3[1] += e1;
  }
  for (int i = t; i < 800; i += 256) {
    const float e = __expf(sc[L::logits + i] - m3[2]);
    sc[L::logits + i] = e;
    s3[2] += e;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) s3[r] = wave_sum(s3[r]);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) sc[L::red + r * 4 + wid] = s3[r];
  }
  __syncthreads();
  if (live) {
    const float i0 = 1.0f / (sc[L::red + 0] + sc[L::red + 1] + sc[L::red + 2] + sc[L::red + 3]);
    const float i1 = 1.0f / (sc[L::red + 4] + sc[L::red + 5] + sc[L::red + 6] + sc[L::red + 7]);
    const float i2 = 1.0f / (sc[L::red + 8] + sc[L::red + 9] + sc[L::red + 10] + sc[L::red + 11]);
    for (int i = t; i < 362; i += 256) {
      out[kOffMoveProbs + i] = sc[L::pi + i] * i0;
      out[kOffOptProbs + i] = sc[L::opt + i] * i1;
      if (res) {
        res[kOffMoveProbs + i] = sc[L::pi + i] * i0;
        res[kOffOptProbs + i] = sc[L::opt + i] * i1;
      }
    }
    for (int i = t; i < 800; i += 256) {
      out[kOffScoreProbs + i] = sc[L::logits + i] * i2;
      if (res) res[kOffScoreProbs + i] = sc[L::logits + i] * i2;
    }
    if (t == 0) {
      const float v0 = sc[L::misc], v1 = sc[L::misc + 1];
      const float m = fmaxf(v0, v1);
      const float e0 = __expf(v0 - m), e1 = __expf(v1 - m);
      out[kOffValueProbs] = e0 / (e0 + e1);
      out[kOffValueProbs + 1] = e1 / (e0 + e1);
      if (res) {
        res[kOffValueProbs] = e0 / (e0 + e1);
        res[kOffValueProbs + 1] = e1 / (e0 + e1);
      }
    }
  }
  __syncthreads();
