// heads_dense_phase.inc — the small dense layers of k_heads<H, V> and k_headsx<C, H, V> (kernels.hip), included inside
// the position loop as text: the pooled-g bias, the outcome / gamma / score embeddings, the two pass logits, then the
// outcome logits, err2 and gamma.
// In scope: H, V, L = HeadsLds<H, V>, hl (the staged weights), sc (the group's scratch), t, live, out, res and the scalars
// pass_b0, opt_pass_b, gamma_out_b.  In: sc[L::gp], sc[L::vp] (pooled g and v) behind a barrier.
// Out: sc[L::gbias] after the inner barrier; sc[L::emb / gpre / base], sc[L::pi + 361], sc[L::opt + 361] and sc[L::misc ..
// misc + 2] after the including kernel's next barrier.
  if (t < H) {
    float s = hl[L::gd_b + t];
#pragma unroll 8
    for (int k = 0; k < 2 * H; ++k) s += sc[L::gp + k] * hl[L::gd_w + k * H + t];
    sc[L::gbias + t] = s;
  } else if (t >= 64 && t < 64 + V) {
    const int o = t - 64;
    float s = hl[L::oq_embed_b + o], gm = hl[L::gamma_pre_b + o], b = hl[L::score_pre_b + o];
#pragma unroll 8
    for (int k = 0; k < 2 * H; ++k) {
      const float x = sc[L::vp + k];
      s += x * hl[L::oq_embed_w + k * V + o];
      gm += x * hl[L::gamma_pre_w + k * V + o];
      b += x * hl[L::score_pre_w + k * V + o];
    }
    sc[L::emb + o] = mish_f(s);
    sc[L::gpre + o] = mish_f(gm);
    sc[L::base + o] = b;
  } else if (t == 192) {
    float s0 = pass_b0, so = opt_pass_b;
#pragma unroll 8
    for (int k = 0; k < 2 * H; ++k) {
      s0 += sc[L::gp + k] * hl[L::pass_w + k * 2];
      so += sc[L::gp + k] * hl[L::opt_pass_w + k];
    }
    sc[L::pi + 361] = s0 - 3.0f;
    sc[L::opt + 361] = so - 3.0f;
  }
  __syncthreads();
  if (t < 14) {
    float s = hl[L::oq_out_b + t];
#pragma unroll 8
    for (int k = 0; k < V; ++k) s += sc[L::emb + k] * hl[L::oq_out_w + k * 14 + t];
    if (t < 2) sc[L::misc + t] = s;
    if (live) {
      if (t < 2) out[kOffOutcomeLogits + t] = s;
      if (t == 5) {
        out[kOffErr2] = 4.0f / (1.0f + __expf(-s));
        if (res) res[kOffErr2] = out[kOffErr2];
      }
    }
  } else if (t == 64) {
    float s = gamma_out_b;
#pragma unroll 8
    for (int k = 0; k < V; ++k) s += sc[L::gpre + k] * hl[L::gamma_out_w + k];
    if (live) out[kOffGamma] = s;
    const float sp = s > 20.0f ? s : log1pf(__expf(s));
    sc[L::misc + 2] = fminf(sp, 10.0f);
  }
