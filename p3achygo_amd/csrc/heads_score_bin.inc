// heads_score_bin.inc — the logit of score bin sidx before gamma: score_out . mish(base + sv * score_pre[2H]) + b.
// In k_heads (kernels.hip) and k_heads_points (edge_split.hip), included as text inside the loop over a thread's bins.
// In scope: V, sidx, score_out_b and, in LDS, base [V], w_sp [V] (row 2H of score_pre_w), w_so [V].  Declares s.
  const float sv = 0.05f * (float)(sidx - 400) + 0.025f;
  float s = score_out_b;
  const int z = launder(0);   // keeps the LDS reads inside the bin loop
#pragma unroll 8
  for (int k = 0; k < V; ++k) s += mish_f(base[z + k] + sv * w_sp[z + k]) * w_so[z + k];
