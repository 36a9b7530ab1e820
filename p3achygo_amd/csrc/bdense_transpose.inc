// bdense_transpose.inc — a thread's six pairs of board points scattered, transposed, from its prefetch registers into
// Tt[c][i] in LDS: t[pos][cblk][loc][8] -> Tt[c][i], one ds_write_b32 per channel and pair.  In bdense_body
// (layer_kernels.h) and k_bdense_split (edge_split.hip), included as text under the caller's guard (this thread's
// channel block is one that the pass / item stages), which stays with each caller.
// In scope: xr (XRegs, filled by the caller's pair_load), combo (channel block of the pass), l32, smem.
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int loc = 2 * (l32 + 32 * i);
    if (loc >= kNLoc) continue;
    const h8 v0 = xr.v[2 * i];
    h8 v1 = xr.v[2 * i + 1];
    if (loc + 1 >= kNLoc) v1 = h8{0, 0, 0, 0, 0, 0, 0, 0};   // board point 361 is padding (K = 384)
#pragma unroll
    for (int e = 0; e < 8; ++e) *(h2*)(smem + (combo * 8 + e) * kTtStride + loc * 2) = h2{v0[e], v1[e]};
  }
