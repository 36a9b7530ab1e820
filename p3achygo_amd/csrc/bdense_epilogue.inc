// bdense_epilogue.inc — the epilogue of one broadcast-dense pass, in bdense_passes (layer_kernels.h: k_bdense,
// k_bdense_any and the fused tail of k_block) and bdense_one_pass (edge_split.hip: k_bdense_split), included as text
// after the pass's K loop: + dense bias, mish(bn1(.)), -> u in the piece layout.  Rows = channel (regs), cols = j (lanes).
// In scope: acc2 (the pass's accumulators), jp, jg, ct, lr, h, p_bias, p_scale, p_shift, u, pos, half, C, CH.  A wave
// whose channel tile is inactive leaves before this text (`continue` / `return`), which stays with each caller.
  const f32x16 acc[2] = {acc2[0][0], acc2[1][0]};
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int j = jp * 128 + jg * 64 + mt * 32 + lr;
    if (j >= kNLoc) continue;
    const float bj = p_bias[j];
    // channel blocks g4 = 2*gp and 2*gp + 1: each lane's quad is one 8-byte half of a
    // block's piece; after the swap lanes 0-31 hold the whole piece of block 2*gp, lanes
    // 32-63 that of block 2*gp + 1 (see epilogue_store in conv_core.h)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      h4 o[2];
      {
        const int g4 = 2 * gp;
        const int c = half * CH + ct * 32 + g4 * 8 + h * 4;
        const f32x4 sc0 = scale_log2e(*(const f32x4*)(p_scale + c)), sh0 = scale_log2e(*(const f32x4*)(p_shift + c));
        const f32x4 sc1 = scale_log2e(*(const f32x4*)(p_scale + c + 8)), sh1 = scale_log2e(*(const f32x4*)(p_shift + c + 8));
        const f32x4 v0 = {acc[mt][g4 * 4] + bj, acc[mt][g4 * 4 + 1] + bj, acc[mt][g4 * 4 + 2] + bj, acc[mt][g4 * 4 + 3] + bj};
        const f32x4 v1 = {acc[mt][g4 * 4 + 4] + bj, acc[mt][g4 * 4 + 5] + bj, acc[mt][g4 * 4 + 6] + bj, acc[mt][g4 * 4 + 7] + bj};
        bn_mish8_l2(v0, v1, sc0, sh0, sc1, sh1, o[0], o[1]);
      }
      half_swap32(o[0], o[1]);
      const h8 piece = {o[0][0], o[0][1], o[0][2], o[0][3], o[1][0], o[1][1], o[1][2], o[1][3]};
      const int cb = (half * CH + ct * 32) / 8 + 2 * gp + h;   // this lane's channel block
      *(h8*)(u + ((size_t)pos * (C / 8) + cb) * (kNLoc * 8) + j * 8) = piece;
    }
  }
