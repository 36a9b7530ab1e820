// stem_epilogue.inc — the epilogue of one output pass of the stem, in init_body (layer_kernels.h) and k_init_split
// (edge_split.hip), included as text after the pass's K loop: + (gs . Wg + b)[c]  -> x.
// In scope: acc (the pass's accumulators), cp, CP, G, T, lg, lr, h, InitArgs a, pos, C, bias_lds (the game-state dense in
// LDS) and bias_cp, the pass at which bias_lds begins: init_body keeps all C channels (cp), k_init_split its own pass's (0).
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int cl = acc_chan<G, CP>(mt, g4), c = cp * CP + cl;
      const f32x4 bias = *(const f32x4*)(bias_lds + (bias_cp * CP + cl));
#pragma unroll
      for (int j = 0; j < T::NT; ++j) {
        const int t = lg + j * T::LG;
        if (t >= G::NT_TOTAL) continue;
        const int r = t * 32 + lr;
        int loc;
        if (!row_valid<G::S>(r, loc)) continue;
        h4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (_Float16)(acc[mt][j][g4 * 4 + i] + bias[i]);
        *(h4*)(a.x + ((size_t)pos * (C / 8) + (c >> 3)) * (kNLoc * 8) + loc * 8 + h * 4) = o;
      }
    }
