// stem_planes.inc — a position's input of the stem, in init_body (layer_kernels.h) and k_init_split (edge_split.hip),
// included inside the position loop as text: the 15 binary feature planes expanded from the packed features into the
// act buffer in LDS (one thread per board point; channel 15 is a zero pad), and the eight game-state scalars gsv[8]
// (LoadPlanes / LoadFeatures).  A changed feature offset or a new plane is changed here, for both stems.
// In scope: InitArgs a, pos, smem, G = Geo<1, 16, 5>.  Declares f (the position's p3hip_features bytes), color, gsv[8].
  const unsigned char* f = (const unsigned char*)a.feats + (size_t)pos * FeatOff::size;
  const int color = (signed char)f[FeatOff::color];
  // ---- planes -> LDS (one thread per board point) ---------------------------------
  for (int loc = threadIdx.x; loc < kNLoc; loc += kWG) {
    h8 lo = {0, 0, 0, 0, 0, 0, 0, 0}, hi = {0, 0, 0, 0, 0, 0, 0, 0};
    auto our = [&](int off) {
      return (_Float16)((signed char)f[off + loc] == color ? 1.0f : 0.0f);
    };
    auto opp = [&](int off) {
      return (_Float16)((signed char)f[off + loc] == -color ? 1.0f : 0.0f);
    };
    lo[0] = our(FeatOff::board); lo[1] = opp(FeatOff::board);
    lo[7] = our(FeatOff::atari); hi[0] = opp(FeatOff::atari);
    hi[1] = our(FeatOff::two); hi[2] = opp(FeatOff::two);
    hi[3] = our(FeatOff::three); hi[4] = opp(FeatOff::three);
    hi[5] = our(FeatOff::ladder); hi[6] = opp(FeatOff::ladder);
    const int y = (loc * 3450) >> 16, xx = loc - y * kBL;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      const int* lm = (const int*)(f + FeatOff::last + m * 8);
      if (lm[0] == y && lm[1] == xx) lo[2 + m] = (_Float16)1.0f;  // pass {19,0}/noop never match
    }
    const int s = G::PADTOP + y * G::S + xx;
    *(h8*)(smem + s * G::SLOTB) = lo;
    *(h8*)(smem + s * G::SLOTB + 16) = hi;
  }
  // ---- game-state scalars (LoadFeatures) ------------------------------------------
  float gsv[8];
  gsv[0] = color == 1 ? 1.0f : 0.0f;
  gsv[1] = color == 1 ? 0.0f : 1.0f;
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    const int* lm = (const int*)(f + FeatOff::last + m * 8);
    gsv[2 + m] = (lm[0] == 19 && lm[1] == 0) ? 1.0f : 0.0f;
  }
  gsv[7] = (color == 1 ? -1.0f : 1.0f) * (*(const float*)(f + FeatOff::komi)) / 15.0f;
