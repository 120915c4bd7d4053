// The whole launch of ONE model by the calling workgroup: the body of dense_mb_bf16_kernel and of
// dense_mb_bf16_fleet_kernel (dense_minibatch_bf16.hip), which include this text inside their braces.
// It is text, not a __device__ function: the kernel runs at 255 of 256 VGPRs, and as a function, with
// the argument structs handed over by value or by reference, the single-model entry came out 3 % slower
// (by value, layer tables read from the kernel-argument segment) or with a private segment (by
// reference: the dynamically indexed tables a.L[l] / P.L[l] then live in a scratch copy).  Included in
// the kernel that owns the arguments, the single-model entry compiles to the code it had before.
// In scope at the point of inclusion:
//   a    const DenseMBArgs        what a fleet shares: layer table, batch, Adam constants
//   P    const DenseMBPlanBF16    the LDS plan
//   run  anything with the members of DenseMBRun (sml_dense_fleet.h): the model's own state, rows and
//        steps -- the arguments themselves in the single-model entry, the rebased run in the fleet entry
  extern __shared__ __attribute__((aligned(16))) lds_t S[];
  __shared__ DenseMBLayer sL[DMB_MAXLAYERS];
  __shared__ DenseMBLayerPlanBF16 sP[DMB_MAXLAYERS];
  const int tid = threadIdx.x, nl = a.nl;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, c = lane & 15, g = lane >> 4;
  if (tid == 0) {
#pragma unroll
    for (int l = 0; l < DMB_MAXLAYERS; ++l) {
      sL[l] = a.L[l];
      sP[l] = P.L[l];
    }
  }
  if (tid < P.ntiles) {   // tile table: layer, input block, unit block (unit blocks fastest)
    int l = 0;
    for (int k = 1; k < nl; ++k)
      if (tid >= P.L[k].tile0) l = k;
    const int k = tid - P.L[l].tile0, nj = P.L[l].up >> 4;
    reinterpret_cast<int*>(S + P.ltile)[tid] = (l << 16) | ((k / nj) << 8) | (k % nj);
  }
  if (tid < 3) fptr(S, P.lstat)[STAT_TOT + tid] = 0.0f;
  __syncthreads();

  // ---- the tiles this wave owns: fp32 masters and moments into registers, bf16 image into LDS ----
  f32x4 Tw[SLOTS], Tg[SLOTS], Tm[SLOTS], Tv[SLOTS];
  int ti[SLOTS];
#pragma unroll
  for (int u = 0; u < SLOTS; ++u) {
    const int id = wave + NW * u;
    ti[u] = id < P.ntiles ? __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(S + P.ltile)[id]) : -1;
  }
#pragma unroll
  for (int u = 0; u < SLOTS; ++u) {
    Tw[u] = Tg[u] = Tm[u] = Tv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    TilePos t;
    if (!tile_of(ti[u], t)) continue;
    const DenseMBLayer& L = sL[t.l];
    const int j = t.j0 + c;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = t.i0 + 4 * g + e;
      if (i < L.in && j < L.units) {
        const unsigned f = (unsigned)(L.w_off + i * L.units + j);
        Tw[u][e] = run.flat[f];
        Tm[u][e] = run.m[f];
        Tv[u][e] = run.v[f];
      }
    }
    *reinterpret_cast<bf16x4*>(S + sP[t.l].lw + 2 * (j * sP[t.l].ws + t.i0 + 4 * g)) = pack4(Tw[u]);
  }
  // biases: thread (layer tid / 128 + 4k, unit tid % 128); state b, m, v, gradient = 4 x [up] fp32
  for (int l = tid >> 7; l < nl; l += NT / DMB_MAXW) {
    const int j = tid & (DMB_MAXW - 1), up = sP[l].up;
    if (j >= up) continue;
    const bool real = sL[l].has_bias && j < sL[l].units;
    const unsigned f = (unsigned)(sL[l].b_off + j);
    float* bs = fptr(S, sP[l].lb);
    bs[j] = real ? run.flat[f] : 0.0f;
    bs[up + j] = real ? run.m[f] : 0.0f;
    bs[2 * up + j] = real ? run.v[f] : 0.0f;
    bs[3 * up + j] = 0.0f;
  }

  const int64_t it0 = *run.iter;
  const int O = sL[nl - 1].units, op = sP[nl - 1].up;
  const int64_t avail = run.n - run.row0;
  const int64_t maxsteps = avail > 0 ? (avail + a.batch - 1) / a.batch : 0;
  const int steps = (int)(maxsteps < run.nsteps ? maxsteps : run.nsteps);

  Stage st;
  stage_load(a, run, O, 0, 0, steps, st);
  for (int s = 0; s < steps; ++s) {
    const int64_t left = avail - (int64_t)s * a.batch;
    const int rows_s = left < a.batch ? (int)left : a.batch;
    const int chunks = (rows_s + CH - 1) / CH;
    const float inv_rows = 1.0f / (float)rows_s, inv_n = 1.0f / ((float)rows_s * (float)O);
    for (int k = 0; k < chunks; ++k) {
      const int rows = rows_s - k * CH < CH ? rows_s - k * CH : CH;
      stage_store(S, run, P, op, st);
      if (k + 1 < chunks) stage_load(a, run, O, s, k + 1, steps, st);
      else stage_load(a, run, O, s + 1, 0, steps, st);
      __syncthreads();
      // ---- forward ----
      for (int l = 0; l < nl; ++l) {
        fwd_layer(S, a.L[l], P.L[l], l == 0 ? P.lxb : P.L[l - 1].lhb, l == 0 ? P.xbs : P.L[l - 1].bs, l == nl - 1, wave, c, g);
        __syncthreads();
      }
      loss_phase(S, sL, sP, nl, P.lyt, P.ys, P.lstat, rows, inv_n, inv_rows);
      __syncthreads();
      // ---- backward ----
      for (int l = nl - 1; l >= 1; --l) {
        bwd_layer(S, P.L[l], a.L[l - 1], P.L[l - 1], rows, inv_rows, wave, c, g);
        __syncthreads();
      }
      // ---- weight gradients into the owners' registers: dW[i][j] += sum_r h^T[i][r] dz[r][j] ----
#pragma unroll
      for (int u = 0; u < SLOTS; ++u) {
        TilePos t;
        if (!tile_of(ti[u], t)) continue;
        const int lp = t.l > 0 ? t.l - 1 : 0;
        const int lh = t.l == 0 ? P.lxb : P.L[lp].lhb, sh = t.l == 0 ? P.xbs : P.L[lp].bs;
        const s16x8 ha = tr8(S, lh, 2 * sh, 0, CH, t.i0, c, g);
        const s16x8 db = tr8(S, P.L[t.l].ld, 2 * P.L[t.l].bs, 0, CH, t.j0, c, g);
        Tg[u] = mma(ha, db, Tg[u]);
      }
      // ---- bias gradients: fp32 column sums of the unrounded dz, rows ascending ----
      for (int l = tid >> 7; l < nl; l += NT / DMB_MAXW) {
        const int j = tid & (DMB_MAXW - 1), up = sP[l].up;
        if (j >= up || !sL[l].has_bias) continue;
        const float* dp = fptr(S, sP[l].la) + j;
        float* gb = fptr(S, sP[l].lb) + 3 * up + j;
        float sum = *gb;
        for (int r = 0; r < CH; ++r) sum += dp[r * sP[l].hs];
        *gb = sum;
      }
      if (tid < 3) {   // the step's squared error / correct rows / penalty, rows ascending
        float* stt = fptr(S, P.lstat);
        float tot = stt[STAT_TOT + tid];
        for (int r = 0; r < rows; ++r) tot += stt[CH * tid + r];
        stt[STAT_TOT + tid] = tot;
      }
      __syncthreads();
    }
    // ---- Adam on the owned masters; the bf16 image is re-derived from them ----
    const float lr_t = adam_lr_t(run.lr, a.beta1, a.beta2, (float)(it0 + s + 1));
#pragma unroll
    for (int u = 0; u < SLOTS; ++u) {
      TilePos t;
      if (!tile_of(ti[u], t)) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float mm, vv, pn;
        adam_update(Tg[u][e], Tm[u][e], Tv[u][e], Tw[u][e], lr_t, a.beta1, a.beta2, a.eps, 1.0f, mm, vv, pn);
        Tm[u][e] = mm;
        Tv[u][e] = vv;
        Tw[u][e] = pn;
      }
      Tg[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<bf16x4*>(S + P.L[t.l].lw + 2 * ((t.j0 + c) * P.L[t.l].ws + t.i0 + 4 * g)) = pack4(Tw[u]);
    }
    for (int l = tid >> 7; l < nl; l += NT / DMB_MAXW) {
      const int j = tid & (DMB_MAXW - 1), up = sP[l].up;
      if (j >= up) continue;
      float* bs = fptr(S, sP[l].lb);
      float mm, vv, pn;
      adam_update(bs[3 * up + j], bs[up + j], bs[2 * up + j], bs[j], lr_t, a.beta1, a.beta2, a.eps, 1.0f, mm, vv, pn);
      bs[j] = pn;
      bs[up + j] = mm;
      bs[2 * up + j] = vv;
      bs[3 * up + j] = 0.0f;
    }
    if (tid == 0) {
      const float* tot = fptr(S, P.lstat) + STAT_TOT;
      run.out[2 * s] = tot[0] * inv_n + tot[2] * inv_rows;
      run.out[2 * s + 1] = tot[1];
    }
    __syncthreads();
    if (tid < 3) fptr(S, P.lstat)[STAT_TOT + tid] = 0.0f;   // next touched after the next chunk's barriers
  }

  // ---- write the real parameters and their moments back ----
#pragma unroll
  for (int u = 0; u < SLOTS; ++u) {
    TilePos t;
    if (!tile_of(ti[u], t)) continue;
    const DenseMBLayer& L = sL[t.l];
    const int j = t.j0 + c;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = t.i0 + 4 * g + e;
      if (i < L.in && j < L.units) {
        const unsigned f = (unsigned)(L.w_off + i * L.units + j);
        run.flat[f] = Tw[u][e];
        run.m[f] = Tm[u][e];
        run.v[f] = Tv[u][e];
      }
    }
  }
  for (int l = tid >> 7; l < nl; l += NT / DMB_MAXW) {
    const int j = tid & (DMB_MAXW - 1), up = sP[l].up;
    if (!sL[l].has_bias || j >= sL[l].units) continue;
    const unsigned f = (unsigned)(sL[l].b_off + j);
    const float* bs = fptr(S, sP[l].lb);
    run.flat[f] = bs[j];
    run.m[f] = bs[up + j];
    run.v[f] = bs[2 * up + j];
  }
  if (tid == 0) *run.iter = it0 + steps;
