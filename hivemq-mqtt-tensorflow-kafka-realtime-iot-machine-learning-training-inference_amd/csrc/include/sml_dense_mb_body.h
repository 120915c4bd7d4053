// The whole launch of ONE model by the calling workgroup: the body of dense_mb_kernel and of
// dense_mb_fleet_kernel (dense_minibatch.hip), which include this text inside their braces.  It is
// text, not a __device__ function, for the reason given in sml_dense_mb_bf16_body.h: included in the
// kernel that owns the arguments, the single-model entry compiles to the instructions it had before
// the fleet entry existed (as a function it came out with other registers: 246 VGPRs for 248).
// In scope at the point of inclusion:
//   a    const DenseMBArgs   what a fleet shares: layer table, plan, batch, Adam constants
//   run  anything with the members of DenseMBRun (sml_dense_fleet.h): the model's own state, rows and
//        steps -- the arguments themselves in the single-model entry, the rebased run in the fleet entry
  extern __shared__ __attribute__((aligned(16))) float S[];
  __shared__ DenseMBLayer sL[DMB_MAXLAYERS];
  __shared__ DenseMBLayerPlan sP[DMB_MAXLAYERS];
  const int tid = threadIdx.x, nl = a.nl;
  if (tid == 0) {
#pragma unroll
    for (int l = 0; l < DMB_MAXLAYERS; ++l) {
      sL[l] = a.L[l];
      sP[l] = a.P.L[l];
    }
  }
  for (int i = a.P.wimg0 + tid; i < a.P.wimg1; i += NT) S[i] = 0.0f;
  if (tid < 3) S[a.P.lstat + STAT_TOT + tid] = 0.0f;
  __syncthreads();

  // ---- the tiles this thread owns: tid, tid + NT, ... ----
  Tile T[DMB_TPT];
#pragma unroll
  for (int u = 0; u < DMB_TPT; ++u) {
    Tile& t = T[u];
    const int id = tid + u * NT;
    t.l = -1;
    t.iq = t.jq = 0;
    if (id < a.P.ntiles) {
      for (int l = 0; l < nl; ++l)
        if (id >= sP[l].tile0) t.l = l;
      const int k = id - sP[t.l].tile0, nq = sP[t.l].up >> 2;
      t.iq = k / nq;
      t.jq = k - t.iq * nq;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) t.m[e] = t.v[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    t.mb = t.vb = f32x4{0.f, 0.f, 0.f, 0.f};
    tile_params<true>(
        S, t, sL, sP,
        [&](int e, int c, unsigned f, float* p) {
          *p = run.flat[f];
          t.m[e][c] = run.m[f];
          t.v[e][c] = run.v[f];
        },
        [&](int c, unsigned f, float* p) {
          *p = run.flat[f];
          t.mb[c] = run.m[f];
          t.vb[c] = run.v[f];
        });
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
#pragma unroll
    for (int u = 0; u < DMB_TPT; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) T[u].g[e] = f32x4{0.f, 0.f, 0.f, 0.f};
      T[u].gb = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int k = 0; k < chunks; ++k) {
      const int rows = rows_s - k * CH < CH ? rows_s - k * CH : CH;
      stage_store(S, a, run, op, st);
      if (k + 1 < chunks) stage_load(a, run, O, s, k + 1, steps, st);
      else stage_load(a, run, O, s + 1, 0, steps, st);
      __syncthreads();
      // ---- forward ----
      for (int l = 0; l < nl; ++l) {
        const int la_prev = l == 0 ? a.P.la0 : sP[l - 1].la;
        by_row_tile(rows, sP[l].up >> 2, [&](auto rt) { fwd_layer<decltype(rt)::value>(S, sL[l], sP[l], la_prev, rows); });
        __syncthreads();
      }
      loss_phase(S, sL, sP, nl, a.P.lyt, a.P.lstat, rows, inv_n, inv_rows);
      __syncthreads();
      // ---- backward ----
      for (int l = nl - 1; l >= 1; --l) {
        by_row_tile(rows, sP[l].ip >> 2,
                    [&](auto rt) { bwd_layer<decltype(rt)::value>(S, sP[l], sL[l - 1], sP[l - 1], rows, inv_rows); });
        __syncthreads();
      }
      // ---- weight / bias gradients into the owners' registers, rows ascending ----
#pragma unroll
      for (int u = 0; u < DMB_TPT; ++u) {
        Tile& t = T[u];
        if (t.l < 0) continue;
        const DenseMBLayerPlan& P = sP[t.l];
        const float* hp = S + (t.l == 0 ? a.P.la0 : sP[t.l > 0 ? t.l - 1 : 0].la) + 4 * t.iq;
        const float* dp = S + P.ld + 4 * t.jq;
#pragma unroll 4
        for (int r = 0; r < rows; ++r) {
          const f32x4 h = ld4(hp + r * P.ip), d = ld4(dp + r * P.up);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 4; ++c) t.g[e][c] = fmaf(h[e], d[c], t.g[e][c]);
          if (t.iq == 0) t.gb += d;   // only the tiles of rows 0..3 own bias elements
        }
      }
      if (tid < 3) {   // the step's squared error / correct rows / penalty, rows ascending
        float tot = S[a.P.lstat + STAT_TOT + tid];
        for (int r = 0; r < rows; ++r) tot += S[a.P.lstat + CH * tid + r];
        S[a.P.lstat + STAT_TOT + tid] = tot;
      }
      __syncthreads();
    }
    // ---- Adam on the owned parameters; the LDS image is updated in place ----
    const float lr_t = adam_lr_t(run.lr, a.beta1, a.beta2, (float)(it0 + s + 1));
#pragma unroll
    for (int u = 0; u < DMB_TPT; ++u) {
      Tile& t = T[u];
      tile_params<false>(
          S, t, sL, sP,
          [&](int e, int c, unsigned, float* p) {
            float mm, vv, pn;
            adam_update(t.g[e][c], t.m[e][c], t.v[e][c], *p, lr_t, a.beta1, a.beta2, a.eps, 1.0f, mm, vv, pn);
            t.m[e][c] = mm;
            t.v[e][c] = vv;
            *p = pn;
          },
          [&](int c, unsigned, float* p) {
            float mm, vv, pn;
            adam_update(t.gb[c], t.mb[c], t.vb[c], *p, lr_t, a.beta1, a.beta2, a.eps, 1.0f, mm, vv, pn);
            t.mb[c] = mm;
            t.vb[c] = vv;
            *p = pn;
          });
    }
    if (tid == 0) {
      const float* tot = S + a.P.lstat + STAT_TOT;
      run.out[2 * s] = tot[0] * inv_n + tot[2] * inv_rows;
      run.out[2 * s + 1] = tot[1];
    }
    __syncthreads();
    if (tid < 3) S[a.P.lstat + STAT_TOT + tid] = 0.0f;   // next touched after the next chunk's barriers
  }

  // ---- write the real parameters and their moments back ----
#pragma unroll
  for (int u = 0; u < DMB_TPT; ++u) {
    Tile& t = T[u];
    tile_params<true>(
        S, t, sL, sP,
        [&](int e, int c, unsigned f, float* p) {
          run.flat[f] = *p;
          run.m[f] = t.m[e][c];
          run.v[f] = t.v[e][c];
        },
        [&](int c, unsigned f, float* p) {
          run.flat[f] = *p;
          run.m[f] = t.mb[c];
          run.v[f] = t.vb[c];
        });
  }
  if (tid == 0) *run.iter = it0 + steps;
