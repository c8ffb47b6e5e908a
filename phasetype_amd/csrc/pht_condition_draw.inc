/* pht_condition_draw.inc — the draw body of cond_kernel, included once in the runtime-n build's inline
 * walk and once in the compile-time-n builds' unit_walk lambda.  In scope: d, K, mu, abar, tab (the draw), c, st,
 * pwt, live (the unit) and the kernel's constants. */
        const double *F = a.F + d * fstride;
        const double *vec = a.vec + d * nvec; /* m[n], r[nh][n], scales[1 + nh] */
        int bad;
        pht_es_win_t win;
        (void)pht_es_window(tab, sinvk, K, mu, abar, c, 1, &bad, &win);
        const bool good = live && !bad;
        double v[NV];
#pragma unroll
        for (int j = 0; j < NV; j++) v[j] = 0.0;
        double ml = 0.0;
        if (good) {
          pht_cd_phase(F, n, NV, sinvk, &win, v);
          pht_cd_phi(n, NV, v);
          ml = pht_cd_dot(n, NV, v, vec);
        }
        /* pointwise: this (draw, unit)'s [phi n, MRL, D nh] */
        double *pw = PW ? pwt + (size_t)d * (size_t)(n + 1 + nh) : nullptr;
        unsigned long long *sw = ssum + d * WL;
        /* the phases: word j, the unit's phisum_j, the pointwise value */
#pragma unroll
        for (int j = 0; j < NV; j++) {
          if (j < n) {
            long long w = good ? pht_cd_fixed(v[j]) : 0;
            if (good) st[j] = st[j] + v[j];
            if (PW && live) pw[j] = good ? v[j] : NAN;
            w = wave_sum(w);
            if ((tid & 63) == 0) atomicAdd(sw + j, (unsigned long long)w);
          }
        }
        {
          long long w = good ? pht_cd_fixed_scaled(ml, vec[n + nh * n]) : 0;
          if (good) st[n] = st[n] + ml;
          if (PW && live) pw[n] = good ? ml : NAN;
          w = wave_sum(w);
          if ((tid & 63) == 0) atomicAdd(sw + pht_cd_w_L(n), (unsigned long long)w);
        }
        for (int h = 0; h < nh; h++) {
          const double dv = good ? pht_cd_dot(n, NV, v, vec + n + h * n) : 0.0;
          long long w = good ? pht_cd_fixed_scaled(dv, vec[n + nh * n + 1 + h]) : 0;
          if (good) st[n + 1 + h] = st[n + 1 + h] + dv;
          if (PW && live) pw[n + 1 + h] = good ? dv : NAN;
          w = wave_sum(w);
          if ((tid & 63) == 0) atomicAdd(sw + pht_cd_w_D(n, h), (unsigned long long)w);
        }
        {
          long long w = (live && bad) ? 1 : 0;
          if (good) st[n + 1 + nh] = st[n + 1 + nh] + 1.0; /* cnt, a whole number below 2^53 */
          w = wave_sum(w);
          if ((tid & 63) == 0) atomicAdd(sw + pht_cd_w_nbad(n, nh), (unsigned long long)w);
        }
