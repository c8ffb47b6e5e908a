/* pht_spares_draw.inc — the draw body of spares_kernel, included once in the runtime-n build's inline
 * walk and once in the compile-time-n builds' unit_walk lambda.  In scope: d, K, mu, abar, tab (the draw), c, st,
 * pwt, live (the unit) and the kernel's constants. */
        const double *F = a.F + d * fstride;
        const double *vec = a.vec + d * nvec; /* r[nh][n], q[nh][n], dscale[nh], vscale[nh] */
        int bad;
        pht_es_win_t win;
        (void)pht_es_window(tab, sinvk, K, mu, abar, c, 1, &bad, &win);
        const bool good = live && !bad;
        double v[NV];
#pragma unroll
        for (int j = 0; j < NV; j++) v[j] = 0.0;
        if (good) {
          pht_cd_phase(F, n, NV, sinvk, &win, v);
          pht_cd_phi(n, NV, v);
        }
        /* pointwise: this (draw, unit)'s [D nh, var nh] */
        double *pw = PW ? pwt + (size_t)d * (size_t)(2 * nh) : nullptr;
        unsigned long long *sw = ssum + d * WL;
        for (int h = 0; h < nh; h++) {
          const double dv = good ? pht_cd_dot(n, NV, v, vec + h * n) : 0.0;
          const double qv = good ? pht_cd_dot(n, NV, v, vec + (nh + h) * n) : 0.0;
          const double vv = pht_sp_var(dv, qv);
          long long wd = good ? pht_cd_fixed_scaled(dv, vec[2 * nh * n + h]) : 0;
          long long wv = good ? pht_cd_fixed_scaled(vv, vec[2 * nh * n + nh + h]) : 0;
          if (good) {
            st[h] = st[h] + dv;
            st[nh + h] = st[nh + h] + vv;
            st[2 * nh + h] = st[2 * nh + h] + dv * dv;
          }
          if (PW && live) {
            pw[h] = good ? dv : NAN;
            pw[nh + h] = good ? vv : NAN;
          }
          wd = wave_sum(wd);
          wv = wave_sum(wv);
          if ((tid & 63) == 0) {
            atomicAdd(sw + h, (unsigned long long)wd);
            atomicAdd(sw + kSparesMaxH + h, (unsigned long long)wv);
          }
        }
        {
          long long w = (live && bad) ? 1 : 0;
          if (good) st[3 * nh] = st[3 * nh] + 1.0; /* cnt, a whole number below 2^53 */
          w = wave_sum(w);
          if ((tid & 63) == 0) atomicAdd(sw + 2 * kSparesMaxH, (unsigned long long)w);
        }
