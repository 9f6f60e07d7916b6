// mpf_body.inc - the statements of the single-workgroup filter kernel (mpf.hpp has the account), included TEXTUALLY into each kernel that
// runs them: mpf_optimize_kernel<P, CART> and mpf_optimize_batch_kernel<P, CART>.  Text, not a function, for the reason amppi_body.inc
// gives: the lone instances are to stay the instructions they were.  In scope at the point of inclusion:
//   P (int), CART (bool), a (const MpfArgs; the batched kernel: MpfEnvArgs, one environment's view with the same member names)
//   MPF_UNIFORM(v) (macro): v, a value every lane of the workgroup computes alike - the lone kernel takes it as it is, the batched kernel
//   moves it to scalar registers (the lone kernel's arguments are there already; an environment's come from memory)
// The text has no `return`: the including kernel may go on behind it.
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int Mp = a.Mp;
  const int Mpad = (Mp + 63) & ~63, R = blockDim.x / Mpad;
  const int r = __builtin_amdgcn_readfirstlane((int)threadIdx.x / Mpad), i = (int)threadIdx.x - r * Mpad;
  double *dbuf = reinterpret_cast<double *>(sm);  // [R][Mpad][2 P] partial sums (prior: zs + acc[P]; Stein: gk[P] + ks[P])
  float *xs = reinterpret_cast<float *>(dbuf + (size_t)R * Mpad * 2 * P);  // [Mp][P]
  float *sc = xs + Mp * P;    // [Mp][P] scores
  float *nrm = sc + Mp * P;   // [Mp] squared norms
  float *red = nrm + Mp;      // [32]
  const bool on = i < Mp;
  const int per = (Mp + R - 1) / R, k0 = r * per, k1 = min(Mp, k0 + per);
  if (on && r == 0)
    _Pragma("unroll") for (int p = 0; p < P; ++p) xs[i * P + p] = a.x[i * P + p];
  wg_sync();
  const float bw2 = MPF_UNIFORM((float)((double)a.bw * (double)a.bw));
  double inv_pbw[4], inv_pbw2[4];
  _Pragma("unroll") for (int p = 0; p < 4; ++p) {
    inv_pbw[p] = MPF_UNIFORM(1.0 / (double)a.prior_bwv[p < P ? p : 0]);
    inv_pbw2[p] = MPF_UNIFORM(inv_pbw[p] * inv_pbw[p]);
  }
  const double inv_bw2 = MPF_UNIFORM(1.0 / ((double)a.bw * (double)a.bw)), inv_obs2 = MPF_UNIFORM(1.0 / ((double)a.obs_std * (double)a.obs_std));
  float am[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};  // optimiser state of this lane's particle (registers for the whole launch)
  if (on && r == 0)
    _Pragma("unroll") for (int p = 0; p < P; ++p) {
      if (a.opt_s0) am[p] = a.opt_s0[i * P + p];
      if (a.opt_s1) av[p] = a.opt_s1[i * P + p];
      if (a.opt_s2) a2[p] = a.opt_s2[i * P + p];
    }
  for (int it = 0; it < a.n_steps; ++it) {
    float xi[4] = {0.f, 0.f, 0.f, 0.f};
    if (on) {
      _Pragma("unroll") for (int p = 0; p < P; ++p) xi[p] = xs[i * P + p];
      // prior score (mpf.py:45): means alias the CURRENT particles (covariance prior_bw^2 I, uniform mixture), so the
      // i-th logit is exactly 0 and no other is larger: the softmax needs no max pass
      double zs = 0.0, acc[4] = {0, 0, 0, 0};
      for (int k = k0; k < k1; ++k) {
        double q = 0.0;
        _Pragma("unroll") for (int p = 0; p < P; ++p) {
          const double z = ((double)xi[p] - (double)xs[k * P + p]) * inv_pbw[p];
          q += z * z;
        }
        const double w = (double)expf((float)(-0.5 * q));
        zs += w;
        _Pragma("unroll") for (int p = 0; p < P; ++p) acc[p] += w * ((double)xs[k * P + p] - (double)xi[p]);
      }
      double *d = dbuf + ((size_t)r * Mpad + i) * 2 * P;
      d[0] = zs;
      _Pragma("unroll") for (int p = 0; p < P; ++p) d[1 + p] = acc[p];  // 1 + P <= 2 P slots
    }
    wg_sync();
    if (on && r == 0) {
      double zs = 0.0, acc[4] = {0, 0, 0, 0};
      for (int rr = 0; rr < R; ++rr) {
        const double *d = dbuf + ((size_t)rr * Mpad + i) * 2 * P;
        zs += d[0];
        _Pragma("unroll") for (int p = 0; p < P; ++p) acc[p] += d[1 + p];
      }
      double s[4];
      _Pragma("unroll") for (int p = 0; p < P; ++p) s[p] = acc[p] / zs * inv_pbw2[p];
      // likelihood score (mpf.py:46-50, likelihoods.py:30-49)
      if (CART) {
        double gl[4];
        mpf_cart_score<P>(a.cpl, a.log_space, xi, inv_obs2, gl);
        _Pragma("unroll") for (int p = 0; p < P; ++p) sc[i * P + p] = (float)(s[p] + gl[p]);
      } else if (a.dm.model == DUST_MODEL_SKID_STEER) {
        double gl[4];
        mpf_skid_score<P>(a.skl, a.log_space, xi, inv_obs2, gl);
        _Pragma("unroll") for (int p = 0; p < P; ++p) sc[i * P + p] = (float)(s[p] + gl[p]);
      } else {
        float pred[4];
        for (int k = 0; k < 4; ++k) pred[k] = k < a.ds ? a.past_obs[k] : 0.f;
        const Coef cf = make_coef(a.dm, xi);
        const float pa[2] = {a.act_seq ? a.act_seq[2 * it] : a.past_action[0], a.act_seq ? a.act_seq[2 * it + 1] : a.past_action[1]};
        if (a.dm.model == DUST_MODEL_PENDULUM) model_step<DUST_MODEL_PENDULUM>(a.dm, cf, pred, pa);
        else model_step<DUST_MODEL_PARTICLE>(a.dm, cf, pred, pa);
        double J[4][4];
        step_jacobian<P>(a.dm, a.past_obs, pa, xi, J);
        _Pragma("unroll") for (int p = 0; p < P; ++p) {
          double g = 0.0;
          _Pragma("unroll") for (int k = 0; k < 4; ++k)
            if (k < a.ds) g += J[k][p] * ((double)a.obs[k] - (double)pred[k]);
          s[p] += g * inv_obs2;
          sc[i * P + p] = (float)s[p];
        }
      }
      float nn = 0.f;
      _Pragma("unroll") for (int p = 0; p < P; ++p) nn = nn + xi[p] * xi[p];
      nrm[i] = nn;
    }
    wg_sync();
    // kernel + phi (svgd.py:92-99, mpf.py:52-56).  squared_distance's fp32 addmm rounding is followed: it is part of the
    // reference's result (d^2 / bw^2 amplifies it) - dot as an fma chain, then |b|^2 - 2 a.b, then + |a|^2, clamp 0.
    if (on) {
      double gk[4] = {0, 0, 0, 0}, ks[4] = {0, 0, 0, 0};
      const float ni = nrm[i];
      for (int j = k0; j < k1; ++j) {
        float dot = xi[0] * xs[j * P];
        _Pragma("unroll") for (int q = 1; q < P; ++q) dot = fmaf(xi[q], xs[j * P + q], dot);
        float q = (nrm[j] + (-2.0f * dot)) + ni;
        q = fmaxf(q, 0.f);
        const double k = (double)expf(((-q) / bw2) / 2.0f);
        _Pragma("unroll") for (int p = 0; p < P; ++p) {
          gk[p] -= k * ((double)xi[p] - (double)xs[j * P + p]);
          ks[p] += k * (double)sc[j * P + p];
        }
      }
      double *d = dbuf + ((size_t)r * Mpad + i) * 2 * P;
      _Pragma("unroll") for (int p = 0; p < P; ++p) {
        d[p] = gk[p];
        d[P + p] = ks[p];
      }
    }
    wg_sync();
    float ph[4] = {0.f, 0.f, 0.f, 0.f};
    if (on && r == 0) {
      double gk[4] = {0, 0, 0, 0}, ks[4] = {0, 0, 0, 0};
      for (int rr = 0; rr < R; ++rr) {
        const double *d = dbuf + ((size_t)rr * Mpad + i) * 2 * P;
        _Pragma("unroll") for (int p = 0; p < P; ++p) {
          gk[p] += d[p];
          ks[p] += d[P + p];
        }
      }
      _Pragma("unroll") for (int p = 0; p < P; ++p) ph[p] = (float)(gk[p] * inv_bw2 + ks[p] / Mp);
    }
    float n2 = 0.f;
    _Pragma("unroll") for (int p = 0; p < P; ++p) n2 += ph[p] * ph[p];
    n2 = block_reduce<RED_SUM>(n2, red);
    if (threadIdx.x == 0 && a.grad_norms) a.grad_norms[it] = sqrtf(n2);
    if (on && r == 0 && it == 0 && a.phi_out)
      _Pragma("unroll") for (int p = 0; p < P; ++p) a.phi_out[i * P + p] = ph[p];
    if (on && r == 0) {
      // x.grad = -phi; optimizer.step() (mpf.py:59-62)
      _Pragma("unroll") for (int p = 0; p < P; ++p) xs[i * P + p] = opt_step(a.opt, xi[p], -ph[p], am[p], av[p], a2[p], (float)(a.t0 + it + 1));
    }
    wg_sync();
  }
  if (on && r == 0) {
    _Pragma("unroll") for (int p = 0; p < P; ++p) a.x[i * P + p] = xs[i * P + p];
    _Pragma("unroll") for (int p = 0; p < P; ++p) {
      if (a.opt_s0) a.opt_s0[i * P + p] = am[p];
      if (a.opt_s1) a.opt_s1[i * P + p] = av[p];
      if (a.opt_s2) a.opt_s2[i * P + p] = a2[p];
    }
  }
