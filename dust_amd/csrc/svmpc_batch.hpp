// svmpc_batch.hpp - SVMPC over a batch of plants: B independent ticks (n_steps SVGD iterations and / or SVMPC.forward) in ONE launch.
// Workgroup b runs the whole tick of environment b - from its own state, particles, prior, a_mat, optimiser state and Philox stream -
// and talks to no other workgroup: there is no arrival word, nothing to spin on, and the launch count does not depend on B.
//
// Replaces, per environment (reference file:line): SVMPC.step / optimize svmpc.py:32-126, CostLikelihood.sample likelihoods.py:81-101,
// MultiDISCO._rollout / _compute_cost / forward disco.py:139-394, SVMPC.get_weights / roll / update_prior / forward svmpc.py:128-200.
//
// One SVGD iteration, phases separated by workgroup barriers only:
//   0  particles, prior means, mixture log-weights and the M dynamics samples' coefficients -> LDS (svmpc_prior_batch_kernel: lane m < M
//      first draws sample m from its environment's dynamics filter, the stream of mpf.hpp mpf_sample_kernel)
//   A  actions[s][n] = theta[n] + chol_a eps[s][n] (eps recorded, or Philox: the lone kernels' counter layout - block j >> 3 of row
//      s N + n, common.hpp philox_normal8) -> the environment's action rows in device memory;
//      prior logits[i][k] = logmix[k] - |theta_i - mu_k|^2 / (2 sigma_p^2) -> LDS
//   B  grad_pri[i] = sum_k softmax_k(logits[i]) (mu_k - theta_i) / sigma_p^2 -> LDS (lane = (particle, column))
//   C  the N S M rollouts through the family's own device step and cost functions (common.hpp step_with_cost / term_cost and the
//      Pendulum's shared-reduction trig of rollout.hpp, skid.hpp skid_step - in the navigation instances with w_obs collision() on
//      every state, skid_rollout_body<false, true>'s arithmetic -, cartpole.hpp cartpole_step): lane = (sample s, particle n,
//      dynamics group g), the group's samples m = g, g + G, .. in sequence; costs[s][n] = mean over m, the G group partials (doubles
//      in LDS) added in the order g = 0 .. G - 1
//   D  per particle (one wave each, round-robin): min and sum of its S costs, w = exp(-alpha (c - min)), omega = exp(-(c - min) /
//      temp), their masses, log_l, eta; then a_mix = softmax_N(eta) (disco.py:393).  The reference subtracts ONE beta - the global
//      minimum - before omega's softmax over S (disco.py:380-383); the shift cancels in a softmax, and the per-particle minimum (what
//      rollout.hpp subtracts) keeps a particle whose costs all lie far above the best one from underflowing to 0 / 0
//   E  grad_lik[n] = sum_s w (a - theta) / sigma_a^2 / Z_w, a_mat[n] += sum_s omega (a - a_seq) / Z_o, score = grad_lik + grad_pri:
//      lane = (Q-th share of the samples, particle, column), the Q partials added in the order q = 0 .. Q - 1
//   F  Gram matrix k(theta_i, theta_j) -> LDS (K1: gpytorch RBF with lengthscale ln 2; IMQ), then lane = (particle, column):
//      phi = sum_j k' (theta_i - theta_j) / l^2 + sum_j k score_j / N, the optimiser step (handoff.hpp opt_step: every optimiser of
//      dust_set_optimizer) on grad = -phi, the new particle -> device memory (and the prior means, while they alias the particles:
//      svgd.py:87)
// forward(): logits of the prior in force at the new particles -> log_p, log_w = log_l + log_p, p = softmax_N, first maximum, a_seq =
// its particle BEFORE the roll, the roll ("repeat" / "mean"), prior means = the rolled particles, mixture = ones or p, optimiser state
// and step count restarted, Philox position {tick + 1, 0}.
//
// Every sum runs in an order fixed by (N, S, M, H, d_a) and the workgroup size alone: lane strides, then DPP wave reductions, then
// fixed-order walks over LDS partials.  Nothing depends on B, on the block index or on timing, so an environment computes the same
// bits alone, in any slot of any batch, and beside inactive neighbours.
//
// Choices, and the alternatives that have NOT been measured:
//   * 512 lanes per workgroup (two waves per SIMD, up to 256 VGPRs per lane).  With 1024 lanes - four waves per SIMD, 128 VGPRs - the
//     demo shape (N 3, S 128, M 8: 3 072 rollouts) would be three rollouts per lane in phase C instead of six, but three of the four
//     instances then spill (9 / 10 / 26 VGPRs: the argument block alone parks ~400 scalars in VGPR lanes), and a spilling build has not
//     been timed.  256 lanes have not been timed either.
//   * The action rows [S][N][D] and the costs / weights [S][N] live in per-environment device memory (they are the ACTIONS / COSTS
//     records anyway; N S D floats reach 32 MiB at the corner of the box and cannot all be LDS); the workgroup re-reads them through its
//     CU's L1 / the XCD's L2 after a barrier.  Staging the tile in LDS when it fits (46 KiB at the demo shape), as rollout.hpp does,
//     has not been timed.
//   * LDS holds what every lane reads many times: particles, prior means, score (3 N D floats), the N x N logits / Gram matrix, the
//     coefficients of the M dynamics samples and 16 KiB of partial sums - 135 KiB at N = 64, D = 128 (of 160 KiB), 19 KiB at the demo.
//   * Particle's occupancy map is read in place (device memory, one map for the whole batch); a copy in LDS, as rollout.hpp keeps up to
//     16 KiB of it, has not been timed.
//   * The skid-steer navigation instances (svmpc_skid_nav_batch_kernel / svmpc_skid_nav_prior_batch_kernel) follow skid.hpp instead: a
//     map of up to 4096 words is staged once per launch into the LDS behind the tick's own (135 KiB + 16 KiB at the corner of the box, of
//     160 KiB), a larger one - or any map under DUST_NAV_GRID_HBM=1 - is read in place.  Both paths, and the plain instance on the same
//     shape, HAVE been timed, once (tools/svmpc_batch_time.py skid / skid_nav / skid_nav_hbm at B = 1 .. 256: DESIGN.md section 5 has
//     the run).  Not measured: what the lookups cost inside phase C (no counters were read), and a per-iteration restaging.
//   * Phases B and F walk the N x N pairs on the VALU; N <= 64 here, far below where the MFMA passes of stein.hpp pay.
#pragma once
#include "cartpole.hpp"
#include "handoff.hpp"

namespace dust {

#define SVB_THREADS 512
enum { SVB_MAX_N = 64, SVB_MAX_S = 1024, SVB_MAX_M = 64, SVB_PART = 2048 /* doubles of partial sums in LDS */, SVB_COEF = 10 };

struct SvmpcBatchArgs {
  DevModel dm;   // Pendulum / Particle
  SkidModel sk;  // skid-steer
  CartModel cp;  // cart-pole
  OptArgs opt;
  int N, S, M, H, da, D, P;
  int n_steps, do_forward;
  int philox;  // draw eps (otherwise `eps` holds the caller's)
  int kernel;  // PAIR_K1 / PAIR_IMQ
  int lik, roll_strategy, weighted_prior;
  int G;  // dynamics-sample groups of phase C (G N S <= SVB_PART when G > 1)
  int Q;  // sample shares of phase E (Q N D <= SVB_THREADS when Q > 1)
  float alpha, temp, dt;
  float chol_a[2], sigma_a[2], inv_sp[2], inv_sp2[2];
  float log_norm, inv_ell, inv_l2, inv_n, s0_restart;
  const float *states;          // [B][8]
  const uint64_t *seeds;        // [B]
  const unsigned char *active;  // [B] or nullptr: everybody
  const float *eps;             // [B][n_steps][S][N][D] or nullptr
  const float *params;          // [B][n_steps][M][P] or nullptr
  const float *a_seq;           // [D] the controller's nominal sequence (shared: MultiDISCO.step is no part of an SVMPC tick)
  // per environment: what a tick starts from and leaves behind
  float *theta, *mu, *a_mat;  // [B][N][D]
  float *mixw, *logmix;       // [B][N]
  int *alias;                 // [B]: the prior means alias the particles (after a forward, svgd.py:87)
  uint32_t *ctr;              // [B][4] {tick, iter, optimiser step, ..}
  float *opt_s0, *opt_s1, *opt_s2;  // [B][N][D] or nullptr
  // per environment: records of the last iteration / forward
  float *acts;              // [B][S][N][D]
  float *costs, *wts, *omg;  // [B][S][N]
  float *score, *phi;       // [B][N][D]
  float *logl, *logp, *eta, *a_mix, *pw;  // [B][N]
  float *a_seq_out;         // [B][D]
};

template <int MODEL>
struct SvbDims {
  static constexpr int DS = MODEL == DUST_MODEL_PENDULUM ? 2 : (MODEL == DUST_MODEL_SKID_STEER ? 5 : 4);
};

// floats of the tick's dynamic LDS (svb_tick lays them out); a staged navigation map lies behind them
__host__ __device__ __forceinline__ int svb_lds_floats(int N, int D, int M) { return 2 * SVB_PART + 3 * N * D + N * N + M * SVB_COEF + 4 * N + 4; }

// the barrier between two phases: device-memory rows written in one are read in the next (same CU: one L1), LDS likewise
__device__ __forceinline__ void svb_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// what one dynamics sample keeps constant over its rollouts -> cf[SVB_COEF]
// ARGS: SvmpcBatchArgs, or an AMPPI environment's view (amppi_episode.hpp): the members dm, sk, cp and dt under the same names
template <int MODEL, class ARGS>
__device__ __forceinline__ void svb_coef(const ARGS &a, const float *prow, float *cf) {
  if constexpr (MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_PARTICLE) {
    const Coef c = make_coef(a.dm, prow);
    cf[0] = c.c0;
    cf[1] = c.c1;
  } else if constexpr (MODEL == DUST_MODEL_SKID_STEER) {
    cf[0] = skid_param(a.sk.x_icr, prow, a.dm.log_space);
    cf[1] = skid_param(a.sk.wheel_radius, prow, a.dm.log_space);
    cf[2] = skid_param(a.sk.axial_distance, prow, a.dm.log_space);
  } else {
    const bool have_rows = prow != nullptr;  // (as cartpole.hpp: without rows a parameter named as sampled stays the constructor's Python float)
    const bool pm_py = (a.cp.par[CP_MP].kind == DUST_PARAM_PYFLOAT || (a.cp.par[CP_MP].kind == DUST_PARAM_SAMPLED && !have_rows)) &&
                       (a.cp.par[CP_LEN].kind == DUST_PARAM_PYFLOAT || (a.cp.par[CP_LEN].kind == DUST_PARAM_SAMPLED && !have_rows));
    float v[CP_NPAR];
#pragma unroll
    for (int q = 0; q < CP_NPAR; ++q) v[q] = skid_param(a.cp.par[q], prow, a.dm.log_space);
    const CartCoef k = cartpole_coef(v, pm_py, a.cp.par[CP_MP].value * a.cp.par[CP_LEN].value, a.dt);
    cf[0] = k.g;
    cf[1] = k.mp;
    cf[2] = k.len;
    cf[3] = k.muc;
    cf[4] = k.mup;
    cf[5] = k.fmag;
    cf[6] = k.mass;
    cf[7] = k.pm;
    cf[8] = k.k43;
    cf[9] = k.dt;
  }
}

// One rollout: the trajectory cost sum_t inst(x_t, a_t) + term(x_H) of action row `act` [H][da] under the coefficients `cf`.
// NAV (skid-steer alone): the navigation cost family of skid.hpp, skid_rollout_body<false, true>'s arithmetic operation by operation -
// inst = (quad + ctrl) + w_obs occ(x_0, x_1) on the state BEFORE the step, term = quad + w_obs occ(x_0, x_1); `map`: where collision()
// finds the occupancy bits (LDS or device memory).  A template parameter: the plain instances keep their instructions.
template <int MODEL, bool NAV = false>
__device__ __forceinline__ float svb_traj(const SvmpcBatchArgs &a, const float *act, const float *cf, const float *x0, const bool fast_trig,
                                          const float w_obs = 0.f, const DevModel *map = nullptr) {
  constexpr int DS = SvbDims<MODEL>::DS;
  const int H = a.H;
  float x[DS];
#pragma unroll
  for (int k = 0; k < DS; ++k) x[k] = x0[k];
  if constexpr (MODEL == DUST_MODEL_PENDULUM) {
    Coef c;
    c.c0 = cf[0];
    c.c1 = cf[1];
    if (fast_trig && fabsf(c.c0) <= 3.0e38f && fabsf(c.c1) <= 3.0e38f) {
      // rollout.hpp's finite-operand loop, operation for operation: one argument reduction serves sin(theta + pi) and cos(theta), the
      // clamps are v_med3_f32 - which would swallow a NaN action that torch.clamp propagates: such a row takes the general loop below
      const float dt = (float)a.dm.dt, mt = a.dm.max_torque, ms = a.dm.max_speed_pend;
      const v2f W = {a.dm.w_cos, a.dm.w_vel};
      CostSum<MODEL> tot;
      bool nan_act = false;
      float sn, cs;
      for (int t = 0; t < H; ++t) {
        pendulum_trig(x[0], &sn, &cs);
        v2f q = {cs - 1.0f, x[1]};
        q = W * (q * q);
        tot.add(q.x + q.y, t);
        const float ur = act[t];
        nan_act |= ur != ur;
        const float u = __builtin_amdgcn_fmed3f(ur, -mt, mt);
        float thd = x[1] + dt * (c.c0 * sn + c.c1 * u);
        thd = __builtin_amdgcn_fmed3f(thd, -ms, ms);
        x[0] = x[0] + thd * dt;
        x[1] = thd;
      }
      if (!nan_act) {
        pendulum_trig(x[0], &sn, &cs);
        v2f q = {cs - 1.0f, x[1]};
        q = W * (q * q);
        return (float)tot.total() + (q.x + q.y);
      }
#pragma unroll
      for (int k = 0; k < DS; ++k) x[k] = x0[k];
    }
    CostSum<MODEL> tot;
    for (int t = 0; t < H; ++t) {
      const float at[1] = {act[t]};
      tot.add(step_with_cost<MODEL>(a.dm, c, x, at), t);
    }
    return (float)tot.total() + term_cost<MODEL>(a.dm, x);
  } else if constexpr (MODEL == DUST_MODEL_PARTICLE) {
    Coef c;
    c.c0 = cf[0];
    c.c1 = cf[1];
    CostSum<MODEL> tot;
    for (int t = 0; t < H; ++t) {
      const float at[2] = {act[2 * t], act[2 * t + 1]};
      tot.add(step_with_cost<MODEL>(a.dm, c, x, at), t);
    }
    return (float)tot.total() + term_cost<MODEL>(a.dm, x);
  } else if constexpr (MODEL == DUST_MODEL_SKID_STEER) {
    const float xicr = cf[0], wr = cf[1], ad = cf[2];
    double tot = 0.0;
    for (int t = 0; t < H; ++t) {
      const float a0 = act[2 * t], a1 = act[2 * t + 1];
      double sc = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float d = x[k] - a.sk.goal[k];
        sc += (double)((d * d) * a.sk.w_state[k]);
      }
      const double cc = (double)((a0 * a0) * a.sk.w_ctrl[0]) + (double)((a1 * a1) * a.sk.w_ctrl[1]);
      if constexpr (NAV) tot += (double)(((float)sc + (float)cc) + w_obs * collision(*map, x[0], x[1]));  // (quad + ctrl) + obst
      else tot += (double)((float)sc + (float)cc);
      skid_step(x, clampf(a0, a.sk.lo[0], a.sk.hi[0]), clampf(a1, a.sk.lo[1], a.sk.hi[1]), xicr, wr, ad, a.dt);
    }
    double tc = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float d = x[k] - a.sk.goal[k];
      tc += (double)((d * d) * a.sk.w_term[k]);
    }
    if constexpr (NAV) return (float)tot + ((float)tc + w_obs * collision(*map, x[0], x[1]));
    else return (float)tot + (float)tc;
  } else {
    CartCoef kf;
    kf.g = cf[0];
    kf.mp = cf[1];
    kf.len = cf[2];
    kf.muc = cf[3];
    kf.mup = cf[4];
    kf.fmag = cf[5];
    kf.mass = cf[6];
    kf.pm = cf[7];
    kf.k43 = cf[8];
    kf.dt = cf[9];
    double tot = 0.0;
    for (int t = 0; t < H; ++t) {
      const float a0 = act[t];
      double sc = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = x[k] - a.cp.goal[k];
        sc += (double)((d * d) * a.cp.w_state[k]);
      }
      const double cc = (double)((a0 * a0) * a.cp.w_ctrl[0]);
      tot += (double)((float)sc + (float)cc);
      cartpole_step(x, clampf(a0, -1.0f, 1.0f), kf, fast_sinf(x[2]), fast_cosf(x[2]));
    }
    double tc = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = x[k] - a.cp.goal[k];
      tc += (double)((d * d) * a.cp.w_term[k]);
    }
    return (float)tot + (float)tc;
  }
}

// logits[i][k] = logmix[k] - |x_i - y_k|^2 / (2 sigma_p^2) over the N x N pairs (stein.hpp pairwise_body<PRIOR>, pass A)
__device__ __forceinline__ void svb_prior_logits(const SvmpcBatchArgs &a, const float *th, const float *mu, const float *lmx, float *kv) {
  const int N = a.N, D = a.D;
  for (int p = (int)threadIdx.x; p < N * N; p += SVB_THREADS) {
    const int i = p / N, k = p - i * N;
    const float *x = th + i * D, *y = mu + k * D;
    float dd = 0.f;
    for (int d = 0; d < D; ++d) {
      const float z = (x[d] - y[d]) * ((a.da == 2 && (d & 1)) ? a.inv_sp[1] : a.inv_sp[0]);
      dd = fmaf(z, z, dd);
    }
    kv[p] = lmx[k] - 0.5f * dd;
  }
}

// Where svmpc_prior_batch_kernel finds its dynamics samples (dust_svmpc_dual_batch_tick): the B filters' particles and prior bandwidths,
// read in place - the batched filter kernel wrote them just ahead on the same stream - and the Philox key of every environment's draws
struct SvbPrior {
  const float *means;     // [B][K][P]
  int K, P;
  const float *bwv;       // [B][4]
  const uint64_t *seeds;  // [B]
  float *params_out;      // [B][n_steps][M][P] or nullptr
};
struct SvmpcPriorBatchArgs {
  SvmpcBatchArgs k;
  SvbPrior pr;
};

// Row i = it M + m of mpf.prior.sample([n_steps M]) of environment env's filter as mpf_sample_kernel (mpf.hpp) draws it under the key
// seeds[env] - the same counters, the same operations in the same order - into row[4]
__device__ __forceinline__ void svb_draw_row(const SvmpcBatchArgs &a, const SvbPrior &pri, const int env, const int it, const int m, float *row) {
  const uint32_t i = (uint32_t)(it * a.M + m);
  const uint64_t key = pri.seeds[env];
  uint32_t r[4];
  philox4x32_10(i, 0x6d7066u, 0u, 0u, (uint32_t)key, (uint32_t)(key >> 32), r);
  const int kc = (int)(((unsigned long long)r[0] * (unsigned long long)pri.K) >> 32);
  float zp[4];
  philox_normal4(key, i, 0x6d7067u, 1u, 0u, zp);
  const float *mean = pri.means + ((size_t)env * (size_t)pri.K + (size_t)kc) * (size_t)pri.P;
  const float *bw = pri.bwv + (size_t)env * 4;
#pragma unroll
  for (int p = 0; p < 4; ++p)
    if (p < pri.P) row[p] = mean[p] + bw[p] * zp[p];
}

// What one tick of an environment starts from and hands to the next beside its device rows: the state, the Philox position {tick, iter},
// the optimiser's step count and whether the prior means alias the particles.  Every lane keeps the same copy in registers; svb_begin
// reads it, svb_tick advances it, svb_end stores it (lane 0).  A kernel that runs several ticks in one launch (svmpc_episode.hpp) keeps
// it in registers between them: these words sit at one address per environment, and a uniform-address read of what lane 0 stored a
// tick earlier could be served by the scalar cache.
template <int MODEL>
struct SvbCarry {
  float x0[SvbDims<MODEL>::DS];
  uint32_t ctr_tick, ctr_iter, opt_t;
  bool alias;
};

// The tick of environment blockIdx.x from the carry `cy`.  PRIOR: the dynamics samples are drawn in phase 0 from the environment's filter
// (`pri`), not read from `params` ([B][n_steps][M][P], this tick's rows); nothing else differs.  NAV: the skid-steer tick with the
// navigation cost family - `map`, `w_obs`: what svb_begin made of the SkidNav.  EPISODE (svmpc_episode.hpp): forward() also hands out the
// first action of the sequence it chose (`act0` [da], every lane) and writes its particle weights to `pw_rec` ([N] or nullptr) too.
template <int MODEL, bool PRIOR, bool NAV, bool EPISODE>
__device__ __forceinline__ void svb_tick(const SvmpcBatchArgs &a, const SvbPrior *pri, const float *params, SvbCarry<MODEL> &cy, const DevModel &map,
                                         const float w_obs, float *pw_rec = nullptr, float *act0 = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int T = SVB_THREADS;
  constexpr float LOG2E = 1.44269504088896340736f;
  const int env = (int)blockIdx.x;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, S = a.S, M = a.M, H = a.H, da = a.da, D = a.D;
  const int ND = N * D, NS = N * S;

  // ---- LDS: partial sums first (doubles), then the rows every lane reads
  double *accp = reinterpret_cast<double *>(lds);  // [SVB_PART] phase C group partials
  float *part = lds;                               // [2][T] phase E share partials (the same bytes, another phase)
  float *th = lds + 2 * SVB_PART;                  // [N][D] particles
  float *mu = th + ND;                             // [N][D] prior means
  float *sc = mu + ND;                             // [N][D] grad_pri, then score
  float *kv = sc + ND;                             // [N][N] prior logits, then the Gram matrix
  float *coef = kv + N * N;                        // [M][SVB_COEF]
  float *zw = coef + M * SVB_COEF;                 // [N] mass of w
  float *zo = zw + N;                              // [N] mass of omega
  float *lmx = zo + N;                             // [N] mixture log-weights
  float *lw = lmx + N;                             // [N] eta, then log_w
  int *misc = reinterpret_cast<int *>(lw + N);     // [1] argmax

  // ---- this environment's rows
  float *g_th = a.theta + (size_t)env * ND, *g_mu = a.mu + (size_t)env * ND, *g_amat = a.a_mat + (size_t)env * ND;
  float *g_score = a.score + (size_t)env * ND, *g_phi = a.phi + (size_t)env * ND;
  float *g_acts = a.acts + (size_t)env * NS * D;
  float *g_costs = a.costs + (size_t)env * NS, *g_wts = a.wts + (size_t)env * NS, *g_omg = a.omg + (size_t)env * NS;
  float *g_logl = a.logl + (size_t)env * N, *g_eta = a.eta + (size_t)env * N;
  float *s0p = a.opt_s0 ? a.opt_s0 + (size_t)env * ND : nullptr;
  float *s1p = a.opt_s1 ? a.opt_s1 + (size_t)env * ND : nullptr;
  float *s2p = a.opt_s2 ? a.opt_s2 + (size_t)env * ND : nullptr;
  const bool alias = cy.alias;
  const uint64_t seed = a.seeds[env];
  uint32_t &ctr_tick = cy.ctr_tick, &ctr_iter = cy.ctr_iter, &opt_t = cy.opt_t;
  const float *x0 = cy.x0;
  const bool fast_trig = MODEL == DUST_MODEL_PENDULUM && fabsf(x0[1]) <= 3.0e38f &&
                         (fabsf(x0[0]) + a.dm.max_speed_pend * (float)a.dm.dt * (float)H < 5.0e4f);
  const bool same_w = (a.alpha * a.temp == 1.0f);  // temperature = 1 / alpha (every demo): omega and w are the same softmax
  auto col2 = [&](const float *v, const int j) { return (da == 2 && (j & 1)) ? v[1] : v[0]; };

  for (int it = 0; it < a.n_steps; ++it) {
    // ---- 0: stage
    if constexpr (PRIOR) {
      // one lane per dynamics sample (M <= SVB_MAX_M < T).  The row waits in the partial sums' LDS - idle in this phase - for svb_coef,
      // which indexes it by the parameters' columns (a register row would go to scratch); the caller's copy leaves behind the barrier.
      // (The argument block keeps ~380 scalars in spilled lanes, and the register allocator is sensitive to what this phase adds: with
      // the copy written here, or with the key forced into vector registers, it leaves 36 - 68 bytes of never-used stack slots behind
      // in one or two of the instances.  tests/test_svmpc_dual_batch_cpu.py holds all four to a private segment of 0.)
      if (tid < M) svb_draw_row(a, *pri, env, it, tid, part + tid * 4);
    }
    for (int i = tid; i < ND; i += T) {
      const float v = g_th[i];
      th[i] = v;
      mu[i] = alias ? v : g_mu[i];
    }
    for (int i = tid; i < N; i += T) lmx[i] = a.logmix[(size_t)env * N + i];
    for (int m = tid; m < M; m += T) {
      const float *prow = PRIOR ? part + m * 4 : (params ? params + (((size_t)env * a.n_steps + it) * M + m) * a.P : nullptr);
      float cf[SVB_COEF];
      svb_coef<MODEL>(a, prow, cf);
      constexpr int NC = (MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_PARTICLE) ? 2 : (MODEL == DUST_MODEL_SKID_STEER ? 3 : SVB_COEF);
#pragma unroll
      for (int q = 0; q < NC; ++q) coef[m * SVB_COEF + q] = cf[q];
    }
    svb_sync();
    if constexpr (PRIOR) {  // the drawn rows for the caller: [n_steps][M][P] of this environment, M P <= 256 floats
      if (pri->params_out && tid < M * pri->P) {
        const int m = tid / pri->P, p = tid - m * pri->P;
        pri->params_out[(((size_t)env * a.n_steps + it) * M + m) * (size_t)pri->P + p] = part[m * 4 + p];
      }
    }

    // ---- A: actions, prior logits
    if (a.philox) {
      const int nb8 = (D + 7) >> 3;
      for (int w = tid; w < NS * nb8; w += T) {
        const int row = w / nb8, j8 = w - row * nb8, n = row % N;
        float z[8];
        philox_normal8(seed, (uint32_t)j8, (uint32_t)row, ctr_iter, ctr_tick, z);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int j = j8 * 8 + q;
          if (j < D) g_acts[(size_t)row * D + j] = th[n * D + j] + col2(a.chol_a, j) * z[q];
        }
      }
    } else {
      const float *e = a.eps + ((size_t)env * a.n_steps + it) * (size_t)NS * D;
      for (int w = tid; w < NS * D; w += T) {
        const int row = w / D, j = w - row * D, n = row % N;
        g_acts[w] = th[n * D + j] + col2(a.chol_a, j) * e[w];
      }
    }
    svb_prior_logits(a, th, mu, lmx, kv);
    svb_sync();

    // ---- B: grad_pri (svmpc.py:38-41 through autograd: sum_k r_ik (mu_k - x_i) / sigma_p^2)
    for (int e = tid; e < ND; e += T) {
      const int i = e / D, d = e - i * D;
      const float *lg = kv + i * N;
      float m = -INFINITY;
      for (int k = 0; k < N; ++k) m = fmaxf(m, lg[k]);
      const float xi = th[e];
      float l = 0.f, acc = 0.f;
      for (int k = 0; k < N; ++k) {
        const float w = __builtin_amdgcn_exp2f((lg[k] - m) * LOG2E);
        l += w;
        acc = fmaf(w, mu[k * D + d] - xi, acc);
      }
      sc[e] = (acc / l) * col2(a.inv_sp2, d);
    }

    // ---- C: rollouts
    {
      const int G = a.G;
      for (int w = tid; w < NS * G; w += T) {
        const int g = w / NS, row = w - g * NS;
        const float *act = g_acts + (size_t)row * D;
        double acc = 0.0;
        for (int m = g; m < M; m += G) {
          // scalar-event params_dist quirk (disco.py:177-179): rollout r = (m, s, n) flattened uses params[r % M]
          const int pidx = a.dm.interleave ? (int)(((long)m * NS + row) % M) : m;
          if constexpr (NAV) acc += (double)svb_traj<MODEL, true>(a, act, coef + pidx * SVB_COEF, x0, fast_trig, w_obs, &map);
          else acc += (double)svb_traj<MODEL>(a, act, coef + pidx * SVB_COEF, x0, fast_trig);
        }
        if (G == 1) g_costs[row] = M == 1 ? (float)acc : (float)(acc / M);
        else accp[w] = acc;
      }
      if (G > 1) {
        svb_sync();
        for (int row = tid; row < NS; row += T) {
          double acc = accp[row];
          for (int g = 1; g < G; ++g) acc += accp[g * NS + row];
          g_costs[row] = (float)(acc / M);
        }
      }
    }
    svb_sync();

    // ---- D: per particle, one wave each: weights of the likelihood (alpha) and of MultiDISCO (1 / temp), log_l, eta
    for (int n = wave; n < N; n += T / 64) {
      float cmin = INFINITY, csum = 0.f;
      for (int s = lane; s < S; s += 64) {
        const float c = g_costs[s * N + n];
        cmin = fminf(cmin, c);
        csum += c;
      }
      cmin = wave_min(cmin);
      csum = wave_sum(csum);
      float mw = 0.f, mo = 0.f;
      for (int s = lane; s < S; s += 64) {
        const float c = g_costs[s * N + n];
        const float ew = expf(-c * a.alpha - (-cmin * a.alpha));  // svmpc.py:51 softmax(-costs * alpha)
        g_wts[s * N + n] = ew;
        mw += ew;
        if (!same_w) {
          const float eo = expf((-1.0f * (c - cmin)) / a.temp);  // disco.py:381
          g_omg[s * N + n] = eo;
          mo += eo;
        }
      }
      mw = wave_sum(mw);
      mo = same_w ? mw : wave_sum(mo);
      if (lane == 0) {
        zw[n] = mw;
        zo[n] = mo;
        g_logl[n] = a.lik == DUST_LIK_EXP_UTILITY ? ((-cmin * a.alpha) + logf(mw)) - logf((float)S)  // likelihoods.py:127-135
                                                  : -a.alpha * (csum / (float)S);                     // likelihoods.py:113-119
        const float eta = (-cmin / a.temp) + logf(mo);
        g_eta[n] = eta;
        lw[n] = eta;
      }
    }
    svb_sync();
    if (wave == 0) {  // a_mix = softmax_n(eta), disco.py:393
      const float v = lane < N ? lw[lane] : -INFINITY;
      const float m = wave_max(v);
      const float z = wave_sum(lane < N ? expf(v - m) : 0.f);
      const float lz = m + logf(z);
      if (lane < N) a.a_mix[(size_t)env * N + lane] = expf(v - lz);
    }

    // ---- E: grad_lik, a_mat, score
    {
      const int Q = a.Q;
      auto finish = [&](const int e, const float g, const float am) {
        const int n = e / D;
        const float gs = g / zw[n];
        g_amat[e] = g_amat[e] + am / zo[n];  // a_mat += sum_s omega eps (disco.py:387-392)
        const float s = gs + sc[e];
        sc[e] = s;
        g_score[e] = s;
      };
      auto share = [&](const int e, const int q0, const int qs, float &g, float &am) {
        const int n = e / D, j = e - n * D;
        const float thj = th[e], base = a.a_seq[j];  // the actions reach MultiDISCO as external ones: eps = a - a_seq (disco.py:161-164)
        const float sg = col2(a.sigma_a, j);
        const float is2 = 1.0f / (sg * sg);
        const float *wo = same_w ? g_wts : g_omg;
        g = 0.f;
        am = 0.f;
        for (int s = q0; s < S; s += qs) {
          const int row = s * N + n;
          const float av = g_acts[(size_t)row * D + j];
          g = fmaf(g_wts[row], (av - thj) * is2, g);
          am = fmaf(wo[row], av - base, am);
        }
      };
      if (Q == 1) {
        for (int e = tid; e < ND; e += T) {
          float g, am;
          share(e, 0, 1, g, am);
          finish(e, g, am);
        }
      } else {
        if (tid < Q * ND) {
          const int q = tid / ND;
          float g, am;
          share(tid - q * ND, q, Q, g, am);
          part[tid] = g;
          part[T + tid] = am;
        }
        svb_sync();
        if (tid < ND) {
          float g = part[tid], am = part[T + tid];
          for (int q = 1; q < Q; ++q) {
            g += part[q * ND + tid];
            am += part[T + q * ND + tid];
          }
          finish(tid, g, am);
        }
      }
    }

    // ---- F: Gram matrix, phi, optimiser step
    for (int p = tid; p < N * N; p += T) {
      const int i = p / N, j = p - i * N;
      const float *x = th + i * D, *y = th + j * D;
      float dd = 0.f;
      for (int d = 0; d < D; ++d) {
        const float z = (x[d] - y[d]) * a.inv_ell;
        dd = fmaf(z, z, dd);
      }
      // K1: exp(-dd / 2) = 2^(-dd / (2 ln 2)); IMQ: (1 + d^2 / l^2)^(-1/2) (the bare v_exp_f32 / v_rsq_f32 of stein.hpp)
      kv[p] = a.kernel == PAIR_K1 ? __builtin_amdgcn_exp2f(-0.72134752044448170f * dd) : __builtin_amdgcn_rsqf(1.0f + dd);
    }
    svb_sync();
    opt_t += 1u;
    for (int e = tid; e < ND; e += T) {
      const int i = e / D, d = e - i * D;
      const float xi = th[e];
      float sa = 0.f, sb = 0.f;
      for (int j = 0; j < N; ++j) {
        const float k = kv[i * N + j];
        const float kp = a.kernel == PAIR_K1 ? -k : -(k * k) * k;  // d k / d x_i up to (x_i - x_j) / l^2
        sa = fmaf(k, sc[j * D + d], sa);
        sb = fmaf(kp, xi - th[j * D + d], sb);
      }
      const float phi = sb * a.inv_l2 + sa * a.inv_n;  // svmpc.py:83
      g_phi[e] = phi;
      const float nv = opt_apply(a.opt, s0p, s1p, s2p, (size_t)e, xi, -phi, (float)opt_t);  // theta.grad = -phi; optimizer.step()
      g_th[e] = nv;
      if (alias) g_mu[e] = nv;
    }
    ctr_iter += 1u;
    svb_sync();
  }

  if (a.do_forward) {
    // ---- SVMPC.forward: weights, first maximum, a_seq, roll, prior refresh (svmpc.py:128-200)
    float *g_logp = a.logp + (size_t)env * N, *g_pw = a.pw + (size_t)env * N;
    for (int i = tid; i < ND; i += T) {
      const float v = g_th[i];
      th[i] = v;
      mu[i] = alias ? v : g_mu[i];
    }
    for (int i = tid; i < N; i += T) lmx[i] = a.logmix[(size_t)env * N + i];
    svb_sync();
    svb_prior_logits(a, th, mu, lmx, kv);
    svb_sync();
    for (int i = tid; i < N; i += T) {  // prior.log_prob(theta), then log_w = log_l + log_p (svmpc.py:137-138)
      const float *lg = kv + i * N;
      float m = -INFINITY;
      for (int k = 0; k < N; ++k) m = fmaxf(m, lg[k]);
      float l = 0.f;
      for (int k = 0; k < N; ++k) l += __builtin_amdgcn_exp2f((lg[k] - m) * LOG2E);
      const float lp = (m + logf(l)) + a.log_norm;
      g_logp[i] = lp;
      lw[i] = g_logl[i] + lp;
    }
    svb_sync();
    if (wave == 0) {
      const float v = lane < N ? lw[lane] : -INFINITY;
      const float m = wave_max(v);
      const float z = wave_sum(lane < N ? expf(v - m) : 0.f);
      const float lz = m + logf(z);
      const float p = lane < N ? expf(v - lz) : 0.f;
      if (lane < N) g_pw[lane] = p;
      if constexpr (EPISODE) {
        if (pw_rec && lane < N) pw_rec[lane] = p;
      }
      float best = lane < N ? p : -INFINITY;  // first index of the maximum (torch.argmax on CPU)
      int bi = lane < N ? lane : 0x7fffffff;
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) {
          best = ob;
          bi = oi;
        }
      }
      if (lane == 0) misc[0] = bi < N ? bi : 0;
      // the new mixture: Categorical(probs = w / sum w) -> logits = log(clamp(probs, eps, 1 - eps)) -> log_softmax (forward.hpp)
      float *g_mixw = a.mixw + (size_t)env * N, *g_logmix = a.logmix + (size_t)env * N;
      if (!a.weighted_prior) {
        const float l = logf(fminf(fmaxf(1.0f / (float)N, 1.1920929e-07f), 1.0f - 1.1920929e-07f));
        const float lzz = l + logf((float)N);
        if (lane < N) {
          g_mixw[lane] = 1.0f;
          g_logmix[lane] = l - lzz;
        }
      } else {
        const float psum = wave_sum(p);
        float pp = p / psum;
        pp = fminf(fmaxf(pp, 1.1920929e-07f), 1.0f - 1.1920929e-07f);
        const float l = lane < N ? logf(pp) : -INFINITY;
        const float lm = wave_max(l);
        const float zs = wave_sum(lane < N ? expf(l - lm) : 0.f);
        const float lzz = lm + logf(zs);
        if (lane < N) {
          g_mixw[lane] = p;
          g_logmix[lane] = l - lzz;
        }
      }
    }
    svb_sync();
    const int bi = misc[0];
    for (int d = tid; d < D; d += T) a.a_seq_out[(size_t)env * D + d] = th[bi * D + d];
    if constexpr (EPISODE) {  // a_seq[0] for the plant, from the LDS row every lane can read
      act0[0] = th[bi * D];
      if (da == 2) act0[1] = th[bi * D + 1];
    }
    for (int e = tid; e < ND; e += T) {  // theta.roll(-1, dims=-2), the last row by strategy (svmpc.py:142-158)
      const int n = e / D, j = e - n * D, t = j / da, c = j - t * da;
      const float *row = th + n * D;
      float out = row[min(t + 1, H - 1) * da + c];
      if (a.roll_strategy == DUST_ROLL_MEAN && t == H - 1) {
        float s = 0.f;
        for (int u = 0; u < H; ++u) s += row[u * da + c];
        out = s / (float)H;
      }
      g_th[e] = out;
      g_mu[e] = out;  // get_gmm(self.theta, ...): the new means are the rolled particles
      if (s0p) s0p[e] = a.s0_restart;  // a NEW parameter tensor: torch's optimiser state restarts with it
      if (s1p) s1p[e] = 0.f;
      if (s2p) s2p[e] = 0.f;
    }
    if (tid == 0) a.alias[env] = 1;
    cy.alias = true;
    ctr_tick += 1u;
    ctr_iter = 0u;
    opt_t = 0u;
  }
}

// The carry of environment blockIdx.x from its device words and the call's state.  NAV: `map` / `w_obs` from the SkidNav (one map for
// the whole batch) - a map of nav->grid_words > 0 words is staged ONCE per launch into the dynamic LDS behind the tick's own, ahead of
// the iteration loop; otherwise the lookups of phase C read it in place.
template <int MODEL, bool NAV>
__device__ __forceinline__ void svb_begin(const SvmpcBatchArgs &a, const SkidNav *nav, SvbCarry<MODEL> &cy, DevModel &map, float &w_obs) {
  static_assert(!NAV || MODEL == DUST_MODEL_SKID_STEER, "the navigation cost family is the skid-steer robot's");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int DS = SvbDims<MODEL>::DS;
  const int env = (int)blockIdx.x;
  const uint32_t *ctr = a.ctr + (size_t)env * 4;
  cy.alias = a.alias[env] != 0;
  cy.ctr_tick = ctr[0];
  cy.ctr_iter = ctr[1];
  cy.opt_t = ctr[2];
#pragma unroll
  for (int k = 0; k < DS; ++k) cy.x0[k] = a.states[(size_t)env * 8 + k];
  w_obs = 0.f;
  if constexpr (NAV) {  // what collision() reads: skid.hpp skid_nav_map's fields
    map.inv_cell = nav->inv_cell;
    map.off_x = nav->off_x;
    map.off_y = nav->off_y;
    map.nx = nav->nx;
    map.ny = nav->ny;
    map.grid_bits = nav->grid_bits;
    w_obs = nav->w_obs;
    if (nav->grid_words > 0 && a.n_steps > 0) {  // (the same for every lane of the launch; a lone forward() looks nothing up)
      // behind svmpc_batch_lds_bytes(): 4 nav->grid_words bytes
      uint32_t *grid = reinterpret_cast<uint32_t *>(lds + svb_lds_floats(a.N, a.D, a.M));
      const int words = (nav->nx * nav->ny + 31) >> 5;  // (grid_words is this rounded up to 4: the allocation ends at `words`)
      for (int w = (int)threadIdx.x; w < words; w += SVB_THREADS) grid[w] = nav->grid_bits[w];
      map.grid_bits = grid;
      svb_sync();
    }
  }
}

// lane 0 stores the carry's counters (the alias flag: forward() stored it)
template <int MODEL>
__device__ __forceinline__ void svb_end(const SvmpcBatchArgs &a, const SvbCarry<MODEL> &cy) {
  if (threadIdx.x == 0) {
    uint32_t *ctr = a.ctr + (size_t)blockIdx.x * 4;
    ctr[0] = cy.ctr_tick;
    ctr[1] = cy.ctr_iter;
    ctr[2] = cy.opt_t;
  }
}

// one tick per launch: optimize, forward, or both
template <int MODEL, bool PRIOR, bool NAV = false>
__device__ __forceinline__ void svb_body(const SvmpcBatchArgs &a, const SvbPrior *pri, const SkidNav *nav = nullptr) {
  if (a.active && a.active[blockIdx.x] == 0) return;
  SvbCarry<MODEL> cy;
  DevModel map;
  float w_obs;
  svb_begin<MODEL, NAV>(a, nav, cy, map, w_obs);
  svb_tick<MODEL, PRIOR, NAV, false>(a, pri, a.params, cy, map, w_obs);
  svb_end(a, cy);
}

template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_batch_kernel(const SvmpcBatchArgs a) {
  svb_body<MODEL, false>(a, nullptr);
}
// ... coupled to B dynamics filters (dust_svmpc_dual_batch_tick): in iteration `it`, lane m < M draws row it M + m of
// dust_mpf_prior_sample(filter env, n_steps M, seeds[env]) itself - no parameter buffer, no launch besides the tick's
template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_prior_batch_kernel(const SvmpcPriorBatchArgs kp) {
  svb_body<MODEL, true>(kp.k, &kp.pr);
}
// The skid-steer tick with the navigation cost family (dust_amd.costs.NavigationCost), in both forms.  The SkidNav travels BESIDE the
// arguments above, as skid.hpp's SkidNavArgs does: the eight instances without the term keep their argument layout - and their
// instructions.  Dynamic LDS: svmpc_batch_lds_bytes() + 4 nav.grid_words bytes.
struct SvmpcNavBatchArgs {
  SvmpcBatchArgs k;
  SkidNav nav;
};
struct SvmpcNavPriorBatchArgs {
  SvmpcBatchArgs k;
  SvbPrior pr;
  SkidNav nav;
};
__global__ __launch_bounds__(SVB_THREADS) void svmpc_skid_nav_batch_kernel(const SvmpcNavBatchArgs kn) {
  svb_body<DUST_MODEL_SKID_STEER, false, true>(kn.k, nullptr, &kn.nav);
}
__global__ __launch_bounds__(SVB_THREADS) void svmpc_skid_nav_prior_batch_kernel(const SvmpcNavPriorBatchArgs kp) {
  svb_body<DUST_MODEL_SKID_STEER, true, true>(kp.k, &kp.pr, &kp.nav);
}
// Per-environment hyper-parameters (dust_svmpc_batch_set_hyper: the trials of the reference's demo/pendulum_tuning.py:30-143 and
// demo/particle_tuning.py:27-99 as the environments of one batch).  Row b holds what environment b reads in place of the launch-uniform
// fields of the same names - the host makes the derived ones (svb_hyper_row, dust_amd.hip: the one function that also makes the
// prototype's) and writes the rows before the launch; no kernel ever writes them, so the workgroup-uniform load below may be a scalar one.
// The workgroup patches ITS copy of the arguments and runs svb_body on it: the uniform kernels' text, arithmetic and order, so a row
// equal to the prototype's gives the uniform kernel's bits.  same_w (svb_tick) is formed from that copy: the one- and the two-softmax
// path may run side by side in one launch.  The horizon stays per batch: strides, the Philox layout and the LDS plan depend on it.
// Not measured: passing the row by reference through a template parameter of svb_tick instead of patching a copy.
// A row is 64 bytes on a 16-byte boundary: the workgroup fetches it whole with one wide load.  The fields are patched by the text of
// SVB_HYPER_APPLY in the kernel's own body: with the same assignments behind a forceinline function taking the copy by reference the
// register allocator left 36 bytes of never-used stack slots behind in the skid-steer episode instance - the sensitivity svb_tick's
// phase 0 notes; tests/test_svmpc_sweep_cpu.py holds all eight instances to a private segment of 0.
struct alignas(16) SvbHyper {
  double lr;
  float alpha, temp;
  float chol_a[2], sigma_a[2], inv_sp[2], inv_sp2[2];
  float log_norm;
  int weighted_prior;
  int pad[2];
};
static_assert(sizeof(SvbHyper) == 64, "one row, one 64-byte load");
struct SvmpcSweepArgs {
  SvmpcBatchArgs k;
  const SvbHyper *rows;  // [B]
};
#define SVB_HYPER_APPLY(a, h)         \
  (a).opt.lr = (h).lr;                \
  (a).alpha = (h).alpha;              \
  (a).temp = (h).temp;                \
  for (int d = 0; d < 2; ++d) {       \
    (a).chol_a[d] = (h).chol_a[d];    \
    (a).sigma_a[d] = (h).sigma_a[d];  \
    (a).inv_sp[d] = (h).inv_sp[d];    \
    (a).inv_sp2[d] = (h).inv_sp2[d];  \
  }                                   \
  (a).log_norm = (h).log_norm;        \
  (a).weighted_prior = (h).weighted_prior
template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_sweep_kernel(const SvmpcSweepArgs ks) {
  const SvbHyper h = ks.rows[blockIdx.x];  // (the whole row, ahead of the copy)
  SvmpcBatchArgs a = ks.k;
  SVB_HYPER_APPLY(a, h);
  svb_body<MODEL, false>(a, nullptr);
}
// the instance of either kernel for a model (the host's launch names the model once for both)
template <int MODEL, bool PRIOR>
static constexpr auto svb_instance() {
  if constexpr (PRIOR) return &svmpc_prior_batch_kernel<MODEL>;
  else return &svmpc_batch_kernel<MODEL>;
}

// dust_svmpc_batch_set(THETA): while an environment's prior means alias its particles they follow them (svgd.py:87); a new parameter
// tensor restarts the optimiser's step count
__global__ void svmpc_batch_theta_set_kernel(const float *theta, float *mu, const int *alias, uint32_t *ctr, const int ND) {
  const int env = (int)blockIdx.x;
  if (threadIdx.x == 0) ctr[(size_t)env * 4 + 2] = 0u;
  if (!alias[env]) return;
  for (int i = (int)threadIdx.x; i < ND; i += (int)blockDim.x) mu[(size_t)env * ND + i] = theta[(size_t)env * ND + i];
}

// dust_svmpc_batch_set(PRIOR_MIX): every environment's mixture log-weights from its weights (forward.hpp logmix_kernel's construction);
// one wave per environment, N <= 64
__global__ __launch_bounds__(64) void svmpc_batch_logmix_kernel(const float *w, float *logmix, const int N) {
  const int env = (int)blockIdx.x, lane = (int)threadIdx.x;
  const float v = lane < N ? w[(size_t)env * N + lane] : 0.f;
  const float s = wave_sum(v);
  float p = v / s;
  p = fminf(fmaxf(p, 1.1920929e-07f), 1.0f - 1.1920929e-07f);
  const float l = lane < N ? logf(p) : -INFINITY;
  const float lm = wave_max(l);
  const float zs = wave_sum(lane < N ? expf(l - lm) : 0.f);
  if (lane < N) logmix[(size_t)env * N + lane] = l - (lm + logf(zs));
}

static inline size_t svmpc_batch_lds_bytes(int N, int D, int M) { return sizeof(float) * (size_t)svb_lds_floats(N, D, M); }

}  // namespace dust
