// disco_batch.hpp - MultiDISCO over a batch of plants: forward(), step() or both of B independent controllers in ONE launch, and T
// closed-loop periods (forward, step, the plant) in ONE launch.  Workgroup b runs environment b - from its own state, a_mat, a_seq,
// a_mix and Philox stream - and talks to no other workgroup: no arrival word, nothing to spin on, the launch count does not depend on B.
//
// Replaces, per environment (reference file:line): MultiDISCO._rollout / _compute_cost / forward disco.py:139-394, MultiDISCO.step
// disco.py:396-417, and the use_svmpc=False branch of run_pendulum_simulation / run_particle_episode (simulations.py:124-126, 231-233).
// The lone pair dust_disco_forward / dust_disco_step (rollout.hpp, forward.hpp amix_kernel / disco_step_kernel / amat_roll_kernel) is
// the model: the same counter layout of the Philox draws, the same eps bases, the same quirks of step().
//
// forward, phases separated by workgroup barriers only (the device functions are svmpc_batch.hpp's: svb_coef, svb_traj; the phases are
// A / C / D / E of svb_tick without the SVGD half):
//   0  a_mat[b] [N][D], a_seq[b] [D] and the coefficients of the M dynamics rows -> LDS
//   A  actions[s][n] = a_mat[n] + chol_a z (z: Philox, block j >> 3 of row s N + n at the environment's {tick, iter} position - the lone
//      kernel's layout), or the caller's recorded actions -> the environment's action rows in device memory
//   C  the N S M rollouts: lane = (sample s, policy n, dynamics group g); costs[s][n] = mean over m, the G group partials (doubles in
//      LDS) added in the order g = 0 .. G - 1; then the control cost a_reg sum_j -(a_j - a_seq_j) (a_mat[n]_j a_pre_j) (disco.py:338-344;
//      eps = actions - a_seq there, whatever drew the actions), accumulated in double over j = 0 .. D - 1 as rollout.hpp does
//   D  per policy (one wave each, round-robin): min of its S costs, omega = exp(-(c - min) / temp), its mass, eta = -min / temp + log
//      mass; then a_mix = softmax_N(eta) (disco.py:393).  The reference subtracts ONE beta - the global minimum (disco.py:380-383); the
//      shift cancels in omega's softmax, and the per-policy minimum keeps a policy far above the best one from underflowing to 0 / 0.
//      eta as written here is the reference's plus beta / temp for every policy alike - carried back to the global beta - so the
//      softmax over N sees the reference's differences
//   E  a_mat[n] += sum_s omega eps / mass (disco.py:387-392): eps = a - a_mat[n] for drawn actions (and recorded ones under
//      DUST_EPS_AROUND_A_MAT), a - a_seq for recorded ones (disco.py:157-164); lane = (Q-th share of the samples, policy, column), the Q
//      partials added in the order q = 0 .. Q - 1.  The Philox position moves to {tick, iter + 1}, as bump_iter_kernel moves the lone one
// step: a_seq = the row of the FIRST maximum of a_mix (clamped IN PLACE: a_mat[argmax] is a view in the reference, disco.py:401, 410),
// a_mat^T a_mix (double accumulation over n = 0 .. N - 1, forward.hpp disco_step_kernel) or the caller's row; clamp; next_actions =
// a_seq[:steps]; a_seq and every a_mat row rolled by `steps` with zeros behind.
//
// Every sum runs in an order fixed by (N, S, M, H, d_a) and the workgroup size alone; nothing depends on B, on the block index or on
// timing, so an environment computes the same bits alone, in any slot of any batch, and beside inactive neighbours.
//
// Launch shape: svmpc_batch.hpp's - 512 lanes, svmpc_batch_lds_bytes() of dynamic LDS (this body's rows fit inside that plan: svb_begin
// stages the navigation map behind it, and finds it there).  Not measured: a smaller LDS plan of its own, 256 or 1024 lanes, the action
// tile in LDS.
//
// SIGMA (the "DISCO" case: MultiDISCO(params_sampling=MerweScaledUTF), disco.py:211-292, 312-323): the M parameter rows are the pts sigma
// points and a rollout's cost is the weighted SUM of the lone kernels (rollout.hpp, skid.hpp, cartpole.hpp)
//     sum_m sum_t mw[(m H + t) mod M] inst(x_{m,t}) + sum_m mw[m] term(x_{m,H})
// - the reference views its flat [rollout][step] block of instantaneous costs as rows of M consecutive entries, so entry (m, t) meets
// weight (m H + t) mod M.  Lane = (sample, policy) with the points in sequence; the weighted terms accumulate in double, the two parts
// are rounded and added in fp32.  A template parameter: the plain instances keep their instructions.
#pragma once
#include "svmpc_episode.hpp"

namespace dust {

struct DiscoBatchArgs {
  // k: dm, sk, cp, N .. P, G, Q, temp, dt, chol_a, philox, states, seeds, active, ctr, alias (svb_begin reads it; nothing here acts on it),
  // eps = the recorded actions [B][S][N][D] or nullptr, params [B][M][P] (an episode: [T][B][M][P]), a_mat [B][N][D], acts [B][S][N][D],
  // costs / wts (unnormalised omega) / omg (omega) [B][S][N], eta / a_mix [B][N]; n_steps = 1
  SvmpcBatchArgs k;
  float a_reg, a_pre[2];
  float min_a[2], max_a[2];
  int do_forward, do_step;
  int around_a_mat;  // recorded actions: eps = a - a_mat[n] (DUST_EPS_AROUND_A_MAT), not a - a_seq
  int strategy, steps;
  float *a_seq;      // [B][D]
  const float *ext;  // [B][D] the caller's rows ("external") or nullptr
  const float *mw;   // [M] the sigma weights (SIGMA instances) or nullptr
  float *next;       // [B][steps][da] or nullptr
};

// One sigma point's share of a rollout's cost: wi += sum_t mw[(m H + t) mod M] inst(x_t, a_t), wt += mw[m] term(x_H), under the
// coefficients `cf` of point m.  The general loops of svb_traj, cost by cost (the Pendulum without the shared-reduction trig, as
// rollout.hpp runs its sigma-point form).
template <int MODEL, bool NAV>
__device__ __forceinline__ void dcb_traj_sigma(const SvmpcBatchArgs &a, const float *act, const float *cf, const float *x0, const float *mw, const int m,
                                               double &wi, double &wt, const float w_obs, const DevModel *map) {
  static_assert(MODEL != DUST_MODEL_PARTICLE, "no sigma-point form for Particle rollouts in the batch");
  constexpr int DS = SvbDims<MODEL>::DS;
  const int H = a.H, M = a.M;
  float x[DS];
#pragma unroll
  for (int k = 0; k < DS; ++k) x[k] = x0[k];
  int wi_idx = (int)(((long)m * H) % M);  // (m H + t) mod M, stepped
  auto next_w = [&]() {
    const double w = (double)mw[wi_idx];
    wi_idx = wi_idx + 1 == M ? 0 : wi_idx + 1;
    return w;
  };
  if constexpr (MODEL == DUST_MODEL_PENDULUM) {
    Coef c;
    c.c0 = cf[0];
    c.c1 = cf[1];
    for (int t = 0; t < H; ++t) {
      const float at[1] = {act[t]};
      const float ci = step_with_cost<MODEL>(a.dm, c, x, at);
      wi += next_w() * (double)ci;
    }
    wt += (double)mw[m] * (double)term_cost<MODEL>(a.dm, x);
  } else if constexpr (MODEL == DUST_MODEL_SKID_STEER) {
    const float xicr = cf[0], wr = cf[1], ad = cf[2];
    for (int t = 0; t < H; ++t) {
      const float a0 = act[2 * t], a1 = act[2 * t + 1];
      double sc = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float d = x[k] - a.sk.goal[k];
        sc += (double)((d * d) * a.sk.w_state[k]);
      }
      const double cc = (double)((a0 * a0) * a.sk.w_ctrl[0]) + (double)((a1 * a1) * a.sk.w_ctrl[1]);
      float ic = (float)sc + (float)cc;
      if constexpr (NAV) ic = ic + w_obs * collision(*map, x[0], x[1]);  // (quad + ctrl) + obst
      wi += next_w() * (double)ic;
      skid_step(x, clampf(a0, a.sk.lo[0], a.sk.hi[0]), clampf(a1, a.sk.lo[1], a.sk.hi[1]), xicr, wr, ad, a.dt);
    }
    double tc = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float d = x[k] - a.sk.goal[k];
      tc += (double)((d * d) * a.sk.w_term[k]);
    }
    float tcf = (float)tc;
    if constexpr (NAV) tcf = tcf + w_obs * collision(*map, x[0], x[1]);
    wt += (double)mw[m] * (double)tcf;
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
    for (int t = 0; t < H; ++t) {
      const float a0 = act[t];
      double sc = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = x[k] - a.cp.goal[k];
        sc += (double)((d * d) * a.cp.w_state[k]);
      }
      const double cc = (double)((a0 * a0) * a.cp.w_ctrl[0]);
      wi += next_w() * (double)((float)sc + (float)cc);
      cartpole_step(x, clampf(a0, -1.0f, 1.0f), kf, fast_sinf(x[2]), fast_cosf(x[2]));
    }
    double tc = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = x[k] - a.cp.goal[k];
      tc += (double)((d * d) * a.cp.w_term[k]);
    }
    wt += (double)mw[m] * (double)(float)tc;
  }
}

// forward() and / or step() of environment blockIdx.x from the carry `cy` (state, Philox position).  `params`: this call's rows
// [B][M][P] or nullptr.  act0 (may be nullptr): the first action of the clamped sequence step() chose, in every lane.
template <int MODEL, bool NAV, bool SIGMA>
__device__ __forceinline__ void disco_tick(const DiscoBatchArgs &da_, const float *params, SvbCarry<MODEL> &cy, const DevModel &map, const float w_obs,
                                           float *act0) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int T = SVB_THREADS;
  const SvmpcBatchArgs &a = da_.k;
  const int env = (int)blockIdx.x;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, S = a.S, M = a.M, H = a.H, da = a.da, D = a.D;
  const int ND = N * D, NS = N * S;

  // ---- LDS: partial sums first (doubles), then the rows every lane reads; all of it inside svb_lds_floats(N, D, M)
  double *accp = reinterpret_cast<double *>(lds);  // [SVB_PART] phase C group partials
  float *part = lds;                               // [T] phase E share partials (the same bytes, another phase)
  float *am = lds + 2 * SVB_PART;                  // [N][D] a_mat
  float *sq = am + ND;                             // [D] a_seq
  float *sn = sq + D;                              // [D] step(): the new sequence before the roll
  float *coef = sn + D;                            // [M][SVB_COEF]
  float *zo = coef + M * SVB_COEF;                 // [N] mass of omega
  float *lw = zo + N;                              // [N] eta, then a_mix
  int *misc = reinterpret_cast<int *>(lw + N);     // [1] argmax

  float *g_amat = a.a_mat + (size_t)env * ND, *g_aseq = da_.a_seq + (size_t)env * D;
  float *g_acts = a.acts + (size_t)env * NS * D;
  float *g_costs = a.costs + (size_t)env * NS, *g_wts = a.wts + (size_t)env * NS, *g_omg = a.omg + (size_t)env * NS;
  float *g_eta = a.eta + (size_t)env * N, *g_amix = a.a_mix + (size_t)env * N;
  auto col2 = [&](const float *v, const int j) { return (da == 2 && (j & 1)) ? v[1] : v[0]; };

  if (da_.do_forward) {
    const uint64_t seed = a.seeds[env];
    const float *x0 = cy.x0;
    const bool fast_trig = MODEL == DUST_MODEL_PENDULUM && fabsf(x0[1]) <= 3.0e38f &&
                           (fabsf(x0[0]) + a.dm.max_speed_pend * (float)a.dm.dt * (float)H < 5.0e4f);
    // ---- 0: stage
    for (int i = tid; i < ND; i += T) am[i] = g_amat[i];
    for (int i = tid; i < D; i += T) sq[i] = g_aseq[i];
    for (int m = tid; m < M; m += T) {
      const float *prow = params ? params + ((size_t)env * M + m) * a.P : nullptr;
      float cf[SVB_COEF];
      svb_coef<MODEL>(a, prow, cf);
      constexpr int NC = (MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_PARTICLE) ? 2 : (MODEL == DUST_MODEL_SKID_STEER ? 3 : SVB_COEF);
#pragma unroll
      for (int q = 0; q < NC; ++q) coef[m * SVB_COEF + q] = cf[q];
    }
    svb_sync();

    // ---- A: actions
    if (a.philox) {
      const int nb8 = (D + 7) >> 3;
      for (int w = tid; w < NS * nb8; w += T) {
        const int row = w / nb8, j8 = w - row * nb8, n = row % N;
        float z[8];
        philox_normal8(seed, (uint32_t)j8, (uint32_t)row, cy.ctr_iter, cy.ctr_tick, z);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int j = j8 * 8 + q;
          if (j < D) g_acts[(size_t)row * D + j] = am[n * D + j] + col2(a.chol_a, j) * z[q];
        }
      }
    } else {
      const float *rec = a.eps + (size_t)env * NS * D;
      for (int w = tid; w < NS * D; w += T) g_acts[w] = rec[w];
    }
    svb_sync();

    // ---- C: rollouts, control cost
    {
      const int G = a.G;
      auto finish = [&](const int row, const double acc, const bool is_sum = false) {
        float cost = (M == 1 || is_sum) ? (float)acc : (float)(acc / M);
        if (da_.a_reg != 0.0f) {  // disco.py:338-346, the diagonal of the [S, N, N] tensordot only
          const int n = row % N;
          const float *act = g_acts + (size_t)row * D;
          double cc = 0.0;
          for (int j = 0; j < D; ++j) {
            const float e = act[j] - sq[j];
            const float ap = am[n * D + j] * col2(da_.a_pre, j);
            cc += (double)(-e) * (double)ap;
          }
          cost = cost + da_.a_reg * (float)cc;
        }
        g_costs[row] = cost;
      };
      if constexpr (SIGMA) {  // lane = (sample, policy), the sigma points in sequence: a weighted sum, not a mean
        for (int row = tid; row < NS; row += T) {
          const float *act = g_acts + (size_t)row * D;
          double wi = 0.0, wt = 0.0;
          for (int m = 0; m < M; ++m) dcb_traj_sigma<MODEL, NAV>(a, act, coef + m * SVB_COEF, x0, da_.mw, m, wi, wt, w_obs, &map);
          finish(row, (double)((float)wi + (float)wt), true);
        }
      } else
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
        if (G == 1) finish(row, acc);
        else accp[w] = acc;
      }
      if (!SIGMA && G > 1) {
        svb_sync();
        for (int row = tid; row < NS; row += T) {
          double acc = accp[row];
          for (int g = 1; g < G; ++g) acc += accp[g * NS + row];
          finish(row, acc);
        }
      }
    }
    svb_sync();

    // ---- D: per policy, one wave each: omega, its mass, eta
    for (int n = wave; n < N; n += T / 64) {
      float cmin = INFINITY;
      for (int s = lane; s < S; s += 64) cmin = fminf(cmin, g_costs[s * N + n]);
      cmin = wave_min(cmin);
      float mo = 0.f;
      for (int s = lane; s < S; s += 64) {
        const float eo = expf((-1.0f * (g_costs[s * N + n] - cmin)) / a.temp);  // disco.py:381
        g_wts[s * N + n] = eo;
        mo += eo;
      }
      mo = wave_sum(mo);
      for (int s = lane; s < S; s += 64) g_omg[s * N + n] = expf((-1.0f * (g_costs[s * N + n] - cmin)) / a.temp) / mo;  // omega, for the getter
      if (lane == 0) {
        zo[n] = mo;
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
      if (lane < N) g_amix[lane] = expf(v - lz);
    }

    // ---- E: a_mat += sum_s omega eps
    {
      const int Q = a.Q;
      const bool around = a.philox || da_.around_a_mat;
      auto share = [&](const int e, const int q0, const int qs) {
        const int n = e / D, j = e - n * D;
        const float base = around ? am[e] : sq[j];
        float acc = 0.f;
        for (int s = q0; s < S; s += qs) {
          const int row = s * N + n;
          acc = fmaf(g_wts[row], g_acts[(size_t)row * D + j] - base, acc);
        }
        return acc;
      };
      if (Q == 1) {
        for (int e = tid; e < ND; e += T) g_amat[e] = am[e] + share(e, 0, 1) / zo[e / D];
      } else {
        if (tid < Q * ND) {
          const int q = tid / ND;
          part[tid] = share(tid - q * ND, q, Q);
        }
        svb_sync();
        if (tid < ND) {
          float acc = part[tid];
          for (int q = 1; q < Q; ++q) acc += part[q * ND + tid];
          g_amat[tid] = am[tid] + acc / zo[tid / D];
        }
      }
    }
    cy.ctr_iter += 1u;
    svb_sync();
  }

  if (da_.do_step) {
    // ---- MultiDISCO.step: the rows as they stand in device memory (this launch's forward has just written them)
    for (int i = tid; i < ND; i += T) am[i] = g_amat[i];
    for (int i = tid; i < N; i += T) lw[i] = g_amix[i];
    svb_sync();
    if (da_.strategy == DUST_STEP_ARGMAX) {
      if (wave == 0) {  // first index of the maximum (torch.argmax on CPU)
        float best = lane < N ? lw[lane] : -INFINITY;
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
      }
      svb_sync();
      const int bi = misc[0];
      for (int j = tid; j < D; j += T) sn[j] = clampf(am[bi * D + j], col2(da_.min_a, j), col2(da_.max_a, j));
      svb_sync();
      for (int j = tid; j < D; j += T) am[bi * D + j] = sn[j];  // quirk: a_mat[argmax] is a view, the in-place clamp_ reaches a_mat too
    } else if (da_.strategy == DUST_STEP_AVERAGE) {
      for (int j = tid; j < D; j += T) {
        double acc = 0.0;
        for (int n = 0; n < N; ++n) acc += (double)am[n * D + j] * (double)lw[n];
        sn[j] = clampf((float)acc, col2(da_.min_a, j), col2(da_.max_a, j));
      }
    } else {
      const float *ext = da_.ext + (size_t)env * D;
      for (int j = tid; j < D; j += T) sn[j] = clampf(ext[j], col2(da_.min_a, j), col2(da_.max_a, j));
    }
    svb_sync();
    const int sh = da_.steps * da;
    if (da_.next)
      for (int j = tid; j < sh; j += T) da_.next[(size_t)env * sh + j] = sn[j];
    for (int j = tid; j < D; j += T) g_aseq[j] = (j + sh < D) ? sn[j + sh] : 0.f;
    for (int e = tid; e < ND; e += T) {
      const int n = e / D, j = e - n * D;
      g_amat[e] = (j + sh < D) ? am[n * D + j + sh] : 0.f;
    }
    if (act0) {
      act0[0] = sn[0];
      if (da == 2) act0[1] = sn[1];
    }
  }
}

// one call per launch: forward, step, or both
template <int MODEL, bool NAV, bool SIGMA>
__device__ __forceinline__ void disco_body(const DiscoBatchArgs &a, const SkidNav *nav) {
  if (a.k.active && a.k.active[blockIdx.x] == 0) return;
  SvbCarry<MODEL> cy;
  DevModel map;
  float w_obs;
  svb_begin<MODEL, NAV>(a.k, nav, cy, map, w_obs);
  disco_tick<MODEL, NAV, SIGMA>(a, a.k.params, cy, map, w_obs, nullptr);
  svb_end(a.k, cy);
}

template <int MODEL, bool SIGMA>
__global__ __launch_bounds__(SVB_THREADS) void disco_batch_kernel(const DiscoBatchArgs a) {
  disco_body<MODEL, false, SIGMA>(a, nullptr);
}
struct DiscoNavBatchArgs {
  DiscoBatchArgs d;
  SkidNav nav;
};
template <bool SIGMA>
__global__ __launch_bounds__(SVB_THREADS) void disco_skid_nav_batch_kernel(const DiscoNavBatchArgs kn) {
  disco_body<DUST_MODEL_SKID_STEER, true, SIGMA>(kn.d, &kn.nav);
}

// T closed-loop periods per launch: forward, step(strategy, 1), the plant under the environment's true row (svb_plant_step), records; with
// rules (has_rules) the reference's episode rules as svb_sim_body applies them - without a warm-up, which this branch of the reference
// does not have.  Whether an environment leaves the loop is computed by EVERY lane from the carry in its registers and read-only data,
// and the loop is left behind a period's closing svb_sync() alone.
struct DiscoEpisodeArgs {
  DiscoBatchArgs d;  // k.params: [T][B][M][P], or [B][M][P] when params_once; do_forward, do_step and k.philox set, steps = 1
  SvbEpisode ep;     // pw_out unused
  SvbRules ru;
  int has_rules, params_once;
};
struct DiscoNavEpisodeArgs {
  DiscoEpisodeArgs e;
  SkidNav nav;
};

template <int MODEL, bool NAV, bool SIGMA>
__device__ __forceinline__ void disco_episode_body(const DiscoEpisodeArgs &ka, const SkidNav *nav) {
  constexpr int DS = SvbDims<MODEL>::DS;
  const DiscoBatchArgs &d = ka.d;
  const SvmpcBatchArgs &a = d.k;
  const SvbEpisode &ep = ka.ep;
  const SvbRules &ru = ka.ru;
  const int env = (int)blockIdx.x, B = (int)gridDim.x;
  if (a.active && a.active[env] == 0) return;
  if (ka.has_rules && ru.status[env] != 0) return;  // (written by the host before the launch; this launch stores it once, at its very end)
  SvbCarry<MODEL> cy;
  DevModel map;
  float w_obs;
  svb_begin<MODEL, NAV>(a, nav, cy, map, w_obs);
  float cf[SVB_COEF];
  svb_coef<MODEL>(a, ep.plant ? ep.plant + (size_t)env * a.P : nullptr, cf);
  const size_t per = ka.params_once ? 0 : (size_t)B * a.M * a.P;  // parameter rows of one period
  float loss = ka.has_rules ? ru.loss[env] : 0.f;
  int status = 0, n = 0;
  for (int t = 0; t < ep.T; ++t) {
    const size_t row = (size_t)t * B + env;
    float act[2] = {0.f, 0.f};
    disco_tick<MODEL, NAV, SIGMA>(d, a.params ? a.params + (size_t)t * per : nullptr, cy, map, w_obs, act);
    svb_plant_step<MODEL>(a, cf, cy.x0, act);
    float cost = 0.f;
    if (ka.has_rules) {
      cost = svb_state_cost<MODEL, NAV>(a, cy.x0, map, w_obs);
      loss += cost;
      if (ru.goal_on) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < DS; ++k) {
          const float dd = ru.goal[k] - cy.x0[k];
          s = k == 0 ? dd * dd : s + dd * dd;
        }
        if (s <= ru.r2) status = 1;
      }
      if (ru.stop_on_crash && svb_crashed<MODEL, NAV>(a, cy.x0, map)) {  // (the crash rule wins)
        status = 2;
        loss = INFINITY;
      }
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < DS; ++k) ep.states_out[row * DS + k] = cy.x0[k];
      ep.actions_out[row * a.da] = act[0];
      if (a.da == 2) ep.actions_out[row * 2 + 1] = act[1];
      if (ka.has_rules) ru.costs_out[row] = cost;
    }
    n = t + 1;
    svb_sync();  // the roll has read the LDS rows, the next period's phase 0 overwrites them
    if (status != 0) break;
  }
  svb_end(a, cy);
  if (ka.has_rules && threadIdx.x == 0) {
    ru.n_run[env] = n;
    ru.status[env] = status;
    ru.loss[env] = loss;
  }
}

template <int MODEL, bool SIGMA>
__global__ __launch_bounds__(SVB_THREADS) void disco_episode_kernel(const DiscoEpisodeArgs ka) {
  disco_episode_body<MODEL, false, SIGMA>(ka, nullptr);
}
template <bool SIGMA>
__global__ __launch_bounds__(SVB_THREADS) void disco_skid_nav_episode_kernel(const DiscoNavEpisodeArgs kn) {
  disco_episode_body<DUST_MODEL_SKID_STEER, true, SIGMA>(kn.e, &kn.nav);
}

}  // namespace dust
