// svmpc_episode.hpp - closed-loop episodes on the device: T control periods of B independent environments in ONE launch.
// Workgroup b runs, for t = 0 .. T - 1, the loop of the reference's run_simulation (dust/utils/simulations.py:104-130) on environment b:
//   1  the tick of svmpc_batch.hpp (svb_tick, the very function svmpc_batch_kernel runs: n_steps SVGD iterations and forward()) from the
//      state the previous period left, with the dynamics rows params[t][b][it][m][:] and device-drawn noise - forward() moves the Philox
//      position to {tick + 1, 0}, so period t draws what the t-th successive dust_svmpc_batch_tick would draw;
//   2  the plant: x <- step(x, a_seq[0]) with the first action of the sequence forward() chose BEFORE the roll, through the family's own
//      device step - the one the rollouts of phase C call (common.hpp model_step, skid.hpp skid_step, cartpole.hpp cartpole_step; for
//      Particle with the collision freeze on its occupancy grid), the action clamped as the rollouts clamp it - under the coefficients
//      svb_coef makes of the environment's TRUE parameter row plant[b][:] (the columns and the space of `params`; NULL: the prototype's
//      nominal model).  Plants are deterministic;
//   3  the records states_out[t][b][:] (the state after the step), actions_out[t][b][:] (the raw a_seq[0]) and pw_out[t][b][:] (the
//      particle weights of forward()).
// As in the batched tick there is no arrival word, nothing to spin on and no traffic between workgroups; the loop is bounded by T.
//
// What a period hands to the next never passes through memory that one lane writes and all lanes re-read at one address: the state, the
// Philox position, the optimiser's step count and the alias flag stay in registers (SvbCarry: every lane computes the same plant step
// from the same a_seq[0], which it reads from the particles' LDS rows); the particles, prior means, mixture log-weights, a_mat and
// optimiser state are per-lane rows in device memory, read by vector loads behind the period's closing svb_sync().  So no scalar load
// can return the previous period's value.
//
// Launch shape: the batched tick's - 512 lanes, one workgroup per environment, svmpc_batch_lds_bytes() of dynamic LDS (plus the map in
// the navigation instance).  The navigation instance stages its map ONCE per launch, ahead of the period loop, as the batched tick
// does ahead of its iteration loop; restaging it every period has not been measured, nor has the difference.
//
// svmpc_sim_kernel / svmpc_skid_nav_sim_kernel / svmpc_rows_sim_kernel (svb_sim_body, dust_svmpc_batch_simulate): the same loop under the
// rules of the reference's run_particle_episode / run_pendulum_simulation (simulations.py:104-130, 217-260) - while the episode warms
// up a period is the tick WITHOUT forward() (what dust_svmpc_batch_optimize runs) and the plant gets a zero action; the family's own
// instantaneous cost of every new state is recorded and summed in fp32 into the loss; a crash (loss = +inf) or the goal ends the
// environment.  A second body beside svb_episode_body: the kernels above keep their text.  The loop has barriers, so whether a workgroup
// leaves it is computed by every lane from the carry in its registers and from read-only data (map, rules) - the same in all lanes by
// construction -, and it is left behind a period's closing svb_sync() alone, through svb_end.  Still no spinning, no traffic between
// workgroups, at most T periods.
//
// svmpc_dual_period_kernel: ONE period of the dual loop (simulations.py:104-138) per launch, for dust_svmpc_dual_batch_episode.  The filter
// update of a period is a launch of its own (mpf_optimize_batch_kernel: 1 024 lanes, another order of partial sums), so the periods of
// that episode are a chain of launches on one stream, with no host in between; what a period hands to the next - the state row and the
// filters' MpfEnvIn row - is written here by lane 0 and read by LATER launches only, so the carry of one period still lives in registers.
//
// svmpc_dual_sim_period_kernel: that period under the rules of svb_sim_body, for dust_svmpc_dual_batch_simulate.  The host sets do_forward
// per launch (0 while the episode warms up: the filters still update, the plant gets the zero action); the loss, the status and the count
// of periods are words in device memory that lane 0 of one launch writes and LATER launches read; a stopping environment clears its
// byte of the call's run mask with its last store, and every later launch of the call - Silverman's rule, the filters' update, this
// kernel - skips the environment.  A second body beside svb_dual_period_body: svmpc_dual_period_kernel keeps its text.
//
// svmpc_sim_hist_kernel / svmpc_dual_sim_hist_period_kernel (dust_svmpc_batch_set_history): the two rule-driven kernels above plus the
// posterior's history - the reference's PolParticles / DynParticles rows (simulations.py:122, 134-137).  Behind the sync that closes a
// period the workgroup copies the environment's particles theta [N][D] - as the period's closing operation left them: the optimiser
// step while the episode warms up, forward()'s roll afterwards - into theta_hist[t][b], and the dual form also the filter's particles
// [Mp][P] its tick drew from into x_hist[t][b]: all 512 lanes, strided, float4 where the rows are whole quads, ordinary vector stores.
// A period that does not run writes nothing.  The copies sit behind `if constexpr (HIST)` in the shared bodies: the instances above
// keep their code.  No launch is added: the copy rides the period's own.
#pragma once
#include "mpf_env.hpp"
#include "svmpc_batch.hpp"

namespace dust {

struct SvbEpisode {
  int T;               // periods
  const float *plant;  // [B][P] true parameter rows or nullptr (nominal plants)
  float *states_out;   // [T][B][ds]
  float *actions_out;  // [T][B][da]
  float *pw_out;       // [T][B][N] or nullptr
};
struct SvmpcEpisodeArgs {
  SvmpcBatchArgs k;  // params: [T][B][n_steps][M][P]; n_steps >= 1, do_forward and philox set
  SvbEpisode ep;
};
struct SvmpcNavEpisodeArgs {
  SvmpcBatchArgs k;
  SvbEpisode ep;
  SkidNav nav;
};

// x <- step(x, act) of the family's plant under the coefficients cf (svb_coef); `act` is the raw action
// ARGS: as svb_coef's
template <int MODEL, class ARGS>
__device__ __forceinline__ void svb_plant_step(const ARGS &a, const float *cf, float *x, const float *act) {
  if constexpr (MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_PARTICLE) {
    Coef c;
    c.c0 = cf[0];
    c.c1 = cf[1];
    model_step<MODEL>(a.dm, c, x, act);
  } else if constexpr (MODEL == DUST_MODEL_SKID_STEER) {
    skid_step(x, clampf(act[0], a.sk.lo[0], a.sk.hi[0]), clampf(act[1], a.sk.lo[1], a.sk.hi[1]), cf[0], cf[1], cf[2], a.dt);
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
    cartpole_step(x, clampf(act[0], -1.0f, 1.0f), kf, fast_sinf(x[2]), fast_cosf(x[2]));
  }
}

template <int MODEL, bool NAV>
__device__ __forceinline__ void svb_episode_body(const SvmpcBatchArgs &a, const SvbEpisode &ep, const SkidNav *nav) {
  constexpr int DS = SvbDims<MODEL>::DS;
  const int env = (int)blockIdx.x, B = (int)gridDim.x;
  if (a.active && a.active[env] == 0) return;
  SvbCarry<MODEL> cy;
  DevModel map;
  float w_obs;
  svb_begin<MODEL, NAV>(a, nav, cy, map, w_obs);
  float cf[SVB_COEF];
  svb_coef<MODEL>(a, ep.plant ? ep.plant + (size_t)env * a.P : nullptr, cf);
  const size_t per = (size_t)B * a.n_steps * a.M * a.P;  // parameter rows of one period
  for (int t = 0; t < ep.T; ++t) {
    const size_t row = (size_t)t * B + env;
    float act[2] = {0.f, 0.f};
    svb_tick<MODEL, false, NAV, true>(a, nullptr, a.params ? a.params + (size_t)t * per : nullptr, cy, map, w_obs,
                                      ep.pw_out ? ep.pw_out + row * a.N : nullptr, act);
    svb_plant_step<MODEL>(a, cf, cy.x0, act);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < DS; ++k) ep.states_out[row * DS + k] = cy.x0[k];
      ep.actions_out[row * a.da] = act[0];
      if (a.da == 2) ep.actions_out[row * 2 + 1] = act[1];
    }
    svb_sync();  // the roll has read the particles' LDS rows, the next period's phase 0 overwrites them
  }
  svb_end(a, cy);
}

template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_episode_kernel(const SvmpcEpisodeArgs ka) {
  svb_episode_body<MODEL, false>(ka.k, ka.ep, nullptr);
}
__global__ __launch_bounds__(SVB_THREADS) void svmpc_skid_nav_episode_kernel(const SvmpcNavEpisodeArgs ka) {
  svb_episode_body<DUST_MODEL_SKID_STEER, true>(ka.k, ka.ep, &ka.nav);
}

// ... with per-environment hyper-parameters (svmpc_batch.hpp SvbHyper): the workgroup's own copy of the arguments, the same body
struct SvmpcSweepEpisodeArgs {
  SvmpcBatchArgs k;
  SvbEpisode ep;
  const SvbHyper *rows;  // [B]
};
template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_sweep_episode_kernel(const SvmpcSweepEpisodeArgs ka) {
  const SvbHyper h = ka.rows[blockIdx.x];  // (the whole row, ahead of the copy)
  SvmpcBatchArgs a = ka.k;
  SVB_HYPER_APPLY(a, h);
  svb_episode_body<MODEL, false>(a, ka.ep, nullptr);
}

// What a period of the dual episode adds to the PRIOR tick's arguments
struct SvbDualPeriod {
  const float *plant;  // [B][P] true parameter rows or nullptr (nominal plants)
  float *state;        // [B][8]: the rows SvmpcBatchArgs::states names; x_{t+1} for the next period's launch
  MpfEnvIn *in;        // [B]: what the NEXT period's filter update reads
  float *states_out;   // [B][ds], this period's rows of the records
  float *actions_out;  // [B][da]
  float *pw_out;       // [B][N] or nullptr
  const float *bw;     // [B] the bandwidths Silverman's rule gave this period's update, or nullptr (no update, or a fixed bandwidth)
  float *bw_out;       // [B] or nullptr: ... recorded (0 where no update ran)
  int t0_add;          // the optimiser steps this period's filter update took (0: no update ran)
  int condition;       // 0 in the call's last period: (a_{T-1}, x_T) stays pending, the row keeps the pair the last update read
};
struct SvmpcDualPeriodArgs {
  SvmpcBatchArgs k;  // states: the device state rows; n_steps >= 1, do_forward and philox set
  SvbPrior pr;       // seeds: this period's row of prior_seeds
  SvbDualPeriod dp;
};

// One period of environment blockIdx.x: the PRIOR tick on the state the previous launch left, the plant's step, the records, and
// GaussianLikelihood.condition (likelihoods.py:51-64) for the next period's update - mpfb_enqueue's host arithmetic (mpf.hpp) on the
// environment's device row: past_obs <- obs, obs <- x_{t+1}, past_action <- a_t (zero-padded), t0 advanced by the steps just taken
template <int MODEL>
__device__ __forceinline__ void svb_dual_period_body(const SvmpcBatchArgs &a, const SvbPrior &pri, const SvbDualPeriod &dp) {
  static_assert(MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_PARTICLE, "the other families' likelihood rows are made on the host");
  constexpr int DS = SvbDims<MODEL>::DS;
  const int env = (int)blockIdx.x;
  if (a.active && a.active[env] == 0) return;
  SvbCarry<MODEL> cy;
  DevModel map;
  float w_obs;
  svb_begin<MODEL, false>(a, nullptr, cy, map, w_obs);
  float cf[SVB_COEF];
  svb_coef<MODEL>(a, dp.plant ? dp.plant + (size_t)env * a.P : nullptr, cf);
  float act[2] = {0.f, 0.f};
  svb_tick<MODEL, true, false, true>(a, &pri, nullptr, cy, map, w_obs, dp.pw_out ? dp.pw_out + (size_t)env * a.N : nullptr, act);
  svb_plant_step<MODEL>(a, cf, cy.x0, act);
  if (threadIdx.x == 0) {
    float *xs = dp.state + (size_t)env * 8;
    MpfEnvIn *in = dp.in + env;
#pragma unroll
    for (int k = 0; k < DS; ++k) {
      dp.states_out[(size_t)env * DS + k] = cy.x0[k];
      xs[k] = cy.x0[k];
    }
    dp.actions_out[(size_t)env * a.da] = act[0];
    if (a.da == 2) dp.actions_out[(size_t)env * 2 + 1] = act[1];
    if (dp.bw_out) dp.bw_out[env] = dp.bw ? dp.bw[env] : 0.f;
    if (dp.condition) {
#pragma unroll
      for (int k = 0; k < 4; ++k) in->past_obs[k] = in->obs[k];
#pragma unroll
      for (int k = 0; k < DS; ++k) in->obs[k] = cy.x0[k];
      in->past_action[0] = act[0];
      in->past_action[1] = act[1];
    }
    if (dp.t0_add) in->t0 += dp.t0_add;
  }
  svb_end(a, cy);
}

template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_dual_period_kernel(const SvmpcDualPeriodArgs ka) {
  svb_dual_period_body<MODEL>(ka.k, ka.pr, ka.dp);
}

// The posterior's history (dust_svmpc_batch_set_history): where the recording kernels put a period's rows.  svmpc_sim_hist_kernel: the
// call's blocks [T][B][..]; svmpc_dual_sim_hist_period_kernel: this period's rows [B][..].  nullptr: that kind is not recorded
struct SvbHist {
  float *theta;  // [N][D] per (period, environment)
  float *x;      // [Mp][P] per (period, environment): the dual form alone
};
// n floats src -> dst by every lane of the workgroup, behind a svb_sync() that made `src` visible.  Both rows start n floats times an
// index behind a hipMalloc'ed base: with n a multiple of 4 they lie on 16-byte boundaries and move as float4
__device__ __forceinline__ void svb_hist_copy(float *dst, const float *src, const int n) {
  if ((n & 3) == 0) {
    const float4 *s4 = reinterpret_cast<const float4 *>(src);
    float4 *d4 = reinterpret_cast<float4 *>(dst);
    for (int i = (int)threadIdx.x; i < (n >> 2); i += SVB_THREADS) d4[i] = s4[i];
  } else {
    for (int i = (int)threadIdx.x; i < n; i += SVB_THREADS) dst[i] = src[i];
  }
}

// The reference's episode rules (run_particle_episode / run_pendulum_simulation, simulations.py:104-130, 217-260) for
// dust_svmpc_batch_simulate: what svb_sim_body adds to svb_episode_body.  Period t of the call is period g = t0 + t of the episode.
struct SvbRules {
  int t0, warm_up;    // g < warm_up: optimize only (no forward), the plant gets a zero action
  int stop_on_crash;  // the new position on an occupied cell: loss = +inf, status 2
  int goal_on;        // |goal - x|^2 <= r2: status 1
  float r2;           // (float)(radius * radius), made once on the host
  float goal[8];
  float *costs_out;  // [T][B] the instantaneous cost of the state after the step
  float *loss;       // [B] in-out: the fp32 running sum of the costs in period order
  int *status;       // [B] in-out: 0 running, 1 goal, 2 crash
  int *n_run;        // [B] out: the periods this call ran
};
struct SvmpcSimArgs {
  SvmpcBatchArgs k;
  SvbEpisode ep;
  SvbRules ru;
};
struct SvmpcNavSimArgs {
  SvmpcBatchArgs k;
  SvbEpisode ep;
  SvbRules ru;
  SkidNav nav;
};
struct SvmpcRowsSimArgs {
  SvmpcBatchArgs k;
  SvbEpisode ep;
  SvbRules ru;
  const SvbHyper *rows;  // [B]
};

// controller.inst_cost_fn(state) of the plant's new state: the family's own instantaneous cost, the one the rollouts of phase C call, with
// a zero action (Particle: w_obs collision() included; skid-steer / cart-pole: the quadratic state cost of svb_traj, NAV: plus the map term)
// ARGS: as svb_coef's (the AMPPI periods under the rules, amppi_episode.hpp, hand it their environment's view)
template <int MODEL, bool NAV, class ARGS>
__device__ __forceinline__ float svb_state_cost(const ARGS &a, const float *x, const DevModel &map, const float w_obs) {
  if constexpr (MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_PARTICLE) {
    const float zero[2] = {0.f, 0.f};
    return inst_cost<MODEL>(a.dm, x, zero);
  } else {
    constexpr int DS = SvbDims<MODEL>::DS;
    double sc = 0.0;
#pragma unroll
    for (int k = 0; k < DS; ++k) {
      float d, w;
      if constexpr (MODEL == DUST_MODEL_SKID_STEER) {
        d = x[k] - a.sk.goal[k];
        w = a.sk.w_state[k];
      } else {
        d = x[k] - a.cp.goal[k];
        w = a.cp.w_state[k];
      }
      sc += (double)((d * d) * w);
    }
    if constexpr (NAV) return (float)sc + w_obs * collision(map, x[0], x[1]);
    else return (float)sc;
  }
}

// obst_map.get_collisions(state[:2]) of the new position: Particle on its own map, the skid-steer navigation instance on its own
template <int MODEL, bool NAV, class ARGS>
__device__ __forceinline__ bool svb_crashed(const ARGS &a, const float *x, const DevModel &map) {
  if constexpr (MODEL == DUST_MODEL_PARTICLE) return collision(a.dm, x[0], x[1]) != 0.f;
  else if constexpr (NAV) return collision(map, x[0], x[1]) != 0.f;
  else return false;  // (the host refuses the rule for every other family)
}

// svb_episode_body's loop under the rules.  Whether an environment leaves the loop is computed by EVERY lane from the carry in its
// registers (cy.x0) and from read-only data (map, rules) - never from a word one lane stored earlier in the launch -, so the decision is
// the same in all 512 lanes by construction; the loop is left at a period's end alone, behind its closing svb_sync(), and through svb_end.
// HIST (svmpc_sim_hist_kernel): behind the period's closing sync the particles also go to hs->theta[t][env]
template <int MODEL, bool NAV, bool HIST = false>
__device__ __forceinline__ void svb_sim_body(const SvmpcBatchArgs &a, const SvbEpisode &ep, const SvbRules &ru, const SkidNav *nav,
                                             const SvbHist *hs = nullptr) {
  constexpr int DS = SvbDims<MODEL>::DS;
  const int env = (int)blockIdx.x, B = (int)gridDim.x;
  if (a.active && a.active[env] == 0) return;
  if (ru.status[env] != 0) return;  // (written by the host before the launch; this launch stores it once, at its very end)
  SvbCarry<MODEL> cy;
  DevModel map;
  float w_obs;
  svb_begin<MODEL, NAV>(a, nav, cy, map, w_obs);
  float cf[SVB_COEF];
  svb_coef<MODEL>(a, ep.plant ? ep.plant + (size_t)env * a.P : nullptr, cf);
  const size_t per = (size_t)B * a.n_steps * a.M * a.P;  // parameter rows of one period
  SvmpcBatchArgs ap = a;                                // the period's own copy: do_forward = 0 while the episode warms up
  const int warm = ru.warm_up - ru.t0;                  // periods of this call that are still warm-up (<= 0: none)
  float loss = ru.loss[env];
  int status = 0, n = 0;
  for (int t = 0; t < ep.T; ++t) {
    const size_t row = (size_t)t * B + env;
    ap.do_forward = t < warm ? 0 : 1;
    float act[2] = {0.f, 0.f};  // (warm-up: no forward() writes it - the plant gets the zero action)
    svb_tick<MODEL, false, NAV, true>(ap, nullptr, a.params ? a.params + (size_t)t * per : nullptr, cy, map, w_obs,
                                      ep.pw_out ? ep.pw_out + row * a.N : nullptr, act);
    svb_plant_step<MODEL>(a, cf, cy.x0, act);
    const float cost = svb_state_cost<MODEL, NAV>(a, cy.x0, map, w_obs);
    loss += cost;
    if (ru.goal_on) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < DS; ++k) {
        const float d = ru.goal[k] - cy.x0[k];
        s = k == 0 ? d * d : s + d * d;
      }
      if (s <= ru.r2) status = 1;
    }
    if (ru.stop_on_crash && svb_crashed<MODEL, NAV>(a, cy.x0, map)) {  // (the crash rule wins)
      status = 2;
      loss = INFINITY;
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < DS; ++k) ep.states_out[row * DS + k] = cy.x0[k];
      ep.actions_out[row * a.da] = act[0];
      if (a.da == 2) ep.actions_out[row * 2 + 1] = act[1];
      ru.costs_out[row] = cost;
    }
    n = t + 1;
    svb_sync();  // the roll has read the particles' LDS rows, the next period's phase 0 overwrites them
    if constexpr (HIST) {  // (the rows every lane stored are visible; the next store to them lies behind phase 0's sync)
      const int ND = a.N * a.D;
      svb_hist_copy(hs->theta + row * ND, a.theta + (size_t)env * ND, ND);
    }
    if (status != 0) break;
  }
  svb_end(a, cy);
  if (threadIdx.x == 0) {
    ru.n_run[env] = n;
    ru.status[env] = status;
    ru.loss[env] = loss;
  }
}

// What a period of dust_svmpc_dual_batch_simulate adds to svb_dual_period_body's: the rules' words of the call, carried from launch to
// launch in device memory - written by lane 0 of one launch, read by LATER launches only
struct SvbDualSim {
  int stop_on_crash, goal_on;  // as SvbRules'
  float r2;
  float goal[8];
  float *costs_out;    // [B] this period's row of the cost records
  float *loss;         // [B] the fp32 running sum of the costs in period order
  int *status;         // [B] 0 running, 1 goal, 2 crash
  int *n_run;          // [B] the periods this call has run
  unsigned char *run;  // [B] the run mask every launch of the call takes (SvmpcBatchArgs::active names the same bytes)
};
struct SvmpcDualSimPeriodArgs {
  SvmpcBatchArgs k;  // do_forward: 0 while the episode warms up, set by the host per launch; active: the run mask
  SvbPrior pr;
  SvbDualPeriod dp;  // pw_out: nullptr in a warm-up period
  SvbDualSim ds;
};

// svb_dual_period_body's period under the rules of svb_sim_body: the PRIOR tick - without forward() while the episode warms up, the plant
// then gets the zero action -, the plant's step, the cost of the new state, crash and goal, the records, and the conditioning for the next
// period unless the environment has just stopped: (a_{n-1}, x_n) then stays pending, as behind a call's last period.  Whether it stops is
// computed by every lane from the carry in its registers and read-only data; lane 0 stores all of it, and clears the environment's byte
// of the run mask with its LAST store: the filter launches and period launches queued behind this one skip the environment.
// HIST (svmpc_dual_sim_hist_period_kernel): behind a sync of its own the particles also go to hs->theta[env], and the filter's particles
// the tick drew from - read-only in this launch - to hs->x[env]
template <int MODEL, bool HIST = false>
__device__ __forceinline__ void svb_dual_sim_period_body(const SvmpcBatchArgs &a, const SvbPrior &pri, const SvbDualPeriod &dp, const SvbDualSim &ru,
                                                         const SvbHist *hs = nullptr) {
  static_assert(MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_PARTICLE, "the other families' likelihood rows are made on the host");
  constexpr int DS = SvbDims<MODEL>::DS;
  const int env = (int)blockIdx.x;
  if (a.active[env] == 0) return;  // (the run mask: never NULL here; an earlier LAUNCH may have cleared the byte)
  SvbCarry<MODEL> cy;
  DevModel map;
  float w_obs;
  svb_begin<MODEL, false>(a, nullptr, cy, map, w_obs);
  float cf[SVB_COEF];
  svb_coef<MODEL>(a, dp.plant ? dp.plant + (size_t)env * a.P : nullptr, cf);
  float loss = ru.loss[env];
  float act[2] = {0.f, 0.f};  // (warm-up: no forward() writes it - the plant gets the zero action)
  svb_tick<MODEL, true, false, true>(a, &pri, nullptr, cy, map, w_obs, dp.pw_out ? dp.pw_out + (size_t)env * a.N : nullptr, act);
  if constexpr (HIST) {
    svb_sync();  // the roll's stores (the last iteration's, while the episode warms up) are visible to every lane
    const int ND = a.N * a.D, KP = pri.K * pri.P;
    if (hs->theta) svb_hist_copy(hs->theta + (size_t)env * ND, a.theta + (size_t)env * ND, ND);
    if (hs->x) svb_hist_copy(hs->x + (size_t)env * KP, pri.means + (size_t)env * KP, KP);
  }
  svb_plant_step<MODEL>(a, cf, cy.x0, act);
  const float cost = svb_state_cost<MODEL, false>(a, cy.x0, map, w_obs);
  loss += cost;
  int status = 0;
  if (ru.goal_on) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < DS; ++k) {
      const float d = ru.goal[k] - cy.x0[k];
      s = k == 0 ? d * d : s + d * d;
    }
    if (s <= ru.r2) status = 1;
  }
  if (ru.stop_on_crash && svb_crashed<MODEL, false>(a, cy.x0, map)) {  // (the crash rule wins)
    status = 2;
    loss = INFINITY;
  }
  svb_end(a, cy);
  if (threadIdx.x == 0) {
    float *xs = dp.state + (size_t)env * 8;
    MpfEnvIn *in = dp.in + env;
#pragma unroll
    for (int k = 0; k < DS; ++k) {
      dp.states_out[(size_t)env * DS + k] = cy.x0[k];
      xs[k] = cy.x0[k];
    }
    dp.actions_out[(size_t)env * a.da] = act[0];
    if (a.da == 2) dp.actions_out[(size_t)env * 2 + 1] = act[1];
    if (dp.bw_out) dp.bw_out[env] = dp.bw ? dp.bw[env] : 0.f;
    ru.costs_out[env] = cost;
    ru.loss[env] = loss;
    ru.n_run[env] += 1;
    if (dp.condition && status == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) in->past_obs[k] = in->obs[k];
#pragma unroll
      for (int k = 0; k < DS; ++k) in->obs[k] = cy.x0[k];
      in->past_action[0] = act[0];
      in->past_action[1] = act[1];
    }
    if (dp.t0_add) in->t0 += dp.t0_add;
    if (status != 0) {
      ru.status[env] = status;
      ru.run[env] = 0;  // the launch's last store for this environment
    }
  }
}

template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_dual_sim_period_kernel(const SvmpcDualSimPeriodArgs ka) {
  svb_dual_sim_period_body<MODEL>(ka.k, ka.pr, ka.dp, ka.ds);
}

template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_sim_kernel(const SvmpcSimArgs ka) {
  svb_sim_body<MODEL, false>(ka.k, ka.ep, ka.ru, nullptr);
}
__global__ __launch_bounds__(SVB_THREADS) void svmpc_skid_nav_sim_kernel(const SvmpcNavSimArgs ka) {
  svb_sim_body<DUST_MODEL_SKID_STEER, true>(ka.k, ka.ep, ka.ru, &ka.nav);
}
template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_rows_sim_kernel(const SvmpcRowsSimArgs ka) {
  const SvbHyper h = ka.rows[blockIdx.x];  // (the whole row, ahead of the copy)
  SvmpcBatchArgs a = ka.k;
  SVB_HYPER_APPLY(a, h);
  svb_sim_body<MODEL, false>(a, ka.ep, ka.ru, nullptr);
}

// The recording forms (dust_svmpc_batch_set_history): new kernels over new argument blocks, the bodies above with HIST set.  Plain cost,
// launch-uniform hyper-parameters: the navigation and the per-environment instances have no recording form (the host refuses)
struct SvmpcSimHistArgs {
  SvmpcBatchArgs k;
  SvbEpisode ep;
  SvbRules ru;
  SvbHist hs;  // theta: [T][B][N][D]
};
template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_sim_hist_kernel(const SvmpcSimHistArgs ka) {
  svb_sim_body<MODEL, false, true>(ka.k, ka.ep, ka.ru, nullptr, &ka.hs);
}
struct SvmpcDualSimHistPeriodArgs {
  SvmpcBatchArgs k;
  SvbPrior pr;
  SvbDualPeriod dp;
  SvbDualSim ds;
  SvbHist hs;  // this period's rows: theta [B][N][D], x [B][Mp][P]; either may be nullptr
};
template <int MODEL>
__global__ __launch_bounds__(SVB_THREADS) void svmpc_dual_sim_hist_period_kernel(const SvmpcDualSimHistPeriodArgs ka) {
  svb_dual_sim_period_body<MODEL, true>(ka.k, ka.pr, ka.dp, ka.ds, &ka.hs);
}

}  // namespace dust
