// amppi_episode.hpp - closed-loop episodes on the device for the batched AMPPI tick (dust_amppi_batch_episode): ONE control period of B
// independent environments per launch, T launches chained on the batch's stream with no host wait, event or copy between them.
// Not one persistent launch: the tick's phase 2 runs in whichever workgroup of an environment arrives LAST (amppi.hpp), so periods would
// have to meet across workgroups, and nothing in this project spins on another workgroup.
//
// amppi_period_kernel<MODEL> / amppi_skid_nav_period_kernel: the grid, the arguments and the statements of amppi_batch_kernel /
// amppi_skid_nav_batch_kernel - phases 1 and 2 are amppi_body.inc, included as text, untouched - and then, in the reducer workgroup of
// environment b alone (every other workgroup has returned inside the body text), amppi_period_tail:
//   1  the action: a_seq[0 .. da) of the sequence the reducer has just written (updated and clamped, BEFORE the roll).  Lane j < D reads
//      back its OWN store a_seq[j] and puts it into LDS; behind a wg_sync() lane 0 takes the action - and, further down, every lane its
//      rolled value - from there: no lane re-reads device memory that another lane of the workgroup stored a moment ago;
//   2  the plant: x <- step(x, a) through the family's own device step, the action clamped as the rollouts clamp it, under the
//      coefficients svb_coef makes of the environment's TRUE parameter row plant[b][:] (the columns of the tick's parameter rows; NULL:
//      the prototype's nominal model) - svb_coef / svb_plant_step of the SVMPC episode (svmpc_episode.hpp), the same functions.  Plants
//      are deterministic;
//   3  the records states_out[b][:] (the state after the step), actions_out[b][:] (the raw a_seq[0]), and optionally costs_out[b][S],
//      omega_out[b][S] and a_seq_out[b][D] (the sequence before the roll);
//   4  x_{t+1} into row b of the device state array [B][8] the tick reads its states from: the NEXT launch reads it there;
//   5  the roll of amppi_batch_roll_kernel: a_seq shifted left by `shift` values, zeros behind - the lane's new value comes from LDS;
//   6  the ticket: lane 0 stores 0 into the environment's arrival word with an agent-scope atomic store.  The reducer drew the last
//      ticket of its environment, so every other workgroup's add is behind it and nobody touches the word again in this launch: ONE
//      memset ahead of the first period is all an episode needs (an inactive environment's word is never touched).
// The Philox position moves as in the tick (the reducer advances `iter`), the roll does not touch it: period t draws what the t-th
// successive dust_amppi_batch_update would draw.
// dust_amppi_dual_batch_episode (mpf.hpp) chains the same kernels behind each period's filter update - amppi_prior_period_kernel where
// the lanes draw their rows from the filters' priors - and has lane 0 condition the environment's MpfEnvIn row for the next update.
//
// amppi_sim_period_kernel<MODEL> / amppi_skid_nav_sim_period_kernel / amppi_prior_sim_period_kernel (dust_amppi_batch_simulate,
// dust_amppi_dual_batch_simulate): the same periods under the reference's episode rules - the cost of every new state summed into a loss,
// a crash that costs inf, a stop inside the goal radius -, further down; the kernels above keep their text.
#pragma once
#include "amppi.hpp"
#include "svmpc_episode.hpp"

namespace dust {

// What a period adds to the batched tick's arguments
struct AmppiPeriod {
  const float *plant;  // [B][P] true parameter rows or nullptr (nominal plants)
  float *state;        // [B][8]: the rows AmppiBatchArgs::states names; x_{t+1} for the next period's launch
  float *states_out;   // [B][ds], this period's rows of the records
  float *actions_out;  // [B][da]
  float *costs_out;    // [B][S] or nullptr
  float *omega_out;    // [B][S] or nullptr
  float *a_seq_out;    // [B][D] or nullptr: the sequence before the roll
  int shift;           // roll_steps * da, at most D
  // dust_amppi_dual_batch_episode (all NULL / 0 otherwise): the filters' side of a period, as SvbDualPeriod (svmpc_episode.hpp) has it
  MpfEnvIn *in;        // [B]: what the NEXT period's filter update reads, or nullptr
  const float *bw;     // [B] the bandwidths Silverman's rule gave this period's update, or nullptr (no update, or a fixed bandwidth)
  float *bw_out;       // [B] or nullptr: ... recorded (0 where no update ran)
  int t0_add;          // the optimiser steps this period's filter update took (0: no update ran)
  int condition;       // 0 in the call's last period: (a_{T-1}, x_T) stays pending
};
struct AmppiPeriodArgs {
  AmppiBatchArgs k;
  AmppiPeriod ep;
};
struct AmppiPriorPeriodArgs {
  AmppiBatchArgs k;
  AmppiPriorBatch pr;  // seeds: this period's row of prior_seeds
  AmppiPeriod ep;
};
struct AmppiNavPeriodArgs {
  AmppiBatchArgs k;
  SkidNav nav;
  AmppiPeriod ep;
};

// The reducer workgroup of environment `env` behind phase 2; lds: the body text's one LDS object, whose column partials [16, 16 + 256)
// every lane has read once the first barrier here is passed - the updated sequence (D <= 128 floats) takes their place
template <int MODEL>
__device__ __forceinline__ void amppi_period_tail(const AmppiEnvArgs &a, const AmppiPeriod &ep, const int env, double *lds) {
  constexpr int DS = AmppiDims<MODEL>::DS;
  const int tid = (int)threadIdx.x, D = a.D, S = a.S, da = a.da;
  float *sq = reinterpret_cast<float *>(lds + 16);
  wg_sync();
  if (tid < D) sq[tid] = a.a_seq[tid];  // (the lane's own store)
  wg_sync();
  // (the copies of costs and omega stand AHEAD of the plant's step, on which they do not depend: behind it the skid-steer instances
  // came out with a 36-byte private segment that no instruction touched - a stack slot of the scalar registers' spills)
  if (ep.costs_out)
    for (int i = tid; i < S; i += AMPPI_THREADS) ep.costs_out[(size_t)env * S + i] = a.costs[i];
  if (ep.omega_out)
    for (int i = tid; i < S; i += AMPPI_THREADS) ep.omega_out[(size_t)env * S + i] = a.omega[i];
  if (tid == 0) {  // one plant per environment: lane 0 steps it and writes its rows
    const float act[2] = {sq[0], da == 2 ? sq[1] : 0.f};
    float cf[SVB_COEF];
    svb_coef<MODEL>(a, ep.plant ? ep.plant + (size_t)env * a.P : nullptr, cf);
    float x[DS];
#pragma unroll
    for (int k = 0; k < DS; ++k) x[k] = a.state[k];
    svb_plant_step<MODEL>(a, cf, x, act);
    float *xs = ep.state + (size_t)env * 8;
#pragma unroll
    for (int k = 0; k < DS; ++k) {
      ep.states_out[(size_t)env * DS + k] = x[k];
      xs[k] = x[k];
    }
    ep.actions_out[(size_t)env * da] = act[0];
    if (da == 2) ep.actions_out[(size_t)env * 2 + 1] = act[1];
    if (ep.bw_out) ep.bw_out[env] = ep.bw ? ep.bw[env] : 0.f;
    if (ep.in) {
      // GaussianLikelihood.condition for the next period's update, the arithmetic of svb_dual_period_body (svmpc_episode.hpp) on the
      // environment's device row: past_obs <- obs, obs <- x_{t+1}, past_action <- a_t (zero-padded), t0 advanced by the steps just taken
      MpfEnvIn *in = ep.in + env;
      if (ep.condition) {
#pragma unroll
        for (int k = 0; k < 4; ++k) in->past_obs[k] = in->obs[k];
#pragma unroll
        for (int k = 0; k < (DS < 4 ? DS : 4); ++k) in->obs[k] = x[k];
        in->past_action[0] = act[0];
        in->past_action[1] = act[1];
      }
      if (ep.t0_add) in->t0 += ep.t0_add;
    }
  }
  if (tid < D) {
    if (ep.a_seq_out) ep.a_seq_out[(size_t)env * D + tid] = sq[tid];
    a.a_seq[tid] = tid + ep.shift < D ? sq[tid + ep.shift] : 0.f;
  }
  if (tid == 0) __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int MODEL>
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_period_kernel(const AmppiPeriodArgs kp) {
  const int env = (int)blockIdx.y;
  if (kp.k.active && kp.k.active[env] == 0) return;
  const AmppiEnvArgs a = amppi_env_view(kp.k, env);
  double *tail_lds;
  {
    constexpr bool NAV = false, PRIOR = false;
    const SkidNav *const nav = nullptr;
    const AmppiPrior *const pri = nullptr;
    uint32_t *const grid_lds = nullptr;
#include "amppi_body.inc"
    tail_lds = lds;
  }
  amppi_period_tail<MODEL>(a, kp.ep, env, tail_lds);
}
// The period of the dual episode in the "extended" mode: lane s draws row s of its environment's filter prior itself, as
// amppi_prior_batch_kernel does.  Pendulum and Particle alone: a skid-steer or cart-pole pair is refused (their likelihood rows are made
// on the host), so a navigation + PRIOR period kernel would have no caller and is not built.
template <int MODEL>
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_prior_period_kernel(const AmppiPriorPeriodArgs kp) {
  static_assert(MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_PARTICLE, "the other families' likelihood rows are made on the host");
  const int env = (int)blockIdx.y;
  if (kp.k.active && kp.k.active[env] == 0) return;
  const AmppiEnvArgs a = amppi_env_view(kp.k, env);
  const AmppiPrior pe = amppi_env_prior(kp.pr, env, a.S);
  double *tail_lds;
  {
    constexpr bool NAV = false, PRIOR = true;
    const SkidNav *const nav = nullptr;
    const AmppiPrior *const pri = &pe;
    uint32_t *const grid_lds = nullptr;
#include "amppi_body.inc"
    tail_lds = lds;
  }
  amppi_period_tail<MODEL>(a, kp.ep, env, tail_lds);
}
// ... with the navigation cost family (the map is the cost's alone: the plant's step does not read it)
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_skid_nav_period_kernel(const AmppiNavPeriodArgs kn) {
  constexpr int MODEL = DUST_MODEL_SKID_STEER;
  extern __shared__ __attribute__((aligned(16))) uint32_t grid_lds[];
  const int env = (int)blockIdx.y;
  if (kn.k.active && kn.k.active[env] == 0) return;
  const AmppiEnvArgs a = amppi_env_view(kn.k, env);
  double *tail_lds;
  {
    constexpr bool NAV = true, PRIOR = false;
    const SkidNav *const nav = &kn.nav;
    const AmppiPrior *const pri = nullptr;
#include "amppi_body.inc"
    tail_lds = lds;
  }
  amppi_period_tail<MODEL>(a, kn.ep, env, tail_lds);
}

// ---- The periods under the reference's episode rules (dust_amppi_batch_simulate, dust_amppi_dual_batch_simulate): the non-SVMPC branch
// of run_particle_episode / run_pendulum_simulation (simulations.py:217-260, 124-160; particle_example.py:191-242).  New kernels beside
// the ones above, which keep their text: the same body, then amppi_sim_period_tail in the reducer workgroup.
// The rules' words of the call, carried from launch to launch in device memory - written by lane 0 of one launch, read by LATER launches
// only: SvbDualSim of the dual SVMPC period (svmpc_episode.hpp), the one definition rules_fill fills; `run` is the run mask every launch
// of the call takes (AmppiBatchArgs::active names the same bytes: never NULL), costs_out this period's row of the instantaneous costs
using AmppiSim = SvbDualSim;
struct AmppiSimPeriodArgs {
  AmppiBatchArgs k;
  AmppiPeriod ep;  // a_seq_out: set in EVERY period - an environment's row ends as its last period's
  AmppiSim ru;
};
struct AmppiPriorSimPeriodArgs {
  AmppiBatchArgs k;
  AmppiPriorBatch pr;
  AmppiPeriod ep;
  AmppiSim ru;
};
struct AmppiNavSimPeriodArgs {
  AmppiBatchArgs k;
  SkidNav nav;
  AmppiPeriod ep;
  AmppiSim ru;
};

// amppi_period_tail under the rules, steps 1 - 6 as there.  Lane 0 also has: the family's instantaneous cost of the new state
// (svb_state_cost, the arithmetic of the SVMPC episodes) into costs_out[env] and, in fp32, into loss[env]; the crash and goal predicates of
// svb_sim_body; n_run[env] += 1.  A stopping environment does not condition its MpfEnvIn row - (a_{n-1}, x_n) stays pending - but still
// rolls and resets its arrival word; lane 0 then stores the status and, as its LAST store, clears the environment's byte of the run mask.
// That is safe within the launch: every other workgroup of the environment read the byte before it drew its ticket, and this workgroup
// drew the last one; only LATER launches depend on the byte.  map / w_obs: the navigation instance's (NAV), unread otherwise
template <int MODEL, bool NAV>
__device__ __forceinline__ void amppi_sim_period_tail(const AmppiEnvArgs &a, const AmppiPeriod &ep, const AmppiSim &ru, const int env, double *lds,
                                                      const DevModel &map, const float w_obs) {
  constexpr int DS = AmppiDims<MODEL>::DS;
  const int tid = (int)threadIdx.x, D = a.D, S = a.S, da = a.da;
  float *sq = reinterpret_cast<float *>(lds + 16);
  wg_sync();
  if (tid < D) sq[tid] = a.a_seq[tid];  // (the lane's own store)
  wg_sync();
  if (ep.costs_out)
    for (int i = tid; i < S; i += AMPPI_THREADS) ep.costs_out[(size_t)env * S + i] = a.costs[i];
  if (ep.omega_out)
    for (int i = tid; i < S; i += AMPPI_THREADS) ep.omega_out[(size_t)env * S + i] = a.omega[i];
  int status = 0;  // (lane 0's alone)
  if (tid == 0) {
    const float act[2] = {sq[0], da == 2 ? sq[1] : 0.f};
    float cf[SVB_COEF];
    svb_coef<MODEL>(a, ep.plant ? ep.plant + (size_t)env * a.P : nullptr, cf);
    float x[DS];
#pragma unroll
    for (int k = 0; k < DS; ++k) x[k] = a.state[k];
    svb_plant_step<MODEL>(a, cf, x, act);
    const float cost = svb_state_cost<MODEL, NAV>(a, x, map, w_obs);
    float loss = ru.loss[env] + cost;
    if (ru.goal_on) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < DS; ++k) {
        const float d = ru.goal[k] - x[k];
        s = k == 0 ? d * d : s + d * d;
      }
      if (s <= ru.r2) status = 1;
    }
    if (ru.stop_on_crash && svb_crashed<MODEL, NAV>(a, x, map)) {  // (the crash rule wins)
      status = 2;
      loss = INFINITY;
    }
    float *xs = ep.state + (size_t)env * 8;
#pragma unroll
    for (int k = 0; k < DS; ++k) {
      ep.states_out[(size_t)env * DS + k] = x[k];
      xs[k] = x[k];
    }
    ep.actions_out[(size_t)env * da] = act[0];
    if (da == 2) ep.actions_out[(size_t)env * 2 + 1] = act[1];
    if (ep.bw_out) ep.bw_out[env] = ep.bw ? ep.bw[env] : 0.f;
    ru.costs_out[env] = cost;
    ru.loss[env] = loss;
    ru.n_run[env] += 1;
    if (ep.in) {
      MpfEnvIn *in = ep.in + env;
      if (ep.condition && status == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) in->past_obs[k] = in->obs[k];
#pragma unroll
        for (int k = 0; k < (DS < 4 ? DS : 4); ++k) in->obs[k] = x[k];
        in->past_action[0] = act[0];
        in->past_action[1] = act[1];
      }
      if (ep.t0_add) in->t0 += ep.t0_add;
    }
  }
  if (tid < D) {
    if (ep.a_seq_out) ep.a_seq_out[(size_t)env * D + tid] = sq[tid];
    a.a_seq[tid] = tid + ep.shift < D ? sq[tid + ep.shift] : 0.f;
  }
  if (tid == 0) {
    __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (status != 0) {
      ru.status[env] = status;
      ru.run[env] = 0;  // the launch's last store for this environment
    }
  }
}

template <int MODEL>
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_sim_period_kernel(const AmppiSimPeriodArgs kp) {
  const int env = (int)blockIdx.y;
  if (kp.k.active[env] == 0) return;  // (the run mask: never NULL here; an earlier LAUNCH may have cleared the byte)
  const AmppiEnvArgs a = amppi_env_view(kp.k, env);
  double *tail_lds;
  {
    constexpr bool NAV = false, PRIOR = false;
    const SkidNav *const nav = nullptr;
    const AmppiPrior *const pri = nullptr;
    uint32_t *const grid_lds = nullptr;
#include "amppi_body.inc"
    tail_lds = lds;
  }
  amppi_sim_period_tail<MODEL, false>(a, kp.ep, kp.ru, env, tail_lds, a.dm, 0.f);
}
template <int MODEL>
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_prior_sim_period_kernel(const AmppiPriorSimPeriodArgs kp) {
  static_assert(MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_PARTICLE, "the other families' likelihood rows are made on the host");
  const int env = (int)blockIdx.y;
  if (kp.k.active[env] == 0) return;
  const AmppiEnvArgs a = amppi_env_view(kp.k, env);
  const AmppiPrior pe = amppi_env_prior(kp.pr, env, a.S);
  double *tail_lds;
  {
    constexpr bool NAV = false, PRIOR = true;
    const SkidNav *const nav = nullptr;
    const AmppiPrior *const pri = &pe;
    uint32_t *const grid_lds = nullptr;
#include "amppi_body.inc"
    tail_lds = lds;
  }
  amppi_sim_period_tail<MODEL, false>(a, kp.ep, kp.ru, env, tail_lds, a.dm, 0.f);
}
// ... with the navigation cost family: the cost's map term and the crash rule read the map the body text staged into LDS
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_skid_nav_sim_period_kernel(const AmppiNavSimPeriodArgs kn) {
  constexpr int MODEL = DUST_MODEL_SKID_STEER;
  extern __shared__ __attribute__((aligned(16))) uint32_t grid_lds[];
  const int env = (int)blockIdx.y;
  if (kn.k.active[env] == 0) return;
  const AmppiEnvArgs a = amppi_env_view(kn.k, env);
  {
    constexpr bool NAV = true, PRIOR = false;
    const SkidNav *const nav = &kn.nav;
    const AmppiPrior *const pri = nullptr;
#include "amppi_body.inc"
    // (inside the body text's scope, on ITS map: a second DevModel made of kn.nav behind the scope left a 36-byte private segment)
    amppi_sim_period_tail<MODEL, true>(a, kn.ep, kn.ru, env, lds, *map, kn.nav.w_obs);
  }
}

}  // namespace dust
