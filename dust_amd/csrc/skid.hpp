// skid.hpp - rollouts of the skid-steer robot family: SkidSteerRobot.step (dust/models/skid_steer_robot.py:73-122) under
// MultiDISCO._rollout / _compute_cost (disco.py:139-209, 294-346) with a QUADRATIC cost family.  The reference ships no cost for this
// model (its MultiDISCO takes any callable); the family here is what `dust_amd.costs.QuadraticCost` evaluates on the host, so that
// the same object can be handed to the reference's controller:
//     inst(x, a) = sum_k w_state[k] (x_k - goal_k)^2 + sum_d w_ctrl[d] a_d^2          (state BEFORE the action, raw action)
//     term(x)    = sum_k w_term[k]  (x_k - goal_k)^2
// One lane = one (action sample s, policy n) pair, the M dynamics samples in sequence; costs go to a [S][N] buffer that the regular
// rollout kernel consumes in its injected-costs mode (weights, likelihood score, a_mat update) - the scheme of rollout_states.hpp.
// This family is a completeness row, not a tuned one: plain loads, no LDS staging.
//
// Arithmetic follows the reference's fp32 tensor expressions operation by operation (Python floats enter as fp32 scalars):
//   linear  = ((r + l) * pi) * wheel_radius            angular = ((((r - l) * 2) * pi) * wheel_radius) / axial_distance
//   forward = linear * dt                               lateral = ((-angular) * x_icr) * dt
//   x' = (x + forward cos th) - lateral sin th          y' = (y + forward sin th) + lateral cos th          th' = th + angular * dt
//   state' = (x', y', th', linear, angular)
#pragma once
#include "rollout.hpp"

namespace dust {

struct SkidModel {
  DevParam x_icr, wheel_radius, axial_distance;
  float lo[2], hi[2];  // action_space bounds (wheel speeds)
  float goal[5], w_state[5], w_term[5], w_ctrl[2];
};

struct SkidArgs {
  SkidModel sk;
  int N_total, n0, n_local, S, M, H, D, P;
  int noise_mode;       // NOISE_EPS / NOISE_ACTIONS / NOISE_PHILOX (rollout.hpp)
  int log_space, interleave;
  float dt;
  float chol_a[2];
  float chol_off;       // full a_cov: L[1][0] (0: diagonal)
  uint64_t seed;
  const uint32_t *ctr;  // {tick, iter, ..}: Philox stream position, as the regular kernel reads it
  const float *noise;   // [S][N][D] eps or actions
  const float *theta;   // [N][D]
  const float *state;   // [5]
  const float *params;  // [M][P] raw samples or nullptr
  float *costs_sn;      // [S][N]
  float *costsT;        // [N][S] the context's cost record (the regular kernel rewrites it in its injected-costs mode only when it adds the a_reg term)
  float *states_out;    // [M][S][N][H+1][5] or nullptr
  float *actions_out;   // [S][N][D] or nullptr
  const float *mw;      // [M] unscented-transform weights (params: the M sigma points) or nullptr: plain mean over m (last: the other offsets stay)
};

// The navigation cost family (dust_amd.costs.NavigationCost): the quadratic family plus the obstacle term of Particle.default_inst_cost /
// default_term_cost (particle.py:170-225) on the position plane (x_0, x_1),
//     inst(x, a) = (quad + ctrl) + w_obs occ(x_0, x_1)          term(x) = quad + w_obs occ(x_0, x_1)
// with occ = ObstacleMap.get_collisions (obstacle_map.py:64-93; common.hpp collision()).  It travels BESIDE SkidArgs / AmppiArgs, in a
// struct of its own, so that the kernels without the term keep their argument layout - and their instructions.
struct SkidNav {
  float inv_cell, off_x, off_y, w_obs;
  int nx, ny;
  int grid_words;             // words of the bit-packed map the workgroup stages into dynamic LDS, or 0: the lookups read device memory
  const uint32_t *grid_bits;  // bit-packed [nx][ny] occupancy, as DevModel's
};

struct SkidNavArgs {
  SkidArgs r;
  SkidNav nav;
};

// The map for collision(): staged into `lds` by the whole workgroup (every lane calls this, then the barrier) or left in device memory
__device__ __forceinline__ DevModel skid_nav_map(const SkidNav &nv, uint32_t *lds) {
  DevModel dm;
  dm.inv_cell = nv.inv_cell;
  dm.off_x = nv.off_x;
  dm.off_y = nv.off_y;
  dm.nx = nv.nx;
  dm.ny = nv.ny;
  dm.grid_bits = nv.grid_bits;
  if (nv.grid_words > 0) {
    const int words = (nv.nx * nv.ny + 31) >> 5;  // (grid_words is this rounded up to 4: the allocation ends at `words`)
    for (int w = (int)threadIdx.x; w < words; w += (int)blockDim.x) lds[w] = nv.grid_bits[w];
    dm.grid_bits = lds;
    __syncthreads();
  }
  return dm;
}

__device__ __forceinline__ float skid_param(const DevParam &p, const float *prow, int log_space) {
  if (p.kind == DUST_PARAM_SAMPLED && prow) {
    const float v = prow[p.col];
    return log_space ? expf(v) : v;
  }
  return (float)p.value;
}

// One SkidSteerRobot.step (skid_steer_robot.py:93-122) in place, operation by operation as the header states it; r, l: the wheel speeds
// AFTER the clamp to the action bounds.  The rollout kernel below and the filter's one-step prediction (mpf.hpp) share it.
// skid_step_cs takes the heading's cosine and sine from its caller: the filter steps every particle from ONE past state, so it evaluates
// them once per call (mpf_skid_heading_kernel) instead of carrying fast_cosf / fast_sinf - with their huge-argument fall-back - in its
// optimisation kernels.
__device__ __forceinline__ void skid_step_cs(float x[5], const float r, const float l, const float xicr, const float wr, const float ad, const float dt,
                                             const float cs, const float sn) {
  const float lin = ((r + l) * PI_F) * wr;
  const float ang = ((((r - l) * 2.0f) * PI_F) * wr) / ad;
  const float fwd = lin * dt, lat = ((-ang) * xicr) * dt;
  const float nx = (x[0] + fwd * cs) - lat * sn;
  const float ny = (x[1] + fwd * sn) + lat * cs;
  x[2] = x[2] + ang * dt;
  x[0] = nx;
  x[1] = ny;
  x[3] = lin;
  x[4] = ang;
}
__device__ __forceinline__ void skid_step(float x[5], const float r, const float l, const float xicr, const float wr, const float ad, const float dt) {
  skid_step_cs(x, r, l, xicr, wr, ad, dt, fast_cosf(x[2]), fast_sinf(x[2]));
}

// UT: the sigma-point form (MultiDISCO._sigma_rollout, disco.py:211-292; the weighted costs of _compute_cost, disco.py:312-323): row m of
// `params` is sigma point m and the lane's cost is the weighted SUM
//     sum_m sum_t mw[(m H + t) mod M] inst(x_{m,t}) + sum_m mw[m] term(x_{m,H})
// - the reference views its flat [rollout][step] block of instantaneous costs as rows of M consecutive entries, and rollout
// (s N + n) M + m runs sigma point m, so entry (m, t) meets weight (m H + t) mod M (rollout.hpp has the Pendulum's form of the rule).
// Weighted terms accumulate in double (CostAcc::add_weighted); the two parts are rounded and added in fp32 as the regular kernel does.
// A template parameter, not a run-time branch: the plain instance is the kernel it was before the sigma-point form existed.
// NAV: the navigation family above; `nav` / `lds` are read by that instance alone.
template <bool UT, bool NAV>
__device__ __forceinline__ void skid_rollout_body(const SkidArgs &a, const SkidNav *nav, uint32_t *lds) {
  DevModel dm;
  if constexpr (NAV) dm = skid_nav_map(*nav, lds);  // (ahead of the bounds check: the lanes past the end stage their share)
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.n_local * a.S) return;
  const int s = idx / a.n_local, n = a.n0 + (idx - s * a.n_local);  // (n fastest: the rows of one sample are adjacent)
  const int D = a.D, H = a.H, N = a.N_total;
  const float *nz = a.noise ? a.noise + ((size_t)s * N + n) * D : nullptr;
  const float *th = a.theta + (size_t)n * D;
  const uint32_t ctr_tick = a.ctr[0], ctr_iter = a.ctr[1];
  auto action = [&](const int j) -> float {  // theta + L eps (an odd column of a full L takes its partner draw too)
    if (a.noise_mode == NOISE_ACTIONS) return nz[j];
    if (a.noise_mode == NOISE_EPS) return (j & 1) && a.chol_off != 0.f ? th[j] + (a.chol_off * nz[j - 1] + a.chol_a[1] * nz[j]) : th[j] + a.chol_a[j & 1] * nz[j];
    float z[8];
    philox_normal8(a.seed, (uint32_t)(j >> 3), (uint32_t)(s * N + n), ctr_iter, ctr_tick, z);  // (the regular kernel's stream)
    return (j & 1) && a.chol_off != 0.f ? th[j] + (a.chol_off * z[(j & 7) - 1] + a.chol_a[1] * z[j & 7]) : th[j] + a.chol_a[j & 1] * z[j & 7];
  };
  if (a.actions_out)
    for (int j = 0; j < D; ++j) a.actions_out[((size_t)s * N + n) * D + j] = action(j);
  float x0[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) x0[k] = a.state[k];
  double acc = 0.0, ut_term = 0.0;
  for (int m = 0; m < a.M; ++m) {
    // scalar-event params_dist quirk (disco.py:177-179): rollout r = (m, s, n) flattened uses params[r % M]
    const int mi = a.interleave ? (int)((((long)m * a.S + s) * N + n) % a.M) : m;
    const float *prow = a.params ? a.params + (size_t)mi * a.P : nullptr;
    const float xicr = skid_param(a.sk.x_icr, prow, a.log_space), wr = skid_param(a.sk.wheel_radius, prow, a.log_space),
                ad = skid_param(a.sk.axial_distance, prow, a.log_space);
    float x[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) x[k] = x0[k];
    float *so = a.states_out ? a.states_out + ((((size_t)m * a.S + s) * N + n) * (size_t)(H + 1)) * 5 : nullptr;
    if (so)
#pragma unroll
      for (int k = 0; k < 5; ++k) so[k] = x[k];
    double tot = 0.0;
    for (int t = 0; t < H; ++t) {
      const float a0 = action(2 * t), a1 = action(2 * t + 1);
      double sc = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float d = x[k] - a.sk.goal[k];
        sc += (double)((d * d) * a.sk.w_state[k]);
      }
      const double cc = (double)((a0 * a0) * a.sk.w_ctrl[0]) + (double)((a1 * a1) * a.sk.w_ctrl[1]);
      if constexpr (NAV) {  // (quad + ctrl) + obst, the reference callable's order
        const float ic = ((float)sc + (float)cc) + nav->w_obs * collision(dm, x[0], x[1]);
        if (UT) tot += (double)a.mw[((long)m * H + t) % a.M] * (double)ic;
        else tot += (double)ic;
      } else {
        if (UT) tot += (double)a.mw[((long)m * H + t) % a.M] * (double)((float)sc + (float)cc);
        else tot += (double)((float)sc + (float)cc);
      }
      skid_step(x, clampf(a0, a.sk.lo[0], a.sk.hi[0]), clampf(a1, a.sk.lo[1], a.sk.hi[1]), xicr, wr, ad, a.dt);
      if (so)
#pragma unroll
        for (int k = 0; k < 5; ++k) so[(size_t)(t + 1) * 5 + k] = x[k];
    }
    double tc = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float d = x[k] - a.sk.goal[k];
      tc += (double)((d * d) * a.sk.w_term[k]);
    }
    if constexpr (NAV) {
      const float tcn = (float)tc + nav->w_obs * collision(dm, x[0], x[1]);
      if (UT) {
        ut_term += (double)a.mw[m] * (double)tcn;
        acc += tot;
      } else {
        acc += (double)((float)tot + tcn);
      }
    } else if (UT) {  // weighted instantaneous and terminal parts are summed separately over the sigma points (disco.py:314-321)
      ut_term += (double)a.mw[m] * (double)(float)tc;
      acc += tot;
    } else {
      acc += (double)((float)tot + (float)tc);
    }
  }
  const float cost = UT ? (float)acc + (float)ut_term : (a.M == 1 ? (float)acc : (float)(acc / a.M));
  a.costs_sn[(size_t)s * N + n] = cost;
  a.costsT[(size_t)n * a.S + s] = cost;
}

__global__ __launch_bounds__(256) void skid_rollout_kernel(const SkidArgs a) { skid_rollout_body<false, false>(a, nullptr, nullptr); }
__global__ __launch_bounds__(256) void skid_ut_rollout_kernel(const SkidArgs a) { skid_rollout_body<true, false>(a, nullptr, nullptr); }
// The navigation instances: dynamic LDS of 4 nav.grid_words bytes (0: the map stays in device memory)
__global__ __launch_bounds__(256) void skid_nav_rollout_kernel(const SkidNavArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t skid_nav_lds[];
  skid_rollout_body<false, true>(a.r, &a.nav, skid_nav_lds);
}
__global__ __launch_bounds__(256) void skid_ut_nav_rollout_kernel(const SkidNavArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t skid_nav_lds[];
  skid_rollout_body<true, true>(a.r, &a.nav, skid_nav_lds);
}

}  // namespace dust
