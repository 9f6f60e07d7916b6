// cartpole.hpp - rollouts of the cart-pole family: CartPoleModel.step (dust/models/cartpole.py:126-172) under MultiDISCO._rollout /
// _compute_cost (disco.py:139-209, 294-346) with the QUADRATIC cost family of skid.hpp (dust_amd.costs.QuadraticCost: 4 state entries,
// 1 control weight; the instantaneous cost sees the state BEFORE the action and the raw action, the terminal cost the state at H).
// One lane = one (action sample s, policy n) pair, the M dynamics samples in sequence; costs go to a [S][N] buffer that the regular
// rollout kernel consumes in its injected-costs mode - the scheme of skid.hpp.  A completeness row, not a tuned one: plain loads.
//
// The reference's step reads `self.__params_dict`, which Python mangles to an attribute the base class never set (cartpole.py:151/156);
// with that one attribute supplied on the instance the model runs, and this file follows its fp32 tensor expressions operation by
// operation (state x, x_d, th, th_d; one action; Python floats enter as fp32 scalars, a product of two Python floats is formed in double):
//   u     = clamp(a, -1, +1) * f_mag                      (the +-1 is in the step, not the action space)          cartpole.py:159
//   mass  = m_c + m_c                                     (sic: the pole mass does not enter the "total mass")    cartpole.py:161
//   pm    = m_p * length                                                                                         cartpole.py:162
//   cf    = mu_c * sign(x_d)                              (sign(0) = 0)                                           cartpole.py:163
//   pf    = (mu_p * th_d) / pm                                                                                   cartpole.py:164
//   fac   = ((u + (pm * sin th) * th_d^2) - cf) / mass                                                           cartpole.py:165
//   num   = (g * sin th - cos th * fac) - pf                                                                     cartpole.py:166
//   den   = length * (4/3 - (m_p * cos^2 th) / mass)                                                             cartpole.py:167
//   th_dd = num / den                                     x_dd = fac - ((pm * th_dd) * cos th) / mass            cartpole.py:168-170
//   state' = state + (x_d, x_dd, th_d, th_dd) * dt                                                               cartpole.py:171-172
// sin th and cos th are evaluated once per step: the reference evaluates them two and three times on the same argument.
#pragma once
#include "skid.hpp"

namespace dust {

// order of params_dict (cartpole.py:79-87): g, mass_cart, mass_pole, length, mu_c, mu_p, f_mag
enum { CP_G = 0, CP_MC = 1, CP_MP = 2, CP_LEN = 3, CP_MUC = 4, CP_MUP = 5, CP_FMAG = 6, CP_NPAR = 7 };

struct CartModel {
  DevParam par[CP_NPAR];
  float goal[4], w_state[4], w_term[4], w_ctrl[1];
};

// what one rollout (one dynamics sample) keeps constant over its time loop
struct CartCoef {
  float g, mp, len, muc, mup, fmag;
  float mass, pm, k43, dt;
};

struct CartArgs {
  CartModel cp;
  int N_total, n0, n_local, S, M, H, D, P;
  int noise_mode;       // NOISE_EPS / NOISE_ACTIONS / NOISE_PHILOX (rollout.hpp)
  int log_space, interleave;
  float dt;
  float chol_a;         // cholesky of the 1 x 1 a_cov
  uint64_t seed;
  const uint32_t *ctr;  // {tick, iter, ..}: Philox stream position, as the regular kernel reads it
  const float *noise;   // [S][N][D] eps or actions
  const float *theta;   // [N][D]
  const float *state;   // [4]
  const float *params;  // [M][P] raw samples or nullptr
  float *costs_sn;      // [S][N]
  float *costsT;        // [N][S] the context's cost record (the regular kernel rewrites it in its injected-costs mode only when it adds the a_reg term)
  float *states_out;    // [M][S][N][H+1][4] or nullptr
  const float *mw;      // [M] unscented-transform weights (params: the M sigma points) or nullptr: plain mean over m (last: the other offsets stay)
};

// mass, pm, 4/3 from the seven fp32 parameter values; pm_py: both factors of pm are Python floats, so is their product (double)
__device__ __forceinline__ CartCoef cartpole_coef(const float v[CP_NPAR], const bool pm_py, const double pm_d, const float dt) {
  CartCoef k;
  k.g = v[CP_G];
  k.mp = v[CP_MP];
  k.len = v[CP_LEN];
  k.muc = v[CP_MUC];
  k.mup = v[CP_MUP];
  k.fmag = v[CP_FMAG];
  k.mass = v[CP_MC] + v[CP_MC];
  k.pm = pm_py ? (float)pm_d : v[CP_MP] * v[CP_LEN];
  k.k43 = (float)(4.0 / 3);
  k.dt = dt;
  return k;
}

// One CartPoleModel.step in place, operation by operation as the header states it; ac: the action AFTER the clamp to +-1, sn / cs: sine
// and cosine of x[2].  The rollout kernel below and the filter's one-step prediction (mpf.hpp) share it.
__device__ __forceinline__ void cartpole_step(float x[4], const float ac, const CartCoef &k, const float sn, const float cs) {
  const float u = ac * k.fmag;
  const float xd = x[1], thd = x[3];
  const float sg = xd > 0.f ? 1.0f : (xd < 0.f ? -1.0f : 0.0f);
  const float cf = k.muc * sg;
  const float pf = (k.mup * thd) / k.pm;
  const float fac = ((u + (k.pm * sn) * (thd * thd)) - cf) / k.mass;
  const float num = (k.g * sn - cs * fac) - pf;
  const float den = k.len * (k.k43 - (k.mp * (cs * cs)) / k.mass);
  const float thdd = num / den;
  const float xdd = fac - ((k.pm * thdd) * cs) / k.mass;
  x[0] = x[0] + xd * k.dt;
  x[1] = xd + xdd * k.dt;
  x[2] = x[2] + thd * k.dt;
  x[3] = thd + thdd * k.dt;
}

// UT: the sigma-point form (MultiDISCO._sigma_rollout, disco.py:211-292; the weighted costs of _compute_cost, disco.py:312-323): row m of
// `params` is sigma point m and the lane's cost is the weighted SUM
//     sum_m sum_t mw[(m H + t) mod M] inst(x_{m,t}) + sum_m mw[m] term(x_{m,H})
// - the reference views its flat [rollout][step] block of instantaneous costs as rows of M consecutive entries, and rollout
// (s N + n) M + m runs sigma point m, so entry (m, t) meets weight (m H + t) mod M (rollout.hpp has the Pendulum's form of the rule).
// Weighted terms accumulate in double (CostAcc::add_weighted); the two parts are rounded and added in fp32 as the regular kernel does.
// A template parameter, not a run-time branch: the plain instance is the kernel it was before the sigma-point form existed.
template <bool UT>
__device__ __forceinline__ void cartpole_rollout_body(const CartArgs &a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.n_local * a.S) return;
  const int s = idx / a.n_local, n = a.n0 + (idx - s * a.n_local);  // (n fastest: the rows of one sample are adjacent)
  const int D = a.D, H = a.H, N = a.N_total;
  const float *nz = a.noise ? a.noise + ((size_t)s * N + n) * D : nullptr;
  const float *th = a.theta + (size_t)n * D;
  const uint32_t ctr_tick = a.ctr[0], ctr_iter = a.ctr[1];
  const uint32_t lane = (uint32_t)(s * N + n);
  float x0[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) x0[k] = a.state[k];
  const bool have_rows = a.params != nullptr;  // (without rows a parameter named as sampled stays the constructor's Python float)
  const bool pm_py = (a.cp.par[CP_MP].kind == DUST_PARAM_PYFLOAT || (a.cp.par[CP_MP].kind == DUST_PARAM_SAMPLED && !have_rows)) &&
                     (a.cp.par[CP_LEN].kind == DUST_PARAM_PYFLOAT || (a.cp.par[CP_LEN].kind == DUST_PARAM_SAMPLED && !have_rows));
  const double pm_d = a.cp.par[CP_MP].value * a.cp.par[CP_LEN].value;
  double acc = 0.0, ut_term = 0.0;
  for (int m = 0; m < a.M; ++m) {
    // scalar-event params_dist quirk (disco.py:177-179): rollout r = (m, s, n) flattened uses params[r % M]
    const int mi = a.interleave ? (int)((((long)m * a.S + s) * N + n) % a.M) : m;
    const float *prow = a.params ? a.params + (size_t)mi * a.P : nullptr;
    float v[CP_NPAR];
#pragma unroll
    for (int q = 0; q < CP_NPAR; ++q) v[q] = skid_param(a.cp.par[q], prow, a.log_space);
    const CartCoef kf = cartpole_coef(v, pm_py, pm_d, a.dt);
    float x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = x0[k];
    float *so = a.states_out ? a.states_out + ((((size_t)m * a.S + s) * N + n) * (size_t)(H + 1)) * 4 : nullptr;
    if (so)
#pragma unroll
      for (int k = 0; k < 4; ++k) so[k] = x[k];
    double tot = 0.0;
    float z[8] = {};
    for (int t = 0; t < H; ++t) {
      float a0;  // theta + L eps
      if (a.noise_mode == NOISE_ACTIONS) {
        a0 = nz[t];
      } else if (a.noise_mode == NOISE_EPS) {
        a0 = th[t] + a.chol_a * nz[t];
      } else {
        if ((t & 7) == 0) philox_normal8(a.seed, (uint32_t)(t >> 3), lane, ctr_iter, ctr_tick, z);  // (the regular kernel's stream; one block serves 8 steps)
        float zt = z[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) zt = (t & 7) == i ? z[i] : zt;  // (selects, not an indexed read: z stays in registers)
        a0 = th[t] + a.chol_a * zt;
      }
      double sc = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = x[k] - a.cp.goal[k];
        sc += (double)((d * d) * a.cp.w_state[k]);
      }
      const double cc = (double)((a0 * a0) * a.cp.w_ctrl[0]);
      if (UT) tot += (double)a.mw[((long)m * H + t) % a.M] * (double)((float)sc + (float)cc);
      else tot += (double)((float)sc + (float)cc);
      cartpole_step(x, clampf(a0, -1.0f, 1.0f), kf, fast_sinf(x[2]), fast_cosf(x[2]));
      if (so)
#pragma unroll
        for (int k = 0; k < 4; ++k) so[(size_t)(t + 1) * 4 + k] = x[k];
    }
    double tc = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = x[k] - a.cp.goal[k];
      tc += (double)((d * d) * a.cp.w_term[k]);
    }
    if (UT) {  // weighted instantaneous and terminal parts are summed separately over the sigma points (disco.py:314-321)
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

__global__ __launch_bounds__(256) void cartpole_rollout_kernel(const CartArgs a) { cartpole_rollout_body<false>(a); }
__global__ __launch_bounds__(256) void cartpole_ut_rollout_kernel(const CartArgs a) { cartpole_rollout_body<true>(a); }

}  // namespace dust
