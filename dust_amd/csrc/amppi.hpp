// amppi.hpp - AMPPI.update_actions (dust/controllers/amppi.py:227-260) in ONE launch: the single-policy information-theoretic MPC of
// Williams et al. 2017 on the four model families.  S independent trajectories, one softmax, one weighted sum.
//
// Phase 1, one LANE per trajectory s (sigma points looped, see below):
//   acts[s] = a_seq + L z (Philox, common.hpp philox_normal8: block j >> 3 of row s) or the caller's actions; eps[s] = acts[s] - a_seq in
//   BOTH cases (amppi.py:129; for drawn noise the reference keeps the draw itself, amppi.py:125-126 - taking the difference makes a tick
//   from returned actions repeat the tick that drew them bit for bit).  Actions are NOT clamped here: the models clamp inside their step.
//   H steps of the family's own device step (common.hpp model_step, skid.hpp skid_step, cartpole.hpp cartpole_step) with this
//   trajectory's parameter row: none (the model's values) / row 0 for everybody / row s / every one of the pts = 2P + 1 sigma points.
//   Costs as amppi.py:193-225: the instantaneous cost on states 1 .. H with NO action (Particle: actions = 0), the terminal cost on
//   state H; sigma points combine as sum_k w_k (sum_t inst[s, k, t]) and sum_k w_k term[s, k] (amppi.py:208-215: a clean [S, pts] view);
//   ctrl[s] = lambda sum_t (a_seq[t] a_pre) . eps[s, t] with the full a_pre (amppi.py:221-223); cost = (term + inst) + ctrl.
// Phase 2, the LAST-ARRIVING workgroup (nobody waits for anybody: nothing can spin):
//   beta = min costs, omega_s = -(costs_s - beta) / lambda - logsumexp, a_seq = clamp(a_seq + sum_s e^omega_s eps[s], min_a, max_a)
//   (amppi.py:250-259).  Every sum runs in an order fixed by (S, D) alone, so the result does not depend on who arrived last.
//
// Hand-off (per-XCD L2s are not coherent): every lane stores its cost (and its drawn actions) with plain stores, every wave drains
// vmcnt, workgroup barrier, lane 0 makes an agent-scope release, drains again and takes a ticket with a relaxed agent-scope add on a
// word that a memset node zeroed ahead of the launch; the workgroup that draws the last ticket makes an agent-scope acquire and reads
// everything with plain loads.
//
// Lane mapping: one lane per TRAJECTORY with the sigma points in a loop, not one lane per (trajectory, point).  The actions of a
// trajectory then exist once (in HBM / L1: D <= 128 values do not fit registers under a run-time index), the weighted combination of the
// points is a lane-local sum in a fixed order, and S - not S pts - decides the grid; the price is a serial chain pts times longer in the
// sigma-point mode, which is the rare one.  256 lanes per workgroup (one wave per SIMD of a CU) is an UNMEASURED choice: lane s reads
// acts[s * D + t], a stride of D values between neighbouring lanes, so a wave's action load touches up to 64 cache lines per step, and
// more waves per SIMD - or 64-lane workgroups, which would spread S = 1024 over 16 CUs instead of 4 - may hide that latency better.
// A transposed [D][S] copy of the actions would coalesce the reads.  Neither alternative has been timed.
// The batched tick below (amppi_batch_kernel: B environments on a grid of (ceil(S / 256), B)) fills the idle CUs with OTHER
// environments' workgroups and runs their reducers side by side (DESIGN.md section 5 has the measured environment-ticks/s); it changes
// nothing inside an environment - the same 256 lanes per workgroup, the same stride-D reads, the same one-workgroup phase 2 - so the
// choice above stays unmeasured, for the lone tick and for every environment of a batch.
#pragma once
#include "cartpole.hpp"
#include "handoff.hpp"

namespace dust {

enum { AMPPI_PARAMS_NONE = 0, AMPPI_PARAMS_SINGLE = 1, AMPPI_PARAMS_EXTENDED = 2, AMPPI_PARAMS_SIGMA = 3 };
#define AMPPI_THREADS 256
#define AMPPI_MAX_SAMPLES 65536

struct AmppiArgs {
  DevModel dm;   // Pendulum / Particle
  SkidModel sk;  // skid-steer: parameters, wheel-speed bounds, quadratic cost
  CartModel cp;  // cart-pole: parameters, quadratic cost
  int S, H, da, D, P, pts;
  int mode;    // AMPPI_PARAMS_*
  int philox;  // draw the actions (otherwise `acts` holds the caller's)
  float lambda, dt;
  float chol[3];  // cholesky(a_cov): L00, L10, L11
  float pre[3];   // inverse(a_cov): P00, P01 (= P10), P11
  float min_a[2], max_a[2];
  float state[8];
  uint64_t seed;
  uint32_t *ctr;        // {tick, iter, ..}: Philox stream position; the reducer advances iter after a drawing tick
  const float *params;  // [1 | S | pts][P] or nullptr
  const float *mw;      // [pts] sigma weights (AMPPI_PARAMS_SIGMA)
  float *acts;          // [S][D]
  float *a_seq;         // [D] in / out
  float *costs, *omega;  // [S]
  float *states_out;     // [S * pts][H + 1][ds] or nullptr
  unsigned int *ticket;
};

// The filter's prior beside AmppiArgs (PRIOR instances): a uniform mixture of K normals N(means[k], diag(bw)^2) over P <= 4 columns
struct AmppiPrior {
  const float *means;  // [K][P]: the filter's particles, read in place
  int K, P;
  float bw[4];
  uint64_t seed;      // the Philox key of dust_mpf_prior_sample(m, S, seed)
  float *params_out;  // [S][P] or nullptr: the rows as drawn
};

// sum_k w[k] (x_k - goal_k)^2 as the quadratic family's kernels form it (skid.hpp / cartpole.hpp), without the control term
template <int DS>
__device__ __forceinline__ float amppi_quad(const float *x, const float *goal, const float *w) {
  double sc = 0.0;
#pragma unroll
  for (int k = 0; k < DS; ++k) {
    const float d = x[k] - goal[k];
    sc += (double)((d * d) * w[k]);
  }
  return (float)sc;
}

template <int MODEL>
struct AmppiDims {
  static constexpr int DS = MODEL == DUST_MODEL_PENDULUM ? 2 : (MODEL == DUST_MODEL_SKID_STEER ? 5 : 4);
};

// ---- a parameter row held in registers (the filter-coupled "extended" mode: AmppiPrior).  A local float[4] read as row[p.col] goes to
// scratch memory; the four entries are read first and the column picks among them (the pattern of mpf.hpp's sel4f).
__device__ __forceinline__ float amppi_row_at(const float *row, const int c) {
  const float v0 = row[0], v1 = row[1], v2 = row[2], v3 = row[3];
  return c == 0 ? v0 : (c == 1 ? v1 : (c == 2 ? v2 : v3));
}
// skid_param(p, row, 0) on such a row
__device__ __forceinline__ float amppi_row_param(const DevParam &p, const float *row) {
  return p.kind == DUST_PARAM_SAMPLED ? amppi_row_at(row, p.col) : (float)p.value;
}
// make_coef(dm, row) (common.hpp) on such a row, log_space = 0
__device__ __forceinline__ Val amppi_row_val(const DevParam &p, const float *row) {
  if (p.kind == DUST_PARAM_SAMPLED) return v_t(amppi_row_at(row, p.col));
  if (p.kind == DUST_PARAM_TENSOR0D) return v_t((float)p.value);
  return v_py(p.value);
}
__device__ __forceinline__ Coef amppi_row_coef(const DevModel &dm, const float *row) {
  Coef c;
  if (dm.model == DUST_MODEL_PENDULUM) {
    Val g = amppi_row_val(dm.g, row), m = amppi_row_val(dm.mass, row), l = amppi_row_val(dm.length, row);
    c.c0 = tof(v_div(v_mul(v_py(-3.0), g), v_mul(v_py(2.0), l)));
    c.c1 = tof(v_div(v_py(3.0), v_mul(m, v_sq(l))));
  } else {
    c.c0 = tof(amppi_row_val(dm.mass, row));
    c.c1 = 0.f;
  }
  return c;
}

// One trajectory on one parameter row: -> sum_t inst(x_t), t = 1 .. H, and term(x_H); `so`: its [H + 1][DS] states or nullptr
// NAV (skid-steer only): the navigation cost family of skid.hpp - w_obs occ(x_0, x_1) joins both parts; `nav` and `map` are read by it alone
// ROW: `prow` is a parameter row the lane drew itself (AmppiPrior below), a local float[4]: its run-time columns are read through selects
// (amppi_row_at), so that the row stays in registers
// ARGS: AmppiArgs, or the per-environment view of a batched tick (AmppiEnvArgs below): the same member names
template <int MODEL, bool NAV, bool ROW = false, class ARGS = AmppiArgs>
__device__ __forceinline__ void amppi_traj(const ARGS &a, const float *acts, const float *prow, float *so, float *inst_out, float *term_out,
                                           const SkidNav *nav, const DevModel *map) {
  constexpr int DS = AmppiDims<MODEL>::DS;
  const int H = a.H;
  float x[DS];
#pragma unroll
  for (int k = 0; k < DS; ++k) x[k] = a.state[k];
  if (so)
#pragma unroll
    for (int k = 0; k < DS; ++k) so[k] = x[k];
  double tot = 0.0;
  if constexpr (MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_PARTICLE) {
    Coef c;
    if constexpr (ROW) c = amppi_row_coef(a.dm, prow);
    else c = make_coef(a.dm, prow);
    const float zero[2] = {0.f, 0.f};  // (Particle.default_inst_cost(states): actions = 0, particle.py:170)
    for (int t = 0; t < H; ++t) {
      float u[2];
      u[0] = acts[t * a.da];
      u[1] = MODEL == DUST_MODEL_PARTICLE ? acts[t * a.da + 1] : 0.f;
      model_step<MODEL>(a.dm, c, x, u);
      tot += (double)inst_cost<MODEL>(a.dm, x, zero);
      if (so)
#pragma unroll
        for (int k = 0; k < DS; ++k) so[(size_t)(t + 1) * DS + k] = x[k];
    }
    *term_out = term_cost<MODEL>(a.dm, x);
  } else if constexpr (MODEL == DUST_MODEL_SKID_STEER) {
    float xicr, wr, ad;
    if constexpr (ROW) {
      xicr = amppi_row_param(a.sk.x_icr, prow);
      wr = amppi_row_param(a.sk.wheel_radius, prow);
      ad = amppi_row_param(a.sk.axial_distance, prow);
    } else {
      xicr = skid_param(a.sk.x_icr, prow, 0);
      wr = skid_param(a.sk.wheel_radius, prow, 0);
      ad = skid_param(a.sk.axial_distance, prow, 0);
    }
    for (int t = 0; t < H; ++t) {
      const float a0 = acts[2 * t], a1 = acts[2 * t + 1];
      skid_step(x, clampf(a0, a.sk.lo[0], a.sk.hi[0]), clampf(a1, a.sk.lo[1], a.sk.hi[1]), xicr, wr, ad, a.dt);
      if constexpr (NAV) tot += (double)(amppi_quad<DS>(x, a.sk.goal, a.sk.w_state) + nav->w_obs * collision(*map, x[0], x[1]));
      else tot += (double)amppi_quad<DS>(x, a.sk.goal, a.sk.w_state);
      if (so)
#pragma unroll
        for (int k = 0; k < DS; ++k) so[(size_t)(t + 1) * DS + k] = x[k];
    }
    if constexpr (NAV) *term_out = amppi_quad<DS>(x, a.sk.goal, a.sk.w_term) + nav->w_obs * collision(*map, x[0], x[1]);
    else *term_out = amppi_quad<DS>(x, a.sk.goal, a.sk.w_term);
  } else {
    const bool have_rows = prow != nullptr;  // (as cartpole.hpp: without rows a parameter named as sampled stays the constructor's Python float)
    const bool pm_py = (a.cp.par[CP_MP].kind == DUST_PARAM_PYFLOAT || (a.cp.par[CP_MP].kind == DUST_PARAM_SAMPLED && !have_rows)) &&
                       (a.cp.par[CP_LEN].kind == DUST_PARAM_PYFLOAT || (a.cp.par[CP_LEN].kind == DUST_PARAM_SAMPLED && !have_rows));
    float v[CP_NPAR];
#pragma unroll
    for (int q = 0; q < CP_NPAR; ++q) {
      if constexpr (ROW) v[q] = amppi_row_param(a.cp.par[q], prow);
      else v[q] = skid_param(a.cp.par[q], prow, 0);
    }
    const CartCoef kf = cartpole_coef(v, pm_py, a.cp.par[CP_MP].value * a.cp.par[CP_LEN].value, a.dt);
    for (int t = 0; t < H; ++t) {
      cartpole_step(x, clampf(acts[t], -1.0f, 1.0f), kf, fast_sinf(x[2]), fast_cosf(x[2]));
      tot += (double)amppi_quad<DS>(x, a.cp.goal, a.cp.w_state);
      if (so)
#pragma unroll
        for (int k = 0; k < DS; ++k) so[(size_t)(t + 1) * DS + k] = x[k];
    }
    *term_out = amppi_quad<DS>(x, a.cp.goal, a.cp.w_term);
  }
  *inst_out = (float)tot;
}

template <int MODEL>
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_kernel(const AmppiArgs a) {
  constexpr bool NAV = false, PRIOR = false;
  const SkidNav *const nav = nullptr;
  const AmppiPrior *const pri = nullptr;
  uint32_t *const grid_lds = nullptr;
#include "amppi_body.inc"
}

// The skid-steer tick with the navigation cost family: dynamic LDS of 4 nav.grid_words bytes behind the static object
struct AmppiNavArgs {
  AmppiArgs a;
  SkidNav nav;
};
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_skid_nav_kernel(const AmppiNavArgs k) {
  constexpr int MODEL = DUST_MODEL_SKID_STEER;
  constexpr bool NAV = true, PRIOR = false;
  const AmppiArgs &a = k.a;
  const SkidNav *const nav = &k.nav;
  const AmppiPrior *const pri = nullptr;
  extern __shared__ __attribute__((aligned(16))) uint32_t grid_lds[];
#include "amppi_body.inc"
}

// The "extended" mode coupled to a dynamics filter (dust_amppi_dual_tick): lane s draws row s of mpf.prior.sample([S]) itself - the
// stream of mpf_sample_kernel (mpf.hpp), bit for bit - and rolls its trajectory out on it: no parameter buffer, no launch of its own.
struct AmppiPriorArgs {
  AmppiArgs a;
  AmppiPrior pr;
};
template <int MODEL>
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_prior_kernel(const AmppiPriorArgs k) {
  constexpr bool NAV = false, PRIOR = true;
  const AmppiArgs &a = k.a;
  const SkidNav *const nav = nullptr;
  const AmppiPrior *const pri = &k.pr;
  uint32_t *const grid_lds = nullptr;
#include "amppi_body.inc"
}
struct AmppiNavPriorArgs {
  AmppiArgs a;
  SkidNav nav;
  AmppiPrior pr;
};
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_skid_nav_prior_kernel(const AmppiNavPriorArgs k) {
  constexpr int MODEL = DUST_MODEL_SKID_STEER;
  constexpr bool NAV = true, PRIOR = true;
  const AmppiArgs &a = k.a;
  const SkidNav *const nav = &k.nav;
  const AmppiPrior *const pri = &k.pr;
  extern __shared__ __attribute__((aligned(16))) uint32_t grid_lds[];
#include "amppi_body.inc"
}

// BaseController.roll(steps) (base.py:68-80) for 1 <= steps: shift the sequence left by `steps` rows, zeros behind
__global__ void amppi_roll_kernel(float *a_seq, const int D, const int shift) {
  const int j = (int)threadIdx.x;
  const float v = (j < D && j + shift < D) ? a_seq[j + shift] : 0.f;
  wg_sync();
  if (j < D) a_seq[j] = v;
}

// ---- B independent ticks in ONE launch (dust_amppi_batch_update): grid (ceil(S / 256), B), blockIdx.y is the environment.  A workgroup
// makes itself the arguments of a lone tick on its environment's slices - states [B][8] (ds values, zero-padded), a_seq [B][D],
// acts [B][S][D], costs / omega [B][S], params [B][rows][P], ticket [B], ctr [B][4], seeds [B] - and runs the SAME body text on them: the
// arithmetic, its order and the hand-off are the lone kernel's, per environment (the workgroup that draws ticket gridDim.x - 1 of
// ticket[b] reduces environment b; the B reducers run side by side and nobody waits for anybody).  Model, cost, lambda, chol, pre, the
// bounds and the sigma weights are shared.  The workgroups of an environment whose `active` byte is 0 return before they touch anything.
struct AmppiBatchArgs {
  AmppiArgs a;                  // the shared fields; its per-environment pointers are environment 0's, `state` and `seed` are unused
  const float *states;          // [B][8]
  const uint64_t *seeds;        // [B]
  const unsigned char *active;  // [B] or nullptr: everybody
  int prow_stride;              // values between two environments' parameter rows (rows * P)
};
// What the body text reads through `a`, for ONE environment: AmppiArgs' member names.  The shared structs and arrays stay where the
// launch put them (references and pointers into the kernel's arguments: a local COPY of AmppiArgs goes to scratch memory as a whole -
// 704 bytes per lane - because the body indexes min_a / max_a at run time); the environment's own values are plain members.
struct AmppiEnvArgs {
  const DevModel &dm;
  const SkidModel &sk;
  const CartModel &cp;
  int S, H, da, D, P, pts, mode, philox;
  float lambda, dt;
  const float *chol, *pre, *min_a, *max_a;
  float state[8];
  uint64_t seed;
  uint32_t *ctr;
  const float *params, *mw;
  float *acts, *a_seq, *costs, *omega, *states_out;
  unsigned int *ticket;
};
__device__ __forceinline__ AmppiEnvArgs amppi_env_view(const AmppiBatchArgs &k, const int env) {
  const AmppiArgs &g = k.a;
  const float *st = k.states + (size_t)env * 8;
  return AmppiEnvArgs{g.dm, g.sk, g.cp, g.S, g.H, g.da, g.D, g.P, g.pts, g.mode, g.philox, g.lambda, g.dt, g.chol, g.pre, g.min_a, g.max_a,
                      {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]},
                      k.seeds[env],
                      g.ctr + (size_t)env * 4,
                      g.params ? g.params + (size_t)env * (size_t)k.prow_stride : nullptr,
                      g.mw,
                      g.acts + (size_t)env * (size_t)g.S * (size_t)g.D,
                      g.a_seq + (size_t)env * (size_t)g.D,
                      g.costs + (size_t)env * (size_t)g.S,
                      g.omega + (size_t)env * (size_t)g.S,
                      nullptr,
                      g.ticket + env};
}

template <int MODEL>
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_batch_kernel(const AmppiBatchArgs k) {
  constexpr bool NAV = false, PRIOR = false;
  const SkidNav *const nav = nullptr;
  const AmppiPrior *const pri = nullptr;
  uint32_t *const grid_lds = nullptr;
  const int env = (int)blockIdx.y;
  if (k.active && k.active[env] == 0) return;
  const AmppiEnvArgs a = amppi_env_view(k, env);
#include "amppi_body.inc"
}
// ... with the navigation cost family: every workgroup stages the one map into its LDS, as the lone navigation kernel does
struct AmppiNavBatchArgs {
  AmppiBatchArgs k;
  SkidNav nav;
};
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_skid_nav_batch_kernel(const AmppiNavBatchArgs kn) {
  constexpr int MODEL = DUST_MODEL_SKID_STEER;
  constexpr bool NAV = true, PRIOR = false;
  const SkidNav *const nav = &kn.nav;
  const AmppiPrior *const pri = nullptr;
  extern __shared__ __attribute__((aligned(16))) uint32_t grid_lds[];
  const int env = (int)blockIdx.y;
  if (kn.k.active && kn.k.active[env] == 0) return;
  const AmppiEnvArgs a = amppi_env_view(kn.k, env);
#include "amppi_body.inc"
}

// ---- the batched tick coupled to B dynamics filters (dust_amppi_dual_batch_tick, "extended"): the grid of amppi_batch_kernel with
// PRIOR = true.  Lane s of environment b draws row s of dust_mpf_prior_sample(filter b, S, prior_seeds[b]) itself: means at
// x + b K P, the bandwidths of environment b's prior_bwv (device memory: the batched filter kernel wrote them just ahead on the same
// stream), the key prior_seeds[b].  A workgroup makes itself the AmppiPrior of its environment - the body reads it by AmppiPrior's names.
struct AmppiPriorBatch {
  const float *means;     // [B][K][P]: the filters' particles, read in place
  int K, P;
  const float *bwv;       // [B][4]
  const uint64_t *seeds;  // [B]
  float *params_out;      // [B][S][P] or nullptr
};
__device__ __forceinline__ AmppiPrior amppi_env_prior(const AmppiPriorBatch &p, const int env, const int S) {
  const float *b = p.bwv + (size_t)env * 4;
  return AmppiPrior{p.means + (size_t)env * (size_t)p.K * (size_t)p.P, p.K, p.P, {b[0], b[1], b[2], b[3]}, p.seeds[env],
                    p.params_out ? p.params_out + (size_t)env * (size_t)S * (size_t)p.P : nullptr};
}
struct AmppiPriorBatchArgs {
  AmppiBatchArgs k;
  AmppiPriorBatch pr;
};
template <int MODEL>
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_prior_batch_kernel(const AmppiPriorBatchArgs kp) {
  constexpr bool NAV = false, PRIOR = true;
  const SkidNav *const nav = nullptr;
  uint32_t *const grid_lds = nullptr;
  const int env = (int)blockIdx.y;
  if (kp.k.active && kp.k.active[env] == 0) return;
  const AmppiEnvArgs a = amppi_env_view(kp.k, env);
  const AmppiPrior pe = amppi_env_prior(kp.pr, env, a.S);
  const AmppiPrior *const pri = &pe;
#include "amppi_body.inc"
}
struct AmppiNavPriorBatchArgs {
  AmppiBatchArgs k;
  SkidNav nav;
  AmppiPriorBatch pr;
};
__global__ __launch_bounds__(AMPPI_THREADS) void amppi_skid_nav_prior_batch_kernel(const AmppiNavPriorBatchArgs kp) {
  constexpr int MODEL = DUST_MODEL_SKID_STEER;
  constexpr bool NAV = true, PRIOR = true;
  const SkidNav *const nav = &kp.nav;
  extern __shared__ __attribute__((aligned(16))) uint32_t grid_lds[];
  const int env = (int)blockIdx.y;
  if (kp.k.active && kp.k.active[env] == 0) return;
  const AmppiEnvArgs a = amppi_env_view(kp.k, env);
  const AmppiPrior pe = amppi_env_prior(kp.pr, env, a.S);
  const AmppiPrior *const pri = &pe;
#include "amppi_body.inc"
}

// dust_amppi_batch_roll: amppi_roll_kernel on a_seq [B][D], one workgroup per environment; inactive environments keep their sequence
__global__ void amppi_batch_roll_kernel(float *a_seq, const int D, const int shift, const unsigned char *active) {
  const int env = (int)blockIdx.x;
  if (active && active[env] == 0) return;
  float *row = a_seq + (size_t)env * D;
  const int j = (int)threadIdx.x;
  const float v = (j < D && j + shift < D) ? row[j + shift] : 0.f;
  wg_sync();
  if (j < D) row[j] = v;
}

}  // namespace dust
