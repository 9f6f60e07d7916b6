// mpf.hpp - dynamics-parameter SVGD filter ("MPF"), included at the end of dust_amd.hip.
//
// Replaces (reference file:line): MPF.phi / step / optimize / update_prior mpf.py:26-86, GaussianLikelihood.sample /
// log_prob / condition likelihoods.py:30-64, default_kernel + squared_distance svgd.py:28-39, 92-99, and the autograd
// calls at mpf.py:45 and mpf.py:50 (closed forms: GMM responsibilities; J^T (y - f(x)) / sigma_o^2 with the analytic
// Jacobian of one model step w.r.t. the uncertain parameters).  Models: Pendulum, Particle (step_jacobian below), SkidSteerRobot
// (mpf_skid_score below, over skid.hpp's step) and CartPoleModel (mpf_cart_score, over cartpole.hpp's step).
//
// The problem is tiny (M_p <= 1024 particles x P <= 4 parameters, n_steps ~ 20 dependent SVGD steps), i.e. pure launch
// latency on a GPU: ALL n_steps run inside ONE single-workgroup kernel with the particles, scores and squared norms in
// LDS; up to 1024 lanes = (particle, slice of the other particles); the only HBM traffic is the final particle
// write-back and the gradient norms.
//
// Reference quirk kept: MPF.update_prior hands `self.x` itself to MultivariateNormal(loc=...), which aliases the
// particle storage, and SGD updates x in place - so the prior means are always the CURRENT particles (mpf.py:26-38).
#pragma once
#include "mpf_env.hpp"  // MpfEnvIn

namespace dust {

struct MpfArgs {
  DevModel dm;
  int Mp, P, ds, da, n_steps, log_space, have_past;
  float prior_bwv[4];  // prior bandwidth per parameter dimension (equal after the first update_prior; MPF(bw=None) starts per-dimension)
  float bw, obs_std;
  float past_obs[4], past_action[2], obs[4];  // (Pendulum / Particle: up to four wide; the skid-steer model's five are in *skl)
  union {  // the likelihood's per-call constants, in device memory (below); one word for both: the argument block keeps its layout
    const struct SkidLik *skl;  // DUST_MODEL_SKID_STEER
    const struct CartLik *cpl;  // DUST_MODEL_CARTPOLE
  };
  // control-channel noise of the one-step prediction (Particle(deterministic=False), particle.py:145-148 reached through
  // likelihoods.py:30-46): `acts` there is the bare action vector, so ONE d_a-vector is drawn per phi() call - i.e. per SVGD step -
  // and shared by all filter particles.  act_seq[step][2] = fl(past_action + fl(dyn_std * z_step)), prepared by the host, or nullptr
  const float *act_seq;
  float *x;           // [Mp][P] in/out
  float *grad_norms;  // [n_steps] or nullptr
  float *phi_out;     // [Mp][P] or nullptr (phi of the first step, when n_steps == 0 semantics are wanted use n_steps=1, lr=0)
  // optimiser (SVGD.__init__ svgd.py:115: the class default is torch.optim.Adam; built once in MPF.__init__ mpf.py:24, so its
  // state persists across optimize() calls): any optimiser of dust_set_optimizer, its state slots [Mp][P] in / out and t0 steps taken so far
  OptArgs opt;  // handoff.hpp opt_step (the bare phi evaluation: plain SGD, no state)
  int t0;
  float *opt_s0, *opt_s1, *opt_s2;  // state slots [Mp][P] or nullptr
};

// d(next state)/d(params) of one model step, as autograd returns it through model.step (incl. clamp masks).
// J is [4][4] (state row, parameter column) and every index below is a compile-time constant or a select: a
// dynamically indexed local array would live in scratch memory.
__device__ __forceinline__ double sel4(const double v[4], int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : (c == 2 ? v[2] : v[3])); }
__device__ __forceinline__ void add_col(double J[4][4], int row, int col, double v) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (k == row && c == col) J[k][c] += v;
}
template <int P>
__device__ __forceinline__ void step_jacobian(const DevModel &dm, const float *x, const float *a, const float prow[4], double J[4][4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c) J[k][c] = 0.0;
  double pv[4] = {0, 0, 0, 0};
#pragma unroll
  for (int p = 0; p < P; ++p) pv[p] = dm.log_space ? exp((double)prow[p]) : (double)prow[p];
  if (dm.model == DUST_MODEL_PENDULUM) {
    const double g = dm.g.kind == DUST_PARAM_SAMPLED ? sel4(pv, dm.g.col) : dm.g.value;
    const double m = dm.mass.kind == DUST_PARAM_SAMPLED ? sel4(pv, dm.mass.col) : dm.mass.value;
    const double l = dm.length.kind == DUST_PARAM_SAMPLED ? sel4(pv, dm.length.col) : dm.length.value;
    const double dt = dm.dt;
    const double u = clampf(a[0], -dm.max_torque, dm.max_torque);
    const double s = sin((double)x[0] + M_PI);
    const double thd = (double)x[1] + dt * (-3.0 * g / (2.0 * l) * s + 3.0 / (m * l * l) * u);
    if (!(thd >= -dm.max_speed_pend && thd <= dm.max_speed_pend)) return;
    const double dg = dt * (-3.0 / (2.0 * l) * s), dmass = dt * (-3.0 / (m * m * l * l) * u);
    const double dl = dt * (3.0 * g / (2.0 * l * l) * s - 6.0 / (m * l * l * l) * u);
    if (dm.g.kind == DUST_PARAM_SAMPLED) {
      const double ch = dm.log_space ? sel4(pv, dm.g.col) : 1.0;
      add_col(J, 1, dm.g.col, dg * ch);
      add_col(J, 0, dm.g.col, dg * dt * ch);
    }
    if (dm.mass.kind == DUST_PARAM_SAMPLED) {
      const double ch = dm.log_space ? sel4(pv, dm.mass.col) : 1.0;
      add_col(J, 1, dm.mass.col, dmass * ch);
      add_col(J, 0, dm.mass.col, dmass * dt * ch);
    }
    if (dm.length.kind == DUST_PARAM_SAMPLED) {
      const double ch = dm.log_space ? sel4(pv, dm.length.col) : 1.0;
      add_col(J, 1, dm.length.col, dl * ch);
      add_col(J, 0, dm.length.col, dl * dt * ch);
    }
  } else {
    if (dm.mass.kind != DUST_PARAM_SAMPLED) return;
    const int col = dm.mass.col;
    const double m = sel4(pv, col), dt = dm.dt;
    double om = 1.0;
    if (dm.can_crash && dm.with_obstacle) om = 1.0 - (double)collision(dm, x[0], x[1]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double acc = (double)a[k] / m;
      const bool live_a = acc >= -dm.max_acc && acc <= dm.max_acc;
      const double accc = acc < -dm.max_acc ? -dm.max_acc : (acc > dm.max_acc ? dm.max_acc : acc);
      const double v = (double)x[2 + k] + accc * dt * om;
      const bool live_v = v >= -dm.max_speed && v <= dm.max_speed;
      if (live_a && live_v) add_col(J, 2 + k, col, dt * om * (-(double)a[k] / (m * m)) * (dm.log_space ? m : 1.0));
    }
  }
}

// The likelihood score J^T (y - f(x)) / sigma_o^2 of ONE particle under the skid-steer model (state x, y, theta, v, omega: five wide).
// Prediction: skid_step in fp32, as the rollout kernel takes it.  Jacobian in fp64 from the closed forms, r, l the wheel speeds after
// the clamp (it acts on the action, not on a parameter: no mask), c = cos(theta), s = sin(theta) of the past state:
//   lin = (r + l) pi wr        ang = 2 pi (r - l) wr / ad        fwd = lin dt        lat = -ang x_icr dt
//   d lin / d wr = (r + l) pi     d ang / d wr = 2 pi (r - l) / ad     d ang / d ad = -ang / ad
//   d lat / d x_icr = -ang dt     d lat / d p = -x_icr dt d ang / d p  (p = wr, ad)
//   rows (x, y, theta, v, omega) = (d fwd c - d lat s, d fwd s + d lat c, d ang dt, d lin, d ang);  log space: column p times p's value.
// With e = y - f(x):  J_p^T e = d lin (dt (c e_x + s e_y) + e_v) + d lat (c e_y - s e_x) + d ang (dt e_theta + e_omega).
// Every parameter is sampled (column `col` of the particle) or fixed; the columns are placed by selects, as add_col does.
// What does not depend on the particle - the clamped wheel speeds, c, s, (r + l) pi, 2 pi (r - l), the two observations - is prepared
// by the host (mpf_skid_prepare; the heading's fp32 cosine and sine by mpf_skid_heading_kernel, with the rollout's own fast_cosf /
// fast_sinf) and read from DEVICE MEMORY inside the model's branch: as kernel arguments these 40 words were loaded ahead of the branch
// and held in scalar registers through the whole kernel, and the trigonometric code inside the branch raised its register peak - both
// cost the Pendulum and Particle paths spilled registers (the register table).
struct SkidLik {
  int smp[3], col[3];        // x_icr, wheel_radius, axial_distance: sampled?  its particle column
  float fix_f[3];            // ... its value when fixed, as the fp32 scalar the step sees
  float r, l, dt;            // wheel speeds after the clamp; (float)delta_t
  float cs, sn;              // fast_cosf / fast_sinf of past theta (mpf_skid_heading_kernel)
  float past[5], obs[5];     // past observation (the state the step starts from), new observation
  double fix_d[3];
  double c, s, sum, dif, dtd;  // cos / sin of past theta, (r + l) pi, 2 pi (r - l), delta_t
};
// (the four entries are read first: a load per arm of the select is folded into ONE load from a selected address, and the array then
// lives in scratch memory)
__device__ __forceinline__ float sel4f(const float *v, int c) {
  const float v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
  return c == 0 ? v0 : (c == 1 ? v1 : (c == 2 ? v2 : v3));
}
template <int P>
__device__ __forceinline__ void mpf_skid_score(const SkidLik *k, const int log_space, const float *xp, const double inv_obs2, double *out) {
  const bool sx = k->smp[0] != 0, sw = k->smp[1] != 0, sa = k->smp[2] != 0;
  const int cx = k->col[0], cw = k->col[1], ca = k->col[2];
  const float rx = sel4f(xp, cx), rw = sel4f(xp, cw), ra = sel4f(xp, ca);
  const float fx = sx ? (log_space ? expf(rx) : rx) : k->fix_f[0], fw = sw ? (log_space ? expf(rw) : rw) : k->fix_f[1],
              fa = sa ? (log_space ? expf(ra) : ra) : k->fix_f[2];
  float pred[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) pred[q] = k->past[q];
  skid_step_cs(pred, k->r, k->l, fx, fw, fa, k->dt, k->cs, k->sn);
  double e[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) e[q] = (double)k->obs[q] - (double)pred[q];
  // (a sampled parameter enters the Jacobian with the fp32 value the prediction was taken at - in log space expf's, as the reference's
  // fp32 autograd differentiates at theta.exp() in fp32)
  const double xicr = sx ? (double)fx : k->fix_d[0], wr = sw ? (double)fw : k->fix_d[1], ad = sa ? (double)fa : k->fix_d[2];
  const double c = k->c, s = k->s, dt = k->dtd;
  const double t_lin = dt * (c * e[0] + s * e[1]) + e[3], t_lat = c * e[1] - s * e[0], t_ang = dt * e[2] + e[4];
  const double dang_w = k->dif / ad, ang = dang_w * wr, dang_a = -ang / ad;
  const double gx = sx ? (-ang * dt * t_lat) * (log_space ? xicr : 1.0) : 0.0;
  const double gw = sw ? (k->sum * t_lin + dang_w * (t_ang - xicr * dt * t_lat)) * (log_space ? wr : 1.0) : 0.0;
  const double ga = sa ? (dang_a * (t_ang - xicr * dt * t_lat)) * (log_space ? ad : 1.0) : 0.0;
#pragma unroll
  for (int p = 0; p < P; ++p) out[p] = ((sx && cx == p ? gx : 0.0) + (sw && cw == p ? gw : 0.0) + (sa && ca == p ? ga : 0.0)) * inv_obs2;
}

__global__ void mpf_skid_heading_kernel(SkidLik *k) {
  if (threadIdx.x == 0) {
    k->cs = fast_cosf(k->past[2]);
    k->sn = fast_sinf(k->past[2]);
  }
}

// The likelihood score J^T (y - f(x)) / sigma_o^2 of ONE particle under the cart-pole model (cartpole.py:126-172 through
// likelihoods.py:30-49).  Prediction: cartpole_step in fp32, as the rollout kernel takes it.  Jacobian in fp64 from the closed forms;
// a = the action after the clamp (it acts on the action, not on a parameter: no mask), s, c = sin, cos of the past angle, w = th_d,
// sg = sign(x_d), mass = 2 m_c, pm = m_p L:
//   fac = (a F + pm s w^2 - mu_c sg) / mass     pf = mu_p w / pm     num = g s - c fac - pf     den = L (4/3 - m_p c^2 / mass)
//   tdd = num / den                             xdd = fac - pm tdd c / mass
// Only the x_d' = x_d + xdd dt and th_d' = th_d + tdd dt rows depend on a parameter.  With A = dt e_xd, B = dt e_thd (e = y - f(x)),
//   Q = (B - A c pm / mass) / den,  R = A - c Q,  T = tdd Q,  U = A (c / mass) tdd
// the seven columns of J^T e are (from d tdd = (d num - tdd d den) / den and d xdd = d fac - (c / mass)(d pm tdd + pm d tdd) - pm tdd c d(1 / mass)):
//   g: s Q      m_c: -(fac / m_c) R - T L m_p c^2 / (mass m_c) + U pm / m_c      m_p: (L s w^2 / mass) R + (pf / m_p) Q + T L c^2 / mass - U L
//   L: (m_p s w^2 / mass) R + (pf / L) Q - T den / L - U m_p      mu_c: -(sg / mass) R      mu_p: -(w / pm) Q      F: (a / mass) R
// and in log space column p is multiplied by p's value.  A sampled parameter is a particle column: `par_of_col` names the parameter of
// each column, so P exponentials are taken, not seven.  What does not depend on the particle - the clamped action, s and c in both
// precisions, w, w^2, sg, the observations - is prepared per call (mpf_cart_prepare on the host, mpf_cart_angle_kernel for the fp32
// sine and cosine) and read from DEVICE MEMORY inside the model's branch, as SkidLik is.
struct CartLik {
  int par_of_col[4];         // parameter index (CP_*) carried by particle column p
  float fix_f[CP_NPAR];      // the seven values as the fp32 scalars the step sees (a sampled one: replaced per particle)
  float ac, dt;              // action after the clamp; (float)dt
  float cs, sn;              // fast_cosf / fast_sinf of past theta (mpf_cart_angle_kernel)
  float past[4], obs[4];     // past observation (the state the step starts from), new observation
  int pm_py, pad;            // m_p and L are both fixed Python floats: their product is a Python float
  double pm_d;
  double fix_d[CP_NPAR];
  double c, s, w, w2, sg, a, dtd;
};
template <int P>
__device__ __forceinline__ void mpf_cart_score(const CartLik *k, const int log_space, const float *xp, const double inv_obs2, double *out) {
  float vf[CP_NPAR];
  double vd[CP_NPAR];
#pragma unroll
  for (int q = 0; q < CP_NPAR; ++q) {
    vf[q] = k->fix_f[q];
    vd[q] = k->fix_d[q];
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int which = k->par_of_col[p];
    const float v = log_space ? expf(xp[p]) : xp[p];
    // (a sampled parameter enters the Jacobian with the fp32 value the prediction was taken at - in log space expf's)
#pragma unroll
    for (int q = 0; q < CP_NPAR; ++q) {
      vf[q] = q == which ? v : vf[q];
      vd[q] = q == which ? (double)v : vd[q];
    }
  }
  const CartCoef kf = cartpole_coef(vf, k->pm_py != 0, k->pm_d, k->dt);
  float pred[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) pred[q] = k->past[q];
  cartpole_step(pred, k->ac, kf, k->sn, k->cs);
  const double dt = k->dtd, c = k->c, s = k->s, w = k->w, w2 = k->w2, sg = k->sg;
  const double A = dt * ((double)k->obs[1] - (double)pred[1]), B = dt * ((double)k->obs[3] - (double)pred[3]);
  const double g = vd[CP_G], mc = vd[CP_MC], mp = vd[CP_MP], L = vd[CP_LEN], muc = vd[CP_MUC], mup = vd[CP_MUP], F = vd[CP_FMAG];
  const double imass = 1.0 / (mc + mc), pm = mp * L, ipm = 1.0 / pm;
  const double fac = (k->a * F + pm * s * w2 - muc * sg) * imass, pf = mup * w * ipm;
  const double den0 = 4.0 / 3 - mp * c * c * imass, den = L * den0, iden = 1.0 / den;
  const double tdd = (g * s - c * fac - pf) * iden;
  const double Q = (B - A * c * pm * imass) * iden, R = A - c * Q, T = tdd * Q, U = A * (c * imass) * tdd;
  const double imc = 1.0 / mc;
  double gj[CP_NPAR];
  gj[CP_G] = s * Q;
  gj[CP_MC] = (-(fac * imc) * R - T * L * mp * c * c * imass * imc + U * pm * imc);
  gj[CP_MP] = (L * s * w2 * imass) * R + (pf / mp) * Q + T * L * c * c * imass - U * L;
  gj[CP_LEN] = (mp * s * w2 * imass) * R + (pf / L) * Q - T * den0 - U * mp;
  gj[CP_MUC] = -(sg * imass) * R;
  gj[CP_MUP] = -(w * ipm) * Q;
  gj[CP_FMAG] = (k->a * imass) * R;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int which = k->par_of_col[p];
    double gsel = 0.0, vsel = 1.0;
#pragma unroll
    for (int q = 0; q < CP_NPAR; ++q) {
      gsel = q == which ? gj[q] : gsel;
      vsel = q == which ? vd[q] : vsel;
    }
    out[p] = gsel * (log_space ? vsel : 1.0) * inv_obs2;
  }
}

// ... for the B environments of a batched filter in one launch: lane b, the same fast_cosf / fast_sinf (LIK: SkidLik or CartLik - both
// keep the past heading / angle in past[2])
template <class LIK>
__global__ void mpf_lik_angle_batch_kernel(LIK *k, const int B, const unsigned char *active) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= B || (active && active[env] == 0)) return;
  k[env].cs = fast_cosf(k[env].past[2]);
  k[env].sn = fast_sinf(k[env].past[2]);
}

__global__ void mpf_cart_angle_kernel(CartLik *k) {
  if (threadIdx.x == 0) {
    k->cs = fast_cosf(k->past[2]);
    k->sn = fast_sinf(k->past[2]);
  }
}

// Lane = (particle i, slice r of the other particles): R = blockDim / Mpad slices share the O(M_p) loops of a particle and
// their partial sums are combined in slice order through LDS (fixed order: reproducible).  No divisions or fp64
// transcendentals inside the O(M_p^2) loops: reciprocals are hoisted (fp64, error 1e-16), weights use expf.
// P is a template parameter: with a run-time P the per-lane arrays are indexed dynamically and live in scratch memory
// (measured: 3 us per inner-loop iteration instead of ~50 ns).
// CART: the cart-pole instances.  The model's score is a template branch, not one more run-time branch: as a run-time branch it cost
// every instance of the one-workgroup kernel spilled registers (P = 1: 4 -> 19) and the P = 4, KC = 16 poll kernel 32 bytes of scratch;
// with it compiled out the Pendulum / Particle / skid-steer instances are the parent's (the register table).
template <int P, bool CART = false>
__global__ __launch_bounds__(1024) void mpf_optimize_kernel(const MpfArgs a) {
#define MPF_UNIFORM(v) (v)
#include "mpf_body.inc"
#undef MPF_UNIFORM
}

// ---- B filters in ONE launch (dust_mpf_batch_optimize, dust_amppi_dual_batch_tick): one workgroup per environment, blockIdx.x is the
// environment.  A workgroup makes itself the arguments of a lone call on its environment's slices - particles and optimiser slots
// [B][Mp][P], the observations, the action, the steps taken so far (MpfEnvIn [B], staged by the host per call), the prior bandwidths
// [B][4], the kernel bandwidth [B] (Silverman's, written by mpf_silverman_batch_kernel just ahead on the same stream; or the call's fixed
// one), grad_norms [B][gn_stride], SkidLik / CartLik [B] - and runs the SAME body text on them: the arithmetic and its order are the lone
// kernel's, per environment.  Model, grid bits, obs_std, the optimiser's options, Mp and P are shared (obs_std, the optimiser's lr and the
// bandwidth per environment: mpf_optimize_rows_kernel below).  Behind the body lane 0 does what
// the host does after a lone call: the prior bandwidths become the kernel bandwidth (update_prior(bw), mpf.py:85) and bw_used[b] records
// it.  The workgroup of an environment whose `active` byte is 0 returns before it touches anything.  No workgroup talks to another one.
// MODEL, LOG, ADAM: the shared model - with it the widths of state and action -, log_space and whether the optimiser is Adam (its step
// takes two fp64 powers per parameter: the other register peak beside the likelihood's) are known to the launch, so each instance is
// told them (assumptions on the arguments, not another text): the other families' branches of the body, the other parameter space's and
// the other optimisers' fold away, and with them the spilled registers the lone kernel's instances carry.  Instances exist for as many
// particle columns as the model has parameters (Pendulum 3, Particle 1, skid-steer 3, cart-pole 4: mpfb_limits refuses the rest).
struct MpfBatchArgs {
  MpfArgs a;                    // the shared fields; x, grad_norms and the optimiser slots are environment 0's; the per-call values are unused
  const MpfEnvIn *in;           // [B]
  float *prior_bwv;             // [B][4] in / out
  float *bw;                    // [B]: the bandwidth of this call, in (bw_fixed <= 0) / out
  float bw_fixed;               // > 0: every environment's bandwidth
  int gn_stride;
  const SkidLik *skl;           // [B] (DUST_MODEL_SKID_STEER)
  const CartLik *cpl;           // [B] (DUST_MODEL_CARTPOLE)
  const unsigned char *active;  // [B] or nullptr: everybody
};
// What the body text reads through `a`, for ONE environment: MpfArgs' member names.  The shared structs stay where the launch put them
// (references into the kernel's arguments, as AmppiEnvArgs keeps them: a local COPY of the whole argument block goes to scratch memory);
// the environment's own values are plain members, every array among them read at compile-time indices only.
struct MpfEnvArgs {
  const DevModel &dm;
  int Mp, P, ds, da, n_steps, log_space;
  float prior_bwv[4];
  float bw, obs_std;
  float past_obs[4], past_action[2], obs[4];
  const SkidLik *skl;
  const CartLik *cpl;
  const float *act_seq;
  float *x, *grad_norms, *phi_out;
  const OptArgs &opt;
  int t0;
  float *opt_s0, *opt_s1, *opt_s2;
};
__device__ __forceinline__ MpfEnvArgs mpf_env_view(const MpfBatchArgs &k, const int env) {
  const MpfArgs &g = k.a;
  const MpfEnvIn &in = k.in[env];
  const float *pb = k.prior_bwv + (size_t)env * 4;
  const size_t np = (size_t)env * (size_t)g.Mp * (size_t)g.P;
  return MpfEnvArgs{g.dm, g.Mp, g.P, g.ds, g.da, g.n_steps, g.log_space,
                    {pb[0], pb[1], pb[2], pb[3]},
                    k.bw_fixed > 0.f ? k.bw_fixed : k.bw[env], g.obs_std,
                    {in.past_obs[0], in.past_obs[1], in.past_obs[2], in.past_obs[3]},
                    {in.past_action[0], in.past_action[1]},
                    {in.obs[0], in.obs[1], in.obs[2], in.obs[3]},
                    k.skl + env, k.cpl + env, nullptr,
                    g.x + np, g.grad_norms + (size_t)env * (size_t)k.gn_stride, nullptr,
                    g.opt, in.t0,
                    g.opt_s0 ? g.opt_s0 + np : nullptr, g.opt_s1 ? g.opt_s1 + np : nullptr, g.opt_s2 ? g.opt_s2 + np : nullptr};
}
// a value that every lane of the workgroup holds alike, moved to scalar registers (the bits stay)
__device__ __forceinline__ float mpf_uniform(const float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ double mpf_uniform(const double v) {
  const long long b = __double_as_longlong(v);
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(b & 0xffffffffll));
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)((unsigned long long)b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | (unsigned long long)lo));
}
template <int P, bool CART, int MODEL, bool LOG, bool ADAM>
__global__ __launch_bounds__(1024) void mpf_optimize_batch_kernel(const MpfBatchArgs k) {
  const int env = (int)blockIdx.x;
  if (k.active && k.active[env] == 0) return;
  __builtin_assume(k.a.dm.model == MODEL);
  __builtin_assume(k.a.ds == (MODEL == DUST_MODEL_PENDULUM ? 2 : (MODEL == DUST_MODEL_SKID_STEER ? 5 : 4)));
  __builtin_assume(k.a.da == (MODEL == DUST_MODEL_PENDULUM || MODEL == DUST_MODEL_CARTPOLE ? 1 : 2));
  __builtin_assume(k.a.dm.log_space == (LOG ? 1 : 0));
  __builtin_assume(k.a.log_space == (LOG ? 1 : 0));
  __builtin_assume(ADAM ? k.a.opt.kind == DUST_OPT_ADAM : k.a.opt.kind != DUST_OPT_ADAM);
  const MpfEnvArgs a = mpf_env_view(k, env);
#define MPF_UNIFORM(v) mpf_uniform(v)
#include "mpf_body.inc"
#undef MPF_UNIFORM
  // (every lane has read prior_bwv and bw into registers ahead of a barrier when n_steps > 0; the barrier here covers n_steps = 0)
  wg_sync();
  if (threadIdx.x == 0) {
    float *pb = k.prior_bwv + (size_t)env * 4;
    _Pragma("unroll") for (int p = 0; p < 4; ++p) pb[p] = a.bw;
    k.bw[env] = a.bw;
  }
}

// ---- the rows form (dust_mpf_batch_set_hyper): every environment under its own lr, obs_std and bandwidth - the B trials of a sweep over
// the filter's settings in the launches of one update.  Instances of their own, as svmpc_sweep_kernel's are: the uniform instances above
// keep their text, argument block and registers.  Workgroup b loads rows[b] once (the row is workgroup-uniform and no kernel writes it:
// scalar loads); the view of its environment is mpf_env_view's with obs_std from the row and, for the optimiser, a copy of the shared
// options whose lr is the row's (88 bytes read at compile-time offsets: scalar registers - only the WHOLE argument block, whose model
// carries arrays, would go to scratch memory).  The bandwidth is always bw[env]: mpf_silverman_rows_kernel, just ahead on the same
// stream, has written the row's fixed value or Silverman's there.  The body is the same text.  Pendulum and Particle only.
struct MpfRowsArgs {
  MpfBatchArgs k;              // bw_fixed is 0
  const dust_mpf_hyper *rows;  // [B]
};
template <int P, int MODEL, bool LOG, bool ADAM>
__global__ __launch_bounds__(1024) void mpf_optimize_rows_kernel(const MpfRowsArgs kr) {
  const MpfBatchArgs &k = kr.k;
  const int env = (int)blockIdx.x;
  if (k.active && k.active[env] == 0) return;
  constexpr bool CART = false;
  __builtin_assume(k.a.dm.model == MODEL);
  __builtin_assume(k.a.ds == (MODEL == DUST_MODEL_PENDULUM ? 2 : 4));
  __builtin_assume(k.a.da == (MODEL == DUST_MODEL_PENDULUM ? 1 : 2));
  __builtin_assume(k.a.dm.log_space == (LOG ? 1 : 0));
  __builtin_assume(k.a.log_space == (LOG ? 1 : 0));
  __builtin_assume(ADAM ? k.a.opt.kind == DUST_OPT_ADAM : k.a.opt.kind != DUST_OPT_ADAM);
  const dust_mpf_hyper &row = kr.rows[env];
  OptArgs opt = k.a.opt;
  opt.lr = row.lr;
  const MpfArgs &g = k.a;
  const MpfEnvIn &in = k.in[env];
  const float *pb = k.prior_bwv + (size_t)env * 4;
  const size_t np = (size_t)env * (size_t)g.Mp * (size_t)g.P;
  const MpfEnvArgs a{g.dm, g.Mp, g.P, g.ds, g.da, g.n_steps, g.log_space,
                     {pb[0], pb[1], pb[2], pb[3]},
                     k.bw[env], row.obs_std,
                     {in.past_obs[0], in.past_obs[1], in.past_obs[2], in.past_obs[3]},
                     {in.past_action[0], in.past_action[1]},
                     {in.obs[0], in.obs[1], in.obs[2], in.obs[3]},
                     nullptr, nullptr, nullptr,
                     g.x + np, g.grad_norms + (size_t)env * (size_t)k.gn_stride, nullptr,
                     opt, in.t0,
                     g.opt_s0 ? g.opt_s0 + np : nullptr, g.opt_s1 ? g.opt_s1 + np : nullptr, g.opt_s2 ? g.opt_s2 + np : nullptr};
#define MPF_UNIFORM(v) mpf_uniform(v)
#include "mpf_body.inc"
#undef MPF_UNIFORM
  wg_sync();
  if (threadIdx.x == 0) {
    float *pbo = k.prior_bwv + (size_t)env * 4;
    _Pragma("unroll") for (int p = 0; p < 4; ++p) pbo[p] = a.bw;
    k.bw[env] = a.bw;
  }
}

// ---- the same optimisation spread over the chip -------------------------------------------------------------------------------------
// The single-workgroup kernel above is bound by the VALU issue rate of ONE compute unit: 2 M_p^2 pair terms of ~40 (mostly fp64)
// instructions per step - 40 us per step at M_p = 256, 815 us for the 20 steps of a filter update (profiles/round3_cfg5_kernel_stats.txt),
// longer than the control tick it runs beside.  Here ONE WAVE owns one particle i (4 waves per workgroup, M_p / 4 workgroups): its lanes
// stride over the other particles, the partial sums are combined by a fixed xor-shuffle tree in fp64 (reproducible), lane 0 adds the
// likelihood score and takes the optimiser step.  Per step the waves exchange the scores and the new particles through global memory
// (write-through stores, one arrival per wave on a counter sharded over 16 lines, one polling wave per workgroup) - two grid-wide
// hand-offs of ~3 us; the arithmetic per particle is the kernel's above, summed in another (fixed) order.
// The grid must be co-resident.  Protocol of tick2.hpp: a START BARRIER (workgroup 0 waits <= 200 us for every workgroup, then
// publishes go / abort; nothing is written before "go"), bounded waits, and a COMMIT - particles and optimiser moments are written
// behind the last hand-off by waves that find the time-out flag clear.  The host runs an aborted or uncommitted call on the kernel
// above, which needs no co-residency.
struct MpfGridArgs {
  MpfArgs a;
  float *xg;             // [2][Mp][P] particle generations (step parity)
  float *scg;            // [2][Mp][P] scores
  float *n2g;            // [n_steps][Mp] |phi_i|^2
  unsigned int *cnt;     // 16 lines of score arrivals | 16 lines of particle arrivals | start arrivals | go   (zeroed by the host per launch)
  unsigned int *status;  // [0] a wait timed out [1] calls that did not start [2] waves that did not commit
  int test;              // test hook: 1 abort at the start barrier, 2 "a wait gave up" before the last hand-off
};
enum { MPF_G_WAVES = 4, MPF_G_NT = 64 * MPF_G_WAVES, MPF_G_NSH = 16, MPF_G_LINE = 32 /* words: one 128-byte line per counter */ };

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int P, bool CART = false>
__global__ __launch_bounds__(MPF_G_NT) void mpf_optimize_grid_kernel(const MpfGridArgs g) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const MpfArgs &a = g.a;
  const int Mp = a.Mp, tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = (int)gridDim.x, b = (int)blockIdx.x, i = b * MPF_G_WAVES + wave;
  float *xs = sm;             // [Mp][P] current particles
  float *sc = xs + Mp * P;    // [Mp][P] scores
  float *nrm = sc + Mp * P;   // [Mp] squared norms
  unsigned int *sig = reinterpret_cast<unsigned int *>(nrm + Mp);
  unsigned int *cnt_sc = g.cnt, *cnt_x = g.cnt + MPF_G_NSH * MPF_G_LINE, *cnt_start = g.cnt + 2 * MPF_G_NSH * MPF_G_LINE, *go = cnt_start + MPF_G_LINE;
  unsigned int *tflag = g.status;
  const bool on = i < Mp, lead = on && lane == 0;
  // ---- start barrier
  if (tid == 0) {
    __hip_atomic_fetch_add(cnt_start, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned int v = 0u;
    if (b == 0) {
      const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
      bool ok = true;
      while ((int)(__hip_atomic_load(cnt_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - (unsigned int)G) < 0) {
        __builtin_amdgcn_s_sleep(2);
        if (__builtin_amdgcn_s_memrealtime() - t_start > 20000ull) {
          ok = false;
          break;
        }
      }
      ok = ok && __hip_atomic_load(tflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u && g.test != 1;
      if (!ok) __hip_atomic_fetch_add(g.status + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v = ok ? 1u : 2u;
      __hip_atomic_store(go, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      unsigned int spins = 0u;
      unsigned long long t_start = 0;
      for (;;) {
        v = __hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) break;
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 255u) == 0u) {
          const unsigned long long now = __builtin_amdgcn_s_memrealtime();
          if (!t_start) t_start = now;
          else if (now - t_start > DUST_SPIN_TIMEOUT_TICKS) {  // workgroup 0 never came
            __hip_atomic_store(tflag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v = 2u;
            break;
          }
        }
      }
    }
    sig[0] = v;
  }
  for (int t = tid; t < Mp * P; t += MPF_G_NT) xs[t] = a.x[t];
  wg_sync();
  if (sig[0] != 1u) return;
  for (int j = tid; j < Mp; j += MPF_G_NT) {
    float nn = 0.f;
    _Pragma("unroll") for (int p = 0; p < P; ++p) nn = nn + xs[j * P + p] * xs[j * P + p];
    nrm[j] = nn;
  }
  wg_sync();

  const float bw2 = (float)((double)a.bw * (double)a.bw);
  double inv_pbw[4], inv_pbw2[4];
  _Pragma("unroll") for (int p = 0; p < 4; ++p) {
    inv_pbw[p] = 1.0 / (double)a.prior_bwv[p < P ? p : 0];
    inv_pbw2[p] = inv_pbw[p] * inv_pbw[p];
  }
  const double inv_bw2 = 1.0 / ((double)a.bw * (double)a.bw), inv_obs2 = 1.0 / ((double)a.obs_std * (double)a.obs_std);
  float am[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f}, xn[4] = {0.f, 0.f, 0.f, 0.f};
  if (lead)
    _Pragma("unroll") for (int p = 0; p < P; ++p) {
      if (a.opt_s0) am[p] = a.opt_s0[i * P + p];
      if (a.opt_s1) av[p] = a.opt_s1[i * P + p];
      if (a.opt_s2) a2[p] = a.opt_s2[i * P + p];
    }
  // lanes [0, 16) of wave 0 wait for the arrivals of every particle's wave on their shard line
  auto poll = [&](unsigned int *lines, const unsigned int phase) {
    if (wave == 0 && lane < MPF_G_NSH) {
      const unsigned int target = (unsigned int)((Mp >> 4) + ((Mp & 15) > lane ? 1 : 0)) * phase;
      if (target) spin_until(lines + lane * MPF_G_LINE, target, tflag);
    }
    wg_sync();
  };
  auto arrive = [&](unsigned int *lines) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lead) __hip_atomic_fetch_add(lines + (i & 15) * MPF_G_LINE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };

  // likelihood score of this wave's particle (mpf.py:46-50, likelihoods.py:30-49): one model step and its Jacobian, on lane 0 - 2.5 us.
  // It depends on the particle alone, so the term of step it + 1 is computed behind the particle store of step it, under the hop.
  double glik[4] = {0, 0, 0, 0};
  auto lik = [&](const float *xp, const int step) {
    if (CART) {
      mpf_cart_score<P>(a.cpl, a.log_space, xp, inv_obs2, glik);
      return;
    }
    const float pa[2] = {a.act_seq ? a.act_seq[2 * step] : a.past_action[0], a.act_seq ? a.act_seq[2 * step + 1] : a.past_action[1]};
    if (a.dm.model == DUST_MODEL_SKID_STEER) {
      mpf_skid_score<P>(a.skl, a.log_space, xp, inv_obs2, glik);
      return;
    }
    float pred[4];
    for (int k = 0; k < 4; ++k) pred[k] = k < a.ds ? a.past_obs[k] : 0.f;
    const Coef cf = make_coef(a.dm, xp);
    if (a.dm.model == DUST_MODEL_PENDULUM) model_step<DUST_MODEL_PENDULUM>(a.dm, cf, pred, pa);
    else model_step<DUST_MODEL_PARTICLE>(a.dm, cf, pred, pa);
    double J[4][4];
    step_jacobian<P>(a.dm, a.past_obs, pa, xp, J);
    _Pragma("unroll") for (int p = 0; p < P; ++p) {
      double gl = 0.0;
      _Pragma("unroll") for (int k = 0; k < 4; ++k)
        if (k < a.ds) gl += J[k][p] * ((double)a.obs[k] - (double)pred[k]);
      glik[p] = gl * inv_obs2;
    }
  };
  if (lead) {
    float x0v[4] = {0.f, 0.f, 0.f, 0.f};
    _Pragma("unroll") for (int p = 0; p < P; ++p) x0v[p] = xs[i * P + p];
    lik(x0v, 0);
  }

  for (int it = 0; it < a.n_steps; ++it) {
    float xi[4] = {0.f, 0.f, 0.f, 0.f};
    if (on) {
      _Pragma("unroll") for (int p = 0; p < P; ++p) xi[p] = xs[i * P + p];
      // prior score (mpf.py:45), as in the kernel above
      double zs = 0.0, acc[4] = {0, 0, 0, 0};
      for (int k = lane; k < Mp; k += 64) {
        double q = 0.0;
        _Pragma("unroll") for (int p = 0; p < P; ++p) {
          const double z = ((double)xi[p] - (double)xs[k * P + p]) * inv_pbw[p];
          q += z * z;
        }
        const double w = (double)expf((float)(-0.5 * q));
        zs += w;
        _Pragma("unroll") for (int p = 0; p < P; ++p) acc[p] += w * ((double)xs[k * P + p] - (double)xi[p]);
      }
      zs = wave_sum_f64(zs);
      _Pragma("unroll") for (int p = 0; p < P; ++p) acc[p] = wave_sum_f64(acc[p]);
      if (lane == 0)
        _Pragma("unroll") for (int p = 0; p < P; ++p)
            st_sc1(g.scg + ((size_t)(it & 1) * Mp + i) * P + p, (float)(acc[p] / zs * inv_pbw2[p] + glik[p]));
    }
    arrive(cnt_sc);
    poll(cnt_sc, (unsigned int)(it + 1));
    for (int t = tid; t < Mp * P; t += MPF_G_NT) sc[t] = ld_sc1(g.scg + (size_t)(it & 1) * Mp * P + t);
    wg_sync();
    // kernel + phi (svgd.py:92-99, mpf.py:52-56), as in the kernel above
    if (on) {
      double gk[4] = {0, 0, 0, 0}, ks[4] = {0, 0, 0, 0};
      const float ni = nrm[i];
      for (int j = lane; j < Mp; j += 64) {
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
      _Pragma("unroll") for (int p = 0; p < P; ++p) {
        gk[p] = wave_sum_f64(gk[p]);
        ks[p] = wave_sum_f64(ks[p]);
      }
      if (lane == 0) {
        float ph[4] = {0.f, 0.f, 0.f, 0.f}, n2 = 0.f;
        _Pragma("unroll") for (int p = 0; p < P; ++p) {
          ph[p] = (float)(gk[p] * inv_bw2 + ks[p] / Mp);
          n2 += ph[p] * ph[p];
        }
        if (g.n2g) st_sc1(g.n2g + (size_t)it * Mp + i, n2);
        if (it == 0 && a.phi_out)
          _Pragma("unroll") for (int p = 0; p < P; ++p) a.phi_out[i * P + p] = ph[p];
        _Pragma("unroll") for (int p = 0; p < P; ++p) {
          xn[p] = opt_step(a.opt, xi[p], -ph[p], am[p], av[p], a2[p], (float)(a.t0 + it + 1));
          st_sc1(g.xg + ((size_t)((it + 1) & 1) * Mp + i) * P + p, xn[p]);
        }
      }
    }
    if (g.test == 2 && it == a.n_steps - 1 && b == G - 1 && tid == 0) __hip_atomic_store(tflag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    arrive(cnt_x);
    if (lead && it + 1 < a.n_steps) lik(xn, it + 1);
    poll(cnt_x, (unsigned int)(it + 1));
    if (it + 1 < a.n_steps) {
      for (int j = tid; j < Mp; j += MPF_G_NT) {
        float nn = 0.f;
        _Pragma("unroll") for (int p = 0; p < P; ++p) {
          const float v = ld_sc1(g.xg + ((size_t)((it + 1) & 1) * Mp + j) * P + p);
          xs[j * P + p] = v;
          nn = nn + v * v;
        }
        nrm[j] = nn;
      }
      wg_sync();
    }
  }
  // COMMIT: one look at the flag per workgroup, behind the last hand-off
  if (tid == 0) sig[1] = __hip_atomic_load(tflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  wg_sync();
  if (sig[1] != 0u) {
    if (lead) __hip_atomic_fetch_add(g.status + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (lead) {
    _Pragma("unroll") for (int p = 0; p < P; ++p) a.x[i * P + p] = xn[p];
    _Pragma("unroll") for (int p = 0; p < P; ++p) {
      if (a.opt_s0) a.opt_s0[i * P + p] = am[p];
      if (a.opt_s1) a.opt_s1[i * P + p] = av[p];
      if (a.opt_s2) a.opt_s2[i * P + p] = a2[p];
    }
  }
  if (b == 0 && a.grad_norms)  // ||phi|| of every step: the per-particle squares in particle order
    for (int it = tid; it < a.n_steps; it += MPF_G_NT) {
      double n2 = 0.0;
      for (int j = 0; j < Mp; ++j) n2 += (double)ld_sc1(g.n2g + (size_t)it * Mp + j);
      a.grad_norms[it] = sqrtf((float)n2);
    }
}

// ---- the same grid with a DATA-POLLED exchange (the default; DUST_MPF_POLL=0 switches it off) ------------------------------------------
// Rows cross as 16-byte pieces {tag, v0, v1, tag}: the owner's lane 0 writes each with ONE write-through store; every lane re-loads
// the pieces of ITS keys (sc1 loads, all in flight at once) until both tag words are this step's.  A piece is written by one aligned
// 16-byte store and the tag sits in its first AND last word, so a reader that finds both has the words between them.  No counters, no
// polling wave, no LDS copy, no workgroup barrier in the loop - a hop costs one store-to-load round trip (2.4 us against 5.0 for
// counter + data in tools/allgather_probe.hip); keys live in registers (KC = 4 / 8 / 16 per lane).  Tags are unique per launch and step
// (launch number x 8192 + 2 step + 1 | 2, kept to bit patterns of normal floats), pieces alternate between two buffers by step
// parity: an owner overwrites the piece of two steps ago only after it has seen every other owner's piece of the step in between,
// i.e. after everybody finished reading the old one.  The likelihood term of the NEXT step is computed behind the particle store,
// under the hop.  Start barrier (monotonic counter, no memset per call), bounded waits, commit and fallback as above.
// A trap met on the way: `.y` / `.z` of the loaded vector were folded to `.x` by the compiler inside the `x == tag && w == tag` branch
// (ISA: v_mov v3, v2) - the words are taken out through memcpy.  (Everything below the one-lane start code is derived from opaque
// copies of the arguments; that was part of the same rewrite and is kept.)
struct MpfPollArgs {
  MpfArgs a;
  float *xpc;            // [2][Mp][NP + 1] pieces: NP pieces of particle values, then {tag, |phi_i|^2, 0, tag}
  float *scp;            // [2][Mp][NP] pieces of scores
  unsigned int *cnt;     // [0] start arrivals (monotonic over launches) [32] go word = launch << 2 | 1 (go) / 2 (abort)
  unsigned int *status;
  unsigned int tag0, seq;
  int test;
};

template <int P, int KC, bool CART = false>
__global__ __launch_bounds__(MPF_G_NT) void mpf_optimize_poll_kernel(const MpfPollArgs g) {
  constexpr int NP = (P + 1) / 2, NX = NP + 1;
  __shared__ unsigned int sig[2];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  // ---- start barrier (one lane per workgroup)
  if (tid == 0) {
    const int G = (int)gridDim.x;
    unsigned int *cnt_start = g.cnt, *go = g.cnt + MPF_G_LINE;
    __hip_atomic_fetch_add(cnt_start, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned int v = 0u;
    if (blockIdx.x == 0) {
      const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
      bool ok = true;
      while ((int)(__hip_atomic_load(cnt_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - g.seq * (unsigned int)G) < 0) {
        __builtin_amdgcn_s_sleep(2);
        if (__builtin_amdgcn_s_memrealtime() - t_start > 20000ull) {
          ok = false;
          break;
        }
      }
      ok = ok && __hip_atomic_load(g.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u && g.test != 1;
      if (!ok) __hip_atomic_fetch_add(g.status + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v = ok ? 1u : 2u;
      __hip_atomic_store(go, (g.seq << 2) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      unsigned int spins = 0u;
      unsigned long long t_start = 0;
      for (;;) {
        const unsigned int w = __hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((w >> 2) == g.seq) {
          v = w & 3u;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 255u) == 0u) {
          const unsigned long long now = __builtin_amdgcn_s_memrealtime();
          if (!t_start) t_start = now;
          else if (now - t_start > DUST_SPIN_TIMEOUT_TICKS) {
            __hip_atomic_store(g.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v = 2u;
            break;
          }
        }
      }
    }
    sig[0] = v;
  }
  wg_sync();
  if (sig[0] != 1u) return;
  // everything below is derived AFTER the barrier from opaque copies of the arguments (nothing scalar lives across the start code)
  const MpfArgs &a = g.a;
  const int Mp = opaque_s(a.Mp), wave = opaque_s(__builtin_amdgcn_readfirstlane(tid >> 6));
  const int G = (int)gridDim.x, b = (int)blockIdx.x, i = b * MPF_G_WAVES + wave;
  unsigned int *tflag = g.status;
  const unsigned int tag0 = (unsigned int)opaque_s((int)g.tag0);
  const bool on = i < Mp;
  const int io = on ? i : 0;
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(g.xpc, 0, 2 * Mp * NX * 16, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(g.scp, 0, 2 * Mp * NP * 16, 0x00020000);
  typedef unsigned int v4u_t __attribute__((ext_vector_type(4)));
  float xk[KC][P], sk[KC][P], nk[KC], n2k[KC];
  // poll the pieces of this lane's keys until both tag words match; the values go straight to their registers (SCORES: sk; else xk
  // and, from the extra piece of a particle row, n2k); `done` is a bit mask over (key, piece)
  auto poll = [&](auto scores, const __amdgpu_buffer_rsrc_t r, const int parity, const unsigned int tag) {
    constexpr bool SC = decltype(scores)::value;
    constexpr int RS = SC ? NP : NX;  // pieces per row
    unsigned long long done = 0ull;
#pragma unroll
    for (int c = 0; c < KC; ++c)
      if (!(lane + 64 * c < Mp)) done |= ((1ull << RS) - 1ull) << (c * RS);  // (nothing to see)
    constexpr unsigned long long all = KC * RS >= 64 ? ~0ull : ((1ull << (KC * RS)) - 1ull);
    unsigned int spins = 0u;
    unsigned long long t0 = 0;
    for (;;) {
#pragma unroll
      for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int q = 0; q < RS; ++q)
          if (!((done >> (c * RS + q)) & 1ull)) {
            const v4u_t t = __builtin_amdgcn_raw_buffer_load_b128(r, ((parity * Mp + lane + 64 * c) * RS + q) * 16, 0, 16);
            unsigned int w[4];
            __builtin_memcpy(w, &t, sizeof w);
            if (w[0] == tag && w[3] == tag) {
              const float v0 = __builtin_bit_cast(float, w[1]), v1 = __builtin_bit_cast(float, w[2]);
              if (SC) {
                sk[c][2 * q < P ? 2 * q : 0] = v0;
                if (2 * q + 1 < P) sk[c][2 * q + 1] = v1;
              } else if (q < NP) {
                xk[c][2 * q < P ? 2 * q : 0] = v0;
                if (2 * q + 1 < P) xk[c][2 * q + 1] = v1;
              } else {
                n2k[c] = v0;
              }
              done |= 1ull << (c * RS + q);
            }
          }
      if (!__any(done != all ? 1 : 0)) break;
      __builtin_amdgcn_s_sleep(1);
      if ((++spins & 63u) == 0u) {
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        if (!t0) t0 = now;
        else if (now - t0 > DUST_SPIN_TIMEOUT_TICKS || __hip_atomic_load(tflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
          __hip_atomic_store(tflag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
    }
  };
  auto put = [&](const __amdgpu_buffer_rsrc_t r, const int piece, const unsigned int tag, const float v0, const float v1) {
    const v4u_t t = {tag, __builtin_bit_cast(unsigned int, v0), __builtin_bit_cast(unsigned int, v1), tag};
    __builtin_amdgcn_raw_buffer_store_b128(t, r, piece * 16, 0, 16);
  };
  auto norms = [&]() {
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      float nn = 0.f;
      _Pragma("unroll") for (int p = 0; p < P; ++p) nn = nn + xk[c][p] * xk[c][p];
      nk[c] = nn;
    }
  };
  const double inv_obs2 = 1.0 / ((double)a.obs_std * (double)a.obs_std);
  double glik[4] = {0, 0, 0, 0};
  auto lik = [&](const float *xp, const int step) {
    if (CART) {
      mpf_cart_score<P>(a.cpl, a.log_space, xp, inv_obs2, glik);
      return;
    }
    const float pa[2] = {a.act_seq ? a.act_seq[2 * step] : a.past_action[0], a.act_seq ? a.act_seq[2 * step + 1] : a.past_action[1]};
    if (a.dm.model == DUST_MODEL_SKID_STEER) {
      mpf_skid_score<P>(a.skl, a.log_space, xp, inv_obs2, glik);
      return;
    }
    float pred[4];
    for (int k = 0; k < 4; ++k) pred[k] = k < a.ds ? a.past_obs[k] : 0.f;
    const Coef cf = make_coef(a.dm, xp);
    if (a.dm.model == DUST_MODEL_PENDULUM) model_step<DUST_MODEL_PENDULUM>(a.dm, cf, pred, pa);
    else model_step<DUST_MODEL_PARTICLE>(a.dm, cf, pred, pa);
    double J[4][4];
    step_jacobian<P>(a.dm, a.past_obs, pa, xp, J);
    _Pragma("unroll") for (int p = 0; p < P; ++p) {
      double gl = 0.0;
      _Pragma("unroll") for (int k = 0; k < 4; ++k)
        if (k < a.ds) gl += J[k][p] * ((double)a.obs[k] - (double)pred[k]);
      glik[p] = gl * inv_obs2;
    }
  };
  float xi[4] = {0.f, 0.f, 0.f, 0.f};
  _Pragma("unroll") for (int p = 0; p < P; ++p) xi[p] = a.x[io * P + p];
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const int k = lane + 64 * c;
    _Pragma("unroll") for (int p = 0; p < P; ++p) xk[c][p] = k < Mp ? a.x[k * P + p] : 0.f;
    n2k[c] = 0.f;
  }
  norms();
  const float bw2 = (float)((double)a.bw * (double)a.bw);
  double inv_pbw[4], inv_pbw2[4];
  _Pragma("unroll") for (int p = 0; p < 4; ++p) {
    inv_pbw[p] = 1.0 / (double)a.prior_bwv[p < P ? p : 0];
    inv_pbw2[p] = inv_pbw[p] * inv_pbw[p];
  }
  const double inv_bw2 = 1.0 / ((double)a.bw * (double)a.bw);
  float am[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
  if (on)
    _Pragma("unroll") for (int p = 0; p < P; ++p) {
      if (a.opt_s0) am[p] = a.opt_s0[io * P + p];
      if (a.opt_s1) av[p] = a.opt_s1[io * P + p];
      if (a.opt_s2) a2[p] = a.opt_s2[io * P + p];
    }
  lik(xi, 0);

  for (int it = 0; it < a.n_steps; ++it) {
    const unsigned int tag_s = 0x40000000u | ((tag0 + 2u * (unsigned int)it + 1u) & 0x3fffffffu), tag_x = 0x40000000u | ((tag0 + 2u * (unsigned int)it + 2u) & 0x3fffffffu);
    {
      double zs = 0.0, acc[4] = {0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < KC; ++c)
        if (lane + 64 * c < Mp) {
          double q = 0.0;
          _Pragma("unroll") for (int p = 0; p < P; ++p) {
            const double z = ((double)xi[p] - (double)xk[c][p]) * inv_pbw[p];
            q += z * z;
          }
          const double w = (double)expf((float)(-0.5 * q));
          zs += w;
          _Pragma("unroll") for (int p = 0; p < P; ++p) acc[p] += w * ((double)xk[c][p] - (double)xi[p]);
        }
      zs = wave_sum_f64(zs);
      _Pragma("unroll") for (int p = 0; p < P; ++p) acc[p] = wave_sum_f64(acc[p]);
      float sv[4] = {0.f, 0.f, 0.f, 0.f};
      _Pragma("unroll") for (int p = 0; p < P; ++p) sv[p] = (float)(acc[p] / zs * inv_pbw2[p] + glik[p]);
      if (on && lane == 0)
#pragma unroll
        for (int q = 0; q < NP; ++q) put(rs_s, ((it & 1) * Mp + i) * NP + q, tag_s, sv[2 * q], sv[2 * q + 1]);
    }
    poll(std::true_type{}, rs_s, it & 1, tag_s);
    float xn[4] = {0.f, 0.f, 0.f, 0.f};
    {
      double gk[4] = {0, 0, 0, 0}, ks[4] = {0, 0, 0, 0};
      float ni = 0.f;
      _Pragma("unroll") for (int p = 0; p < P; ++p) ni = ni + xi[p] * xi[p];
#pragma unroll
      for (int c = 0; c < KC; ++c)
        if (lane + 64 * c < Mp) {
          float dot = xi[0] * xk[c][0];
          _Pragma("unroll") for (int q = 1; q < P; ++q) dot = fmaf(xi[q], xk[c][q], dot);
          float q = (nk[c] + (-2.0f * dot)) + ni;
          q = fmaxf(q, 0.f);
          const double k = (double)expf(((-q) / bw2) / 2.0f);
          _Pragma("unroll") for (int p = 0; p < P; ++p) {
            gk[p] -= k * ((double)xi[p] - (double)xk[c][p]);
            ks[p] += k * (double)sk[c][p];
          }
        }
      _Pragma("unroll") for (int p = 0; p < P; ++p) {
        gk[p] = wave_sum_f64(gk[p]);
        ks[p] = wave_sum_f64(ks[p]);
      }
      float ph[4] = {0.f, 0.f, 0.f, 0.f}, n2 = 0.f;
      _Pragma("unroll") for (int p = 0; p < P; ++p) {
        ph[p] = (float)(gk[p] * inv_bw2 + ks[p] / Mp);
        n2 += ph[p] * ph[p];
      }
      _Pragma("unroll") for (int p = 0; p < P; ++p)
        xn[p] = opt_step(a.opt, xi[p], -ph[p], am[p], av[p], a2[p], (float)(a.t0 + it + 1));
      if (on && lane == 0) {
        const int row = (((it + 1) & 1) * Mp + i) * NX;
#pragma unroll
        for (int q = 0; q < NP; ++q) put(rs_x, row + q, tag_x, xn[2 * q], xn[2 * q + 1]);
        put(rs_x, row + NP, tag_x, n2, 0.f);
        if (it == 0 && a.phi_out)
          _Pragma("unroll") for (int p = 0; p < P; ++p) a.phi_out[i * P + p] = ph[p];
      }
    }
    _Pragma("unroll") for (int p = 0; p < P; ++p) xi[p] = xn[p];
    if (it + 1 < a.n_steps) lik(xi, it + 1);  // (under the hop)
    if (g.test == 2 && it == a.n_steps - 1 && b == G - 1 && tid == 0) __hip_atomic_store(tflag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    {
      poll(std::false_type{}, rs_x, (it + 1) & 1, tag_x);
      double n2s = 0.0;
#pragma unroll
      for (int c = 0; c < KC; ++c)
        if (lane + 64 * c < Mp) n2s += (double)n2k[c];
      norms();
      if (i == 0 && a.grad_norms) {
        n2s = wave_sum_f64(n2s);
        if (lane == 0) a.grad_norms[it] = sqrtf((float)n2s);
      }
    }
  }
  const unsigned int fl = __builtin_amdgcn_readfirstlane(__hip_atomic_load(tflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  if (!on || lane != 0) return;
  if (fl != 0u) {
    __hip_atomic_fetch_add(g.status + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  _Pragma("unroll") for (int p = 0; p < P; ++p) a.x[i * P + p] = xi[p];
  _Pragma("unroll") for (int p = 0; p < P; ++p) {
    if (a.opt_s0) a.opt_s0[i * P + p] = am[p];
    if (a.opt_s1) a.opt_s1[i * P + p] = av[p];
    if (a.opt_s2) a.opt_s2[i * P + p] = a2[p];
  }
}

struct MpfBw {
  float v[4];
};
__global__ void mpf_log_prob_kernel(const float *x, const float *means, int n, int K, int P, const MpfBw bw, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double mx = -INFINITY;
  for (int k = 0; k < K; ++k) {
    double q = 0.0;
    for (int p = 0; p < P; ++p) {
      const double z = ((double)x[i * P + p] - (double)means[k * P + p]) / (double)bw.v[p];
      q += z * z;
    }
    mx = fmax(mx, -0.5 * q);
  }
  double zs = 0.0;
  for (int k = 0; k < K; ++k) {
    double q = 0.0;
    for (int p = 0; p < P; ++p) {
      const double z = ((double)x[i * P + p] - (double)means[k * P + p]) / (double)bw.v[p];
      q += z * z;
    }
    zs += exp(-0.5 * q - mx);
  }
  double ld = 0.0;
  for (int p = 0; p < P; ++p) ld += log((double)bw.v[p]);
  out[i] = (float)(mx + log(zs) - log((double)K) - ld - 0.5 * P * log(2.0 * M_PI));
}

// mpf.prior.sample([n]): categorical over the M_p components (uniform), then N(mean, bw^2 I)
__global__ void mpf_sample_kernel(const float *means, int K, int P, const MpfBw bw, uint64_t seed, int n, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t r[4];
  philox4x32_10((uint32_t)i, 0x6d7066u, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const int k = (int)(((unsigned long long)r[0] * (unsigned long long)K) >> 32);
  float z[4];
  philox_normal4(seed, (uint32_t)i, 0x6d7067u, 1u, 0u, z);
  for (int p = 0; p < P; ++p) out[i * P + p] = means[k * P + p] + bw.v[p] * z[p];
}

// mpf_sample_kernel with n = 1 for B filters in one launch (the "single" mode of a batched dual tick): lane b draws row 0 of
// dust_mpf_prior_sample(filter b, 1, seeds[b]) - the same counters, the same operations in the same order - into out[b * P]
__global__ void mpf_sample_batch_kernel(const float *means, int K, int P, const float *bwv, const uint64_t *seeds, int B, float *out, const unsigned char *active) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= B || (active && active[env] == 0)) return;
  const uint64_t seed = seeds[env];
  uint32_t r[4];
  philox4x32_10(0u, 0x6d7066u, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const int k = (int)(((unsigned long long)r[0] * (unsigned long long)K) >> 32);
  float z[4];
  philox_normal4(seed, 0u, 0x6d7067u, 1u, 0u, z);
  const float *mu = means + ((size_t)env * (size_t)K + (size_t)k) * (size_t)P;
#pragma unroll
  for (int p = 0; p < 4; ++p)
    if (p < P) out[(size_t)env * P + p] = mu[p] + bwv[(size_t)env * 4 + p] * z[p];
}

// Sigma points of mpf.prior for a Merwe scaled unscented transform (MultiDISCO._sigma_rollout, disco.py:240-251, on the prior that
// MPF.update_prior builds, mpf.py:26-38): the mixture's mean and variance (MixtureSameFamily.mean / .variance, uniform weights),
//     mean_p = sum_j x_jp / Mp          var_p = bw_p^2 + sum_j (x_jp - mean_p)^2 / Mp
// and, the covariance being diagonal (so that the reference's upper Cholesky factor is an element-wise square root), the 2P + 1 points
// of MerweScaledUTF.compute_sigma_points (utf.py:93-123) with scale = lambda + n:
//     row 0: mean          row 1 + p: mean + sqrt(scale var_p) e_p          row 1 + P + p: mean - sqrt(scale var_p) e_p
// written `reps` times in a row ([reps][2P + 1][P]: one set per SVGD iteration of the tick that consumes them).  One workgroup; sums in
// double, per-lane strided partials then an LDS tree - a fixed order, the same bits for the same particles.  Mp <= 1024, P <= 4.
__device__ __forceinline__ void mpf_sigma_points_body(const float *x, const int Mp, const int P, const MpfBw &bw, const float scale, const int reps,
                                                      float *out) {
  __shared__ double red[4][256];
  __shared__ double stat[2][4];  // mean, variance
  const int tid = threadIdx.x;
  auto block_sum = [&](const double (&v)[4], double *dst) {
#pragma unroll
    for (int p = 0; p < 4; ++p) red[p][tid] = v[p];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o)
#pragma unroll
        for (int p = 0; p < 4; ++p) red[p][tid] += red[p][tid + o];
      __syncthreads();
    }
    if (tid < 4) dst[tid] = red[tid][0];
    __syncthreads();
  };
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = tid; j < Mp; j += 256)
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (p < P) acc[p] += (double)x[(size_t)j * P + p];
  block_sum(acc, stat[0]);
  double mean[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    mean[p] = stat[0][p] / (double)Mp;
    acc[p] = 0.0;
  }
  for (int j = tid; j < Mp; j += 256)
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (p < P) {
        const double d = (double)x[(size_t)j * P + p] - mean[p];
        acc[p] += d * d;
      }
  block_sum(acc, stat[1]);
  const int pts = 2 * P + 1, per = pts * P;
  for (int i = tid; i < reps * per; i += 256) {
    const int e = i % per, row = e / P, p = e - row * P;
    const float mu = (float)mean[p];
    float v = mu;
    if (row >= 1) {
      const int q = row <= P ? row - 1 : row - 1 - P;  // the axis this point moves along
      if (q == p) {
        const double var = (double)bw.v[p] * (double)bw.v[p] + stat[1][p] / (double)Mp;
        const float u = (float)sqrt((double)scale * var);
        v = row <= P ? mu + u : mu - u;
      }
    }
    out[i] = v;
  }
}
__global__ __launch_bounds__(256) void mpf_sigma_points_kernel(const float *x, const int Mp, const int P, const MpfBw bw, const float scale, const int reps,
                                                               float *out) {
  mpf_sigma_points_body(x, Mp, P, bw, scale, reps, out);
}
// ... of B filters' priors in one launch, one workgroup per environment: particles [B][Mp][P], prior bandwidths [B][4] in device memory,
// one set of points per environment into the batched tick's parameter rows [B][2P + 1][P]
__global__ __launch_bounds__(256) void mpf_sigma_points_batch_kernel(const float *x, const int Mp, const int P, const float *bwv, const float scale, float *out,
                                                                     const unsigned char *active) {
  const int env = (int)blockIdx.x;
  if (active && active[env] == 0) return;
  const float *b = bwv + (size_t)env * 4;
  const MpfBw bw{{b[0], b[1], b[2], b[3]}};
  mpf_sigma_points_body(x + (size_t)env * (size_t)Mp * (size_t)P, Mp, P, bw, scale, 1, out + (size_t)env * (size_t)(2 * P + 1) * (size_t)P);
}

// KDEpy 1.1.0 `silvermans_rule` of the pooled particle values (mpf.py:68-73: `silvermans_rule(self.x.view(-1, 1))`; restated in
// oracle/ref_shim.py - third party, parity unpinned) on the device: sigma = min(std(ddof = 1), IQR / 1.349) (the positive one when one
// of them is 0), bw = sigma (3 n / 4)^(-1/5), times bw_scale; 1 when n = 1 or both spreads are 0.  float64 throughout, as the host rule
// (numpy on the float64 copy): mean and squared deviations in two passes, the quartiles by numpy's linear interpolation
// (`a + (b - a) t`, from the upper end when t >= 1/2) between the order statistics around q (n - 1), which are found by RANK (every lane
// counts the values below its own: n <= 4096 values, n^2 comparisons - 0.26 M at 256 particles x 2 parameters).  One workgroup.
__device__ __forceinline__ void mpf_silverman_body(const float *x, const int n, const float bw_scale, float *out) {
  extern __shared__ float sv_x[];  // [n]
  __shared__ double red[16];
  __shared__ double quart[4];      // order statistics floor / ceil of the two quartile positions
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += 1024) sv_x[i] = x[i];
  __syncthreads();
  auto block_sum = [&](double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < 16; ++w) r += red[w];
    return r;
  };
  double acc = 0.0;
  for (int i = tid; i < n; i += 1024) acc += (double)sv_x[i];
  const double mean = block_sum(acc) / (double)n;
  acc = 0.0;
  for (int i = tid; i < n; i += 1024) {
    const double d = (double)sv_x[i] - mean;
    acc += d * d;
  }
  const double ss = block_sum(acc);
  const double p25 = 0.25 * (double)(n - 1), p75 = 0.75 * (double)(n - 1);
  const int k[4] = {(int)floor(p25), min(n - 1, (int)floor(p25) + 1), (int)floor(p75), min(n - 1, (int)floor(p75) + 1)};
  for (int i = tid; i < n; i += 1024) {
    const float v = sv_x[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float u = sv_x[j];
      rank += (u < v || (u == v && j < i)) ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (rank == k[q]) quart[q] = (double)v;
  }
  __syncthreads();
  if (tid == 0) {
    float bw = 1.0f;
    if (n > 1) {
      const double sd = sqrt(ss / (double)(n - 1));
      auto lerp = [](const double a, const double b, const double t) { return t >= 0.5 ? b - (b - a) * (1.0 - t) : a + (b - a) * t; };
      const double q25 = lerp(quart[0], quart[1], p25 - floor(p25)), q75 = lerp(quart[2], quart[3], p75 - floor(p75));
      const double iqr = (q75 - q25) / 1.3489795003921634;
      double sigma = fmin(sd, iqr);
      if (!(sigma > 0.0)) sigma = fmax(sd, iqr);
      if (sigma > 0.0) bw = (float)(sigma * pow((double)n * 3.0 / 4.0, -0.2) * (double)bw_scale);
      else bw = (float)(1.0 * (double)bw_scale);
    } else {
      bw = (float)(1.0 * (double)bw_scale);
    }
    out[0] = bw;
  }
}
__global__ __launch_bounds__(1024) void mpf_silverman_kernel(const float *x, const int n, const float bw_scale, float *out) {
  mpf_silverman_body(x, n, bw_scale, out);
}
// ... of B filters' particles x [B][n] in one launch, one workgroup per environment: bw[b], where the batched filter kernel reads it
__global__ __launch_bounds__(1024) void mpf_silverman_batch_kernel(const float *x, const int n, const float bw_scale, float *bw, const unsigned char *active) {
  const int env = (int)blockIdx.x;
  if (active && active[env] == 0) return;
  mpf_silverman_body(x + (size_t)env * (size_t)n, n, bw_scale, bw + env);
}
// the rows form (dust_mpf_batch_set_hyper), launched ahead of every update while rows are set: workgroup b writes its row's fixed
// bandwidth and skips the order statistics, or runs Silverman's rule under its row's bw_scale (the branch is workgroup-uniform)
__global__ __launch_bounds__(1024) void mpf_silverman_rows_kernel(const float *x, const int n, const dust_mpf_hyper *rows, float *bw, const unsigned char *active) {
  const int env = (int)blockIdx.x;
  if (active && active[env] == 0) return;
  const float fixed = rows[env].bw;
  if (fixed > 0.f) {
    if (threadIdx.x == 0) bw[env] = fixed;
    return;
  }
  mpf_silverman_body(x + (size_t)env * (size_t)n, n, rows[env].bw_scale, bw + env);
}

}  // namespace dust

struct dust_mpf {
  dust_mpf_config cfg;
  int Mp, P;
  hipStream_t stream;
  DevBuf<float> x, gn, phi, tmp;
  dust_optim_config opt;       // dust_mpf_set_optimizer(_ex); plain SGD at cfg.lr until then
  int opt_t;                   // steps taken so far
  DevBuf<float> opt_s[3];      // state slots [Mp][P] or empty
  DevBuf<uint32_t> grid_bits;
  int nx, ny;
  float off_x, off_y;
  float prior_bwv[4];          // per parameter dimension; equal once update_prior(bw) has run (mpf.py:85)
  float loc[5], past_obs[5], past_action[2];  // (five wide: the skid-steer state)
  bool have_past;
  dust::SkidModel skid;     // DUST_MODEL_SKID_STEER: parameters and wheel-speed bounds (dust_mpf_set_skid_steer)
  dust::SkidLik skl_host;   // ... the likelihood's per-call constants (mpf_skid_prepare) and their device copy
  DevBuf<dust::SkidLik> skl_dev;
  dust::CartModel cart;     // DUST_MODEL_CARTPOLE: the seven parameters (dust_mpf_set_cartpole; its cost fields stay unused)
  dust::CartLik cpl_host;   // ... the likelihood's per-call constants (mpf_cart_prepare) and their device copy
  DevBuf<dust::CartLik> cpl_dev;
  // control-channel noise of the one-step prediction (model_cfg.ctrl_noise; particle.py:145-148 through likelihoods.py:30-46)
  std::vector<float> cz;    // recorded draws [n][da] (dust_mpf_set_ctrl_noise), consumed one per SVGD step
  size_t cz_next;
  std::mt19937_64 rng;      // draws once the recorded ones are used up (seeded on first use: rng_seeded)
  bool rng_seeded;
  DevBuf<float> act_seq;    // device: effective action per step of the current launch [steps][2]
  // the multi-workgroup form of the optimisation (mpf_optimize_grid_kernel): exchange buffers, counters, status; lazily allocated
  DevBuf<float> gbuf;     // xg [2][Mp][P] | scg [2][Mp][P] | n2g [gsteps][Mp]
  DevBuf<unsigned int> gcnt;  // counters (zeroed per launch) followed by the 4 status words
  int gsteps;             // rows of n2g allocated
  DevBuf<float> pbuf;     // data-polled form (experimental): particle pieces | score pieces
  DevBuf<unsigned int> pcnt;  // ... its start counter and go word (monotonic over launches)
  unsigned int pseq;
  PinBuf<float> hpin;     // pinned host staging: gradient norms [4096] + status words (unsigned, at hpin + 4096)
  bool grid_banned;       // a wait of the grid form timed out once (device shared with another process): single-workgroup kernel from then on
  long long n_grid, n_grid_fallback;
  // development switches and test hooks, read ONCE by dust_mpf_create (mpf_env_read): atoi of the value
  struct {
    int grid;       // DUST_MPF_GRID (-1: unset)
    int poll;       // DUST_MPF_POLL (-1: unset)
    int grid_test;  // DUST_MPF_GRID_TEST (0: unset)
  } env;
};

static float clampf_host(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }  // (common.hpp clampf, for the host)
static int mpf_env_int(const char *name, int unset) {
  const char *v = getenv(name);
  return v ? atoi(v) : unset;
}
static void mpf_env_read(dust_mpf *m) {
  m->env.grid = mpf_env_int("DUST_MPF_GRID", -1);
  m->env.poll = mpf_env_int("DUST_MPF_POLL", -1);
  m->env.grid_test = mpf_env_int("DUST_MPF_GRID_TEST", 0);
}

static DevModel mpf_dev_model(const dust_mpf *m) {
  dust_config g = m->cfg.model_cfg;
  g.params_log_space = m->cfg.log_space;
  return make_dev_model(g, m->P, MapView{m->grid_bits, m->nx, m->ny, m->off_x, m->off_y});
}

extern "C" void dust_mpf_destroy(dust_mpf *m) {
  if (!m) return;
  (void)hipSetDevice(m->cfg.device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  const hipStream_t stream = m->stream;
  delete m;  // (memory first, then the stream it was used on - the order this function always had)
  if (stream) (void)hipStreamDestroy(stream);
}

extern "C" int dust_mpf_create(const dust_mpf_config *cfg, const float *init_particles, const float *initial_obs, dust_mpf **out) {
  if (!cfg || !init_particles || !initial_obs || !out) return fail(DUST_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->abi_version != DUST_ABI_VERSION) return fail(DUST_ERR_INVALID, "ABI version mismatch");
  if (cfg->n_particles < 1 || cfg->n_particles > 1024) return fail(DUST_ERR_UNSUPPORTED, "MPF supports 1..1024 particles (one workgroup)");
  if (cfg->dim_p < 1 || cfg->dim_p > 4) return fail(DUST_ERR_INVALID, "dim_p must be 1..4");
  if (!(cfg->init_bw > 0.f)) return fail(DUST_ERR_INVALID, "init_bw must be > 0 (the host layer evaluates bw_silverman)");
  if (cfg->model_cfg.model != DUST_MODEL_PENDULUM && cfg->model_cfg.model != DUST_MODEL_PARTICLE && cfg->model_cfg.model != DUST_MODEL_SKID_STEER &&
      cfg->model_cfg.model != DUST_MODEL_CARTPOLE)
    return fail(DUST_ERR_UNSUPPORTED, "MPF's one-step prediction and its Jacobian exist for the Pendulum, Particle, SkidSteerRobot and CartPoleModel models only");
  if (cfg->model_cfg.model == DUST_MODEL_CARTPOLE) {
    if (cfg->dim_s != 4 || cfg->dim_a != 1) return fail(DUST_ERR_INVALID, "the cart-pole model has dim_s = 4, dim_a = 1");
    if (!(cfg->model_cfg.dt > 0.0)) return fail(DUST_ERR_INVALID, "the cart-pole model needs model_cfg.dt > 0 (base.py:33)");
  }
  if (cfg->model_cfg.model == DUST_MODEL_SKID_STEER) {
    if (cfg->dim_s != 5 || cfg->dim_a != 2) return fail(DUST_ERR_INVALID, "the skid-steer model has dim_s = 5, dim_a = 2");
    if (cfg->dim_p > 3) return fail(DUST_ERR_INVALID, "the skid-steer model has three parameters: dim_p must be 1..3");
    if (!(cfg->model_cfg.dt > 0.0)) return fail(DUST_ERR_INVALID, "the skid-steer model needs model_cfg.dt > 0 (SkidSteerRobot(delta_t=) has no default)");
  }
  if (!(cfg->obs_std > 0.f)) return fail(DUST_ERR_INVALID, "obs_std must be > 0");
  if (cfg->model_cfg.model == DUST_MODEL_PARTICLE && cfg->model_cfg.control_type != DUST_CONTROL_ACCELERATION)
    return fail(DUST_ERR_UNSUPPORTED, "MPF over Particle(control_type='velocity'): the mass does not enter that model's step (particle.py:152-153), there is nothing to filter");
  if (cfg->model_cfg.model != DUST_MODEL_PARTICLE && cfg->model_cfg.ctrl_noise)
    return fail(DUST_ERR_UNSUPPORTED, "ctrl_noise is a Particle field (particle.py:145-148)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(DUST_ERR_NO_DEVICE, "no HIP device: libdust_amd has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(DUST_ERR_NO_DEVICE, "device %d of %d", cfg->device, ndev);
  HIP_TRY(hipSetDevice(cfg->device));
  dust_mpf *m = new (std::nothrow) dust_mpf();
  if (!m) return fail(DUST_ERR_HIP, "out of host memory");
  m->cfg = *cfg;
  m->opt = optim_plain(DUST_OPT_SGD, cfg->lr, 0.f, 0.f, 0.f);
  m->Mp = cfg->n_particles;
  m->P = cfg->dim_p;
  mpf_env_read(m);
  *out = m;
  HIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  TRY(m->x.alloc((size_t)m->Mp * m->P));
  TRY(m->phi.alloc((size_t)m->Mp * m->P));
  TRY(m->gn.alloc((size_t)4096));
  HIP_TRY(hipMemcpyAsync(m->x, init_particles, (size_t)m->Mp * m->P * sizeof(float), hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  for (int p = 0; p < 4; ++p) m->prior_bwv[p] = cfg->init_bw;
  for (int k = 0; k < cfg->dim_s && k < 5; ++k) m->loc[k] = initial_obs[k];
  m->have_past = false;
  if (cfg->model_cfg.model == DUST_MODEL_SKID_STEER) {  // SkidSteerRobot.__init__ defaults (skid_steer_robot.py:19-28), nothing sampled
    m->skid.x_icr = DevParam{DUST_PARAM_PYFLOAT, 0, 0.2};
    m->skid.wheel_radius = DevParam{DUST_PARAM_PYFLOAT, 0, 0.0625};
    m->skid.axial_distance = DevParam{DUST_PARAM_PYFLOAT, 0, 0.475};
    for (int d = 0; d < 2; ++d) {
      m->skid.lo[d] = -0.5f;
      m->skid.hi[d] = 0.5f;
    }
  }
  if (cfg->model_cfg.model == DUST_MODEL_CARTPOLE) cartpole_defaults(m->cart.par);  // cartpole.py:42-51, nothing sampled
  return DUST_OK;
}

// The filter's CartPoleModel: the seven parameters (kind / column / value), validated as dust_set_cartpole does.  The cost fields of the
// struct are not read.
extern "C" int dust_mpf_set_cartpole(dust_mpf *m, const dust_cartpole_config *g) {
  if (!m || !g) return fail(DUST_ERR_INVALID, "null argument");
  if (m->cfg.model_cfg.model != DUST_MODEL_CARTPOLE) return fail(DUST_ERR_STATE, "the filter's model is not DUST_MODEL_CARTPOLE");
  DevParam par[dust::CP_NPAR];
  TRY(cartpole_params(g, m->P, par));
  HIP_TRY(hipSetDevice(m->cfg.device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  for (int q = 0; q < dust::CP_NPAR; ++q) m->cart.par[q] = par[q];
  return DUST_OK;
}

// The filter's SkidSteerRobot: the three parameters (kind / column / value) and the wheel-speed bounds; validated as dust_set_skid_steer
// does.  The cost fields of the struct are not read.
extern "C" int dust_mpf_set_skid_steer(dust_mpf *m, const dust_skid_config *g) {
  if (!m || !g) return fail(DUST_ERR_INVALID, "null argument");
  if (m->cfg.model_cfg.model != DUST_MODEL_SKID_STEER) return fail(DUST_ERR_STATE, "the filter's model is not DUST_MODEL_SKID_STEER");
  const dust_param *ps[3] = {&g->x_icr, &g->wheel_radius, &g->axial_distance};
  unsigned seen = 0u;
  for (const dust_param *p : ps) {
    if (p->kind < 0 || p->kind > DUST_PARAM_TENSOR0D) return fail(DUST_ERR_INVALID, "bad parameter kind %d", p->kind);
    if (p->kind != DUST_PARAM_SAMPLED) continue;
    if (p->column < 0 || p->column >= m->P) return fail(DUST_ERR_INVALID, "sampled parameter column %d outside dim_p = %d", p->column, m->P);
    if (seen & (1u << p->column)) return fail(DUST_ERR_INVALID, "two sampled parameters name column %d", p->column);
    seen |= 1u << p->column;
  }
  for (int d = 0; d < 2; ++d)
    if (!(g->min_wheel_speed[d] <= g->max_wheel_speed[d])) return fail(DUST_ERR_INVALID, "wheel speed bounds: min > max");
  HIP_TRY(hipSetDevice(m->cfg.device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->skid.x_icr = DevParam{g->x_icr.kind, g->x_icr.column, g->x_icr.value};
  m->skid.wheel_radius = DevParam{g->wheel_radius.kind, g->wheel_radius.column, g->wheel_radius.value};
  m->skid.axial_distance = DevParam{g->axial_distance.kind, g->axial_distance.column, g->axial_distance.value};
  for (int d = 0; d < 2; ++d) {
    m->skid.lo[d] = g->min_wheel_speed[d];
    m->skid.hi[d] = g->max_wheel_speed[d];
  }
  return DUST_OK;
}

// A skid-steer filter can run once its sampled parameters name every particle column (dust_mpf_set_skid_steer)
static int mpf_model_ready(const dust_mpf *m) {
  if (m->cfg.model_cfg.model == DUST_MODEL_CARTPOLE) {  // (dust_mpf_set_cartpole has refused a column named twice)
    unsigned seen = 0u;
    for (const DevParam &p : m->cart.par)
      if (p.kind == DUST_PARAM_SAMPLED) seen |= 1u << p.col;
    if (seen == 0u) return fail(DUST_ERR_STATE, "cart-pole filter: no parameter is sampled - call dust_mpf_set_cartpole first");
    if (seen != (1u << m->P) - 1u) return fail(DUST_ERR_STATE, "cart-pole filter: the sampled parameters do not cover the dim_p = %d particle columns", m->P);
    return DUST_OK;
  }
  if (m->cfg.model_cfg.model != DUST_MODEL_SKID_STEER) return DUST_OK;
  unsigned seen = 0u;
  const DevParam *ps[3] = {&m->skid.x_icr, &m->skid.wheel_radius, &m->skid.axial_distance};
  for (const DevParam *p : ps)
    if (p->kind == DUST_PARAM_SAMPLED) seen |= 1u << p->col;
  if (seen == 0u) return fail(DUST_ERR_STATE, "skid-steer filter: no parameter is sampled - call dust_mpf_set_skid_steer first");
  if (seen != (1u << m->P) - 1u) return fail(DUST_ERR_STATE, "skid-steer filter: the sampled parameters do not cover the dim_p = %d particle columns", m->P);
  return DUST_OK;
}

extern "C" int dust_mpf_set_grid(dust_mpf *m, const float *grid, int nx, int ny, float off_x, float off_y) {
  if (!m || !grid || nx < 1 || ny < 1) return fail(DUST_ERR_INVALID, "bad grid");
  const size_t cells = (size_t)nx * ny, words = (cells + 31) / 32;
  std::vector<uint32_t> bits(words, 0u);
  for (size_t i = 0; i < cells; ++i) {
    if (grid[i] == 1.0f) bits[i >> 5] |= 1u << (i & 31);
    else if (grid[i] != 0.0f) return fail(DUST_ERR_UNSUPPORTED, "occupancy grid must be binary");
  }
  HIP_TRY(hipSetDevice(m->cfg.device));
  TRY(m->grid_bits.alloc(words));
  HIP_TRY(hipMemcpyAsync(m->grid_bits, bits.data(), words * 4, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->nx = nx;
  m->ny = ny;
  m->off_x = off_x;
  m->off_y = off_y;
  return DUST_OK;
}

// MPF(optimizer_class=..., **opt_args) (svgd.py:108-122): SGD (the demos' choice) or Adam (the class default).  (Re)starts the state.
extern "C" int dust_mpf_set_optimizer(dust_mpf *m, int optimizer, float beta1, float beta2, float eps) {
  if (!m) return fail(DUST_ERR_INVALID, "null mpf");
  if (optimizer != DUST_OPT_SGD && optimizer != DUST_OPT_ADAM) return fail(DUST_ERR_UNSUPPORTED, "MPF optimiser: SGD or Adam (dust_mpf_set_optimizer_ex: the others)");
  const dust_optim_config o = optim_plain(optimizer, m->cfg.lr, beta1, beta2, eps);
  return dust_mpf_set_optimizer_ex(m, &o);
}

// any optimiser of dust_set_optimizer; its state starts fresh and persists across optimize() calls (built once in MPF.__init__, mpf.py:24)
extern "C" int dust_mpf_set_optimizer_ex(dust_mpf *m, const dust_optim_config *opt) {
  if (!m) return fail(DUST_ERR_INVALID, "null mpf");
  TRY(validate_optim(opt));
  HIP_TRY(hipSetDevice(m->cfg.device));
  const size_t n = (size_t)m->Mp * m->P;
  HIP_TRY(hipStreamSynchronize(m->stream));  // (slots about to be freed may still be read by queued work)
  TRY(optim_slots_alloc(*opt, m->opt_s, n));
  m->opt = *opt;
  m->cfg.lr = (float)opt->lr;
  m->opt_t = 0;
  TRY(optim_restart(m->opt, m->opt_s, n, m->stream));
  return DUST_OK;
}

extern "C" int dust_mpf_clone(const dust_mpf *src, dust_mpf **out) {
  if (!src || !out) return fail(DUST_ERR_INVALID, "null argument");
  std::vector<float> x((size_t)src->Mp * src->P);
  HIP_TRY(hipSetDevice(src->cfg.device));
  HIP_TRY(hipMemcpy(x.data(), src->x, x.size() * sizeof(float), hipMemcpyDeviceToHost));
  TRY(dust_mpf_create(&src->cfg, x.data(), src->loc, out));
  dust_mpf *m = *out;
  memcpy(m->prior_bwv, src->prior_bwv, sizeof m->prior_bwv);
  memcpy(m->loc, src->loc, sizeof m->loc);
  memcpy(m->past_obs, src->past_obs, sizeof m->past_obs);
  memcpy(m->past_action, src->past_action, sizeof m->past_action);
  m->have_past = src->have_past;
  m->skid = src->skid;
  m->cart = src->cart;
  if (memcmp(&src->opt, &m->opt, sizeof m->opt) != 0) {
    TRY(dust_mpf_set_optimizer_ex(m, &src->opt));
    const size_t nb = (size_t)src->Mp * src->P * sizeof(float);
    HIP_TRY(hipStreamSynchronize(m->stream));
    for (int k = 0; k < 3; ++k)
      if (src->opt_s[k]) HIP_TRY(hipMemcpy(m->opt_s[k], src->opt_s[k], nb, hipMemcpyDeviceToDevice));
    m->opt_t = src->opt_t;
  }
  if (src->grid_bits) {
    const size_t words = ((size_t)src->nx * src->ny + 31) / 32;
    TRY(m->grid_bits.alloc(words));
    HIP_TRY(hipMemcpy(m->grid_bits, src->grid_bits, words * 4, hipMemcpyDeviceToDevice));
    m->nx = src->nx;
    m->ny = src->ny;
    m->off_x = src->off_x;
    m->off_y = src->off_y;
  }
  return DUST_OK;
}

enum { MPF_POLL_MAX = 1024 };  // particles up to which the data-polled form is taken (A/B: 512 = counter form above)
enum { MPF_GCNT_WORDS = (2 * dust::MPF_G_NSH + 2) * dust::MPF_G_LINE };
// Whether this call takes a multi-workgroup kernel: an optimisation of >= 2 steps over >= 96 particles - measured, us per 20-step call
// (profiles/round3_mpf_time.txt): single workgroup 64: 151, 96: 231, 128: 270, 256: 797, 512: 2 927, 1024: 11 433; data-polled grid
// 64: 163, 96: 185, 128: 176, 256: 195, 512: 259, 1024: 400; counter grid 256: 363, 512: 498, 1024: 730.
// DUST_MPF_GRID=0 / 1: never / from 8 particles on (tests); DUST_MPF_POLL=0: the counter form.
static bool mpf_grid_ok(const dust_mpf *m, int n_steps, bool optimise) {
  if (!optimise || n_steps < 2 || m->grid_banned) return false;
  if (m->env.grid == 0) return false;
  return m->Mp >= (m->env.grid == 1 ? 8 : 96);
}

// Effective action of every SVGD step of the coming launch when the model carries control noise: acts = past_action + dyn_std * z, one
// z [da] per phi() call (particle.py:145-148; `acts` is the bare action vector at likelihoods.py:44), in fp32 as the reference adds it.
static int mpf_noisy_actions(dust_mpf *m, int n_steps, const float **dev) {
  *dev = nullptr;
  const dust_config &g = m->cfg.model_cfg;
  if (g.model != DUST_MODEL_PARTICLE || !g.ctrl_noise || (g.dyn_std[0] == 0.f && g.dyn_std[1] == 0.f) || n_steps < 1) return DUST_OK;
  if (m->act_seq.cap() < (size_t)2 * n_steps) TRY(m->act_seq.alloc((size_t)2 * std::max(n_steps, 64)));
  std::vector<float> h((size_t)2 * n_steps);
  for (int it = 0; it < n_steps; ++it)
    for (int d = 0; d < 2; ++d) {
      float z;
      if (m->cz_next < m->cz.size()) {
        z = m->cz[m->cz_next++];
      } else {
        if (!m->rng_seeded) m->rng.seed(g.seed ^ 0x6d70666e6f697365ull);
        m->rng_seeded = true;
        z = std::normal_distribution<float>(0.f, 1.f)(m->rng);
      }
      const float nz = g.dyn_std[d] * z;
      h[(size_t)2 * it + d] = m->past_action[d] + nz;
    }
  HIP_TRY(hipMemcpyAsync(m->act_seq, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));  // (h is a local; the filter's calls are synchronous anyway)
  *dev = m->act_seq;
  return DUST_OK;
}

extern "C" int dust_mpf_set_ctrl_noise(dust_mpf *m, const float *z, int n) {
  if (!m) return fail(DUST_ERR_INVALID, "null mpf");
  if (m->cfg.model_cfg.model != DUST_MODEL_PARTICLE || !m->cfg.model_cfg.ctrl_noise)
    return fail(DUST_ERR_STATE, "control noise belongs to a Particle(deterministic=False) model (model_cfg.ctrl_noise)");
  m->cz.clear();
  m->cz_next = 0;
  if (z && n > 0) m->cz.assign(z, z + (size_t)n * m->cfg.dim_a);
  return DUST_OK;
}

// The particle-independent part of the skid-steer likelihood for the coming launch (SkidLik), copied to the device on the filter's
// stream; the heading's fp32 cosine and sine are added there by a one-lane kernel.  (The host copy is a member: every filter call
// synchronises the stream before it returns, so the copy has been read by the time the next call rewrites it.)
// (the host part: `m` gives the model, the rest is one environment's - a batched filter fills one SkidLik per environment with it)
static void mpf_skid_lik(const dust_mpf *m, const float *past_action, const float *past_obs, const float *loc, dust::SkidLik &k) {
  memset(&k, 0, sizeof k);
  const DevParam *ps[3] = {&m->skid.x_icr, &m->skid.wheel_radius, &m->skid.axial_distance};
  for (int q = 0; q < 3; ++q) {
    k.smp[q] = ps[q]->kind == DUST_PARAM_SAMPLED;
    k.col[q] = k.smp[q] ? ps[q]->col : 0;
    k.fix_f[q] = (float)ps[q]->value;
    k.fix_d[q] = ps[q]->value;
  }
  k.r = clampf_host(past_action[0], m->skid.lo[0], m->skid.hi[0]);
  k.l = clampf_host(past_action[1], m->skid.lo[1], m->skid.hi[1]);
  k.dt = (float)m->cfg.model_cfg.dt;
  for (int q = 0; q < 5; ++q) {
    k.past[q] = past_obs[q];
    k.obs[q] = loc[q];
  }
  k.c = std::cos((double)past_obs[2]);
  k.s = std::sin((double)past_obs[2]);
  k.sum = ((double)k.r + (double)k.l) * M_PI;
  k.dif = 2.0 * M_PI * ((double)k.r - (double)k.l);
  k.dtd = m->cfg.model_cfg.dt;
}
static int mpf_skid_prepare(dust_mpf *m, const dust::SkidLik **dev) {
  if (!m->skl_dev) TRY(m->skl_dev.alloc(1));
  dust::SkidLik &k = m->skl_host;
  mpf_skid_lik(m, m->past_action, m->past_obs, m->loc, k);
  HIP_TRY(hipMemcpyAsync(m->skl_dev, &k, sizeof k, hipMemcpyHostToDevice, m->stream));
  dust::mpf_skid_heading_kernel<<<1, 64, 0, m->stream>>>(m->skl_dev);
  HIP_TRY(hipGetLastError());
  *dev = m->skl_dev;
  return DUST_OK;
}

// ... and of the cart-pole likelihood (CartLik); the fp32 sine and cosine of the past angle are added on the device
static void mpf_cart_lik(const dust_mpf *m, const float *past_action, const float *past_obs, const float *loc, dust::CartLik &k) {
  memset(&k, 0, sizeof k);
  for (int q = 0; q < dust::CP_NPAR; ++q) {
    const DevParam &p = m->cart.par[q];
    k.fix_f[q] = (float)p.value;
    k.fix_d[q] = p.kind == DUST_PARAM_TENSOR0D ? (double)(float)p.value : p.value;
    if (p.kind == DUST_PARAM_SAMPLED) k.par_of_col[p.col] = q;
  }
  const DevParam &pmp = m->cart.par[dust::CP_MP], &pl = m->cart.par[dust::CP_LEN];
  k.pm_py = pmp.kind == DUST_PARAM_PYFLOAT && pl.kind == DUST_PARAM_PYFLOAT;
  k.pm_d = pmp.value * pl.value;
  k.ac = clampf_host(past_action[0], -1.0f, 1.0f);
  k.dt = (float)m->cfg.model_cfg.dt;
  for (int q = 0; q < 4; ++q) {
    k.past[q] = past_obs[q];
    k.obs[q] = loc[q];
  }
  k.c = std::cos((double)past_obs[2]);
  k.s = std::sin((double)past_obs[2]);
  k.w = (double)past_obs[3];
  k.w2 = k.w * k.w;
  k.sg = past_obs[1] > 0.f ? 1.0 : (past_obs[1] < 0.f ? -1.0 : 0.0);
  k.a = (double)k.ac;
  k.dtd = m->cfg.model_cfg.dt;
}
static int mpf_cart_prepare(dust_mpf *m, const dust::CartLik **dev) {
  if (!m->cpl_dev) TRY(m->cpl_dev.alloc(1));
  dust::CartLik &k = m->cpl_host;
  mpf_cart_lik(m, m->past_action, m->past_obs, m->loc, k);
  HIP_TRY(hipMemcpyAsync(m->cpl_dev, &k, sizeof k, hipMemcpyHostToDevice, m->stream));
  dust::mpf_cart_angle_kernel<<<1, 64, 0, m->stream>>>(m->cpl_dev);
  HIP_TRY(hipGetLastError());
  *dev = m->cpl_dev;
  return DUST_OK;
}

// The run-time P and a yes / no (cart-pole or not; the batch: log space or not) as compile-time constants: f(p, flag) with p() the P among
// Ps and flag() the bool; false: P is none of Ps.  Ps is what the call site instantiates its kernel for.
template <int... Ps, class F>
static bool mpf_pick(int P, bool flag, F &&f) {
  return ((P == Ps && ((flag ? f(std::integral_constant<int, Ps>(), std::true_type()) : f(std::integral_constant<int, Ps>(), std::false_type())), true)) || ...);
}

static int mpf_grid_ready(const dust_mpf *m) {
  if (m->cfg.model_cfg.model == DUST_MODEL_PARTICLE && m->cfg.model_cfg.with_obstacle && m->cfg.model_cfg.can_crash && !m->grid_bits)
    return fail(DUST_ERR_STATE, "Particle model with obstacles: call dust_mpf_set_grid first");
  return DUST_OK;
}

// What a lone filter's launch and a batch's share of MpfArgs: everything else zero
static void mpf_shared_args(const dust_mpf *m, int n_steps, MpfArgs &a) {
  memset(&a, 0, sizeof a);
  a.dm = mpf_dev_model(m);
  a.Mp = m->Mp;
  a.P = m->P;
  a.ds = m->cfg.dim_s;
  a.da = m->cfg.dim_a;
  a.n_steps = n_steps;
  a.log_space = m->cfg.log_space;
  a.obs_std = m->cfg.obs_std;
}

// The single-workgroup form (mpf_optimize_kernel; one workgroup per environment: mpf_optimize_batch_kernel): block size, dynamic LDS, launch
struct MpfWg {
  int threads;
  size_t lds;
};
static MpfWg mpf_wg(const dust_mpf *m) {
  const int mpad = ((m->Mp + 63) / 64) * 64;
  int R = 1;
  while (mpad * R * 2 <= 1024) R *= 2;
  return MpfWg{mpad * R, sizeof(double) * (size_t)R * mpad * 2 * m->P + sizeof(float) * ((size_t)2 * m->Mp * m->P + m->Mp + 32)};
}
template <class K, class Args>
static int mpf_wg_launch(K kernel, int blocks, const MpfWg &wg, hipStream_t stream, const Args &a) {
  HIP_TRY(launch_on(stream, false, kernel, blocks, wg.threads, wg.lds, a));  // (the filters are never captured)
  return DUST_OK;
}

static int mpf_launch(dust_mpf *m, float bw, float lr, int n_steps, float *gn_dev, float *phi_dev, bool optimise = true, bool grid = false,
                      const float *act_seq_dev = nullptr) {
  serve_cancel_device(m->cfg.device);  // (an armed control tick - closed-loop serving - would hold every CU until its plant state arrives)
  TRY(mpf_grid_ready(m));
  MpfArgs a;
  mpf_shared_args(m, n_steps, a);
  for (int p = 0; p < 4; ++p) a.prior_bwv[p] = m->prior_bwv[p];
  a.bw = bw;
  for (int k = 0; k < 4; ++k) {
    a.past_obs[k] = m->past_obs[k];
    a.obs[k] = m->loc[k];
  }
  if (m->cfg.model_cfg.model == DUST_MODEL_SKID_STEER) TRY(mpf_skid_prepare(m, &a.skl));
  const bool cart = m->cfg.model_cfg.model == DUST_MODEL_CARTPOLE;
  if (cart) TRY(mpf_cart_prepare(m, &a.cpl));
  a.past_action[0] = m->past_action[0];
  a.past_action[1] = m->past_action[1];
  a.act_seq = act_seq_dev;
  a.x = m->x;
  a.grad_norms = gn_dev;
  a.phi_out = phi_dev;
  if (optimise) {
    a.opt = m->opt;  // (its lr is the lr passed, m->cfg.lr, kept in double)
    a.opt_s0 = m->opt_s[0];
    a.opt_s1 = m->opt_s[1];
    a.opt_s2 = m->opt_s[2];
  } else {  // the bare phi evaluation takes no step
    a.opt = optim_plain(DUST_OPT_SGD, lr, 0.f, 0.f, 0.f);
  }
  a.t0 = m->opt_t;
  // the data-polled form (keys in registers) unless DUST_MPF_POLL=0, which selects the counter form
  if (grid && m->Mp <= MPF_POLL_MAX && m->env.poll != 0) {
    const int NP = (m->P + 1) / 2, NX = NP + 1;
    const size_t fx = (size_t)2 * m->Mp * NX * 4, fs = (size_t)2 * m->Mp * NP * 4;  // floats
    if (!m->pbuf) {
      TRY(m->pbuf.alloc(fx + fs));
      HIP_TRY(hipMemsetAsync(m->pbuf, 0, (fx + fs) * sizeof(float), m->stream));  // (tag 0 is never waited for)
    }
    if (!m->pcnt) {
      TRY(m->pcnt.alloc((size_t)2 * MPF_G_LINE));
      HIP_TRY(hipMemsetAsync(m->pcnt, 0, (size_t)2 * MPF_G_LINE * sizeof(unsigned int), m->stream));
    }
    if (!m->gcnt) {
      TRY(m->gcnt.alloc((size_t)MPF_GCNT_WORDS + 4));
      HIP_TRY(hipMemsetAsync(m->gcnt, 0, ((size_t)MPF_GCNT_WORDS + 4) * sizeof(unsigned int), m->stream));
    }
    MpfPollArgs g;
    memset(&g, 0, sizeof g);
    g.a = a;
    g.xpc = m->pbuf;
    g.scp = m->pbuf + fx;
    g.cnt = m->pcnt;
    g.status = m->gcnt + MPF_GCNT_WORDS;
    g.seq = ++m->pseq;
    g.tag0 = g.seq * 8192u;  // (n_steps <= 4096: 2 tags per step)
    g.test = m->env.grid_test;
    const int G = (m->Mp + MPF_G_WAVES - 1) / MPF_G_WAVES;
    mpf_pick<1, 2, 3, 4>(m->P, cart, [&](auto p, auto ct) {
      if (m->Mp <= 256) mpf_optimize_poll_kernel<p(), 4, ct()><<<G, MPF_G_NT, 0, m->stream>>>(g);
      else if (m->Mp <= 512) mpf_optimize_poll_kernel<p(), 8, ct()><<<G, MPF_G_NT, 0, m->stream>>>(g);
      else mpf_optimize_poll_kernel<p(), 16, ct()><<<G, MPF_G_NT, 0, m->stream>>>(g);
    });
    HIP_TRY(hipGetLastError());
    return DUST_OK;
  }
  if (grid) {
    const size_t np = (size_t)m->Mp * m->P;
    if (!m->gbuf || m->gsteps < n_steps) {
      m->gsteps = std::max(n_steps, 32);
      TRY(m->gbuf.alloc(4 * np + (size_t)m->gsteps * m->Mp));
    }
    if (!m->gcnt) {
      TRY(m->gcnt.alloc((size_t)MPF_GCNT_WORDS + 4));
      HIP_TRY(hipMemsetAsync(m->gcnt, 0, ((size_t)MPF_GCNT_WORDS + 4) * sizeof(unsigned int), m->stream));
    }
    HIP_TRY(hipMemsetAsync(m->gcnt, 0, (size_t)MPF_GCNT_WORDS * sizeof(unsigned int), m->stream));
    MpfGridArgs g;
    memset(&g, 0, sizeof g);
    g.a = a;
    g.xg = m->gbuf;
    g.scg = m->gbuf + 2 * np;
    g.n2g = m->gbuf + 4 * np;
    g.cnt = m->gcnt;
    g.status = m->gcnt + MPF_GCNT_WORDS;
    g.test = m->env.grid_test;
    const int G = (m->Mp + MPF_G_WAVES - 1) / MPF_G_WAVES;
    const size_t lds = sizeof(float) * ((size_t)2 * np + m->Mp + 8);
    mpf_pick<1, 2, 3, 4>(m->P, cart, [&](auto p, auto ct) { mpf_optimize_grid_kernel<p(), ct()><<<G, MPF_G_NT, lds, m->stream>>>(g); });
    HIP_TRY(hipGetLastError());
    return DUST_OK;
  }
  int st = DUST_OK;
  mpf_pick<1, 2, 3, 4>(m->P, cart, [&](auto p, auto ct) { st = mpf_wg_launch(mpf_optimize_kernel<p(), ct()>, 1, mpf_wg(m), m->stream, a); });
  TRY(st);
  HIP_TRY(hipGetLastError());
  return DUST_OK;
}

extern "C" int dust_mpf_optimize(dust_mpf *m, const float *action, const float *new_obs, float bw, int n_steps, float *grad_norms) {
  if (!m) return fail(DUST_ERR_INVALID, "null mpf");
  if (n_steps < 0 || n_steps > 4096) return fail(DUST_ERR_INVALID, "n_steps out of range");
  if (!(bw > 0.f)) return fail(DUST_ERR_INVALID, "bw must be > 0 (the host layer evaluates silvermans_rule when bw is None)");
  TRY(mpf_model_ready(m));
  HIP_TRY(hipSetDevice(m->cfg.device));
  if (new_obs) {  // GaussianLikelihood.condition likelihoods.py:51-64
    if (!action) return fail(DUST_ERR_INVALID, "condition() needs the action that produced new_obs");
    memcpy(m->past_obs, m->loc, sizeof m->past_obs);
    for (int k = 0; k < m->cfg.dim_s && k < 5; ++k) m->loc[k] = new_obs[k];
    for (int k = 0; k < 2; ++k) m->past_action[k] = k < m->cfg.dim_a ? action[k] : 0.f;
    m->have_past = true;
  }
  if (!m->have_past) return fail(DUST_ERR_STATE, "Previous action is None. Need at least one observation to start sampling.");
  const bool grid = mpf_grid_ok(m, n_steps, true);
  const float *acts = nullptr;
  TRY(mpf_noisy_actions(m, n_steps, &acts));
  TRY(mpf_launch(m, bw, m->cfg.lr, n_steps, m->gn, nullptr, true, grid, acts));
  const bool want_gn = grad_norms && n_steps > 0;
  if (!m->hpin) TRY(m->hpin.alloc(4096 + 8, hipHostMallocDefault));
  bool gn_read = false;
  if (grid) {  // did the grid form start, and did it commit?  (tick2.hpp's protocol; this call is synchronous anyway)
    // status and gradient norms come back through pinned memory behind ONE synchronisation
    unsigned int *st = reinterpret_cast<unsigned int *>(m->hpin + 4096);
    HIP_TRY(hipMemcpyAsync(st, m->gcnt + MPF_GCNT_WORDS, 3 * sizeof(unsigned int), hipMemcpyDeviceToHost, m->stream));
    if (want_gn) HIP_TRY(hipMemcpyAsync(m->hpin, m->gn, n_steps * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    gn_read = want_gn;
    m->n_grid++;
    if (st[0] | st[1] | st[2]) {
      HIP_TRY(hipMemsetAsync(m->gcnt + MPF_GCNT_WORDS, 0, 4 * sizeof(unsigned int), m->stream));
      if (st[0]) m->grid_banned = true;  // (a wait gave up: another process computes on the device - handoff.hpp)
      if (st[2] != 0u && st[2] != (unsigned int)m->Mp)
        return fail(DUST_ERR_HIP, "MPF: a hand-off wait timed out while some waves were committing (particles invalid: re-seed them); the device seems to be shared with another process");
      if (st[1] || st[2]) {  // nothing was written: the single-workgroup kernel runs the call
        m->n_grid_fallback++;
        TRY(mpf_launch(m, bw, m->cfg.lr, n_steps, m->gn, nullptr, true, false, acts));  // (the same draws: nothing was committed)
        gn_read = false;
      }
    }
  }
  m->opt_t += n_steps;
  for (int p = 0; p < 4; ++p) m->prior_bwv[p] = bw;  // update_prior(bw) mpf.py:85
  if (!gn_read) {
    if (want_gn) HIP_TRY(hipMemcpyAsync(m->hpin, m->gn, n_steps * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  if (want_gn) memcpy(grad_norms, m->hpin, n_steps * sizeof(float));
  return DUST_OK;
}

extern "C" int dust_mpf_stats(dust_mpf *m, long long out[2]) {
  if (!m || !out) return fail(DUST_ERR_INVALID, "null argument");
  out[0] = m->n_grid;
  out[1] = m->n_grid_fallback;
  return DUST_OK;
}

extern "C" int dust_mpf_phi(dust_mpf *m, float bw, float *phi) {
  if (!m || !phi) return fail(DUST_ERR_INVALID, "null argument");
  TRY(mpf_model_ready(m));
  if (!m->have_past) return fail(DUST_ERR_STATE, "Previous action is None. Need at least one observation to start sampling.");
  HIP_TRY(hipSetDevice(m->cfg.device));
  const float *acts = nullptr;
  TRY(mpf_noisy_actions(m, 1, &acts));
  TRY(mpf_launch(m, bw, 0.0f, 1, nullptr, m->phi, false, false, acts));  // lr = 0, SGD form: particles and optimiser state unchanged
  HIP_TRY(hipMemcpyAsync(phi, m->phi, (size_t)m->Mp * m->P * sizeof(float), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return DUST_OK;
}

// GaussianLikelihood.condition without an optimisation (used by the host mirror's condition())
extern "C" int dust_mpf_condition(dust_mpf *m, const float *action, const float *new_obs) {
  if (!m || !new_obs) return fail(DUST_ERR_INVALID, "null argument");
  memcpy(m->past_obs, m->loc, sizeof m->past_obs);
  for (int k = 0; k < m->cfg.dim_s && k < 5; ++k) m->loc[k] = new_obs[k];
  if (action) {
    for (int k = 0; k < 2; ++k) m->past_action[k] = k < m->cfg.dim_a ? action[k] : 0.f;
    m->have_past = true;
  }
  return DUST_OK;
}

extern "C" int dust_mpf_get_particles(dust_mpf *m, float *x) {
  if (!m || !x) return fail(DUST_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(m->cfg.device));
  HIP_TRY(hipMemcpyAsync(x, m->x, (size_t)m->Mp * m->P * sizeof(float), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return DUST_OK;
}
extern "C" int dust_mpf_set_particles(dust_mpf *m, const float *x) {
  if (!m || !x) return fail(DUST_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(m->cfg.device));
  HIP_TRY(hipMemcpyAsync(m->x, x, (size_t)m->Mp * m->P * sizeof(float), hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return DUST_OK;
}
static dust::MpfBw mpf_bw(const dust_mpf *m) {
  dust::MpfBw b;
  for (int p = 0; p < 4; ++p) b.v[p] = m->prior_bwv[p];
  return b;
}

// MPF(bw=None) with P > 1: bw_silverman of the particle columns is a [P] vector and `bw ** 2 * torch.eye(P)` (mpf.py:31-36) turns it
// into the covariance diag(bw_p^2) of the FIRST prior; every later update_prior(bw) (mpf.py:85) is scalar again.
extern "C" int dust_mpf_set_prior_bw(dust_mpf *m, const float *bw, int n) {
  if (!m || !bw) return fail(DUST_ERR_INVALID, "null argument");
  if (n != 1 && n != m->P) return fail(DUST_ERR_INVALID, "prior bandwidths: 1 or P = %d values, got %d", m->P, n);
  for (int p = 0; p < n; ++p)
    if (!(bw[p] > 0.f)) return fail(DUST_ERR_INVALID, "prior bandwidth %d must be > 0", p);
  for (int p = 0; p < 4; ++p) m->prior_bwv[p] = bw[n == 1 ? 0 : (p < n ? p : 0)];
  return DUST_OK;
}

extern "C" int dust_mpf_get_prior_bw(dust_mpf *m, float *bw) {
  if (!m || !bw) return fail(DUST_ERR_INVALID, "null argument");
  for (int p = 0; p < m->P; ++p) bw[p] = m->prior_bwv[p];
  return DUST_OK;
}

extern "C" int dust_mpf_get_prior(dust_mpf *m, float *means, float *bw) {
  if (!m) return fail(DUST_ERR_INVALID, "null mpf");
  if (means) TRY(dust_mpf_get_particles(m, means));
  if (bw) *bw = m->prior_bwv[0];  // (per-dimension bandwidths: dust_mpf_get_prior_bw)
  return DUST_OK;
}
extern "C" int dust_mpf_prior_sample(dust_mpf *m, int n, uint64_t seed, float *samples) {
  if (!m || !samples || n < 1) return fail(DUST_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(m->cfg.device));
  TRY(m->tmp.ensure((size_t)n * m->P));
  mpf_sample_kernel<<<(n + 255) / 256, 256, 0, m->stream>>>(m->x, m->Mp, m->P, mpf_bw(m), seed, n, m->tmp);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(samples, m->tmp, (size_t)n * m->P * sizeof(float), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return DUST_OK;
}
extern "C" int dust_mpf_prior_log_prob(dust_mpf *m, int n, const float *x, float *log_prob) {
  if (!m || !x || !log_prob || n < 1) return fail(DUST_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(m->cfg.device));
  TRY(m->tmp.ensure((size_t)n * (m->P + 1)));
  HIP_TRY(hipMemcpyAsync(m->tmp, x, (size_t)n * m->P * sizeof(float), hipMemcpyHostToDevice, m->stream));
  mpf_log_prob_kernel<<<(n + 255) / 256, 256, 0, m->stream>>>(m->tmp, m->x, n, m->Mp, m->P, mpf_bw(m), m->tmp + (size_t)n * m->P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(log_prob, m->tmp + (size_t)n * m->P, n * sizeof(float), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return DUST_OK;
}

// tf.compute_sigma_points(mpf.prior.mean, mpf.prior.variance.diag()) (disco.py:240-251, utf.py:93-123) on the device; scale = lambda + n
extern "C" int dust_mpf_sigma_points(dust_mpf *m, float scale, float *out) {
  if (!m || !out) return fail(DUST_ERR_INVALID, "null argument");
  if (!(scale > 0.f)) return fail(DUST_ERR_INVALID, "the sigma-point scale lambda + n must be > 0, got %g", (double)scale);
  HIP_TRY(hipSetDevice(m->cfg.device));
  const size_t n = (size_t)(2 * m->P + 1) * m->P;
  TRY(m->tmp.ensure(n));
  mpf_sigma_points_kernel<<<1, 256, 0, m->stream>>>(m->x, m->Mp, m->P, mpf_bw(m), scale, 1, m->tmp);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, m->tmp, n * sizeof(float), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return DUST_OK;
}

// MPF.optimize's `bw = silvermans_rule(self.x.view(-1, 1)) * self.bw_scale` (mpf.py:68-73) on the device: one launch and a 4-byte read-back
// instead of a copy of the particles and a host percentile.
extern "C" int dust_mpf_silverman(dust_mpf *m, float *bw) {
  if (!m || !bw) return fail(DUST_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(m->cfg.device));
  const int n = m->Mp * m->P;
  if (n > 4096) return fail(DUST_ERR_UNSUPPORTED, "Silverman's rule on the device takes up to 4096 pooled values (%d particles x %d parameters)", m->Mp, m->P);
  if (!m->hpin) TRY(m->hpin.alloc(4096 + 8, hipHostMallocDefault));
  TRY(m->tmp.ensure(4));
  mpf_silverman_kernel<<<1, 1024, (size_t)n * sizeof(float), m->stream>>>(m->x, n, m->cfg.bw_scale, m->tmp);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(m->hpin + 4096 + 4, m->tmp, sizeof(float), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  *bw = m->hpin[4096 + 4];
  if (!(*bw > 0.f)) return fail(DUST_ERR_HIP, "Silverman's rule gave a bandwidth of %g", (double)*bw);
  return DUST_OK;
}

// What a controller and a filter must agree on before one call runs a period of both (dust_dual_tick, dust_amppi_dual_tick)
static int dual_pair_check(const dust_ctx *c, const dust_mpf *m) {
  if (c->cfg.dim_p != m->P) return fail(DUST_ERR_INVALID, "the controller samples dim_p = %d dynamics parameters, the filter carries P = %d", c->cfg.dim_p, m->P);
  if (c->cfg.device != m->cfg.device) return fail(DUST_ERR_INVALID, "controller and filter live on different devices");
  if (c->cfg.model == DUST_MODEL_SKID_STEER && m->cfg.model_cfg.model == DUST_MODEL_SKID_STEER) {  // the filter's columns are the controller's
    const DevParam *pc[3] = {&c->skid.x_icr, &c->skid.wheel_radius, &c->skid.axial_distance}, *pm[3] = {&m->skid.x_icr, &m->skid.wheel_radius, &m->skid.axial_distance};
    for (int k = 0; k < 3; ++k)
      if ((pc[k]->kind == DUST_PARAM_SAMPLED) != (pm[k]->kind == DUST_PARAM_SAMPLED) || (pc[k]->kind == DUST_PARAM_SAMPLED && pc[k]->col != pm[k]->col))
        return fail(DUST_ERR_INVALID, "controller and filter name different uncertain skid-steer parameters (or in another column order)");
  }
  if ((c->cfg.model == DUST_MODEL_CARTPOLE) != (m->cfg.model_cfg.model == DUST_MODEL_CARTPOLE))
    return fail(DUST_ERR_INVALID, "a cart-pole controller takes a cart-pole filter, and no other");
  if (c->cfg.model == DUST_MODEL_CARTPOLE) {
    for (int k = 0; k < dust::CP_NPAR; ++k) {
      const DevParam &pc = c->cart.par[k], &pm = m->cart.par[k];
      if ((pc.kind == DUST_PARAM_SAMPLED) != (pm.kind == DUST_PARAM_SAMPLED) || (pc.kind == DUST_PARAM_SAMPLED && pc.col != pm.col))
        return fail(DUST_ERR_INVALID, "controller and filter name different uncertain cart-pole parameters (or in another column order)");
    }
  }
  return DUST_OK;
}

// The filter update of a period (skipped without an action: the first period) with Silverman's rule of the filter's particles on demand
// (bw <= 0; mpf.py:68-73, on the device).  *bw_used: the bandwidth the update ran with (0: no update).
static int dual_filter_update(dust_mpf *m, const float *action_prev, const float *state, float bw, int mpf_steps, float *bw_used) {
  if (action_prev) {
    if (!(bw > 0.f)) TRY(dust_mpf_silverman(m, &bw));
    TRY(dust_mpf_optimize(m, action_prev, state, bw, mpf_steps, nullptr));  // (synchronises the filter's stream: its particles are final)
  }
  if (bw_used) *bw_used = action_prev ? bw : 0.f;
  return DUST_OK;
}

// `waiter` goes on only behind what `ahead` holds now - without waiting on the host
static int dual_stream_after(dust_ctx *c, hipStream_t waiter, hipStream_t ahead) {
  if (!c->ev_dual) HIP_TRY(hipEventCreateWithFlags(&c->ev_dual, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c->ev_dual, ahead));
  HIP_TRY(hipStreamWaitEvent(waiter, c->ev_dual, 0));
  return DUST_OK;
}

// What dust_amppi_dual_tick and dust_amppi_dual_batch_tick both refuse, ahead of any staging launch -> where the parameters come from
static int amppi_dual_check(const dust_ctx *c, const dust_mpf *m, int flags, bool *sigma_out, bool *shared_out) {
  if (m->cfg.log_space) return fail(DUST_ERR_UNSUPPORTED, "a log-space filter under AMPPI: the controller hands samples to the model as drawn (amppi.py:134-139)");
  if (flags & DUST_STORE_STATES) return fail(DUST_ERR_UNSUPPORTED, "the AMPPI dual tick stores no trajectories");
  if (flags & (DUST_EPS_F16 | DUST_STORE_F16)) return fail(DUST_ERR_UNSUPPORTED, "the AMPPI tick has no binary16 storage");
  const bool sigma = c->mw_dev != nullptr;
  if (sigma) {
    if (!(c->sigma_scale > 0.f))
      return fail(DUST_ERR_UNSUPPORTED, "the dual tick over sigma-point weights needs the transform's scale lambda + n (dust_set_sigma_scale)");
    if (c->M != 2 * m->P + 1) return fail(DUST_ERR_INVALID, "sigma-point weights over P = %d parameters take M = 2 P + 1 = %d samples, the controller has M = %d", m->P, 2 * m->P + 1, c->M);
  } else if (c->M != 1) {
    return fail(DUST_ERR_INVALID, "n_params = %d > 1 is the sigma-point form of an AMPPI context: dust_set_param_weights first", c->M);
  }
  *sigma_out = sigma;
  *shared_out = (flags & DUST_AMPPI_PARAMS_SHARED) != 0;
  return DUST_OK;
}

// One control period of the DUAL loop (simulations.py:104-138) in one call: the filter update for the action just applied and the state
// it led to (mpf.optimize(action, state, bw, n_steps): skipped when action_prev is NULL - the first period), then the controller's
// dynamics samples drawn from the filter's refreshed prior ON THE DEVICE, straight into the controller's parameter buffer (n_steps
// draws of [M][P]: disco.py:171, one per SVGD iteration), then the control tick (optimize + forward).  mpf_bw <= 0: Silverman's rule of
// the filter's particles (mpf.py:68-73), evaluated on the device.  Host round trips: the 4-byte bandwidth and the filter's status words
// (the stream is idle there: the caller has just used the previous tick's outputs), then the tick's outputs.  seed: the Philox key of
// this period's draws (dust_mpf_prior_sample's stream).  *bw_used: the bandwidth the filter update ran with (0: no update).
extern "C" int dust_dual_tick(dust_ctx *c, dust_mpf *m, const float *state, const float *action_prev, int n_steps, int mpf_steps, float bw_in,
                              uint64_t seed, float *a_seq, float *p_weights, float *bw_used) {
  if (!c || !m || !state) return fail(DUST_ERR_INVALID, "null argument");
  if (n_steps < 1 || mpf_steps < 0) return fail(DUST_ERR_INVALID, "bad step counts");
  TRY(dual_pair_check(c, m));
  if (comm_active(c)) return fail(DUST_ERR_UNSUPPORTED, "the dual tick runs on an unsharded controller (the filter is replicated: tick it per rank)");
  if (c->mw_dev) {  // a sigma-point controller: its dynamics samples are the sigma points of the filter's prior, not draws from it
    if (!(c->sigma_scale > 0.f))
      return fail(DUST_ERR_UNSUPPORTED, "the dual tick over sigma-point weights needs the transform's scale lambda + n (dust_set_sigma_scale): the "
                                        "dynamics samples are the sigma points of the filter's prior (disco.py:240-251)");
    if (c->M != 2 * m->P + 1) return fail(DUST_ERR_INVALID, "sigma-point weights over P = %d parameters take M = 2 P + 1 = %d samples, the controller has M = %d", m->P, 2 * m->P + 1, c->M);
    if (c->cfg.params_log_space) return fail(DUST_ERR_UNSUPPORTED, "sigma points of a log-space parameter distribution: the reference asserts against it (disco.py:125)");
  }
  HIP_TRY(hipSetDevice(c->cfg.device));
  TRY(dual_filter_update(m, action_prev, state, bw_in, mpf_steps, bw_used));
  TRY(settle_pending(c));
  const int n = n_steps * c->M;
  TRY(c->params_dev.ensure((size_t)n * c->P));
  // (sigma points: the same 2P + 1 points for every SVGD iteration - MultiDISCO._sigma_rollout recomputes them per call; seed unused)
  if (c->mw_dev) dust::mpf_sigma_points_kernel<<<1, 256, 0, c->stream>>>(m->x, m->Mp, m->P, mpf_bw(m), c->sigma_scale, n_steps, c->params_dev);
  else dust::mpf_sample_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(m->x, m->Mp, m->P, mpf_bw(m), seed, n, c->params_dev);
  HIP_TRY(hipGetLastError());
  c->params_staged = true;  // (dust_svmpc_tick finds its dynamics samples in place: no host copy, no one-launch tick - its replay record keeps host samples)
  const int st = dust_svmpc_tick(c, state, n_steps, nullptr, c->params_dev, 0, a_seq, p_weights);
  c->params_staged = false;
  return st;
}

// One control period of the dual loop over an AMPPI controller (simulations.py:104-138 with amppi.py:227-260 as the controller) in one
// call: the filter update for (action_prev, state) - skipped when action_prev is NULL; bw_in <= 0: Silverman's rule on the device -, the
// parameters from the refreshed prior, the AMPPI update, the outputs, the roll.  The parameters:
//   "extended" (no flag)            lane s of the tick's kernel draws row s of dust_mpf_prior_sample(m, S, seed) itself (amppi.hpp:
//                                   amppi_prior_kernel): no parameter buffer, no launch besides the tick's;
//   DUST_AMPPI_PARAMS_SHARED        one row (mpf_sample_kernel, n = 1) staged into the controller's parameter buffer on ITS stream;
//   sigma weights + a scale         the 2P + 1 sigma points of the prior (mpf_sigma_points_kernel), staged the same way.
// params_out (host, or NULL): the rows the tick used - [S][P], [1][P], [2P + 1][P].  a_seq: the sequence after the update, BEFORE the roll.
// The tick's kernels read the filter's particles in place on the controller's stream; the next filter update writes them on the filter's
// stream.  A host copy of an output drains the controller's stream; without one the filter's stream is made to wait for an event behind
// the kernels.
extern "C" int dust_amppi_dual_tick(dust_ctx *c, dust_mpf *m, const float *state, const float *action_prev, const float *actions, int flags,
                                    int mpf_steps, float bw_in, uint64_t seed, int roll_steps, float *costs, float *omega, float *a_seq,
                                    float *params_out, float *bw_used) {
  if (!c || !m || !state) return fail(DUST_ERR_INVALID, "null argument");
  if (mpf_steps < 0 || roll_steps < 0) return fail(DUST_ERR_INVALID, "bad step counts");
  TRY(amppi_check(c));  // (n_policies = 1, not sharded, no params_log_space, ...)
  TRY(dual_pair_check(c, m));
  bool sigma, shared;
  TRY(amppi_dual_check(c, m, flags, &sigma, &shared));
  if (m->P < 1 || m->P > 4 || m->Mp > 1024) return fail(DUST_ERR_UNSUPPORTED, "the AMPPI dual tick takes a filter of up to 1024 particles over 1 .. 4 parameters");
  HIP_TRY(hipSetDevice(c->cfg.device));
  TRY(dual_filter_update(m, action_prev, state, bw_in, mpf_steps, bw_used));
  // no update: whatever wrote the particles last on the filter's stream comes first
  if (!action_prev) TRY(dual_stream_after(c, c->stream, m->stream));
  TRY(settle_pending(c));
  const int P = m->P;
  const size_t prows = sigma ? (size_t)c->M : (shared ? (size_t)1 : (size_t)c->S);
  if (sigma || shared || params_out) TRY(c->params_dev.ensure(prows * P));
  int st;
  if (sigma || shared) {
    if (sigma) dust::mpf_sigma_points_kernel<<<1, 256, 0, c->stream>>>(m->x, m->Mp, P, mpf_bw(m), c->sigma_scale, 1, c->params_dev);
    else dust::mpf_sample_kernel<<<1, 256, 0, c->stream>>>(m->x, m->Mp, P, mpf_bw(m), seed, 1, c->params_dev);
    HIP_TRY(hipGetLastError());
    st = amppi_update_impl(c, state, actions, c->params_dev, flags, nullptr, nullptr, nullptr, true, nullptr);
  } else {
    dust::AmppiPrior pr;
    memset(&pr, 0, sizeof pr);
    pr.means = m->x;
    pr.K = m->Mp;
    pr.P = P;
    const dust::MpfBw b = mpf_bw(m);
    for (int p = 0; p < 4; ++p) pr.bw[p] = b.v[p];
    pr.seed = seed;
    pr.params_out = params_out ? c->params_dev : nullptr;
    st = amppi_update_impl(c, state, actions, nullptr, flags, nullptr, nullptr, nullptr, false, &pr);
  }
  if (st != DUST_OK) return st;
  const bool copies = costs || omega || a_seq || params_out;
  if (costs) TRY(d2h(c, costs, c->costsT, (size_t)c->S * sizeof(float)));
  if (omega) TRY(d2h(c, omega, c->omegaT, (size_t)c->S * sizeof(float)));
  if (a_seq) TRY(d2h(c, a_seq, c->a_seq, (size_t)c->D * sizeof(float)));
  if (params_out) TRY(d2h(c, params_out, c->params_dev, prows * P * sizeof(float)));
  if (roll_steps > 0) TRY(dust_amppi_roll(c, roll_steps));
  // nothing drained the controller's stream: the filter's next update waits for the kernels that read its particles
  if (!copies) TRY(dual_stream_after(c, m->stream, c->stream));
  return DUST_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// B dynamics filters of one configuration (dust_mpf_batch_*): the deep copies of the MPF the reference makes per episode
// (simulations.py:62,78), updated in ONE launch (mpf_optimize_batch_kernel: one workgroup per environment, the single-workgroup form's
// arithmetic).  The batch owns a private clone of the prototype filter - configuration, model, occupancy bits, optimiser options, stream -
// and the per-environment rows: particles, optimiser slots, prior bandwidths and the kernel bandwidth on the device; observations, past
// action and steps taken on the host (they reach the kernel through pinned memory per call: nobody waits for that copy).
struct dust_mpf_batch {
  dust_mpf *m;
  int B;
  DevBuf<float> x;          // [B][Mp][P]
  DevBuf<float> opt_s[3];   // [B][Mp][P] or empty
  DevBuf<float> bw;         // [B] the bandwidth of the last update
  DevBuf<float> prior_bwv;  // [B][4]
  DevBuf<float> gn;         // [B][n_steps] of the last update
  std::vector<float> loc, past_obs, past_action;  // [B][5], [B][5], [B][2]
  std::vector<unsigned char> have_past;
  std::vector<int> opt_t;
  PinnedStage in;      // per-call inputs: MpfEnvIn [B] | prior seeds [B] | SkidLik / CartLik [B] | active mask [B]
  // dust_svmpc_dual_batch_episode: MpfEnvIn [B] - conditioned on the device from period to period - | prior seeds [T][B] | plant rows
  // [B][P], and the pinned bytes they are staged from, once per call (allocated by the first such call)
  DevBuf<unsigned char> ep;
  PinBuf<unsigned char> ep_host;
  hipEvent_t ev_ext;   // behind the last work a dual tick put on a controller batch's stream (AMPPI or SVMPC)
  long long n_launch, n_calls;
  std::vector<dust_mpf_hyper> hyper;  // dust_mpf_batch_set_hyper: the caller's rows [B], or empty (every environment: the prototype's)
  DevBuf<dust_mpf_hyper> hyper_dev;   // [B] while rows are set
};

static size_t mpfb_lik_bytes(const dust_mpf *m) {
  const int model = m->cfg.model_cfg.model;
  return model == DUST_MODEL_SKID_STEER ? sizeof(dust::SkidLik) : (model == DUST_MODEL_CARTPOLE ? sizeof(dust::CartLik) : 0);
}
static size_t mpfb_off_seeds(int B) { return (size_t)B * sizeof(dust::MpfEnvIn); }
static size_t mpfb_off_lik(int B) { return mpfb_off_seeds(B) + (size_t)B * sizeof(uint64_t); }
static size_t mpfb_off_mask(const dust_mpf_batch *mb) { return mpfb_off_lik(mb->B) + (size_t)mb->B * mpfb_lik_bytes(mb->m); }
static size_t mpfb_in_bytes(const dust_mpf_batch *mb) { return mpfb_off_mask(mb) + (size_t)mb->B; }
// where the kernels find the mask a call has staged (nullptr: the call had none - everybody is active), and the prior seeds
static const unsigned char *mpfb_mask_dev(const dust_mpf_batch *mb, const unsigned char *active) { return active ? mb->in.dev.get() + mpfb_off_mask(mb) : nullptr; }
static const uint64_t *mpfb_seeds_dev(const dust_mpf_batch *mb) { return reinterpret_cast<const uint64_t *>(mb->in.dev.get() + mpfb_off_seeds(mb->B)); }
// the typed rows of the stage's bytes (base: a host slot or the device copy): MpfEnvIn [B] in front, SkidLik or CartLik [B], by the model, behind the seeds
static dust::MpfEnvIn *mpfb_in_view(unsigned char *base) { return reinterpret_cast<dust::MpfEnvIn *>(base); }
template <class L>
static L *mpfb_lik_view(unsigned char *base, int B) { return reinterpret_cast<L *>(base + mpfb_off_lik(B)); }

static void mpfb_free(dust_mpf_batch *mb) {
  if (!mb) return;
  if (mb->m) {
    (void)hipSetDevice(mb->m->cfg.device);
    if (mb->ev_ext) (void)hipEventSynchronize(mb->ev_ext);
    (void)hipStreamSynchronize(mb->m->stream);
  }
  dust_mpf *inner = mb->m;
  const hipEvent_t ev = mb->ev_ext;
  delete mb;  // the batch's own rows first, then its event and the filter
  if (ev) (void)hipEventDestroy(ev);
  if (inner) dust_mpf_destroy(inner);
}

// the batch around a filter it takes over: buffers allocated, nothing filled yet
static int mpfb_alloc(dust_mpf *inner, int n_env, dust_mpf_batch **out) {
  dust_mpf_batch *mb = new dust_mpf_batch();
  mb->m = inner;
  mb->B = n_env;
  *out = mb;
  const size_t B = (size_t)n_env, np = (size_t)inner->Mp * inner->P;
  HIP_TRY(hipSetDevice(inner->cfg.device));
  TRY(mb->x.alloc(B * np));
  const DevBuf<float> *const slots = inner->opt_s;
  for (int k = 0; k < 3; ++k)
    if (slots[k]) TRY(mb->opt_s[k].alloc(B * np));
  TRY(mb->bw.alloc(B));
  TRY(mb->prior_bwv.alloc(B * 4));
  HIP_TRY(hipMemset(mb->bw, 0, B * sizeof(float)));
  TRY(mb->in.alloc(mpfb_in_bytes(mb)));
  HIP_TRY(hipEventCreateWithFlags(&mb->ev_ext, hipEventDisableTiming));
  mb->loc.assign(B * 5, 0.f);
  mb->past_obs.assign(B * 5, 0.f);
  mb->past_action.assign(B * 2, 0.f);
  mb->have_past.assign(B, 0);
  mb->opt_t.assign(B, 0);
  return DUST_OK;
}

// work a dual tick left on a controller batch's stream comes first; the filters' own entries are synchronous on their own stream
static int mpfb_settle(dust_mpf_batch *mb) {
  HIP_TRY(hipSetDevice(mb->m->cfg.device));
  HIP_TRY(hipEventSynchronize(mb->ev_ext));
  return DUST_OK;
}

static int mpfb_limits(const dust_mpf *m, int n_env) {
  if (n_env < 1 || n_env > 65535) return fail(DUST_ERR_INVALID, "n_env = %d outside [1, 65535] (one workgroup per environment)", n_env);
  if (m->Mp > 1024 || m->P < 1 || m->P > 4) return fail(DUST_ERR_UNSUPPORTED, "a batched filter takes up to 1024 particles over 1 .. 4 parameters");
  // (the batched kernel's instances are told their model's widths: mpf_optimize_batch_kernel)
  const int model = m->cfg.model_cfg.model, want_ds = model == DUST_MODEL_PENDULUM ? 2 : (model == DUST_MODEL_SKID_STEER ? 5 : 4),
            want_da = (model == DUST_MODEL_PENDULUM || model == DUST_MODEL_CARTPOLE) ? 1 : 2;
  // one particle column per uncertain parameter, as mpf_model_ready asks of a skid-steer or cart-pole filter: the kernel is instantiated
  // for as many columns as the model has parameters
  const int max_p = model == DUST_MODEL_PENDULUM ? 3 : (model == DUST_MODEL_PARTICLE ? 1 : (model == DUST_MODEL_SKID_STEER ? 3 : 4));
  if (m->P > max_p)
    return fail(DUST_ERR_UNSUPPORTED, "a batched filter carries one particle column per uncertain parameter: this model has %d, the filter has dim_p = %d", max_p, m->P);
  if (m->cfg.dim_s != want_ds || m->cfg.dim_a != want_da)
    return fail(DUST_ERR_INVALID, "a batched filter over this model has dim_s = %d, dim_a = %d (got %d, %d)", want_ds, want_da, m->cfg.dim_s, m->cfg.dim_a);
  if (m->cfg.model_cfg.model == DUST_MODEL_PARTICLE && m->cfg.model_cfg.ctrl_noise)
    return fail(DUST_ERR_UNSUPPORTED, "a filter whose model carries control-channel noise draws its per-step actions on the host: no batched form");
  return DUST_OK;
}

extern "C" int dust_mpf_batch_create(const dust_mpf *proto, int n_env, dust_mpf_batch **out) {
  if (!proto || !out) return fail(DUST_ERR_INVALID, "null argument");
  *out = nullptr;
  TRY(mpfb_limits(proto, n_env));
  dust_mpf *inner = nullptr;
  TRY(dust_mpf_clone(proto, &inner));  // (particles, optimiser state, model, occupancy bits)
  dust_mpf_batch *mb = nullptr;
  int st = mpfb_alloc(inner, n_env, &mb);
  if (st == DUST_OK) {
    const size_t np = (size_t)inner->Mp * inner->P;
    const DevBuf<float> *const slots = inner->opt_s;
    std::vector<float> pb((size_t)n_env * 4);
    for (int e = 0; e < n_env && st == DUST_OK; ++e) {
      if (hipMemcpy(mb->x + (size_t)e * np, inner->x, np * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess) st = fail(DUST_ERR_HIP, "hipMemcpy failed");
      for (int k = 0; k < 3 && st == DUST_OK; ++k)
        if (slots[k] && hipMemcpy(mb->opt_s[k] + (size_t)e * np, slots[k], np * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess)
          st = fail(DUST_ERR_HIP, "hipMemcpy failed");
      for (int p = 0; p < 4; ++p) pb[(size_t)e * 4 + p] = inner->prior_bwv[p];
      for (int q = 0; q < 5; ++q) {
        mb->loc[(size_t)e * 5 + q] = inner->loc[q];
        mb->past_obs[(size_t)e * 5 + q] = inner->past_obs[q];
      }
      for (int q = 0; q < 2; ++q) mb->past_action[(size_t)e * 2 + q] = inner->past_action[q];
      mb->have_past[e] = inner->have_past ? 1 : 0;
      mb->opt_t[e] = inner->opt_t;
    }
    if (st == DUST_OK && hipMemcpy(mb->prior_bwv, pb.data(), pb.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) st = fail(DUST_ERR_HIP, "hipMemcpy failed");
  }
  if (st != DUST_OK) {
    mpfb_free(mb);
    return st;
  }
  *out = mb;
  return DUST_OK;
}

extern "C" void dust_mpf_batch_destroy(dust_mpf_batch *mb) { mpfb_free(mb); }

extern "C" int dust_mpf_batch_clone(const dust_mpf_batch *src, dust_mpf_batch **out) {
  if (!src || !out) return fail(DUST_ERR_INVALID, "null argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(src->m->cfg.device));
  HIP_TRY(hipEventSynchronize(src->ev_ext));
  dust_mpf *inner = nullptr;
  TRY(dust_mpf_clone(src->m, &inner));
  dust_mpf_batch *mb = nullptr;
  int st = mpfb_alloc(inner, src->B, &mb);
  if (st == DUST_OK) {
    const size_t B = (size_t)src->B, np = (size_t)inner->Mp * inner->P;
    struct { void *d; const void *s; size_t n; } cp[] = {{mb->x, src->x, B * np * 4}, {mb->opt_s[0], src->opt_s[0], B * np * 4}, {mb->opt_s[1], src->opt_s[1], B * np * 4},
                                                         {mb->opt_s[2], src->opt_s[2], B * np * 4}, {mb->bw, src->bw, B * 4}, {mb->prior_bwv, src->prior_bwv, B * 16}};
    for (auto &c : cp)
      if (st == DUST_OK && c.d && c.s && hipMemcpy(c.d, c.s, c.n, hipMemcpyDeviceToDevice) != hipSuccess) st = fail(DUST_ERR_HIP, "hipMemcpy failed");
    mb->loc = src->loc;
    mb->past_obs = src->past_obs;
    mb->past_action = src->past_action;
    mb->have_past = src->have_past;
    mb->opt_t = src->opt_t;
    if (st == DUST_OK && !src->hyper.empty()) {  // (the host rows are what the device holds: set_hyper uploads before it stores)
      st = mb->hyper_dev.alloc(B);
      if (st == DUST_OK && hipMemcpy(mb->hyper_dev, src->hyper.data(), B * sizeof(dust_mpf_hyper), hipMemcpyHostToDevice) != hipSuccess)
        st = fail(DUST_ERR_HIP, "hipMemcpy failed");
      if (st == DUST_OK) mb->hyper = src->hyper;
    }
  }
  if (st != DUST_OK) {
    mpfb_free(mb);
    return st;
  }
  *out = mb;
  return DUST_OK;
}

// Per-environment filter hyper-parameters: the B trials of a sweep over the filter's own settings as the environments of one batch.
// The rows are checked whole before anything is stored; nothing else of the batch is touched.
static dust_mpf_hyper mpfb_proto_hyper(const dust_mpf *m) {
  dust_mpf_hyper h;
  memset(&h, 0, sizeof h);
  h.lr = m->opt.lr;
  h.obs_std = m->cfg.obs_std;
  h.bw = 0.f;  // (the prototype has no bandwidth of its own: each call names one)
  h.bw_scale = m->cfg.bw_scale;
  return h;
}
extern "C" int dust_mpf_batch_set_hyper(dust_mpf_batch *mb, const dust_mpf_hyper *rows) {
  if (!mb) return fail(DUST_ERR_INVALID, "null batch");
  if (!rows) {  // back to the prototype's: the uniform instances serve the next call
    mb->hyper.clear();
    return DUST_OK;
  }
  const int model = mb->m->cfg.model_cfg.model;
  if (model != DUST_MODEL_PENDULUM && model != DUST_MODEL_PARTICLE)
    return fail(DUST_ERR_UNSUPPORTED, "per-environment filter hyper-parameters are for Pendulum and Particle filters: no rows on a skid-steer or cart-pole filter batch");
  const size_t B = (size_t)mb->B;
  std::vector<dust_mpf_hyper> keep(rows, rows + B);
  for (size_t e = 0; e < B; ++e) {
    dust_mpf_hyper &h = keep[e];
    h.reserved = 0.f;
    auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (!(pos(h.lr) && pos((double)h.obs_std) && pos((double)h.bw_scale) && std::isfinite(h.bw)))
      return fail(DUST_ERR_INVALID, "filter hyper-parameter row %zu: lr, obs_std and bw_scale must be finite and > 0, bw finite (<= 0: Silverman's rule)", e);
  }
  TRY(mpfb_settle(mb));
  TRY(mb->hyper_dev.ensure(B));
  // on the batch's stream, behind every launch that read the old rows
  HIP_TRY(hipMemcpyAsync(mb->hyper_dev, keep.data(), B * sizeof(dust_mpf_hyper), hipMemcpyHostToDevice, mb->m->stream));
  HIP_TRY(hipStreamSynchronize(mb->m->stream));
  mb->hyper.swap(keep);
  return DUST_OK;
}
extern "C" int dust_mpf_batch_get_hyper(dust_mpf_batch *mb, dust_mpf_hyper *rows) {
  if (!mb || !rows) return fail(DUST_ERR_INVALID, "null argument");
  if (!mb->hyper.empty()) std::copy(mb->hyper.begin(), mb->hyper.end(), rows);
  else std::fill(rows, rows + (size_t)mb->B, mpfb_proto_hyper(mb->m));
  return DUST_OK;
}
// while rows are set they carry the bandwidths: the call's own must be <= 0 (ahead of any staging or launch)
static int mpfb_bw_check(const dust_mpf_batch *mb, float bw) {
  if (!mb->hyper.empty() && bw > 0.f)
    return fail(DUST_ERR_INVALID, "the filter batch has per-environment hyper-parameters: the rows carry the bandwidths (rows[b].bw), so the call's bandwidth "
                "must be <= 0 (got %g)", (double)bw);
  return DUST_OK;
}

extern "C" int dust_mpf_batch_set_particles(dust_mpf_batch *mb, const float *x) {
  if (!mb || !x) return fail(DUST_ERR_INVALID, "null argument");
  TRY(mpfb_settle(mb));
  HIP_TRY(hipMemcpyAsync(mb->x, x, (size_t)mb->B * mb->m->Mp * mb->m->P * sizeof(float), hipMemcpyHostToDevice, mb->m->stream));
  HIP_TRY(hipStreamSynchronize(mb->m->stream));
  return DUST_OK;
}
extern "C" int dust_mpf_batch_get_particles(dust_mpf_batch *mb, float *x) {
  if (!mb || !x) return fail(DUST_ERR_INVALID, "null argument");
  TRY(mpfb_settle(mb));
  HIP_TRY(hipMemcpyAsync(x, mb->x, (size_t)mb->B * mb->m->Mp * mb->m->P * sizeof(float), hipMemcpyDeviceToHost, mb->m->stream));
  HIP_TRY(hipStreamSynchronize(mb->m->stream));
  return DUST_OK;
}
extern "C" int dust_mpf_batch_set_obs(dust_mpf_batch *mb, const float *obs) {
  if (!mb || !obs) return fail(DUST_ERR_INVALID, "null argument");
  const int ds = mb->m->cfg.dim_s;
  for (int e = 0; e < mb->B; ++e)
    for (int q = 0; q < ds && q < 5; ++q) mb->loc[(size_t)e * 5 + q] = obs[(size_t)e * ds + q];
  return DUST_OK;
}
extern "C" int dust_mpf_batch_get_prior_bw(dust_mpf_batch *mb, float *bw) {
  if (!mb || !bw) return fail(DUST_ERR_INVALID, "null argument");
  TRY(mpfb_settle(mb));
  HIP_TRY(hipMemcpyAsync(bw, mb->prior_bwv, (size_t)mb->B * 4 * sizeof(float), hipMemcpyDeviceToHost, mb->m->stream));
  HIP_TRY(hipStreamSynchronize(mb->m->stream));
  return DUST_OK;
}
extern "C" int dust_mpf_batch_stats(dust_mpf_batch *mb, long long out[2]) {
  if (!mb || !out) return fail(DUST_ERR_INVALID, "null argument");
  out[0] = mb->n_launch;
  out[1] = mb->n_calls;
  return DUST_OK;
}

// what a batched update refuses, ahead of any copy or launch
static int mpfb_update_check(const dust_mpf_batch *mb, const float *actions, const float *new_obs, int n_steps, const unsigned char *active) {
  const dust_mpf *m = mb->m;
  if (n_steps < 0 || n_steps > 4096) return fail(DUST_ERR_INVALID, "n_steps out of range");
  TRY(mpf_model_ready(m));
  if (new_obs && !actions) return fail(DUST_ERR_INVALID, "condition() needs the action that produced new_obs");
  if (!new_obs)
    for (int e = 0; e < mb->B; ++e)
      if ((!active || active[e]) && !mb->have_past[e]) return fail(DUST_ERR_STATE, "Previous action is None. Need at least one observation to start sampling.");
  return mpf_grid_ready(m);
}

// The per-call inputs through the next pinned slot and - with `update` - the filter side of a period on `stream`: GaussianLikelihood.condition
// of every active environment (likelihoods.py:51-64, on the host rows), the heading / angle terms of all environments in one launch
// (skid-steer, cart-pole), Silverman's rule of all in one launch (bw <= 0), the update of all in one launch.  Nothing waits for the device.
// The host rows an update moves on (observations, past action, steps taken): mpfb_enqueue fills them, the caller commits them once every
// launch of its call has been enqueued - a call that fails on the way leaves the filters' host rows where they were.
struct MpfbRows {
  std::vector<float> loc, past_obs, past_action;
  std::vector<unsigned char> have_past;
  std::vector<int> opt_t;
  bool filled = false;
};
static void mpfb_commit(dust_mpf_batch *mb, MpfbRows &w) {
  if (!w.filled) return;
  mb->loc.swap(w.loc);
  mb->past_obs.swap(w.past_obs);
  mb->past_action.swap(w.past_action);
  mb->have_past.swap(w.have_past);
  mb->opt_t.swap(w.opt_t);
}

// mpf_optimize_batch_kernel of one model, instantiated for the particle columns Ps, x log space or not x Adam or not; false: P is none of Ps
template <int MODEL, int... Ps>
static bool mpfb_launch(const dust_mpf *m, int B, hipStream_t stream, const MpfBatchArgs &k, int *st) {
  constexpr bool CART = MODEL == DUST_MODEL_CARTPOLE;
  return mpf_pick<Ps...>(m->P, m->cfg.log_space != 0, [&](auto p, auto lg) {
    if (m->opt.kind == DUST_OPT_ADAM) *st = mpf_wg_launch(mpf_optimize_batch_kernel<p(), CART, MODEL, lg(), true>, B, mpf_wg(m), stream, k);
    else *st = mpf_wg_launch(mpf_optimize_batch_kernel<p(), CART, MODEL, lg(), false>, B, mpf_wg(m), stream, k);
  });
}

// the rows form (dust_mpf_batch_set_hyper): mpf_optimize_rows_kernel of a Pendulum or Particle filter
template <int MODEL, int... Ps>
static bool mpfb_launch_rows(const dust_mpf *m, int B, hipStream_t stream, const MpfRowsArgs &k, int *st) {
  return mpf_pick<Ps...>(m->P, m->cfg.log_space != 0, [&](auto p, auto lg) {
    if (m->opt.kind == DUST_OPT_ADAM) *st = mpf_wg_launch(mpf_optimize_rows_kernel<p(), MODEL, lg(), true>, B, mpf_wg(m), stream, k);
    else *st = mpf_wg_launch(mpf_optimize_rows_kernel<p(), MODEL, lg(), false>, B, mpf_wg(m), stream, k);
  });
}

// GaussianLikelihood.condition of every active environment (likelihoods.py:51-64) on copies of the host rows (`w`; new_obs NULL: the
// rows as they stand), and what the update of `n_steps` steps reads of them: MpfEnvIn [B] in front of the stage's bytes `hb`, and the
// skid-steer / cart-pole likelihood rows behind the seeds
static void mpfb_rows(const dust_mpf_batch *mb, const float *actions, const float *new_obs, const int n_steps, const unsigned char *active, unsigned char *hb,
                      MpfbRows &w) {
  const dust_mpf *m = mb->m;
  const int B = mb->B, ds = m->cfg.dim_s, da = m->cfg.dim_a, model = m->cfg.model_cfg.model;
  dust::MpfEnvIn *in = mpfb_in_view(hb);
  w.loc = mb->loc;
  w.past_obs = mb->past_obs;
  w.past_action = mb->past_action;
  w.have_past = mb->have_past;
  w.opt_t = mb->opt_t;
  w.filled = true;
  for (int e = 0; e < B; ++e) {
    float *loc = &w.loc[(size_t)e * 5], *past = &w.past_obs[(size_t)e * 5], *pa = &w.past_action[(size_t)e * 2];
    const bool on = !active || active[e];
    if (on && new_obs) {
      memcpy(past, loc, 5 * sizeof(float));
      for (int q = 0; q < ds && q < 5; ++q) loc[q] = new_obs[(size_t)e * ds + q];
      for (int q = 0; q < 2; ++q) pa[q] = q < da ? actions[(size_t)e * da + q] : 0.f;
      w.have_past[e] = 1;
    }
    memset(&in[e], 0, sizeof in[e]);
    for (int q = 0; q < 4; ++q) {
      in[e].past_obs[q] = past[q];
      in[e].obs[q] = loc[q];
    }
    in[e].past_action[0] = pa[0];
    in[e].past_action[1] = pa[1];
    in[e].t0 = w.opt_t[e];
    if (model == DUST_MODEL_SKID_STEER) mpf_skid_lik(m, pa, past, loc, mpfb_lik_view<dust::SkidLik>(hb, B)[e]);
    if (model == DUST_MODEL_CARTPOLE) mpf_cart_lik(m, pa, past, loc, mpfb_lik_view<dust::CartLik>(hb, B)[e]);
    if (on) w.opt_t[e] += n_steps;
  }
}

// The launches of an update on `stream`: the heading / angle terms of all environments in one launch (skid-steer, cart-pole), Silverman's
// rule of all in one launch (bw <= 0), the update of all in one launch.  `in`: the MpfEnvIn rows on the device; `mask`: the staged mask
static int mpfb_update_launch(dust_mpf_batch *mb, hipStream_t stream, const dust::MpfEnvIn *in, const unsigned char *mask, const float bw, const int n_steps) {
  dust_mpf *m = mb->m;
  const int B = mb->B, model = m->cfg.model_cfg.model;
  const bool cart = model == DUST_MODEL_CARTPOLE;
  if (model == DUST_MODEL_SKID_STEER) {
    dust::mpf_lik_angle_batch_kernel<dust::SkidLik><<<(B + 255) / 256, 256, 0, stream>>>(mpfb_lik_view<dust::SkidLik>(mb->in.dev.get(), B), B, mask);
    HIP_TRY(hipGetLastError());
    mb->n_launch++;
  }
  if (cart) {
    dust::mpf_lik_angle_batch_kernel<dust::CartLik><<<(B + 255) / 256, 256, 0, stream>>>(mpfb_lik_view<dust::CartLik>(mb->in.dev.get(), B), B, mask);
    HIP_TRY(hipGetLastError());
    mb->n_launch++;
  }
  const int n = m->Mp * m->P;
  const bool rows = !mb->hyper.empty();  // (Pendulum or Particle: dust_mpf_batch_set_hyper; bw <= 0: mpfb_bw_check)
  if (rows) {
    if (bw > 0.f) return fail(DUST_ERR_INVALID, "the rows carry the bandwidths");
    dust::mpf_silverman_rows_kernel<<<B, 1024, (size_t)n * sizeof(float), stream>>>(mb->x, n, mb->hyper_dev, mb->bw, mask);
    HIP_TRY(hipGetLastError());
    mb->n_launch++;
  } else if (!(bw > 0.f)) {
    dust::mpf_silverman_batch_kernel<<<B, 1024, (size_t)n * sizeof(float), stream>>>(mb->x, n, m->cfg.bw_scale, mb->bw, mask);
    HIP_TRY(hipGetLastError());
    mb->n_launch++;
  }
  MpfBatchArgs k;
  memset(&k, 0, sizeof k);
  MpfArgs &a = k.a;
  mpf_shared_args(m, n_steps, a);
  a.log_space = m->cfg.log_space ? 1 : 0;  // (0 / 1: the instance is told which)
  a.dm.log_space = a.log_space;
  a.x = mb->x;
  a.grad_norms = mb->gn;
  a.opt = m->opt;
  a.opt_s0 = mb->opt_s[0];
  a.opt_s1 = mb->opt_s[1];
  a.opt_s2 = mb->opt_s[2];
  k.in = in;
  k.prior_bwv = mb->prior_bwv;
  k.bw = mb->bw;
  k.bw_fixed = bw > 0.f ? bw : 0.f;
  k.gn_stride = n_steps;
  k.skl = mpfb_lik_view<dust::SkidLik>(mb->in.dev.get(), B);
  k.cpl = mpfb_lik_view<dust::CartLik>(mb->in.dev.get(), B);
  k.active = mask;
  // (P up to the model's parameter count: mpfb_limits has refused the rest)
  int st = DUST_OK;
  if (rows) {
    MpfRowsArgs kr;
    kr.k = k;
    kr.rows = mb->hyper_dev;
    if (model == DUST_MODEL_PARTICLE) {
      if (!mpfb_launch_rows<DUST_MODEL_PARTICLE, 1>(m, B, stream, kr, &st))
        return fail(DUST_ERR_UNSUPPORTED, "no batched filter kernel for a Particle filter over %d particle columns", m->P);
    } else if (!mpfb_launch_rows<DUST_MODEL_PENDULUM, 1, 2, 3>(m, B, stream, kr, &st)) {
      return fail(DUST_ERR_UNSUPPORTED, "no batched filter kernel for a Pendulum filter over %d particle columns", m->P);
    }
  } else if (cart) {
    mpfb_launch<DUST_MODEL_CARTPOLE, 1, 2, 3, 4>(m, B, stream, k, &st);
  } else if (model == DUST_MODEL_SKID_STEER) {
    if (!mpfb_launch<DUST_MODEL_SKID_STEER, 1, 2, 3>(m, B, stream, k, &st))
      return fail(DUST_ERR_UNSUPPORTED, "no batched filter kernel for a skid-steer filter over %d particle columns", m->P);
  } else if (model == DUST_MODEL_PARTICLE) {
    if (!mpfb_launch<DUST_MODEL_PARTICLE, 1>(m, B, stream, k, &st))
      return fail(DUST_ERR_UNSUPPORTED, "no batched filter kernel for a Particle filter over %d particle columns", m->P);
  } else {
    if (!mpfb_launch<DUST_MODEL_PENDULUM, 1, 2, 3>(m, B, stream, k, &st))
      return fail(DUST_ERR_UNSUPPORTED, "no batched filter kernel for a Pendulum filter over %d particle columns", m->P);
  }
  TRY(st);
  HIP_TRY(hipGetLastError());
  mb->n_launch++;
  return DUST_OK;
}

static int mpfb_enqueue(dust_mpf_batch *mb, hipStream_t stream, const bool update, const float *actions, const float *new_obs, const float bw,
                        const int n_steps, const unsigned char *active, const uint64_t *seeds, MpfbRows &w) {
  dust_mpf *m = mb->m;
  const int B = mb->B;
  unsigned char *hb;
  TRY(mb->in.next(&hb));
  if (seeds) memcpy(hb + mpfb_off_seeds(B), seeds, (size_t)B * sizeof(uint64_t));
  if (active) memcpy(hb + mpfb_off_mask(mb), active, (size_t)B);
  if (update) mpfb_rows(mb, actions, new_obs, n_steps, active, hb, w);
  // (without an update the likelihood rows between the seeds and the mask are not read: the copy may carry whatever the slot holds; the
  // seeds lie in the range either way: there is always something to copy)
  TRY(mb->in.send(update ? 0 : mpfb_off_seeds(B), active ? mpfb_in_bytes(mb) : mpfb_off_mask(mb), stream));
  if (!update) return DUST_OK;
  serve_cancel_device(m->cfg.device);  // (as mpf_launch: an armed control tick would hold every CU until its plant state arrives)
  return mpfb_update_launch(mb, stream, mpfb_in_view(mb->in.dev.get()), mpfb_mask_dev(mb, active), bw, n_steps);
}

// room for grad_norms [B][n_steps] (a reallocation frees behind the device's queued work)
static int mpfb_gn_room(dust_mpf_batch *mb, int n_steps) { return mb->gn.ensure((size_t)mb->B * (size_t)(n_steps > 0 ? n_steps : 1)); }

// B x dust_mpf_optimize in one launch (plus one for Silverman's rule when bw <= 0, plus one for the heading / angle terms of a skid-steer /
// cart-pole filter): environment b computes what a lone filter under DUST_MPF_GRID=0 computes on its inputs, bit for bit.
extern "C" int dust_mpf_batch_optimize(dust_mpf_batch *mb, const float *actions, const float *new_obs, float bw, int n_steps, const unsigned char *active,
                                       float *bw_used, float *grad_norms) {
  if (!mb) return fail(DUST_ERR_INVALID, "null batch");
  TRY(mpfb_bw_check(mb, bw));
  TRY(mpfb_update_check(mb, actions, new_obs, n_steps, active));
  TRY(mpfb_settle(mb));
  TRY(mpfb_gn_room(mb, n_steps));
  hipStream_t st = mb->m->stream;
  MpfbRows rows;
  TRY(mpfb_enqueue(mb, st, true, actions, new_obs, bw, n_steps, active, nullptr, rows));
  mpfb_commit(mb, rows);
  mb->n_calls++;
  if (bw_used) TRY(rows_d2h(mb->B, st, bw_used, mb->bw, 1, active));
  if (grad_norms && n_steps > 0) TRY(rows_d2h(mb->B, st, grad_norms, mb->gn, (size_t)n_steps, active));
  HIP_TRY(hipStreamSynchronize(st));
  return DUST_OK;
}

// What the dual ticks of the two controller batches (dust_amppi_dual_batch_tick, dust_svmpc_dual_batch_tick) share.
// The pair: controller and filters agree, and there are as many of one as of the other.  `kind`: the controller batch's name.  (Each
// entry's own refusals lie between these and the filters' in dual_batch_filters.)
static int dual_batch_pair_check(const dust_ctx *c, const char *kind, int B, const dust_mpf_batch *mb) {
  TRY(dual_pair_check(c, mb->m));
  if (B != mb->B) return fail(DUST_ERR_INVALID, "the %s batch has %d environments, the filter batch %d", kind, B, mb->B);
  return DUST_OK;
}

// The filter side of a period on the controller batch's stream: the filters' refusals, ahead of any copy or launch; the controller's
// pending work settled; stage() - what the entry allocates or copies ahead of the filters' launches; then, behind another batch's tick
// on these filters (its stream first, without a host wait), the per-call inputs and the update (skipped when actions_prev is NULL)
template <class Stage>
static int dual_batch_filters(dust_ctx *c, dust_mpf_batch *mb, const float *states, const float *actions_prev, int mpf_steps, float mpf_bw,
                              const uint64_t *prior_seeds, const unsigned char *active, MpfbRows &rows, Stage stage) {
  TRY(mpfb_limits(mb->m, mb->B));
  TRY(mpfb_bw_check(mb, mpf_bw));
  if (actions_prev) TRY(mpfb_update_check(mb, actions_prev, states, mpf_steps, active));
  HIP_TRY(hipSetDevice(c->cfg.device));
  TRY(settle_pending(c));
  // (reallocations free behind the device's queued work; they happen in the first period only)
  if (actions_prev) TRY(mpfb_gn_room(mb, mpf_steps));
  TRY(stage());
  HIP_TRY(hipStreamWaitEvent(c->stream, mb->ev_ext, 0));
  TRY(mpfb_enqueue(mb, c->stream, actions_prev != nullptr, actions_prev, states, mpf_bw, mpf_steps, active, prior_seeds, rows));
  mb->n_calls++;
  return DUST_OK;
}

// the filters' priors as either tick's kernels take them (AmppiPriorBatch, SvbPrior: two types with these fields)
template <class Prior>
static void dual_batch_prior(const dust_mpf_batch *mb, float *params_out, Prior &pr) {
  memset(&pr, 0, sizeof pr);
  pr.means = mb->x;
  pr.K = mb->m->Mp;
  pr.P = mb->m->P;
  pr.bwv = mb->prior_bwv;
  pr.seeds = mpfb_seeds_dev(mb);
  pr.params_out = params_out;
}

// The close of a period, in two steps.  dual_batch_bw, behind the tick's launch and the entry's own output copies: the filters' host
// rows move on (every launch of the period is enqueued) and bw_used is answered - on the host where the call fixed the bandwidth or
// skipped the update, else by a copy of Silverman's values on the stream (*copies is then set).  dual_batch_close: ev_ext behind all of
// it (the filters' own entries, and another batch's tick on these filters, wait for it), and the wait where something was copied out
static int dual_batch_bw(dust_ctx *c, dust_mpf_batch *mb, MpfbRows &rows, const float *actions_prev, float mpf_bw, const unsigned char *active,
                         float *bw_used, bool *copies) {
  mpfb_commit(mb, rows);
  const bool bw_dev = bw_used && actions_prev && !(mpf_bw > 0.f);
  if (bw_used && !bw_dev)
    for (int e = 0; e < mb->B; ++e)
      if (!active || active[e]) bw_used[e] = actions_prev ? mpf_bw : 0.f;
  if (bw_dev) {
    TRY(rows_d2h(mb->B, c->stream, bw_used, mb->bw, 1, active));
    *copies = true;
  }
  return DUST_OK;
}
static int dual_batch_close(dust_ctx *c, dust_mpf_batch *mb, bool copies) {
  HIP_TRY(hipEventRecord(mb->ev_ext, c->stream));
  if (copies) HIP_TRY(hipStreamSynchronize(c->stream));
  return DUST_OK;
}

// One control period of the dual loop for B environments in one call (B x dust_amppi_dual_tick): on the AMPPI batch's stream, in launch
// order and without an event or a wait in between - the filters' update for (actions_prev[b], states[b]) (skipped when actions_prev is
// NULL; mpf_bw <= 0: Silverman's rule per environment, on the device, handed to the update in device memory), the parameters from every
// environment's refreshed prior ("extended": drawn inside the tick's kernel, amppi_prior_batch_kernel; DUST_AMPPI_PARAMS_SHARED: one
// staged row per environment; sigma weights + a scale: staged sigma points), the B ticks, the outputs, the roll.  The number of launches
// does not depend on B.  Environment b's draws take the key prior_seeds[b].  An environment with active[b] = 0 keeps its particles,
// optimiser state, bandwidths, sequence and stream position, and its output rows are not written.  With every output NULL the call
// returns without waiting for the device.
extern "C" int dust_amppi_dual_batch_tick(dust_amppi_batch *b, dust_mpf_batch *mb, const float *states, const float *actions_prev, const float *actions,
                                          int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds, int roll_steps, const unsigned char *active,
                                          float *costs, float *omega, float *a_seq, float *params_out, float *bw_used) {
  if (!b || !mb || !states) return fail(DUST_ERR_INVALID, "null argument");
  if (mpf_steps < 0 || roll_steps < 0) return fail(DUST_ERR_INVALID, "bad step counts");
  dust_ctx *c = b->c;
  dust_mpf *m = mb->m;
  TRY(amppi_check(c));
  TRY(dual_batch_pair_check(c, "AMPPI", b->B, mb));
  bool sigma, shared;
  TRY(amppi_dual_check(c, m, flags, &sigma, &shared));
  if (!sigma && !prior_seeds) return fail(DUST_ERR_INVALID, "null argument: the draws from the filters' priors need prior_seeds [B]");
  const size_t B = (size_t)b->B, S = (size_t)c->S, D = (size_t)c->D, P = (size_t)m->P;
  const size_t prows = sigma ? (size_t)c->M : (shared ? (size_t)1 : S);
  MpfbRows rows;
  TRY(dual_batch_filters(c, mb, states, actions_prev, mpf_steps, mpf_bw, prior_seeds, active, rows, [&]() -> int {
    return sigma || shared || params_out ? b->params.ensure(B * prows * P) : DUST_OK;
  }));
  const unsigned char *mask = mpfb_mask_dev(mb, active);
  int st;
  if (sigma || shared) {
    if (sigma) dust::mpf_sigma_points_batch_kernel<<<b->B, 256, 0, c->stream>>>(mb->x, m->Mp, m->P, mb->prior_bwv, c->sigma_scale, b->params, mask);
    else dust::mpf_sample_batch_kernel<<<(b->B + 255) / 256, 256, 0, c->stream>>>(mb->x, m->Mp, m->P, mb->prior_bwv, mpfb_seeds_dev(mb), b->B, b->params, mask);
    HIP_TRY(hipGetLastError());
    mb->n_launch++;
    st = batch_update_launch(b, states, actions, b->params, flags, active, true, nullptr);
  } else {
    dust::AmppiPriorBatch pr;
    dual_batch_prior(mb, params_out ? b->params : nullptr, pr);
    st = batch_update_launch(b, states, actions, nullptr, flags, active, false, &pr);
  }
  if (st != DUST_OK) return st;
  bool copies = costs || omega || a_seq || params_out;
  if (costs) TRY(rows_d2h(b->B, c->stream, costs, b->costs, S, active));
  if (omega) TRY(rows_d2h(b->B, c->stream, omega, b->omega, S, active));
  if (a_seq) TRY(rows_d2h(b->B, c->stream, a_seq, b->a_seq, D, active));
  if (params_out) TRY(rows_d2h(b->B, c->stream, params_out, b->params, prows * P, active));
  TRY(dual_batch_bw(c, mb, rows, actions_prev, mpf_bw, active, bw_used, &copies));
  if (roll_steps > 0) TRY(batch_roll_launch(b, roll_steps, active));  // (dust_amppi_batch_roll on the mask this call has staged already)
  return dual_batch_close(c, mb, copies);
}

// One control period of the DuSt-MPC loop (simulations.py:104-138) for B environments in one call (B x dust_dual_tick): on the SVMPC
// batch's stream, in launch order and without an event or a wait in between - the filters' update for (actions_prev[b], states[b])
// (skipped when actions_prev is NULL; mpf_bw <= 0: Silverman's rule per environment, on the device), then ONE launch of
// svmpc_prior_batch_kernel: n_steps SVGD iterations, whose dynamics samples every workgroup draws from its environment's refreshed prior
// (row it M + m of dust_mpf_prior_sample(filter b, n_steps M, prior_seeds[b])), and forward().  Recorded noise from the host is staged
// AHEAD of the filters' launches (that copy waits for the stream).  The number of launches does not depend on B.  An environment with
// active[b] = 0 keeps everything on both sides, and its output rows are not written.  With every output NULL the call returns without
// waiting for the device.
// do_forward = false: the period WITHOUT forward() (dust_svmpc_dual_batch_optimize) - the same launches, svmpc_prior_batch_kernel told so
static int svb_dual_period_call(dust_svmpc_batch *b, dust_mpf_batch *mb, const float *states, const float *actions_prev, int n_steps, const void *eps,
                                int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds, const unsigned char *active, const bool do_forward,
                                float *a_seq, float *p_weights, float *params_out, float *bw_used) {
  if (!b || !mb || !states) return fail(DUST_ERR_INVALID, "null argument");
  if (n_steps < 1 || mpf_steps < 0) return fail(DUST_ERR_INVALID, "bad step counts");
  dust_ctx *c = b->c;
  TRY(svb_call_check(b, states, n_steps, nullptr, true, flags, do_forward));  // (sigma-point weights among it: no batched sigma rollouts)
  TRY(dual_batch_pair_check(c, "SVMPC", b->B, mb));
  if (!prior_seeds) return fail(DUST_ERR_INVALID, "null argument: the draws from the filters' priors need prior_seeds [B]");
  const size_t prow = (size_t)n_steps * (size_t)c->M * (size_t)mb->m->P;
  const float *eps_dev;
  MpfbRows rows;
  TRY(dual_batch_filters(c, mb, states, actions_prev, mpf_steps, mpf_bw, prior_seeds, active, rows, [&]() -> int {
    if (params_out) TRY(b->params.ensure((size_t)b->B * prow));
    return svb_stage(b, n_steps, eps, nullptr, flags, &eps_dev);
  }));
  dust::SvbPrior pr;
  dual_batch_prior(mb, params_out ? b->params : nullptr, pr);
  // (a REFUSAL cannot come from here on: every check ran above.  A runtime error of svb_go - a pinned slot, a failed launch - leaves the
  // filters' update enqueued without mpfb_commit: their host rows (loc / past / opt_t) then lag the device, as under
  // dust_amppi_dual_batch_tick; such an error is not recoverable for the pair)
  TRY(svb_go(b, states, n_steps, eps_dev, nullptr, flags, active, do_forward, &pr));
  bool copies = a_seq || p_weights || params_out;
  TRY(svb_outputs_copy(b, active, a_seq, p_weights));
  if (params_out) TRY(rows_d2h(b->B, c->stream, params_out, b->params, prow, active));
  TRY(dual_batch_bw(c, mb, rows, actions_prev, mpf_bw, active, bw_used, &copies));
  return dual_batch_close(c, mb, copies);
}
extern "C" int dust_svmpc_dual_batch_tick(dust_svmpc_batch *b, dust_mpf_batch *mb, const float *states, const float *actions_prev, int n_steps,
                                          const void *eps, int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds,
                                          const unsigned char *active, float *a_seq, float *p_weights, float *params_out, float *bw_used) {
  return svb_dual_period_call(b, mb, states, actions_prev, n_steps, eps, flags, mpf_steps, mpf_bw, prior_seeds, active, true, a_seq, p_weights,
                              params_out, bw_used);
}
// One WARM-UP period of the loop (simulations.py:104-117 while step < warm_up): the tick above without forward() - the filters' update,
// then the one launch of svmpc_prior_batch_kernel with do_forward = 0: n_steps SVGD iterations under rows drawn from the refreshed priors.
// The batch is left where dust_svmpc_batch_optimize fed params_out leaves it; the Philox position moves by the iterations alone.
extern "C" int dust_svmpc_dual_batch_optimize(dust_svmpc_batch *b, dust_mpf_batch *mb, const float *states, const float *actions_prev, int n_steps,
                                              const void *eps, int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds,
                                              const unsigned char *active, float *params_out, float *bw_used) {
  return svb_dual_period_call(b, mb, states, actions_prev, n_steps, eps, flags, mpf_steps, mpf_bw, prior_seeds, active, false, nullptr, nullptr,
                              params_out, bw_used);
}

// The epilogue of a dual episode (dust_svmpc_dual_batch_episode, dust_amppi_dual_batch_episode) behind its one wait: bw_out where it is
// answered on the host, and the filters' host rows moved to where T ticks leave them, from the MpfEnvIn rows read back (in_host)
// ran (dust_svmpc_dual_batch_simulate): the periods environment e ran, in place of T - none: its rows stay where they were
static void dual_episode_commit(dust_mpf_batch *mb, MpfbRows &rows, const std::vector<dust::MpfEnvIn> &in_host, size_t n_periods, bool first, bool silverman,
                                float mpf_bw, const unsigned char *active, float *bw_out, const int *ran = nullptr) {
  const size_t B = (size_t)mb->B;
  for (size_t e = 0; e < B; ++e) {
    if (active && !active[e]) continue;
    const size_t T = ran ? (size_t)ran[e] : n_periods;
    if (T == 0) continue;
    if (bw_out) {  // what bw_used of the period's dual tick is: 0 without an update, the fixed bandwidth, or Silverman's (recorded above)
      if (!first) bw_out[e] = 0.f;
      if (!silverman)
        for (size_t t = first ? 0 : 1; t < T; ++t) bw_out[t * B + e] = mpf_bw;
    }
    // the filters' host rows: what the last update read, and the steps taken since
    const dust::MpfEnvIn &r = in_host[e];
    float *loc = &rows.loc[e * 5], *past = &rows.past_obs[e * 5];
    if (T > 1) {  // (conditioned on the device at least once: condition() copies the five-wide row, whose fifth column no state here reaches)
      past[4] = loc[4];
      rows.have_past[e] = 1;
    }
    for (int q = 0; q < 4; ++q) {
      loc[q] = r.obs[q];
      past[q] = r.past_obs[q];
    }
    rows.past_action[e * 2] = r.past_action[0];
    rows.past_action[e * 2 + 1] = r.past_action[1];
    rows.opt_t[e] = r.t0;
  }
  mpfb_commit(mb, rows);
}

// What the two dual episodes stage for their filters, once per call, through the filter batch's pinned block: the MpfEnvIn rows as period
// 0's update reads them (or, without one, as they stand), the seeds [T][B], the plant rows [B][P] - and what they read back of it
struct DualEpisodeStage {
  dust_mpf_batch *mb;
  size_t T, B, off_seeds, off_plant, n_stage;
  bool first;  // period 0 has an update
  MpfbRows rows;
  std::vector<dust::MpfEnvIn> in_host;
  DualEpisodeStage(dust_mpf_batch *filters, size_t periods, size_t n_env, size_t P, bool has_first)
      : mb(filters), T(periods), B(n_env), off_seeds(n_env * sizeof(dust::MpfEnvIn)), off_plant(off_seeds + periods * n_env * sizeof(uint64_t)),
        n_stage(off_plant + n_env * P * sizeof(float)), first(has_first), in_host(n_env) {}
  // room (reallocations free behind the device's queued work)
  int room(int mpf_steps) {
    TRY(mpfb_gn_room(mb, mpf_steps));
    TRY(mb->ep.ensure(n_stage));
    if (mb->ep_host.cap() < n_stage) TRY(mb->ep_host.alloc(n_stage, hipHostMallocDefault));
    return DUST_OK;
  }
  // the rows of the environments of `on`, seeds and plants -> the device in one copy on the controller's stream, behind the filters' last work
  int stage(const dust_ctx *c, const float *states, const float *actions_prev, int mpf_steps, const unsigned char *on, const uint64_t *prior_seeds,
            const float *plant_params) {
    unsigned char *hb = mb->ep_host;  // (free: every call that wrote it has waited for its stream)
    mpfb_rows(mb, actions_prev, first ? states : nullptr, first ? mpf_steps : 0, on, hb, rows);
    memcpy(hb + off_seeds, prior_seeds, off_plant - off_seeds);
    if (plant_params) memcpy(hb + off_plant, plant_params, n_stage - off_plant);
    HIP_TRY(hipStreamWaitEvent(c->stream, mb->ev_ext, 0));
    HIP_TRY(hipMemcpyAsync(mb->ep, hb, plant_params ? n_stage : off_plant, hipMemcpyHostToDevice, c->stream));
    return DUST_OK;
  }
  dust::MpfEnvIn *in_dev() const { return mpfb_in_view(mb->ep.get()); }
  const uint64_t *seeds_dev(size_t t) const { return reinterpret_cast<const uint64_t *>(mb->ep.get() + off_seeds) + t * B; }
  const float *plant_dev(const float *plant_params) const { return plant_params ? reinterpret_cast<const float *>(mb->ep.get() + off_plant) : nullptr; }
  // behind the periods: the records and the advanced rows come back, ...
  int read_back(const dust_ctx *c, std::vector<float> &host, const float *rec) {
    HIP_TRY(hipMemcpyAsync(host.data(), rec, host.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(in_host.data(), in_dev(), B * sizeof(dust::MpfEnvIn), hipMemcpyDeviceToHost, c->stream));
    return DUST_OK;
  }
  // ... the call waits once (the filters' own stream waits for ev_ext before it touches the rows again), ...
  int wait(const dust_ctx *c) {
    HIP_TRY(hipEventRecord(mb->ev_ext, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DUST_OK;
  }
  // ... and the filters' host rows move to where the periods left them
  void commit(float mpf_bw, const unsigned char *on, float *bw_out, const int *ran = nullptr) {
    dual_episode_commit(mb, rows, in_host, T, first, !(mpf_bw > 0.f), mpf_bw, on, bw_out, ran);
  }
};

// T control periods of the DuSt-MPC loop (simulations.py:104-138) for B environments in one call: T successive dust_svmpc_dual_batch_tick
// calls with device-drawn noise, and between them the plant of dust_svmpc_batch_episode - x_{t+1} = step(x_t, a_t) under the true rows
// plant_params - stepped on the device.  Everything is staged once (states and mask through the controller batch's pinned slot; the
// filters' MpfEnvIn rows, the seeds [T][B] and the plant rows through the filter batch's); then, on the controller batch's stream and in
// launch order, period t is: Silverman's rule (mpf_bw <= 0) and the filters' update, when the period has an action (t >= 1, or
// actions_prev), reading the MpfEnvIn rows IN DEVICE MEMORY, and one launch of svmpc_dual_period_kernel - the PRIOR tick under the key row
// prior_seeds + t B, the plant, the records, and the conditioning of the MpfEnvIn rows for period t + 1.  No host wait, event or copy lies
// between two periods; the call waits once, for the records, reads the MpfEnvIn rows back and moves the filters' host rows to where T
// ticks leave them: the pair (a_{T-1}, x_T) is NOT folded in (the last period conditions nothing).
//
// rules (dust_svmpc_dual_batch_simulate; NULL: dust_svmpc_dual_batch_episode): the episode under the reference's rules
// (run_pendulum_simulation(mpf=...), simulations.py:104-138; the Particle loop's crash and goal, 217-260).  The mask that is staged - always,
// so that it is never NULL - is then the RUN MASK active[b] && status[b] == 0: every launch of the call - Silverman, the update, the period
// kernel - takes it, and lane 0 of svmpc_dual_sim_period_kernel clears an environment's byte in the period that stops it, so a stopped
// environment takes no further update and no tick.  The rules' words [B] loss | status | n_run lie behind the records.  The host queues T
// period launches whatever stops; per launch it sets do_forward = (t0 + t >= warm_up).  Afterwards environment b is, on both sides, where
// n_run[b] per-period calls would have left it (dust_svmpc_dual_batch_optimize while warming up, dust_svmpc_dual_batch_tick afterwards):
// the filters' host rows are committed from n_run[b], not from T.
static int svb_dual_episode_call(dust_svmpc_batch *b, dust_mpf_batch *mb, const float *states, const float *actions_prev, int n_periods, int n_steps,
                                 int mpf_steps, float mpf_bw, const uint64_t *prior_seeds, const float *plant_params, const dust_episode_rules *rules,
                                 int flags, const unsigned char *active, float *states_out, float *actions_out, float *pw_out, float *bw_out,
                                 float *costs_out, float *loss, int *status, int *n_run, float *a_seq) {
  if (!b || !mb || !states || !states_out || !actions_out) return fail(DUST_ERR_INVALID, "null argument");
  if (rules && (!loss || !status || !n_run || !costs_out)) return fail(DUST_ERR_INVALID, "null argument: loss, status, n_run and costs_out are required");
  if (!prior_seeds) return fail(DUST_ERR_INVALID, "null argument: the draws from the filters' priors need prior_seeds [T][B]");
  TRY(episode_periods_check(n_periods, "the queue of one call stays short on a shared device: chain a longer episode"));
  if (n_steps < 1 || mpf_steps < 0) return fail(DUST_ERR_INVALID, "bad step counts");
  if (flags != 0) return fail(DUST_ERR_UNSUPPORTED, "a dual episode draws its noise on the device and keeps no actions: flags must be 0 (got %d)", flags);
  dust_ctx *c = b->c;
  dust_mpf *m = mb->m;
  TRY(episode_plant_check(c, plant_params));
  const size_t T = (size_t)n_periods, B = (size_t)b->B, N = (size_t)c->N, P = (size_t)c->cfg.dim_p, D = (size_t)c->D;
  bool forward = true;  // some period of the call runs forward()
  if (rules) {
    TRY(rules_check(c, rules, B, active, status, false, true));
    forward = rules->t0 + n_periods > rules->warm_up;
  }
  const int record = rules ? b->hist_what : 0;  // (the rule-driven episode alone records: dust_svmpc_batch_set_history)
  const size_t x_row = (size_t)m->Mp * (size_t)m->P;
  TRY(svb_hist_check(b, record, T, x_row));
  TRY(svb_call_check(b, states, n_steps, nullptr, true, 0, forward));
  TRY(dual_batch_pair_check(c, "SVMPC", b->B, mb));
  auto host_lik = [](int model) { return model == DUST_MODEL_SKID_STEER || model == DUST_MODEL_CARTPOLE; };
  if (host_lik(c->cfg.model) || host_lik(m->cfg.model_cfg.model))
    return fail(DUST_ERR_UNSUPPORTED,
                "a dual episode conditions the filters on the device: Pendulum and Particle pairs (a skid-steer or cart-pole filter's likelihood rows "
                "carry the host's sin / cos of the past heading: dust_svmpc_dual_batch_tick per period)");
  TRY(mpfb_limits(m, mb->B));
  TRY(mpfb_bw_check(mb, mpf_bw));
  const bool first = actions_prev != nullptr;  // period 0 has an update
  // (the periods behind the first always have one; its refusals depend on whether its arguments are there, not on their values)
  if (first || n_periods > 1) TRY(mpfb_update_check(mb, first ? actions_prev : states, states, mpf_steps, active));
  HIP_TRY(hipSetDevice(c->cfg.device));
  TRY(settle_pending(c));
  // ---- who takes part: the caller's mask, or (rules) the run mask
  std::vector<unsigned char> run(rules ? B : 0);
  for (size_t e = 0; e < run.size(); ++e) run[e] = ((!active || active[e]) && status[e] == 0) ? 1 : 0;
  const unsigned char *on = rules ? run.data() : active;
  // ---- room
  const bool bw_dev = bw_out && !(mpf_bw > 0.f);  // Silverman's bandwidths are the device's to record
  DualEpisodeStage st(mb, T, B, P, first);
  TRY(st.room(mpf_steps));
  // the records [T][B]: states | actions | weights | bandwidths | (rules) costs, then (rules) the words [B] loss | status | n_run
  EpisodeRecords lay(T, B);
  const RecSection sec_s = lay.add((size_t)c->ds), sec_a = lay.add((size_t)c->da), sec_pw = lay.add(N, pw_out != nullptr), sec_bw = lay.add(1, bw_dev),
                   sec_c = lay.add(1, rules != nullptr);
  const size_t words = lay.words(rules != nullptr), n_rec = lay.total();
  TRY(b->rec.ensure(n_rec));
  if (record & DUST_HIST_THETA) TRY(svb_hist_room(b, b->hist_theta, T, N * D));
  if (record & DUST_HIST_FILTER) TRY(svb_hist_room(b, b->hist_x, T, x_row));
  // ---- staged once: states and mask; the filters' rows, seeds, plants
  TRY(b->in.stage(c, states, on));
  TRY(st.stage(c, states, actions_prev, mpf_steps, on, prior_seeds, plant_params));
  if (rules) TRY(h2d(c, b->rec + words, rules_words_in(loss, status, B).data(), 3 * B * sizeof(float)));
  if (first || n_periods > 1) serve_cancel_device(m->cfg.device);  // (as mpfb_enqueue, once for the call)
  // ---- the periods
  dust::MpfEnvIn *in_dev = st.in_dev();
  const unsigned char *mask = b->in.mask_dev(on);
  SvmpcDualSimPeriodArgs ka;  // (its first three members are the plain period's arguments)
  svb_args(b, n_steps, nullptr, nullptr, on, true, ka.k);
  dual_batch_prior(mb, nullptr, ka.pr);
  memset(&ka.ds, 0, sizeof ka.ds);
  if (rules) {
    rules_fill(ka.ds, rules, c->ds, nullptr, b->rec + words, B);
    ka.ds.run = const_cast<unsigned char *>(mask);
  }
  const size_t lds = svmpc_batch_lds_bytes(c->N, c->D, c->M);
  const size_t warm = rules_warm(rules);
  for (size_t t = 0; t < T; ++t) {
    const bool update = t > 0 || first;
    if (update) TRY(mpfb_update_launch(mb, c->stream, in_dev, mask, mpf_bw, mpf_steps));
    mb->n_calls++;
    ka.k.do_forward = t >= warm ? 1 : 0;
    ka.pr.seeds = st.seeds_dev(t);
    ka.dp.plant = st.plant_dev(plant_params);
    ka.dp.state = const_cast<float *>(b->in.states_dev());
    ka.dp.in = in_dev;
    ka.dp.states_out = sec_s.at(b->rec, t);
    ka.dp.actions_out = sec_a.at(b->rec, t);
    ka.dp.pw_out = t >= warm ? sec_pw.at(b->rec, t) : nullptr;
    ka.dp.bw = bw_dev && update ? mb->bw.get() : nullptr;
    ka.dp.bw_out = sec_bw.at(b->rec, t);
    ka.dp.t0_add = update ? mpf_steps : 0;
    ka.dp.condition = t + 1 < T ? 1 : 0;
    ka.ds.costs_out = b->rec + sec_c.off + t * B;
    Prof pr(c, DUST_K_SVMPC_BATCH);
    const hipError_t launched = by_model(c, [&](auto M) -> hipError_t {
      if constexpr (M() == DUST_MODEL_PENDULUM || M() == DUST_MODEL_PARTICLE) {
        if (record) {  // the recording instance: the same period, plus this period's rows of the history
          SvmpcDualSimHistPeriodArgs kh;
          kh.k = ka.k;
          kh.pr = ka.pr;
          kh.dp = ka.dp;
          kh.ds = ka.ds;
          kh.hs.theta = (record & DUST_HIST_THETA) ? b->hist_theta.rows.get() + t * B * N * D : nullptr;
          kh.hs.x = (record & DUST_HIST_FILTER) ? b->hist_x.rows.get() + t * B * x_row : nullptr;
          return launch_on(c->stream, false, &svmpc_dual_sim_hist_period_kernel<M()>, b->B, SVB_THREADS, lds, kh);
        }
        if (rules) return launch_on(c->stream, false, &svmpc_dual_sim_period_kernel<M()>, b->B, SVB_THREADS, lds, ka);
        SvmpcDualPeriodArgs kp;
        kp.k = ka.k;
        kp.pr = ka.pr;
        kp.dp = ka.dp;
        return launch_on(c->stream, false, &svmpc_dual_period_kernel<M()>, b->B, SVB_THREADS, lds, kp);
      } else return hipErrorInvalidValue;  // (refused above)
    });
    HIP_TRY(launched);
  }
  b->have_costs = true;
  b->acts_kept = false;
  if (forward) b->have_forward = true;
  // ---- the records, the words and the advanced rows come back once; the rows of inactive environments stay out of the caller's arrays
  std::vector<float> host(n_rec), seq(a_seq && rules ? B * D : 0);
  TRY(st.read_back(c, host, b->rec));
  if (a_seq && rules) HIP_TRY(hipMemcpyAsync(seq.data(), b->a_seq_out, B * D * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  else TRY(svb_outputs_copy(b, active, a_seq, nullptr));
  TRY(st.wait(c));
  // (rules) the periods every environment ran - none where it did not take part: nothing of it is written past row ran[e] - 1
  const std::vector<int> ran_v = rules ? rules_ran(host.data() + words, B, run.data()) : std::vector<int>();
  const int *ran = rules ? ran_v.data() : nullptr;
  records_scatter(states_out, host.data(), sec_s, on, ran);
  records_scatter(actions_out, host.data(), sec_a, on, ran);
  if (pw_out) records_scatter(pw_out, host.data(), sec_pw, on, ran, warm);
  if (bw_dev) records_scatter(bw_out, host.data(), sec_bw, on, ran);
  if (rules) {
    records_scatter(costs_out, host.data(), sec_c, on, ran);
    rules_words_out(host.data() + words, B, active, ran, loss, status, n_run);
    if (a_seq) env_rows_out(a_seq, seq.data(), B, D, active, ran, warm);
  }
  st.commit(mpf_bw, on, bw_out, ran);
  if (record & DUST_HIST_THETA) svb_hist_done(b, b->hist_theta, T, ran, on);
  if (record & DUST_HIST_FILTER) svb_hist_done(b, b->hist_x, T, ran, on);
  return DUST_OK;
}

extern "C" int dust_svmpc_dual_batch_episode(dust_svmpc_batch *b, dust_mpf_batch *mb, const float *states, const float *actions_prev, int n_periods,
                                             int n_steps, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds, const float *plant_params, int flags,
                                             const unsigned char *active, float *states_out, float *actions_out, float *pw_out, float *bw_out, float *a_seq) {
  return svb_dual_episode_call(b, mb, states, actions_prev, n_periods, n_steps, mpf_steps, mpf_bw, prior_seeds, plant_params, nullptr, flags, active,
                               states_out, actions_out, pw_out, bw_out, nullptr, nullptr, nullptr, nullptr, a_seq);
}

// ... under the reference's episode rules: warm-up with the filters updating, the cost, crash and goal
extern "C" int dust_svmpc_dual_batch_simulate(dust_svmpc_batch *b, dust_mpf_batch *mb, const float *states, const float *actions_prev, int n_periods,
                                              int n_steps, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds, const float *plant_params,
                                              const dust_episode_rules *rules, int flags, const unsigned char *active, float *states_out,
                                              float *actions_out, float *pw_out, float *bw_out, float *costs_out, float *loss, int *status, int *n_run,
                                              float *a_seq) {
  if (!rules) return fail(DUST_ERR_INVALID, "null rules");
  return svb_dual_episode_call(b, mb, states, actions_prev, n_periods, n_steps, mpf_steps, mpf_bw, prior_seeds, plant_params, rules, flags, active,
                               states_out, actions_out, pw_out, bw_out, costs_out, loss, status, n_run, a_seq);
}

// T control periods of the dual loop over the AMPPI batch for B environments in one call: T successive dust_amppi_dual_batch_tick calls
// with device-drawn noise and roll_steps >= 1, and between them the plant of dust_amppi_batch_episode, stepped on the device.  Staged
// once as in dust_svmpc_dual_batch_episode (states and mask through the controller batch's pinned slot; MpfEnvIn rows, seeds [T][B] and
// plant rows through the filter batch's); then, on the controller batch's stream and in launch order, period t is: Silverman's rule and
// the filters' update (when the period has an action), reading the MpfEnvIn rows in device memory; in the single and sigma modes the
// staging launch of the tick's parameter rows under the key row prior_seeds + t B; ONE launch of the period kernel (amppi_episode.hpp:
// amppi_prior_period_kernel in the "extended" mode, amppi_period_kernel on b->params otherwise), whose reducer also conditions the
// environment's MpfEnvIn row for period t + 1.  No host wait, event or copy lies between two periods; the call waits once, reads the
// rows back and commits them as the SVMPC episode does (dual_episode_commit): the pair (a_{T-1}, x_T) is NOT folded in.
//
// rules (dust_amppi_dual_batch_simulate; NULL: dust_amppi_dual_batch_episode): the loop under the reference's rules, as
// svb_dual_episode_call runs the SVMPC pair under them - the run mask active[b] && status[b] == 0 is what every launch of the call takes
// (Silverman's rule, the filters' update, the parameter staging of the single / sigma modes, the period kernel), the reducer of
// amppi_sim_period_kernel / amppi_prior_sim_period_kernel clears an environment's byte in the period that stops it and leaves its pair
// pending, and the filters' host rows are committed from n_run[b].  This branch of the reference has no warm-up.
static int amppi_dual_episode_call(dust_amppi_batch *b, dust_mpf_batch *mb, const float *states, const float *actions_prev, int n_periods, int flags,
                                   int mpf_steps, float mpf_bw, const uint64_t *prior_seeds, int roll_steps, const float *plant_params,
                                   const dust_episode_rules *rules, const unsigned char *active, float *states_out, float *actions_out,
                                   float *costs_out, float *omega_out, float *bw_out, float *inst_costs_out, float *loss, int *status, int *n_run,
                                   float *a_seq) {
  if (!b || !mb || !states || !states_out || !actions_out) return fail(DUST_ERR_INVALID, "null argument");
  if (rules && (!loss || !status || !n_run || !inst_costs_out))
    return fail(DUST_ERR_INVALID, "null argument: loss, status, n_run and inst_costs_out are required");
  if (!prior_seeds) return fail(DUST_ERR_INVALID, "null argument: the draws from the filters' priors need prior_seeds [T][B]");
  TRY(episode_periods_check(n_periods, "the queue of one call stays short on a shared device: chain a longer episode"));
  if (mpf_steps < 0) return fail(DUST_ERR_INVALID, "bad step counts");
  if (roll_steps < 1) return fail(DUST_ERR_INVALID, "roll(steps = %d): steps >= 1", roll_steps);
  if (flags & ~DUST_AMPPI_PARAMS_SHARED)
    return fail(DUST_ERR_UNSUPPORTED, "an AMPPI dual episode draws its noise on the device and stores neither trajectories nor binary16: flags may hold "
                "DUST_AMPPI_PARAMS_SHARED alone (got %d)", flags);
  dust_ctx *c = b->c;
  dust_mpf *m = mb->m;
  TRY(amppi_check(c));
  TRY(episode_plant_check(c, plant_params));
  if (rules) TRY(rules_check(c, rules, (size_t)b->B, active, status, true, true));
  TRY(dual_batch_pair_check(c, "AMPPI", b->B, mb));
  bool sigma, shared;
  TRY(amppi_dual_check(c, m, flags, &sigma, &shared));
  auto host_lik = [](int model) { return model == DUST_MODEL_SKID_STEER || model == DUST_MODEL_CARTPOLE; };
  if (host_lik(c->cfg.model) || host_lik(m->cfg.model_cfg.model))
    return fail(DUST_ERR_UNSUPPORTED,
                "a dual episode conditions the filters on the device: Pendulum and Particle pairs (a skid-steer or cart-pole filter's likelihood rows "
                "carry the host's sin / cos of the past heading: dust_amppi_dual_batch_tick per period)");
  const bool staged = sigma || shared;
  int mode = AMPPI_PARAMS_NONE, pts = 1;
  size_t prows = 0;
  dust::AmppiPrior one;  // (amppi_params_mode reads the prior's P alone)
  memset(&one, 0, sizeof one);
  one.P = m->P;
  TRY(amppi_params_mode(c, staged, flags, staged ? nullptr : &one, &mode, &pts, &prows));
  TRY(mpfb_limits(m, mb->B));
  TRY(mpfb_bw_check(mb, mpf_bw));
  const bool first = actions_prev != nullptr;  // period 0 has an update
  const size_t T = (size_t)n_periods, B = (size_t)b->B, S = (size_t)c->S, P = (size_t)m->P;
  // who takes part: the caller's mask, or (rules) the run mask - an environment that enters stopped does nothing, and is not checked
  std::vector<unsigned char> run(rules ? B : 0);
  for (size_t e = 0; e < run.size(); ++e) run[e] = ((!active || active[e]) && status[e] == 0) ? 1 : 0;
  const unsigned char *on = rules ? run.data() : active;
  if (first || n_periods > 1) TRY(mpfb_update_check(mb, first ? actions_prev : states, states, mpf_steps, on));
  const bool bw_dev = bw_out && !(mpf_bw > 0.f);  // Silverman's bandwidths are the device's to record
  const AmppiRecords lay(c, T, B, costs_out != nullptr, omega_out != nullptr, bw_dev, a_seq != nullptr, rules != nullptr);
  const size_t n_rec = lay.n_rec;
  if (n_rec > DUST_AMPPI_EPISODE_MAX_FLOATS)
    return fail(DUST_ERR_UNSUPPORTED, "%zu record values for %d periods exceed %zu: split the episode into shorter calls (or leave costs / omega out)", n_rec,
                n_periods, DUST_AMPPI_EPISODE_MAX_FLOATS);
  HIP_TRY(hipSetDevice(c->cfg.device));
  TRY(settle_pending(c));
  // ---- room
  DualEpisodeStage st(mb, T, B, P, first);
  TRY(st.room(mpf_steps));
  if (staged) TRY(b->params.ensure(B * prows * P));
  TRY(b->rec.ensure(n_rec));
  // ---- staged once
  TRY(b->in.stage(c, states, on));
  TRY(st.stage(c, states, actions_prev, mpf_steps, on, prior_seeds, plant_params));
  if (rules) TRY(h2d(c, b->rec + lay.words, rules_words_in(loss, status, B).data(), 3 * B * sizeof(float)));
  HIP_TRY(hipMemsetAsync(b->ticket, 0, B * sizeof(unsigned int), c->stream));
  if (first || n_periods > 1) serve_cancel_device(m->cfg.device);  // (as mpfb_enqueue, once for the call)
  // ---- the periods
  dust::MpfEnvIn *in_dev = st.in_dev();
  const unsigned char *mask = b->in.mask_dev(on);
  AmppiPriorSimPeriodArgs ka;  // (its first three members are the plain period's arguments)
  batch_tick_args(b, mode, pts, prows, true, on, ka.k);
  dual_batch_prior(mb, nullptr, ka.pr);
  memset(&ka.ep, 0, sizeof ka.ep);
  memset(&ka.ru, 0, sizeof ka.ru);
  if (rules) {
    rules_fill(ka.ru, rules, c->ds, nullptr, b->rec + lay.words, B);
    ka.ru.run = const_cast<unsigned char *>(mask);
  }
  const long shift = (long)roll_steps * c->da;
  ka.ep.plant = st.plant_dev(plant_params);
  ka.ep.state = const_cast<float *>(b->in.states_dev());
  ka.ep.shift = shift > c->D ? c->D : (int)shift;
  ka.ep.in = in_dev;
  const dim3 grid((unsigned)((S + AMPPI_THREADS - 1) / AMPPI_THREADS), (unsigned)B);
  b->acts_valid = true;  // (ahead of the chain, as in dust_amppi_batch_episode)
  if (on) b->last_active.assign(on, on + B);
  else b->last_active.clear();
  for (size_t t = 0; t < T; ++t) {
    const bool update = t > 0 || first;
    if (update) TRY(mpfb_update_launch(mb, c->stream, in_dev, mask, mpf_bw, mpf_steps));
    mb->n_calls++;
    if (staged) {
      if (sigma) dust::mpf_sigma_points_batch_kernel<<<b->B, 256, 0, c->stream>>>(mb->x, m->Mp, m->P, mb->prior_bwv, c->sigma_scale, b->params, mask);
      else dust::mpf_sample_batch_kernel<<<(b->B + 255) / 256, 256, 0, c->stream>>>(mb->x, m->Mp, m->P, mb->prior_bwv, st.seeds_dev(t), b->B, b->params, mask);
      HIP_TRY(hipGetLastError());
      mb->n_launch++;
    }
    ka.pr.seeds = st.seeds_dev(t);
    lay.period(ka.ep, b->rec, t, rules != nullptr);
    ka.ru.costs_out = lay.ic.at(b->rec, t);
    ka.ep.bw = bw_dev && update ? mb->bw.get() : nullptr;
    ka.ep.bw_out = lay.bw.at(b->rec, t);
    ka.ep.t0_add = update ? mpf_steps : 0;
    ka.ep.condition = t + 1 < T ? 1 : 0;
    Prof pr(c, DUST_K_AMPPI);
    const hipError_t launched = by_model(c, [&](auto M) -> hipError_t {
      if constexpr (M() == DUST_MODEL_PENDULUM || M() == DUST_MODEL_PARTICLE) {
        if (rules) {
          if (staged) return launch_on(c->stream, false, &amppi_sim_period_kernel<M()>, grid, AMPPI_THREADS, 0, AmppiSimPeriodArgs{ka.k, ka.ep, ka.ru});
          return launch_on(c->stream, false, &amppi_prior_sim_period_kernel<M()>, grid, AMPPI_THREADS, 0, ka);
        }
        if (staged) return launch_on(c->stream, false, &amppi_period_kernel<M()>, grid, AMPPI_THREADS, 0, AmppiPeriodArgs{ka.k, ka.ep});
        return launch_on(c->stream, false, &amppi_prior_period_kernel<M()>, grid, AMPPI_THREADS, 0, AmppiPriorPeriodArgs{ka.k, ka.pr, ka.ep});
      } else return hipErrorInvalidValue;  // (refused above)
    });
    HIP_TRY(launched);
  }
  // ---- the records and the advanced rows come back once; the rows of inactive environments stay out of the caller's arrays
  std::vector<float> host(n_rec);
  TRY(st.read_back(c, host, b->rec));
  TRY(st.wait(c));
  // (rules) the periods every environment ran - none where it did not take part: nothing of it is written past row ran[e] - 1
  const std::vector<int> ran_v = rules ? rules_ran(host.data() + lay.words, B, run.data()) : std::vector<int>();
  const int *ran = rules ? ran_v.data() : nullptr;
  lay.out(host.data(), on, ran, states_out, actions_out, costs_out, omega_out, bw_out, inst_costs_out, a_seq);
  if (rules) rules_words_out(host.data() + lay.words, B, active, ran, loss, status, n_run);
  st.commit(mpf_bw, on, bw_out, ran);
  return DUST_OK;
}

extern "C" int dust_amppi_dual_batch_episode(dust_amppi_batch *b, dust_mpf_batch *mb, const float *states, const float *actions_prev, int n_periods,
                                             int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds, int roll_steps, const float *plant_params,
                                             const unsigned char *active, float *states_out, float *actions_out, float *costs_out, float *omega_out,
                                             float *bw_out, float *a_seq) {
  return amppi_dual_episode_call(b, mb, states, actions_prev, n_periods, flags, mpf_steps, mpf_bw, prior_seeds, roll_steps, plant_params, nullptr, active,
                                 states_out, actions_out, costs_out, omega_out, bw_out, nullptr, nullptr, nullptr, nullptr, a_seq);
}

// ... under the reference's episode rules: the cost, crash and goal
extern "C" int dust_amppi_dual_batch_simulate(dust_amppi_batch *b, dust_mpf_batch *mb, const float *states, const float *actions_prev, int n_periods,
                                              int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds, int roll_steps,
                                              const float *plant_params, const dust_episode_rules *rules, const unsigned char *active, float *states_out,
                                              float *actions_out, float *costs_out, float *omega_out, float *bw_out, float *inst_costs_out, float *loss,
                                              int *status, int *n_run, float *a_seq) {
  if (!rules) return fail(DUST_ERR_INVALID, "null rules");
  return amppi_dual_episode_call(b, mb, states, actions_prev, n_periods, flags, mpf_steps, mpf_bw, prior_seeds, roll_steps, plant_params, rules, active,
                                 states_out, actions_out, costs_out, omega_out, bw_out, inst_costs_out, loss, status, n_run, a_seq);
}
