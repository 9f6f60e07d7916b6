/*
 * dust_amd.h - C ABI of libdust_amd.so: the MI355X-native (HIP, gfx950) SVGD-MPC inner loop.
 *
 * Drop-in boundary for the one hot path of lubaroli/dust.  The reference is pure Python and
 * has no FFI of its own; each entry point below replaces one reference METHOD (cited file:line into lubaroli/dust) and
 * is what a ctypes binding on the reference side would call (INTEGRATION.md shows that binding).
 *
 * Conventions
 *  - plain C, opaque handles, `int` status (0 = DUST_OK), no exceptions, no callbacks; dust_last_error() gives text;
 *  - all arrays are fp32, C-contiguous, in the reference's own layouts (e.g. actions [S][N][H][da]);
 *  - pointers are HOST pointers unless the call has a `flags` argument carrying DUST_PTR_DEVICE, in which case the
 *    bulk noise/action arrays are device pointers already resident in HBM (benchmarks, fused pipelines);
 *  - one HIP stream per context; a context is not thread-safe; every call returns after its results are on the host
 *    (calls with no host outputs are asynchronous on the context's stream; dust_sync() waits);
 *  - there is NO CPU fallback: without a usable HIP device dust_create fails with DUST_ERR_NO_DEVICE.
 *
 * Symbols: N = n_policies (Stein particles), S = n_samples (action samples per policy), M = n_params (dynamics
 * samples), H = horizon, da/ds = action/state dims, D = H*da, P = number of uncertain model parameters.
 */
#ifndef DUST_AMD_H
#define DUST_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DUST_ABI_VERSION 3

enum dust_status {
  DUST_OK = 0,
  DUST_ERR_INVALID = 1,     /* bad argument / shape (the reference raises ValueError / AssertionError) */
  DUST_ERR_UNSUPPORTED = 2, /* a configuration outside the HIP kernels' families (the reference would run Python) */
  DUST_ERR_NO_DEVICE = 3,
  DUST_ERR_HIP = 4,
  DUST_ERR_STATE = 5 /* call order (e.g. phi before any likelihood sample) */
};

enum dust_model { DUST_MODEL_PENDULUM = 0, DUST_MODEL_PARTICLE = 1, DUST_MODEL_SKID_STEER = 2, DUST_MODEL_CARTPOLE = 3 };
/* cost families: pendulum demo cost (demo/pendulum_example.py:21-28), Particle.default_*_cost (particle.py:170-225) */
enum dust_cost { DUST_COST_PENDULUM_QUADCOS = 0, DUST_COST_PARTICLE_DEFAULT = 1, DUST_COST_QUADRATIC = 2 };
/* K1: gpytorch RBFKernel semantics, lengthscale ln 2 (svmpc.py:76-83); K2: iid_mp(RBF) per-dimension median bandwidth
 * (svmpc.py:64-74, composite_kernels.py:33-64); K2_SHARED: indep_controls=False; IMQ: new, no reference. */
enum dust_kernel { DUST_KERNEL_K1_RBF = 0, DUST_KERNEL_K2_IIDMP = 1, DUST_KERNEL_K2_SHARED = 2, DUST_KERNEL_IMQ = 3 };
enum dust_likelihood { DUST_LIK_EXP_UTILITY = 0, DUST_LIK_EXPECTED_COST = 1 }; /* likelihoods.py:122-135 / 106-119 */
/* svgd.py:115, demos use SGD.  dust_config.optimizer takes SGD / Adam only; RMSprop / Adagrad (and AdamW: Adam with
 * DUST_OPTF_DECOUPLED_WD) are chosen through dust_set_optimizer / dust_mpf_set_optimizer_ex. */
enum dust_optimizer { DUST_OPT_SGD = 0, DUST_OPT_ADAM = 1, DUST_OPT_RMSPROP = 2, DUST_OPT_ADAGRAD = 3 };
enum dust_optim_flags {
  DUST_OPTF_MAXIMIZE = 1,        /* maximize=True (every class) */
  DUST_OPTF_NESTEROV = 2,        /* SGD(nesterov=True) */
  DUST_OPTF_AMSGRAD = 4,         /* Adam / AdamW(amsgrad=True) */
  DUST_OPTF_DECOUPLED_WD = 8,    /* Adam(decoupled_weight_decay=True), i.e. AdamW: param *= 1 - lr * weight_decay */
  DUST_OPTF_CENTERED = 16        /* RMSprop(centered=True) */
};
enum dust_roll { DUST_ROLL_REPEAT = 0, DUST_ROLL_MEAN = 1, DUST_ROLL_RESAMPLE = 2 }; /* svmpc.py:142-158 */
enum dust_step_strategy { DUST_STEP_ARGMAX = 0, DUST_STEP_AVERAGE = 1, DUST_STEP_EXTERNAL = 2 }; /* disco.py:396-417 */
/* how a model parameter enters the arithmetic: a Python float (double), a 0-dim fp32 tensor, or a sampled column */
enum dust_param_kind { DUST_PARAM_PYFLOAT = 0, DUST_PARAM_SAMPLED = 1, DUST_PARAM_TENSOR0D = 2 };
/* Particle(control_type=) particle.py:41-60, 149-153.  Velocity control is a TWO-state model (x, y; dim_s = 2): the action is clamped to
 * +-max_speed and integrated directly, and the closing clamp of the step (particle.py:165) lands on the positions. */
enum dust_control_type { DUST_CONTROL_ACCELERATION = 0, DUST_CONTROL_VELOCITY = 1 };
/* DUST_EPS_AROUND_A_MAT: the external actions were drawn around a_mat (MultiDISCO's own sampling, disco.py:155-160) */
enum dust_flags {
  DUST_PTR_DEVICE = 1,
  DUST_STORE_STATES = 2,
  DUST_EPS_AROUND_A_MAT = 4,
  /* fp16 STORAGE of the rollout's bulk data, fp32 arithmetic (BASELINE.json config 5 "fp16 rollout / fp32 SVGD"; the reference
   * itself is fp32 only).  DUST_EPS_F16: the `eps` / `actions` argument points to IEEE binary16 values (same layout, host or
   * device) - the rollout kernel's HBM read traffic halves.  DUST_STORE_F16: the stored `states` / `actions_out` are binary16
   * (the caller's output buffers receive binary16 values, half the bytes; 5.5 GB instead of 11 GB of states at config 3). */
  DUST_EPS_F16 = 8,
  DUST_STORE_F16 = 16,
  /* ABI 3, dust_amppi_update: `params` is ONE row that every trajectory uses (AMPPI(params_sampling="single"), amppi.py:91-93) */
  DUST_AMPPI_PARAMS_SHARED = 32,
  /* ABI 3, dust_svmpc_batch_optimize / _tick: keep the last iteration's actions for dust_svmpc_batch_get(DUST_SVB_ACTIONS) */
  DUST_SVMPC_BATCH_KEEP_ACTIONS = 64
};

typedef struct dust_param {
  int32_t kind;   /* dust_param_kind */
  int32_t column; /* column of `params` when kind == DUST_PARAM_SAMPLED */
  double value;   /* default value otherwise */
} dust_param;

typedef struct dust_config {
  int32_t abi_version; /* DUST_ABI_VERSION */
  int32_t device;      /* HIP device ordinal */
  /* sizes: MultiDISCO(n_policies, action_samples, params_samples, hz_len) disco.py:16-137 */
  int32_t n_policies;       /* N, total over all shards */
  int32_t n_samples;        /* S */
  int32_t n_params;         /* M (1 when params_sampling is off) */
  int32_t horizon;          /* H */
  int32_t dim_a, dim_s, dim_p;
  /* data-parallel shard of the policy index owned by this context: [shard_offset, shard_offset + shard_size) */
  int32_t shard_offset, shard_size; /* shard_size 0 = all */
  int32_t model, cost, kernel, likelihood, optimizer, roll_strategy;
  int32_t weighted_prior;    /* SVMPC(weighted_prior=) svmpc.py:21 */
  int32_t params_log_space;  /* MultiDISCO(params_log_space=) disco.py:173 */
  int32_t params_interleave; /* scalar-event params_dist quirk, disco.py:177-179: rollout r uses params[r % M] */
  float alpha;               /* likelihood alpha */
  float temperature;         /* MultiDISCO temperature */
  float a_reg;               /* temperature * (1 - ctrl_penalty) disco.py:90 */
  float lr, adam_beta1, adam_beta2, adam_eps;
  float chol_a[4];  /* diagonal of cholesky(a_cov): policy-noise scale (likelihoods.py:85-90) */
  float sigma_a[4]; /* sqrt(diag(a_dist.covariance_matrix)) as svmpc.py:107-111 computes it */
  float a_pre[4];   /* diagonal of inverse(a_cov) disco.py:98 */
  float sigma_p[4]; /* sqrt of the prior component covariance diagonal (svgd.py:84-89) */
  float bw_scale;   /* RBF(bw_scale=) base_kernels.py:44 */
  float imq_ell;
  float min_a[4], max_a[4]; /* action_space bounds, disco.py:408-410 */
  uint64_t seed;            /* device Philox stream for internally drawn noise */
  /* model: dust/models/pendulum.py, dust/models/particle.py */
  double dt;
  dust_param g, mass, length; /* pendulum; `mass` is also the particle mass */
  double max_torque, max_speed_pend;
  double w_cos, w_vel;        /* pendulum cost weights */
  float max_speed, max_accel; /* particle */
  int32_t can_crash, with_obstacle;
  double cell_size;
  float target[4], w_state[4], w_term[4], w_ctrl[2], w_obs;
  /* ABI 2: Particle(control_type=, deterministic=, noise_std=) particle.py:13-31.  ctrl_noise = `not deterministic` (the reference's
   * constructor default is deterministic=False with noise_std = zeros(2)): every model step adds dyn_std * N(0, I) to the actions that
   * drive the dynamics (particle.py:145-148; the costs see the raw actions).  Draws: a device Philox stream, or the recorded tensors
   * handed to dust_set_ctrl_noise / dust_mpf_set_ctrl_noise (parity runs). */
  int32_t control_type; /* dust_control_type */
  int32_t ctrl_noise;
  float dyn_std[2];
  /* ABI 2: FULL 2 x 2 covariances (dim_a = 2).  MultiDISCO(a_cov=<any SPD matrix>) disco.py:91-98: policy noise actions = theta + L_a eps
   * with L_a = cholesky(a_cov) (likelihoods.py:85-90) - chol_a[0..1] stay its diagonal, chol_a_off = L_a[1][0]; a_pre = inverse(a_cov)
   * in the control cost (disco.py:338-346) - a_pre[0..1] stay its diagonal, a_pre_off = a_pre[0][1]; sigma_a stays sqrt(diag a_cov)
   * (svmpc.py:107-111).  Prior components with a full covariance Sigma_p = L_p L_p^T (get_gmm svgd.py:84-89): chol_p = {L_p[0][0],
   * L_p[1][0], L_p[1][1]}, sigma_p[0..1] stay sqrt(diag Sigma_p).  full_cov != 0 switches these on (all zero: the diagonal forms). */
  int32_t full_cov;
  float chol_a_off, a_pre_off;
  float chol_p[3];
} dust_config;

/* SkidSteerRobot (dust/models/skid_steer_robot.py:19-52, step :73-122; model = DUST_MODEL_SKID_STEER, dim_s = 5: x, y, theta, v,
 * omega; dim_a = 2: right / left wheel speed) with the quadratic cost family DUST_COST_QUADRATIC - the reference ships no cost for
 * this model, its MultiDISCO takes any callable (disco.py:294-346); the family is what dust_amd.costs.QuadraticCost evaluates:
 *   inst(x, a) = sum_k w_state[k] (x_k - goal_k)^2 + sum_d w_ctrl[d] a_d^2 ,   term(x) = sum_k w_term[k] (x_k - goal_k)^2 .
 * dust_create gives the reference's constructor defaults; dust_set_skid_steer replaces them.  Sampled parameters
 * (kind DUST_PARAM_SAMPLED) name columns of the `params` rows in the order of `uncertain_params`.
 * The dynamics filter takes the same struct (dust_mpf_set_skid_steer: parameters and bounds; the cost fields are ignored there). */
typedef struct dust_skid_config {
  dust_param x_icr, wheel_radius, axial_distance;
  float min_wheel_speed[2], max_wheel_speed[2]; /* action_space bounds: the step clamps the wheel speeds to them */
  float goal[5], w_state[5], w_term[5], w_ctrl[2];
} dust_skid_config;

/* CartPoleModel (dust/models/cartpole.py:42-106, step :126-172; model = DUST_MODEL_CARTPOLE, dim_s = 4: x, x_d, theta, theta_d; dim_a = 1:
 * the push, clamped to +-1 INSIDE the step, cartpole.py:159) with the quadratic cost family DUST_COST_QUADRATIC of dust_skid_config
 * (4 state entries, 1 control weight).  The reference's step reads a name-mangled attribute the base class never set
 * (cartpole.py:151/156); with that attribute supplied on the instance it runs, and the kernels follow it operation by operation -
 * `mass = m_c + m_c` (cartpole.py:161) included.  dust_create gives the constructor's defaults (g 9.8, f_mag 10, mass_cart 1,
 * mass_pole 0.1, length 1, mu_c 5e-4, mu_p 2e-6), unit state weights and no goal; dust_set_cartpole replaces them.  Any of the seven
 * parameters may be sampled (kind DUST_PARAM_SAMPLED): it names a column of the `params` rows, in the order of `uncertain_params`
 * (base.py params_to_dict), dim_p <= 4 of them at once.  The dynamics filter takes the same struct (dust_mpf_set_cartpole: the cost
 * fields are ignored there). */
typedef struct dust_cartpole_config {
  dust_param g, f_mag, mass_cart, mass_pole, length, mu_c, mu_p; /* CartPoleModel.__init__ order, cartpole.py:42-51 */
  float goal[4], w_state[4], w_term[4], w_ctrl[1];
} dust_cartpole_config;

/* A torch.optim optimiser with its options (dust_set_optimizer, dust_mpf_set_optimizer_ex).  Each step follows the installed torch's
 * single-tensor CPU function operation by operation - torch/optim/sgd.py _single_tensor_sgd, adam.py _single_tensor_adam (AdamW
 * included), rmsprop.py _single_tensor_rmsprop, adagrad.py _single_tensor_adagrad - on grad = -phi: Python-float scalars are formed
 * in double from these fields, as Python forms them, then rounded to fp32 where the tensor op takes them.  Fields a class does not
 * have are ignored.  The step count (Adam's bias corrections, Adagrad's lr_decay, SGD's first momentum step) is the device's own
 * step counter, which restarts with the state. */
typedef struct dust_optim_config {
  int32_t kind;  /* dust_optimizer */
  int32_t flags; /* dust_optim_flags */
  double lr;
  double beta1, beta2;  /* Adam betas */
  double eps;           /* Adam / RMSprop / Adagrad */
  double weight_decay;  /* every class */
  double momentum;      /* SGD / RMSprop */
  double dampening;     /* SGD */
  double alpha;         /* RMSprop smoothing constant */
  double lr_decay;      /* Adagrad */
  double initial_accumulator_value; /* Adagrad: the value its sum starts (and restarts) at */
} dust_optim_config;

typedef struct dust_ctx dust_ctx;
typedef struct dust_mpf dust_mpf;

const char *dust_last_error(void);
int dust_abi_version(void);
int dust_device_count(int *count);

/* lifecycle.  dust_clone is what copy.deepcopy(controller/svmpc) maps to (simulations.py:62, particle_example.py:166-175) */
int dust_create(const dust_config *cfg, dust_ctx **out);
int dust_clone(const dust_ctx *src, dust_ctx **out);
void dust_destroy(dust_ctx *ctx);
int dust_sync(dust_ctx *ctx);
/* Which device path served the SVMPC.optimize / forward calls so far (svmpc.py:97-200; sticky counts since creation):
 * out[0] one-launch ticks, owner-computes form (tick2.hpp) - launched-ahead ticks of closed-loop serving included, also cancelled ones;
 * out[1] always 0 (the tiled one-launch tick of rounds 2-5 is retired); out[2] ticks answered through the pinned done word of closed-loop serving;
 * out[3] ticks whose one-launch kernel found the device shared with other work (its workgroups were not all resident) and that
 * were therefore run on the launch-per-iteration path instead - late, on unchanged state, never lost. */
int dust_tick_stats(dust_ctx *ctx, long long out[4]);
int dust_get_config(const dust_ctx *ctx, dust_config *out);
/* model.params_dict[...] = v after construction (particle_example.py:178-179) */
int dust_set_model_param(dust_ctx *ctx, const char *name, double value, int kind);
/* Unscented-transform rollouts (MultiDISCO(params_sampling=MerweScaledUTF), disco.py:211-292, 312-323): the n_params
 * dynamics samples passed to forward / optimize are the 2 n + 1 sigma points and the cost of a rollout is their weighted
 * combination with `w[n_params]` (utf.py loc_weights; the reference's (sigma, step) weight pattern is reproduced) instead
 * of the mean.  NULL switches back to the mean over sampled parameters. */
int dust_set_param_weights(dust_ctx *ctx, const float *w);
/* lambda + n of the transform whose weights dust_set_param_weights set (utf.py:93-123: the sigma points are the mean +- the columns of
 * sqrt((lambda + n) K)).  dust_dual_tick needs it to compute the sigma points of the filter's prior on the device (disco.py:240-251);
 * rollouts with host-computed sigma points do not.  0 clears it; so does dust_set_param_weights(NULL).  dust_clone carries it.
 * DUST_ERR_INVALID for a negative or non-finite scale, DUST_ERR_STATE without weights. */
int dust_set_sigma_scale(dust_ctx *ctx, float scale);
int dust_set_skid_steer(dust_ctx *ctx, const dust_skid_config *cfg);
/* CartPoleModel(g, f_mag, ...) cartpole.py:42-88 and its quadratic cost.  A sampled column outside dim_p, or named by two parameters:
 * DUST_ERR_INVALID.  The family runs the launch-per-iteration path (pass 1: cartpole.hpp, pass 2: the regular kernel on injected
 * costs); binary16 storage returns DUST_ERR_UNSUPPORTED, and so do sigma-point weights together with a non-zero control weight or
 * a_reg != 0 (disco.py:306-309, 338-340: the reference cannot compute either).  dust_clone copies the model. */
int dust_set_cartpole(dust_ctx *ctx, const dust_cartpole_config *cfg);
/* Recorded control-channel noise for the NEXT rollouts of a Particle(deterministic=False) context (particle.py:145-148): z holds n_sets
 * tensors [H][M*S*N][da] of standard-normal draws in the reference's own order - one `torch.randn_like(acts)` per model.step call of
 * MultiDISCO._rollout (disco.py:193-200), rollout r = (m*S + s)*N + n, N = n_policies (all shards).  Every rollout launch that follows
 * (one per likelihood sample, i.e. per SVGD iteration) consumes one set; when they are used up - or after z = NULL - the draws come
 * from the context's Philox stream again.  Host pointer; copied before the call returns. */
int dust_set_ctrl_noise(dust_ctx *ctx, const float *z, int n_sets);
/* ObstacleMap occupancy grid [nx][ny] (obstacle_map.py:13-43); offsets are the map centre in cells */
int dust_set_grid(dust_ctx *ctx, const float *grid, int nx, int ny, float off_x, float off_y);
/* The obstacle term of a skid-steer context's cost (the navigation family, dust_amd.costs.NavigationCost): w_obs occ(x, y) joins the
 * instantaneous and the terminal cost as in Particle.default_inst_cost / default_term_cost (particle.py:170-225), occ =
 * ObstacleMap.get_collisions (obstacle_map.py:64-93) on the map of dust_set_grid with dust_config.cell_size.  w_obs = 0 (the default)
 * returns the context to the kernels without the term.  Skid-steer contexts only: DUST_ERR_UNSUPPORTED for every other model (Particle
 * carries w_obs in dust_config; the Pendulum and the cart-pole have no position plane).  DUST_ERR_INVALID for a negative or non-finite
 * weight, and for a weight != 0 on a context whose dust_config.cell_size is not a finite size > 0.  With w_obs != 0 and no map the first rollout returns DUST_ERR_STATE.  Pending launches are settled and captured graphs
 * dropped, as by dust_set_grid; dust_clone copies the weight with the map. */
int dust_set_obstacle_cost(dust_ctx *ctx, float w_obs);

/* particle / prior / controller state (all [N][H][da] or [N]) */
int dust_set_theta(dust_ctx *ctx, const float *theta);                                /* SVMPC.theta svmpc.py:25 */
/* SVMPC(optimizer_class=, **opt_args) svgd.py:109-125, svmpc.py:87-95: replaces the context's optimiser (dust_config.optimizer / lr /
 * adam_* give plain SGD or Adam until then) and restarts its state.  The state - up to three [N][D] slots: SGD's momentum buffer;
 * Adam's exp_avg, exp_avg_sq and AMSGrad max; RMSprop's square_avg, momentum buffer and grad_avg; Adagrad's sum - restarts at every
 * roll (SVMPC.roll builds a new parameter tensor), at dust_set_theta and here; dust_clone copies it.  Every device path that takes
 * an SVGD step applies it.  Adagrad differs from the reference here: torch's Adagrad creates its `sum` in __init__ only, so the
 * reference's SVMPC raises KeyError('sum') at the first step after a roll; the device restarts `sum` at initial_accumulator_value as a
 * fresh Adagrad on the rolled tensor would.  DUST_ERR_UNSUPPORTED names an option outside the table (e.g. SGD(nesterov=True) with dampening != 0). */
int dust_set_optimizer(dust_ctx *ctx, const dust_optim_config *opt);
int dust_get_optimizer(const dust_ctx *ctx, dust_optim_config *out);
/* RBF(bandwidth=, minimum_bw=) of the K2 kernels (base_kernels.py:44-92): bandwidth < 0 = median trick (default), every
 * per-dimension h = max(bw_scale * median / log(N + 1), minimum_bw); otherwise the fixed h = clip(bw_scale * bandwidth^2 / log(N + 1),
 * minimum_bw) replaces the medians.  minimum_bw > 0 (the reference's default is 1e-5). */
int dust_set_k2_bandwidth(dust_ctx *ctx, float bandwidth, float minimum_bw);
int dust_get_theta(dust_ctx *ctx, float *theta);
int dust_set_prior(dust_ctx *ctx, const float *means, const float *mix_weights);      /* get_gmm svgd.py:84-89 */
int dust_get_prior(dust_ctx *ctx, float *means, float *mix_probs);
int dust_set_a_mat(dust_ctx *ctx, const float *a_mat);                                /* MultiDISCO.a_mat disco.py:101-109 */
int dust_get_a_mat(dust_ctx *ctx, float *a_mat);
int dust_get_a_mix(dust_ctx *ctx, float *a_mix);                                      /* disco.py:393 */
int dust_set_a_seq(dust_ctx *ctx, const float *a_seq);                                /* BaseController.a_seq base.py:34-37 */
int dust_get_a_seq(dust_ctx *ctx, float *a_seq);

/* MultiDISCO.forward(state, model, params_dist, ext_actions) disco.py:348-394.
 * actions [S][N][H][da] (NULL: drawn on device as a_mat + L z, disco.py:155-160); params [M][P] raw samples or NULL.
 * outputs may be NULL: costs [S][N], states [M][S][N][H+1][ds], actions_out [S][N][H][da], omega [S][N].
 * Side effects as in the reference: a_mat += sum_s omega eps, a_mix refreshed. */
int dust_disco_forward(dust_ctx *ctx, const float *state, const float *actions, const float *params, int flags,
                       float *costs, float *states, float *actions_out, float *omega);
/* MultiDISCO.step(strategy, steps, ext_actions) disco.py:396-417 -> next_actions [steps][da] */
int dust_disco_step(dust_ctx *ctx, int strategy, int steps, const float *ext_actions, float *next_actions);

/* CostLikelihood.sample(theta, state, params_dist) likelihoods.py:81-101: actions = theta + L eps, then forward.
 * eps [S][N][H][da] standard-normal draws (NULL: device Philox).  costs [S][N], actions_out optional. */
int dust_likelihood_sample(dust_ctx *ctx, const float *state, const float *eps, const float *params, int flags,
                           float *costs, float *actions_out);
/* likelihood.log_prob(costs) likelihoods.py:113-135 on the last sampled costs -> [N] */
int dust_likelihood_log_prob(dust_ctx *ctx, float *log_l);

/* SVMPC.phi(log_p, bw, sigma) svmpc.py:32-85 with the costs/actions a user-supplied log_p returned
 * (costs [S][N], actions [S][N][H][da]); NULL/NULL = use the last likelihood sample held on the device.
 * outputs optional: phi, grad_lik, grad_pri each [N][H][da]. */
int dust_svmpc_phi(dust_ctx *ctx, const float *costs, const float *actions, float *phi, float *grad_lik, float *grad_pri);
/* SVMPC.step(state, params_dist, bw, sigma) svmpc.py:87-95: sample, phi, optimiser step on theta */
int dust_svmpc_step(dust_ctx *ctx, const float *state, const float *eps, const float *params, int flags);
/* SVMPC.optimize(state, params_dist, n_steps) svmpc.py:97-126. eps [n_steps][S][N][H][da] or NULL, params [n_steps][M][P] or NULL */
int dust_svmpc_optimize(dust_ctx *ctx, const float *state, int n_steps, const float *eps, const float *params, int flags);
/* SVMPC.forward(state, params_dist, fast_pred=True) svmpc.py:172-200: weights, argmax, roll, prior refresh.
 * a_seq [H][da], p_weights [N] (either may be NULL) */
int dust_svmpc_forward(dust_ctx *ctx, float *a_seq, float *p_weights);
/* The pieces of SVMPC.forward as the reference exposes them (svmpc.py:128-170), for callers that use them one by one:
 * get_weights (fast_pred=True: the costs of the last sample; weights only - theta and the prior stay as they are),
 * roll(steps, strategy) - theta.roll(steps, dims=-2) is CIRCULAR, the strategy then rewrites the last row; strategy "resample" takes
 * the last action of a prior sample per particle, drawn by the caller (`last_row` [N][da]; the reference draws prior.sample([N])) -
 * and update_prior(weights) (weights NULL: ones).  dust_svmpc_forward_ex = forward(steps, ...) with the context's roll strategy. */
int dust_svmpc_get_weights(dust_ctx *ctx, float *p_weights);
int dust_svmpc_roll(dust_ctx *ctx, int steps, int strategy, const float *last_row);
int dust_svmpc_update_prior(dust_ctx *ctx, const float *weights);
int dust_svmpc_forward_ex(dust_ctx *ctx, int steps, const float *resample_last_row, float *a_seq, float *p_weights);
/* CostLikelihood.sample(theta, state, params_dist) for a theta that is NOT the optimiser's (likelihoods.py:81-101 takes theta as an
 * argument and touches neither SVMPC.theta nor the optimiser state): rollouts around `theta` [N][H][da], the context's particles,
 * Adam moments and a_mat side effects as in the reference (a_mat is MultiDISCO state and does change). */
int dust_likelihood_sample_at(dust_ctx *ctx, const float *state, const float *theta, const float *eps, const float *params, int flags,
                              float *costs, float *actions_out);
/* one whole control tick = optimize(n_steps) + forward(), enqueued without host round trips (one persistent launch where eligible) */
int dust_svmpc_tick(dust_ctx *ctx, const float *state, int n_steps, const float *eps, const float *params, int flags,
                    float *a_seq, float *p_weights);

/* Closed-loop serving: the loop of dust/utils/simulations.py:104-123 - optimize, forward, first action to the plant, new state, repeat -
 * with the host's share off the device's critical path.  Between dust_svmpc_serve_start and dust_svmpc_serve_stop a call
 *   dust_svmpc_tick(ctx, state, n_steps, NULL, NULL, 0, a_seq, p_weights)        (device noise, the n_steps given here)
 * (1) receives its outputs through pinned host memory - the kernel writes them there and publishes a sequence number the call spins on:
 * no device-to-host copy, no stream synchronisation - and (2) launches the NEXT tick ahead of its plant state: that launch exchanges
 * its particles, draws its noise and runs its prior pass while the caller steps the plant, and its rollouts start when the next call
 * posts the state to a pinned mailbox.  Results are those of the same calls without serving, bit for bit.
 * The launched-ahead tick waits at most wait_us microseconds for its state (it occupies the whole device while it waits): a state that
 * comes later finds a launch that has given up - nothing written - and the tick is run then, late but correctly; after three such
 * misses in a row the context stops launching ahead.  wait_us = 0: outputs through pinned memory only.  Every other entry point of
 * the context, dust_create on the same device and the dynamics filter's calls cancel a waiting launch first (it leaves no trace).
 * Needs the one-launch tick's shape (K1 / IMQ kernel, N % 4 == 0, N / 4 <= CUs, H * da <= 32, one GPU, no sampled dynamics). */
int dust_svmpc_serve_start(dust_ctx *ctx, int n_steps, double wait_us);
int dust_svmpc_serve_stop(dust_ctx *ctx);

/* ---- AMPPI (dust/controllers/amppi.py): the single-policy information-theoretic MPC of Williams et al. 2017, ABI 3 ----
 * An AMPPI controller is a context created with n_policies = 1: n_samples = S trajectories, temperature = lambda_ (amppi.py:79),
 * chol_a / chol_a_off and a_pre / a_pre_off the factors of a_cov (amppi.py:83-86; a full 2 x 2 a_cov: full_cov = 1), min_a / max_a the
 * action space, seed the Philox key of device-drawn noise.  dust_set_a_seq / dust_get_a_seq hold BaseController.a_seq (base.py:34-37),
 * dust_set_grid / dust_set_skid_steer / dust_set_cartpole / dust_set_model_param describe the model as for any context, dust_clone is
 * copy.deepcopy(controller), and dust_profile_* counts the tick's kernel as DUST_K_AMPPI.  The cost families are the context's, with
 * the instantaneous cost ACTION-FREE (amppi.py:205 hands it states only: Particle's runs with actions = 0, the quadratic family's
 * control weights must be zero) and on states 1 .. H, so that state H takes the instantaneous and the terminal cost (amppi.py:205-207).
 *
 * dust_amppi_update = AMPPI.update_actions(model, state, actions) amppi.py:227-260 in ONE kernel launch (dust_amd/csrc/amppi.hpp):
 *   actions [S][H][da] (NULL: a_seq + L z drawn on the device, amppi.py:123-126; host pointer, or device with DUST_PTR_DEVICE); they are
 *     not clamped - the models clamp inside their step - and eps = actions - a_seq (amppi.py:129).  DUST_PTR_DEVICE speaks of `actions`
 *     alone: `state` and `params` are ALWAYS host pointers;
 *   params selects AMPPI(params_sampling=) amppi.py:88-104:
 *     NULL                                         "none": the model's own values (amppi.py:137);
 *     [1][P] with DUST_AMPPI_PARAMS_SHARED         "single": one row for every trajectory;
 *     [S][P]                                       "extended": row s for trajectory s (amppi.py:134-139);
 *     [2P + 1][P] after dust_set_param_weights     a MerweScaledUTF: every trajectory rolls all sigma points with the same actions and
 *                                                  their costs combine with the weights (amppi.py:142-191, 208-215); the context was
 *                                                  created with n_params = 2P + 1;
 *   outputs, each may be NULL: costs [S] (amppi.py:224), omega [S] (amppi.py:255), a_seq [H][da] AFTER the update (amppi.py:256-259).
 *   With DUST_STORE_STATES the trajectories stay on the device for dust_get_states_rows, row s * pts + k = trajectory s, sigma point k
 *   (the reference's [S pts][H + 1][ds], amppi.py:183-190; pts = 1 without a transform); dust_get_actions gives `acts` [S][H][da] and
 *   dust_get_costs the costs again.
 * DUST_ERR_UNSUPPORTED: S > 65536, H * da > 128 (dust_create), dim_p > 4, sharded contexts, params_log_space, binary16 storage,
 * Particle with velocity control or control-channel noise.  DUST_ERR_INVALID: n_policies != 1, params without uncertain parameters,
 * sigma weights without params or with n_params != 2 dim_p + 1, n_params > 1 without sigma weights (dim_p > 4: dust_create). */
int dust_amppi_update(dust_ctx *ctx, const float *state, const float *actions, const float *params, int flags,
                      float *costs, float *omega, float *a_seq);
/* BaseController.roll(steps) base.py:68-80: a_seq moves `steps` rows towards the front, the rows behind it are zeros.  steps >= 1
 * (the reference's slice arithmetic gives steps = 0 an all-zero sequence and negative steps a mixture: DUST_ERR_INVALID here). */
int dust_amppi_roll(dust_ctx *ctx, int steps);

/* ---- AMPPI over a batch of plants: B independent controllers of one configuration, ONE kernel launch per tick (ABI 3, additive) ----
 * The reference evaluates a controller over many episodes with a deep copy each (simulations.py); a batch is those B copies on one
 * device: every environment has its own state, nominal sequence, Philox stream and parameter rows, while the model, the cost, the
 * horizon, S, lambda and a_cov are shared.  The launch is a grid of (ceil(S / 256), B) workgroups (dust_amd/csrc/amppi.hpp
 * amppi_batch_kernel); environment b computes exactly what a lone dust_amppi_update computes on its inputs, bit for bit, and its
 * device-drawn noise continues the stream of a lone context created with seed seeds[b] that has made the same drawing calls.
 *
 * dust_amppi_batch_create: the batch keeps a private dust_clone of `proto` (model, cost, occupancy grid, navigation cost, sigma
 *   weights, profile counters): `proto` may be destroyed afterwards and later changes to it do not reach the batch.  seeds [n_env]
 *   (NULL: proto's seed + b); every environment starts from proto's a_seq and proto's stream position.  DUST_ERR_INVALID:
 *   n_env outside [1, 65535], n_policies != 1; DUST_ERR_UNSUPPORTED: whatever dust_amppi_update refuses of a context (sharded,
 *   params_log_space, Particle with velocity control or control-channel noise, ...).
 * dust_amppi_batch_clone: copy.deepcopy - an independent batch with the same sequences, stream positions and last actions.
 * dust_amppi_batch_set_a_seq / _get_a_seq: the nominal sequences [B][H][da].
 * dust_amppi_batch_ctx: the inner context, BORROWED (never dust_destroy it), for dust_sync and dust_profile_*: a batched tick counts
 *   as one DUST_K_AMPPI launch, a batched roll as one DUST_K_FORWARD launch. */
typedef struct dust_amppi_batch dust_amppi_batch;
int dust_amppi_batch_create(const dust_ctx *proto, int n_env, const uint64_t *seeds, dust_amppi_batch **out);
void dust_amppi_batch_destroy(dust_amppi_batch *batch);
int dust_amppi_batch_clone(const dust_amppi_batch *batch, dust_amppi_batch **out);
int dust_amppi_batch_set_a_seq(dust_amppi_batch *batch, const float *a_seq);
int dust_amppi_batch_get_a_seq(dust_amppi_batch *batch, float *a_seq);
int dust_amppi_batch_ctx(dust_amppi_batch *batch, dust_ctx **ctx);
/* dust_amppi_batch_update = B x dust_amppi_update in ONE launch behind ONE memset node that zeroes the B arrival words:
 *   states [B][ds], host;
 *   actions [B][S][H][da] (NULL: drawn on the device, environment b with key seeds[b] and its own counters; host pointer, or device
 *     with DUST_PTR_DEVICE, which speaks of `actions` alone);
 *   params by mode, host: NULL "none"; [B][1][P] with DUST_AMPPI_PARAMS_SHARED "single"; [B][S][P] "extended"; [B][2P + 1][P] sigma
 *     points of a prototype with dust_set_param_weights - one parameter distribution per environment;
 *   active [B] bytes, host, or NULL (all): the workgroups of an environment with active[b] = 0 return at once - its a_seq, its stream
 *     position and its device rows stay untouched, and its rows of the outputs are NOT written;
 *   outputs, each may be NULL: costs [B][S], omega [B][S], a_seq [B][H][da] after the update.  With all three NULL - and actions
 *     and params NULL or on the device - the call returns without waiting for the device.
 * DUST_ERR_UNSUPPORTED (before any launch): DUST_STORE_STATES, binary16 storage (DUST_EPS_F16 / DUST_STORE_F16), and what
 * dust_amppi_update refuses; the filter-coupled tick of a batch is dust_amppi_dual_batch_tick (below).  DUST_ERR_INVALID: NULL states,
 * params without uncertain parameters, sigma weights without params. */
int dust_amppi_batch_update(dust_amppi_batch *batch, const float *states, const float *actions, const float *params, int flags,
                            const unsigned char *active, float *costs, float *omega, float *a_seq);
/* dust_amppi_roll on every environment with active[b] != 0 (NULL: all) in one launch; steps >= 1. */
int dust_amppi_batch_roll(dust_amppi_batch *batch, int steps, const unsigned char *active);
/* The actions the last tick used, [B][S][H][da]; the rows of environments that were inactive in that tick are not written. */
int dust_amppi_batch_get_actions(dust_amppi_batch *batch, float *actions);
/* dust_amppi_batch_episode: n_periods closed-loop periods of every active environment, the plants stepped on the device - what the
 * reference's run_pendulum_simulation / run_particle_episode loop does per period (update_actions, the plant's step with the first
 * planned action, roll), without the host between two periods.  Period t is ONE launch (amppi_episode.hpp): the tick of
 * dust_amppi_batch_update with device-drawn noise from the state the previous period left, x <- step(x, a_seq[0]) under the environment's
 * true parameters through the family's own device step, the records, and dust_amppi_batch_roll(roll_steps).  The launches are chained on
 * the batch's stream behind one memset of the arrival words; the call waits once, for the records.
 *   states [B][ds], host: where the episodes start;
 *   params by mode, host, as dust_amppi_batch_update takes them with a leading [T]: NULL; [T][B][1][P] with DUST_AMPPI_PARAMS_SHARED;
 *     [T][B][S][P]; [T][B][2P + 1][P] sigma points.  Staged ONCE ahead of the first launch: at most 2^28 values (1 GiB) - and at most 2^28
 *     record values - per call, beyond which the call refuses with DUST_ERR_UNSUPPORTED and asks for a split episode;
 *   flags: DUST_AMPPI_PARAMS_SHARED alone (recorded actions, DUST_PTR_DEVICE, DUST_STORE_STATES, binary16: DUST_ERR_UNSUPPORTED);
 *   roll_steps >= 1; n_periods in [1, 4096];
 *   plant_params [B][P], host: every environment's TRUE parameter row, in the columns of `params`; NULL: the prototype's nominal model;
 *   active [B] bytes or NULL (all): inactive environments keep everything, and their rows of the outputs are NOT written;
 *   states_out [T][B][ds] (the state after every step) and actions_out [T][B][da] (the first action of the updated, clamped sequence)
 *     are required; costs_out / omega_out [T][B][S] and a_seq [B][H][da] (the last period's sequence BEFORE its roll) may be NULL.
 * Afterwards the batch is where n_periods x (dust_amppi_batch_update on the recorded states, dust_amppi_batch_roll) leave it, bit for
 * bit: sequences, stream positions, dust_amppi_batch_get_actions (the last period's); the profile counts n_periods DUST_K_AMPPI launches
 * and no DUST_K_FORWARD launch.  Every refusal comes before anything is staged or launched. */
int dust_amppi_batch_episode(dust_amppi_batch *batch, const float *states, int n_periods, const float *params, int flags, int roll_steps,
                             const float *plant_params, const unsigned char *active, float *states_out, float *actions_out, float *costs_out,
                             float *omega_out, float *a_seq);

/* ---- SVMPC over a batch of plants: B independent SVMPC controllers of one configuration, ONE kernel launch per call (ABI 3, additive) ----
 * The reference evaluates a controller over many episodes with a deep copy of the controller each (simulations.py:62,78); a batch is
 * those B copies on one device.  Every environment has its own state, particles, prior (means and mixture), a_mat, optimiser state,
 * Philox stream and dynamics samples; the model, the cost, N, S, M, H, the covariances, the Stein kernel and the optimiser's options
 * are shared.  The launch is a grid of B workgroups (dust_amd/csrc/svmpc_batch.hpp svmpc_batch_kernel): workgroup b runs the whole
 * call for environment b and talks to no other workgroup.  Environment b's results do not depend on B, on its slot or on its
 * neighbours, bit for bit; against a lone context on the same inputs they agree to rounding (other summation orders), and its
 * device-drawn noise continues the stream of a lone context created with seed seeds[b] that has made the same calls.
 *
 * The box (DUST_ERR_UNSUPPORTED / DUST_ERR_INVALID from dust_svmpc_batch_create, before anything is allocated): 1 <= n_policies <= 64,
 * 1 <= n_samples <= 1024, 1 <= n_params <= 64, H dim_a <= 128, dim_p <= 4, 1 <= n_env <= 65535, the K1 or the IMQ kernel, a_reg = 0
 * (ctrl_penalty = 1), diagonal covariances.  Not supported: sigma-point weights, Particle with velocity control or control-channel
 * noise, binary16 storage, DUST_STORE_STATES, roll strategy "resample", sharded contexts, contexts that are serving.
 * Every model family's cost runs in the batch.  A skid-steer prototype with an obstacle weight (dust_set_obstacle_cost: the navigation
 * cost family) ticks in instances of its own (svmpc_skid_nav_batch_kernel, svmpc_skid_nav_prior_batch_kernel, counted under
 * DUST_K_SVMPC_BATCH like the others): ONE map, the prototype's (dust_set_grid), serves the B environments - staged into the workgroup's
 * LDS up to 4096 words, read in place from device memory beyond (or with DUST_NAV_GRID_HBM=1), the same bits either way.  Without a map
 * dust_svmpc_batch_create and every call of the batch answer DUST_ERR_STATE ("no occupancy grid was supplied") before any launch.
 *
 * dust_svmpc_batch_create: the batch keeps a private dust_clone of `proto`: `proto` may be destroyed afterwards and later changes to it
 *   do not reach the batch.  Every environment starts from proto's particles, prior, a_mat, optimiser configuration and state, and
 *   stream position.  seeds [n_env] (NULL: proto's seed + b).
 * dust_svmpc_batch_clone: copy.deepcopy - an independent batch that continues exactly as its source would.
 * dust_svmpc_batch_ctx: the inner context, BORROWED (never dust_destroy it), for dust_sync and dust_profile_*: each of optimize,
 *   forward and tick counts as one DUST_K_SVMPC_BATCH launch. */
typedef struct dust_svmpc_batch dust_svmpc_batch;
enum dust_svmpc_batch_what {
  DUST_SVB_THETA = 0,       /* [B][N][H][da] set / get; set restarts the optimiser state, as dust_set_theta does */
  DUST_SVB_PRIOR_MEANS = 1, /* [B][N][H][da] set / get; after a forward the means ARE the particles (svgd.py:87) until they are set */
  DUST_SVB_PRIOR_MIX = 2,   /* [B][N] set: mixture weights >= 0; get: the probabilities */
  DUST_SVB_A_MAT = 3,       /* [B][N][H][da] set / get */
  /* get only, of the last iteration (DUST_ERR_STATE before one) or forward: */
  DUST_SVB_COSTS = 4,       /* [B][S][N] */
  DUST_SVB_SCORE = 5,       /* [B][N][H][da] */
  DUST_SVB_PHI = 6,         /* [B][N][H][da] */
  DUST_SVB_LOG_L = 7,       /* [B][N] */
  DUST_SVB_LOG_P = 8,       /* [B][N], of the last forward */
  DUST_SVB_A_MIX = 9,       /* [B][N] */
  DUST_SVB_ACTIONS = 10     /* [B][S][N][H][da], kept only when the call carried DUST_SVMPC_BATCH_KEEP_ACTIONS */
};
int dust_svmpc_batch_create(const dust_ctx *proto, int n_env, const uint64_t *seeds, dust_svmpc_batch **out);
void dust_svmpc_batch_destroy(dust_svmpc_batch *batch);
int dust_svmpc_batch_clone(const dust_svmpc_batch *batch, dust_svmpc_batch **out);
int dust_svmpc_batch_ctx(dust_svmpc_batch *batch, dust_ctx **ctx);
int dust_svmpc_batch_set(dust_svmpc_batch *batch, int what, const float *in);
int dust_svmpc_batch_get(dust_svmpc_batch *batch, int what, float *out);
/* dust_svmpc_batch_optimize = B x dust_svmpc_optimize in ONE launch (no memset node: there are no arrival words):
 *   states [B][ds], host;
 *   eps [B][n_steps][S][N][H][da], host, or device with DUST_PTR_DEVICE (which speaks of `eps` alone), or NULL: environment b draws
 *     with key seeds[b] in the lone kernels' counter layout;
 *   params [B][n_steps][M][P], host; NULL exactly when dim_p = 0 - one parameter distribution per environment;
 *   flags: DUST_PTR_DEVICE, DUST_SVMPC_BATCH_KEEP_ACTIONS;
 *   active [B] bytes, host, or NULL (all): the workgroup of an environment with active[b] = 0 returns at once and everything of that
 *     environment stays as it was.
 * The call returns without waiting for the device when eps and params are NULL or on the device.
 * dust_svmpc_batch_forward = B x dust_svmpc_forward in one launch: a_seq [B][H][da] (the best particle BEFORE the roll) and p_weights
 *   [B][N], each may be NULL; the rows of inactive environments are NOT written; with both NULL the call does not wait for the device.
 *   DUST_ERR_STATE before any step of the batch has produced costs.
 * dust_svmpc_batch_tick = optimize + forward in ONE launch.
 * DUST_ERR_UNSUPPORTED (before any launch): DUST_STORE_STATES, DUST_EPS_F16 / DUST_STORE_F16.  DUST_ERR_INVALID: NULL states,
 * n_steps < 0 (tick: < 1), params without uncertain parameters or uncertain parameters without params. */
int dust_svmpc_batch_optimize(dust_svmpc_batch *batch, const float *states, int n_steps, const void *eps, const float *params, int flags,
                              const unsigned char *active);
int dust_svmpc_batch_forward(dust_svmpc_batch *batch, const unsigned char *active, float *a_seq, float *p_weights);
int dust_svmpc_batch_tick(dust_svmpc_batch *batch, const float *states, int n_steps, const void *eps, const float *params, int flags,
                          const unsigned char *active, float *a_seq, float *p_weights);
/* dust_svmpc_batch_episode = T closed-loop periods of simulations.py:104-130 for every active environment in ONE launch
 * (dust_amd/csrc/svmpc_episode.hpp): per period the tick dust_svmpc_batch_tick runs, with device-drawn noise - period t draws what the
 * t-th successive tick would draw -, then the plant's step x <- step(x, a_seq[0]) through the family's own device step (the one the
 * rollouts call, Particle's collision freeze included; the action clamped as the rollouts clamp it) under the environment's TRUE
 * parameters, then the new state into the next tick.  Plants are deterministic.
 *   states [B][ds], host: where the episodes start;
 *   params [T][B][n_steps][M][P], host: params[t] is what dust_svmpc_batch_tick takes for period t; NULL exactly when dim_p = 0;
 *   plant_params [B][P], host, in the columns and the space (params_log_space) of `params`; NULL: the prototype's nominal model;
 *   flags: 0;
 *   records, host, copied back once after the launch; the rows of inactive environments are NOT written: states_out [T][B][ds] (the
 *     state after the step), actions_out [T][B][da] (the raw a_seq[0]), pw_out [T][B][N] or NULL (the particle weights), a_seq
 *     [B][H][da] of the LAST period (before the roll) or NULL.
 * Afterwards the batch is in the state T ticks would have left it in (getters, counters, noise streams).  The call waits for the device.
 * DUST_ERR_INVALID (before any launch): NULL states / states_out / actions_out, n_steps < 1, n_periods outside [1, 4096] (a launch runs
 * T ticks' worth of time; the cap keeps one launch on a shared device short - split a longer episode, the pieces concatenate bit for
 * bit), params or plant_params with dim_p = 0, missing params with dim_p > 0.  DUST_ERR_UNSUPPORTED: any flag. */
int dust_svmpc_batch_episode(dust_svmpc_batch *batch, const float *states, int n_periods, int n_steps, const float *params,
                             const float *plant_params, int flags, const unsigned char *active, float *states_out, float *actions_out,
                             float *pw_out, float *a_seq);
/* Per-environment hyper-parameters: a tuning sweep as ONE batch.  The reference tunes by running one episode per trial, each with its
 * own lr, alpha (temperature = 1 / alpha) and prior_sigma (demo/pendulum_tuning.py:30-143), ctrl_sigma and prior_weighted besides
 * (demo/particle_tuning.py:27-99); here the B trials are the B environments of a batch and dust_svmpc_batch_episode evaluates them in
 * one launch.  Row b replaces, for environment b alone, the fields of dust_config / dust_optim_config it names; alpha and temperature are
 * independent (temperature = 1 / alpha is the caller's line).  The horizon is NOT per environment: strides, the noise streams' layout
 * and the LDS plan depend on it - a horizon sweep is one batch per value.
 * dust_svmpc_batch_set_hyper: rows [B], host, copied (and uploaded on the batch's stream) before the call returns; NULL: back to the
 *   prototype's values.  Nothing else changes: particles, prior, a_mat, optimiser state and step counts, noise streams stay.
 *   DUST_ERR_INVALID, with the stored rows unchanged: a value that is not finite; lr, alpha, temperature, sigma_a, chol_a or sigma_p
 *   <= 0 (entry 1 of the three arrays is ignored when dim_a = 1, but must be finite); weighted_prior other than 0 or 1.
 * dust_svmpc_batch_get_hyper: the rows as they were set, or B times the prototype's values where none are set.
 * While rows are set, dust_svmpc_batch_optimize / _forward / _tick and dust_svmpc_batch_episode launch instances of their own
 * (svmpc_sweep_kernel, svmpc_sweep_episode_kernel: one launch per call, counted under DUST_K_SVMPC_BATCH): workgroup b reads row b and
 * runs the uniform kernels' text on its own copy of the arguments, so an environment whose row equals a prototype's values computes that
 * prototype's bits, whatever its neighbours' rows.  dust_svmpc_batch_clone copies the rows.  DUST_ERR_UNSUPPORTED while rows are set,
 * before anything is staged or launched: dust_svmpc_dual_batch_tick, dust_svmpc_dual_batch_episode, and every call of a batch whose
 * prototype has the navigation cost family. */
typedef struct dust_svmpc_hyper { /* one environment's row; the fields of dust_config / dust_optim_config it overrides */
  double lr;
  float alpha, temperature;
  float sigma_a[2], chol_a[2], sigma_p[2]; /* diagonal covariances: entry 1 ignored when dim_a = 1 */
  int weighted_prior;
} dust_svmpc_hyper;
int dust_svmpc_batch_set_hyper(dust_svmpc_batch *batch, const dust_svmpc_hyper *rows /* [B], or NULL: back to the prototype's */);
int dust_svmpc_batch_get_hyper(dust_svmpc_batch *batch, dust_svmpc_hyper *rows /* [B]: the prototype's values where none are set */);
/* dust_svmpc_batch_simulate = dust_svmpc_batch_episode under the reference's episode rules (run_particle_episode / run_pendulum_simulation,
 * simulations.py:104-130 and 217-260), still ONE launch (svmpc_episode.hpp svb_sim_body).  Period t of the call is period g = t0 + t of
 * the episode:
 *   warm-up    g < warm_up: the period is what dust_svmpc_batch_optimize runs (no forward: no roll, no prior refresh; the Philox position
 *              and the optimiser count move as an optimize call moves them), the plant gets a zero action; pw_out's row and a_seq are
 *              not written.  Otherwise the period is the tick;
 *   cost       the family's own instantaneous cost (the rollouts' - Particle with w_obs x collision, skid-steer / cart-pole the
 *              quadratic state cost, plus the map term under the navigation cost) of the state AFTER the step, with a zero action:
 *              costs_out[t][b], and loss[b] += cost as an fp32 running sum in period order;
 *   crash      stop_on_crash: the new position lies on an occupied cell of the batch's map -> loss[b] = +inf, status[b] = 2, stop;
 *   goal       goal_radius > 0: in fp32, d_k = goal[k] - x[k], s = ((d_0 d_0 + d_1 d_1) + d_2 d_2) + .. over the ds state entries,
 *              s <= (float)(goal_radius * goal_radius) -> status[b] = 1, stop.  The crash rule wins when both hold.
 * loss [B] and status [B] are read at entry and written at the end, so calls chain (t0: the periods the episode has run so far); an
 * environment that enters with status != 0 does nothing and nothing of it is written, except n_run[b] = 0.  n_run[b]: the periods
 * environment b ran in this call.  Afterwards environment b is where n_run[b] calls would have left it - dust_svmpc_batch_optimize
 * while warming up, then dust_svmpc_batch_tick: getters, counters, noise streams.  Rows t >= n_run[b] of states_out / actions_out /
 * pw_out / costs_out are NOT written, nor are the rows of inactive environments (loss, status and n_run included); a_seq [B][H][da] (may
 * be NULL) receives the row of an environment only when one of its periods ran forward().  With per-environment rows set the sweep
 * instances launch.  Everything else as dust_svmpc_batch_episode.
 * Refused before anything is staged, the batch and the in-out arrays unchanged - DUST_ERR_INVALID: what dust_svmpc_batch_episode
 * refuses; NULL rules, loss, status, n_run or costs_out; t0 < 0 or warm_up < 0; a goal or radius that is not finite; an entry status
 * outside 0 .. 2.  DUST_ERR_UNSUPPORTED: stop_on_crash on a batch with no occupancy map (Particle's with_obstacle map, or the
 * navigation cost's). */
typedef struct dust_episode_rules {
  int t0, warm_up, stop_on_crash;
  float goal_radius; /* <= 0: no goal rule */
  float goal[8];     /* the first ds entries are read */
} dust_episode_rules;
int dust_svmpc_batch_simulate(dust_svmpc_batch *batch, const float *states, int n_periods, int n_steps, const float *params,
                              const float *plant_params, const dust_episode_rules *rules, int flags, const unsigned char *active,
                              float *states_out, float *actions_out, float *pw_out, float *costs_out /* [T][B] */,
                              float *loss /* [B] in-out */, int *status /* [B] in-out */, int *n_run /* [B] out */, float *a_seq);
/* The posterior's history: the reference's per-period PolParticles / DynParticles rows (run_pendulum_simulation, simulations.py:122 and
 * 134-137; what plot_stein_particles and plot_dist_ridgeplot draw) out of the device episodes, written by the episodes' own kernels -
 * recording forms of the two rule-driven kernels (svmpc_episode.hpp svmpc_sim_hist_kernel / svmpc_dual_sim_hist_period_kernel) whose
 * workgroups copy their rows behind a period's closing sync.  No launch, copy or host round trip is added to a call, and nothing a call
 * computes changes.
 * dust_svmpc_batch_set_history(batch, what): what later calls record, a mask of DUST_HIST_THETA | DUST_HIST_FILTER; 0: nothing, and the
 *   buffers are released.  Nothing else of the batch changes.  DUST_ERR_INVALID for any other bit.
 *   While a bit is set dust_svmpc_batch_simulate records theta (DUST_HIST_THETA; with DUST_HIST_FILTER alone it records nothing) and
 *   dust_svmpc_dual_batch_simulate records theta (DUST_HIST_THETA) and the filters' particles (DUST_HIST_FILTER), into device buffers the
 *   batch owns, grown on demand.  Every other entry ignores the setting: it records nothing and the last recording stays.
 *   theta_hist[t] is what dust_svmpc_batch_get(DUST_SVB_THETA) returns after the t-th per-period call - dust_svmpc_batch_optimize /
 *   dust_svmpc_dual_batch_optimize while the episode warms up, the tick afterwards.  x_hist[t] is what dust_mpf_batch_get_particles returns
 *   after the t-th per-period dual call: the particles period t's dynamics samples were drawn from - in a period 0 without actions_prev
 *   the particles at entry.
 *   Refused by a recording call before anything is allocated, staged or launched, the batch and the in-out arrays unchanged, with
 *   DUST_ERR_UNSUPPORTED: more than DUST_SVMPC_HISTORY_MAX_FLOATS values of one kind (T B N H da, or T B Mp P: split the episode into
 *   shorter calls); a batch with per-environment controller rows (dust_svmpc_batch_set_hyper) or with the navigation cost - neither has a
 *   recording instance: dust_svmpc_batch_set_history(batch, 0) first.  Per-environment FILTER rows (dust_mpf_batch_set_hyper) touch the
 *   filters' kernels alone and keep working.  dust_svmpc_batch_clone copies the setting, not the recorded rows.
 * dust_svmpc_batch_get_history(batch, which, n_periods, out): the last recording of ONE kind (DUST_HIST_THETA or DUST_HIST_FILTER; anything
 *   else DUST_ERR_INVALID); DUST_ERR_STATE when no call has recorded that kind (or since set_history(batch, 0)).  *n_periods (may be
 *   NULL) receives T of the recording call; out (host; may be NULL to ask for T alone) is [T][B][N][H][da], or [T][B][Mp][P], copied
 *   once.  Rows (t, b) the call did not run - t >= n_run[b], inactive environments, environments that entered stopped - are NOT written:
 *   the caller's fill stays (the reference fills with NaN). */
enum { DUST_HIST_THETA = 1, DUST_HIST_FILTER = 2 };
#define DUST_SVMPC_HISTORY_MAX_FLOATS ((size_t)1 << 28) /* per kind and call: 1 GiB */
int dust_svmpc_batch_set_history(dust_svmpc_batch *batch, int what);
int dust_svmpc_batch_get_history(dust_svmpc_batch *batch, int which, int *n_periods, float *out);

/* ---- MultiDISCO over a batch of plants (ABI 3): B independent controllers - the MPPI baseline of the reference's demo/pendulum_example.py,
 * disco.py:139-417 - whose forward(), step() or both are ONE kernel launch (csrc/disco_batch.hpp), counted under DUST_K_ROLLOUT, the slot
 * of the lone dust_disco_forward's launch.  Per environment: a state, a_mat [N][H][da], a_seq [H][da], a_mix [N] (ones until a forward),
 * a Philox stream (key seeds[b]; NULL: the prototype's seed + b) and parameter rows; model, cost, map, N, S, M, H, temperature,
 * ctrl_penalty and a_cov are the prototype's.  Environment b's device-drawn actions are, bit for bit, those of a lone context created
 * with seed seeds[b] after the same calls, and an environment computes the same bits alone, in any slot of any batch and beside
 * inactive neighbours.
 * The box (dust_disco_batch_create: DUST_ERR_UNSUPPORTED before anything is allocated): dust_svmpc_batch_create's without its a_reg = 0 and
 * Stein-kernel conditions - N <= 64, S <= 1024, M <= 64, H da <= 128, dim_p <= 4, a diagonal a_cov, Particle with acceleration control
 * and no control-channel noise, one GPU.  Sigma-point rollouts (a prototype with dust_set_param_weights: the "DISCO" case) run on Pendulum,
 * skid-steer - with and without the navigation cost - and cart-pole, as dust_disco_forward runs them: the M rows of `params` are then the
 * pts = M <= 9 sigma points and a rollout's cost is the weighted sum of disco.py:312-323, not the mean.  Refused under sigma weights:
 * Particle, more than 9 points, no uncertain parameter, and - skid-steer and cart-pole - a non-zero control weight or a_reg != 0
 * (ctrl_penalty != 1), the two cases dust_disco_forward refuses.
 *   forward   states [B][ds]; actions [B][S][N][H][da] recorded (host) or NULL (drawn: a_mat + chol_a z); params [B][M][P] - every
 *             environment's sampled rows, or its sigma points [B][pts][P] under sigma weights -, or NULL exactly when the prototype has no
 *             uncertain parameters; flags: DUST_EPS_AROUND_A_MAT (recorded actions: eps = a - a_mat[n],
 *             not a - a_seq, as dust_disco_forward reads it) and DUST_SVMPC_BATCH_KEEP_ACTIONS (the ACTIONS getter serves this call's
 *             actions); every other flag DUST_ERR_UNSUPPORTED.  Updates a_mat, a_mix and the records COSTS / OMEGA.
 *   step      strategy: dust_step_strategy (DUST_STEP_EXTERNAL reads ext_actions [B][H][da]); steps in [1, H]; next_actions
 *             [B][steps][da] receives the rows of active environments.  "argmax" is the FIRST maximum of a_mix and clamps that row of
 *             a_mat in place, as dust_disco_step does.
 *   tick      forward then step in ONE launch.
 *   episode   n_periods (1 .. 4096) closed-loop periods in ONE launch: forward (drawn noise), step(strategy, 1), the plant's step under
 *             plant_params [B][P] (NULL: the nominal model), the records states_out [T][B][ds], actions_out [T][B][da].  params
 *             [T][B][M][P], or [B][M][P] serving every period with DUST_DISCO_PARAMS_ONCE (the only flag).  rules NULL: every active
 *             environment runs its T periods, costs_out / loss / status / n_run are not touched (may be NULL).  Otherwise the rules of
 *             dust_svmpc_batch_simulate - cost, fp32 running loss, crash, goal, chaining through t0 and the in-out loss / status, rows past
 *             n_run[b] not written - with warm_up = 0: this branch of the reference has no warm-up (anything else DUST_ERR_INVALID).
 *             t0 is checked as dust_svmpc_batch_simulate checks it and otherwise unused: without a warm-up no period depends on its
 *             index, and two calls chain through loss and status alone.
 *             DUST_STEP_EXTERNAL is refused.  a_seq [B][H][da] (may be NULL): every environment's sequence after its last period.
 * `active` [B] (NULL: everybody): an inactive environment runs nothing, none of its rows or output rows is written.
 * Refused before anything is staged or launched, in-out arrays untouched - DUST_ERR_INVALID: NULL arguments, a strategy outside 0 .. 2 or
 * "external" without rows, steps outside [1, H], params given without uncertain parameters or missing with them, what
 * dust_svmpc_batch_simulate refuses of rules; DUST_ERR_UNSUPPORTED: a flag not named above, stop_on_crash without a map; DUST_ERR_STATE: the
 * navigation cost family without its map. */
typedef struct dust_disco_batch dust_disco_batch;
enum dust_disco_batch_quantity {
  DUST_DCB_A_MAT = 0,  /* [B][N][H][da] set / get */
  DUST_DCB_A_SEQ = 1,  /* [B][H][da] set / get */
  DUST_DCB_A_MIX = 2,  /* [B][N] */
  DUST_DCB_COSTS = 3,  /* [B][S][N], of the last forward */
  DUST_DCB_OMEGA = 4,  /* [B][S][N] */
  DUST_DCB_ACTIONS = 5 /* [B][S][N][H][da], kept only when the call carried DUST_SVMPC_BATCH_KEEP_ACTIONS */
};
enum { DUST_DISCO_PARAMS_ONCE = 128 }; /* dust_disco_batch_episode: params is [B][M][P] and serves every period */
int dust_disco_batch_create(const dust_ctx *proto, int n_env, const uint64_t *seeds, dust_disco_batch **out);
void dust_disco_batch_destroy(dust_disco_batch *batch);
int dust_disco_batch_clone(const dust_disco_batch *batch, dust_disco_batch **out);
int dust_disco_batch_ctx(dust_disco_batch *batch, dust_ctx **ctx); /* borrowed: sync, profile counters */
int dust_disco_batch_set(dust_disco_batch *batch, int what, const float *in);
int dust_disco_batch_get(dust_disco_batch *batch, int what, float *out);
int dust_disco_batch_forward(dust_disco_batch *batch, const float *states, const float *actions, const float *params, int flags,
                             const unsigned char *active);
int dust_disco_batch_step(dust_disco_batch *batch, int strategy, int steps, const float *ext_actions, const unsigned char *active,
                          float *next_actions);
int dust_disco_batch_tick(dust_disco_batch *batch, const float *states, const float *actions, const float *params, int flags,
                          const unsigned char *active, int strategy, int steps, const float *ext_actions, float *next_actions);
int dust_disco_batch_episode(dust_disco_batch *batch, const float *states, int n_periods, const float *params, const float *plant_params,
                             int strategy, const dust_episode_rules *rules, int flags, const unsigned char *active, float *states_out,
                             float *actions_out, float *costs_out, float *loss, int *status, int *n_run, float *a_seq);

/* stage outputs of the last call, for parity tests ([S][N] / [N][H][da] / [N]) */
int dust_get_costs(dust_ctx *ctx, float *costs);
int dust_get_actions(dust_ctx *ctx, float *actions);
/* Trajectories of the states the last stored-states sample left on the device (MultiDISCO.forward's `states` [M][S][N][H+1][ds],
 * disco.py:190-200, 394 - 11 GB at BASELINE configs[2]; kept in HBM by dust_likelihood_sample(flags & DUST_STORE_STATES) and by
 * dust_disco_forward): rows[i] = (m*S + s)*N + n selects one rollout, out receives n_rows x [H+1][ds] values - fp32, or binary16 when
 * the sample ran with DUST_STORE_F16.  For callers (and parity tests) that need some rollouts, not an 11 GB copy. */
int dust_get_states_rows(dust_ctx *ctx, const long long *rows, int n_rows, void *out);
int dust_get_score(dust_ctx *ctx, float *score);
int dust_get_phi(dust_ctx *ctx, float *phi);
/* the two halves of the score of the last SVGD iteration: grad_lik (svmpc.py:50-53) and grad_pri (svmpc.py:38-41), [N][H][da] each;
   either pointer may be NULL */
int dust_get_score_parts(dust_ctx *ctx, float *grad_lik, float *grad_pri);
int dust_get_log_weights(dust_ctx *ctx, float *log_l, float *log_p);
int dust_get_bandwidths(dust_ctx *ctx, float *h); /* K2: [H*da] or [H] */

/* multi-GPU: the pairwise stages read every shard's theta/score from context-owned gather buffers ([N][D] each).
 * The caller all-gathers them in place with RCCL between dust_svmpc_local_score and dust_svmpc_apply_phi. */
int dust_gather_buffers(dust_ctx *ctx, void **theta_all, void **score_all, size_t *shard_bytes);
int dust_svmpc_local_score(dust_ctx *ctx, const float *state, const float *eps, const float *params, int flags);
/* dust_svmpc_local_score in two calls, so that the all-gather of theta (issued after dust_svmpc_apply_phi) can run while
 * the rollouts - which read only this rank's particles - execute: local_rollout (costs, weights, grad_lik, a_mat), then,
 * once every rank's theta has arrived, local_prior_score (prior pass over all particles; score = grad_lik + grad_pri). */
int dust_svmpc_local_rollout(dust_ctx *ctx, const float *state, const float *eps, const float *params, int flags);
int dust_svmpc_local_prior_score(dust_ctx *ctx);
int dust_svmpc_apply_phi(dust_ctx *ctx);
int dust_svmpc_forward_local(dust_ctx *ctx, void **log_w_all, size_t *shard_bytes);
int dust_svmpc_forward_finish(dust_ctx *ctx, float *a_seq, float *p_weights);
/* C-side multi-GPU tick (BASELINE.json north_star: "particle batches shard across the 8 GPUs of one node with an
 * RCCL all-gather over xGMI of particle states before the pairwise kernel step").  One process per GPU, each with a context created
 * for its shard (shard_offset = rank * N / world, shard_size = N / world).  Rank 0 calls dust_comm_unique_id and hands the bytes to
 * every rank out of band (MPI, a file, torch.distributed.broadcast_object_list, ...); every rank then calls dust_comm_init
 * (ncclCommInitRank - collective).  From then on dust_svmpc_tick / _optimize / _forward run the sharded tick themselves: the
 * in-place all-gathers of score and theta (per SVGD iteration) and of the log-weights and rolled particles (per tick) are issued
 * on the context's stream between the kernels - no host synchronisation, no Python in the loop.  RCCL is bound at run time
 * (dlopen of librccl.so): single-GPU hosts need none. */
#define DUST_COMM_ID_BYTES 128
int dust_comm_unique_id(void *id /* DUST_COMM_ID_BYTES */);
/* dust_comm_validate: the LOCAL checks of dust_comm_init (rank / world sane, the context's shard is rank's equal share, no communicator
 * yet, librccl loadable) and nothing else - no collective.  ABORT RULE: ncclCommInitRank has no time-out, so a rank that fails its checks
 * while the others enter it leaves them hanging; a launcher therefore calls dust_comm_validate on every rank, lets the ranks AGREE on the
 * result out of band (an all-gather of the status over the same channel that carries the id), and calls dust_comm_init only when every
 * rank passed (dust_amd/parallel.py ShardedSVMPC does exactly that). */
int dust_comm_validate(dust_ctx *ctx, int rank, int world);
int dust_comm_init(dust_ctx *ctx, const void *id, int rank, int world);
int dust_comm_destroy(dust_ctx *ctx);
/* The all-gathers of one sharded tick alone (per SVGD iteration: score rows and particles; per tick: the log-weights), `reps` times
 * back to back on the context's stream between one pair of HIP events -> microseconds per tick when nothing overlaps them.
 * Collective over all ranks; the context's particles are not touched.  (Measurement aid; no reference counterpart.) */
int dust_comm_probe(dust_ctx *ctx, int n_steps, int reps, double *us_per_tick);
/* The tick's all-gathers as DIRECT PEER STORES (dust_amd/csrc/peer_gather.hpp): the GPUs of a node are one xGMI hop apart, the pieces are
 * small (a rank's score / particle rows, its log-weights), so every rank writes its piece straight into every peer's buffer - mapped once,
 * here, through HIP IPC - and raises one arrival word per peer; a one-wave kernel in front of the first consumer waits for the words.
 * on != 0: map the peers' buffers (COLLECTIVE: the IPC handles travel through one all-gather of the communicator - every rank calls it,
 * or none); on == 0: back to the collective library's all-gathers.  DUST_PEER_GATHER=1 in the environment makes dust_comm_init call it.
 * Its outcome is collective as well: if ANY rank cannot map its peers (no IPC between the devices), every rank returns DUST_ERR_UNSUPPORTED and
 * keeps the collective library's all-gathers.  A piece that does not arrive within 1 s is reported by the next dust_sync / tick output as DUST_ERR_HIP.  (No reference counterpart:
 * the reference is single-device.) */
int dust_comm_peer_gather(dust_ctx *ctx, int on);
/* run the context's kernels on an external HIP stream (hipStream_t), e.g. torch's current stream */
int dust_set_stream(dust_ctx *ctx, void *hip_stream);

/* timing / roofline support: HIP-event timing of each kernel family on the context's stream */
enum dust_kernel_id {
  DUST_K_ROLLOUT = 0, DUST_K_PRIOR_SCORE = 1, DUST_K_STEIN = 2, DUST_K_UPDATE = 3, DUST_K_FORWARD = 4, DUST_K_BANDWIDTH = 5,
  DUST_K_MPF = 6, DUST_K_ROLLOUT_STATES = 7 /* whole-line stored-states rollouts */, DUST_K_AMPPI = 8 /* dust_amppi_update */, DUST_K_COUNT = 9 /* the ids of ABI 3's first list, above: frozen */,
  /* appended behind that list: */
  DUST_K_SVMPC_BATCH = 9 /* dust_svmpc_batch_optimize / _forward / _tick */, DUST_K_ALL = 10 /* every id is < DUST_K_ALL */
};
int dust_profile_enable(dust_ctx *ctx, int on);
int dust_profile_get(dust_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);
int dust_profile_reset(dust_ctx *ctx);
/* reps back-to-back launches of the standalone rollout kernel over device-resident eps [n_slices][S][N][D] (slice r %
 * n_slices per launch) between one pair of HIP events on the context's stream; *avg_ms = elapsed / reps.
 * flags: DUST_EPS_F16 when eps_dev holds binary16 values; DUST_STORE_STATES (| DUST_STORE_F16): the stored-states form - it may
 * be two launches (rollout_states.hpp + the injected-costs pass), so a second series of `reps` launches is then timed one event
 * pair per launch into the per-kernel slots (dust_profile_get: DUST_K_ROLLOUT_STATES, DUST_K_ROLLOUT; earlier totals are reset). */
int dust_profile_rollout(dust_ctx *ctx, const float *state, const float *eps_dev, int n_slices, int reps, int flags, double *avg_ms);
const char *dust_kernel_name(int kernel_id);
/* algorithmic bytes one launch of the rollout kernel moves (SURVEY.md section 8d B_roll) */
int dust_rollout_algorithmic_bytes(const dust_ctx *ctx, int flags, double *bytes);
/* device scratch for benchmarks: allocate/fill standard-normal noise in HBM with the context's Philox stream
 * (n values; flags: DUST_EPS_F16 -> binary16 values, n * 2 bytes) */
int dust_device_noise_alloc(dust_ctx *ctx, size_t n_floats, uint64_t seed, int flags, void **dptr);
int dust_device_free(dust_ctx *ctx, void *dptr);

/* ---- MPF: dynamics-parameter SVGD filter (mpf.py:13-86, likelihoods.py:12-64, svgd.py:92-99) ---- */
typedef struct dust_mpf_config {
  int32_t abi_version, device;
  int32_t n_particles; /* M_p */
  int32_t dim_p, dim_s, dim_a;
  int32_t model;
  int32_t log_space;   /* GaussianLikelihood(log_space=) */
  float obs_std, lr, bw_scale;
  float init_bw;       /* MPF(bw=): bandwidth of the initial prior; <= 0: bw_silverman of the particles (svgd.py:55-81) */
  dust_config model_cfg; /* only the model fields are read */
} dust_mpf_config;
/* Models: DUST_MODEL_PENDULUM, DUST_MODEL_PARTICLE (acceleration control), DUST_MODEL_SKID_STEER (dim_s = 5, dim_a = 2, dim_p = 1..3;
 * model_cfg.dt is SkidSteerRobot's delta_t; model_cfg.ctrl_noise stays a Particle field) and DUST_MODEL_CARTPOLE (dim_s = 4, dim_a = 1,
 * dim_p = 1..4; dust_mpf_set_cartpole). */
int dust_mpf_create(const dust_mpf_config *cfg, const float *init_particles, const float *initial_obs, dust_mpf **out);
/* The filter's SkidSteerRobot (skid_steer_robot.py:19-52): the three parameters with kind / column / value - a sampled one names its
 * particle column, in any order - and the wheel-speed bounds; the cost fields of the struct are ignored.  Validated as
 * dust_set_skid_steer validates (a sampled column outside dim_p, or named twice: DUST_ERR_INVALID).  Until the call the constructor's
 * defaults hold with nothing sampled, and dust_mpf_phi / dust_mpf_optimize return DUST_ERR_STATE; they do so as well while the sampled
 * columns do not cover dim_p.  dust_mpf_clone copies the model.  dust_dual_tick takes a skid-steer controller and filter that name the
 * same uncertain parameters in the same columns. */
int dust_mpf_set_skid_steer(dust_mpf *mpf, const dust_skid_config *cfg);
/* The filter's CartPoleModel (cartpole.py:42-88; likelihoods.py:30-46 steps every particle once from the past observation): the seven
 * parameters with kind / column / value; the cost fields are ignored.  Validated as dust_set_cartpole validates.  Until the call the
 * constructor's defaults hold with nothing sampled, and dust_mpf_phi / dust_mpf_optimize return DUST_ERR_STATE; they do so as well
 * while the sampled columns do not cover dim_p.  model_cfg.dt is the model's dt (0.05 in the reference, base.py); model_cfg.ctrl_noise
 * stays a Particle field.  dust_mpf_clone copies the model.  dust_dual_tick takes a cart-pole controller and filter that name the same
 * uncertain parameters in the same columns. */
int dust_mpf_set_cartpole(dust_mpf *mpf, const dust_cartpole_config *cfg);
int dust_mpf_clone(const dust_mpf *src, dust_mpf **out);
/* MPF(optimizer_class=, **opt_args) svgd.py:108-122, mpf.py:24: DUST_OPT_SGD (default here, the demos' choice) or DUST_OPT_ADAM (the
 * reference's class default; betas / eps as torch.optim.Adam).  The optimiser state starts at zero and persists across
 * dust_mpf_optimize calls, as the reference's does (the optimiser is built once in MPF.__init__). */
int dust_mpf_set_optimizer(dust_mpf *mpf, int optimizer, float beta1, float beta2, float eps);
/* Any optimiser of dust_set_optimizer for the filter; opt->lr replaces the config's lr.  The state (and the step count) starts at
 * its initial value and persists across dust_mpf_optimize calls; dust_mpf_clone copies it. */
int dust_mpf_set_optimizer_ex(dust_mpf *mpf, const dust_optim_config *opt);
void dust_mpf_destroy(dust_mpf *mpf);
/* MPF.optimize(action, new_obs, bw, n_steps) mpf.py:64-86 -> grad_norms [n_steps] */
int dust_mpf_optimize(dust_mpf *mpf, const float *action, const float *new_obs, float bw, int n_steps, float *grad_norms);
int dust_mpf_phi(dust_mpf *mpf, float bw, float *phi); /* MPF.phi mpf.py:40-57 */
/* GaussianLikelihood.condition(action, new_obs) likelihoods.py:51-64 */
int dust_mpf_condition(dust_mpf *mpf, const float *action, const float *new_obs);
/* Control-channel noise inside the filter's one-step prediction (likelihoods.py:30-46 -> Particle.step particle.py:145-148 with
 * model_cfg.ctrl_noise): `acts` there is the bare past action, so ONE da-vector is drawn per MPF.phi call - per SVGD step - and shared
 * by all filter particles.  z [n][da]: recorded draws consumed one per step by the following dust_mpf_phi / dust_mpf_optimize calls;
 * when used up (or z = NULL) a host generator seeded from model_cfg.seed draws them. */
int dust_mpf_set_ctrl_noise(dust_mpf *mpf, const float *z, int n);
/* occupancy grid for the Particle model's crash mask inside the one-step prediction */
int dust_mpf_set_grid(dust_mpf *mpf, const float *grid, int nx, int ny, float off_x, float off_y);
int dust_mpf_get_particles(dust_mpf *mpf, float *x);
int dust_mpf_set_particles(dust_mpf *mpf, const float *x);
int dust_mpf_get_prior(dust_mpf *mpf, float *means, float *bw);
/* MPF(bw=None) with P > 1 parameters (mpf.py:29-38): bw_silverman (svgd.py:55-81) of the particle columns is a [P] vector and
 * `bw ** 2 * torch.eye(P)` makes it the covariance diag(bw_p^2) of the FIRST prior; n = 1 or P values.  Every later
 * update_prior(bw) (mpf.py:85, at the end of optimize) is scalar again.  dust_mpf_get_prior reports bw[0]; _get_prior_bw all P. */
int dust_mpf_set_prior_bw(dust_mpf *mpf, const float *bw, int n);
int dust_mpf_get_prior_bw(dust_mpf *mpf, float *bw);
/* How dust_mpf_optimize calls ran: out[0] calls served by a multi-workgroup kernel (>= 96 particles, >= 2 steps; mpf.hpp), out[1]
 * those among them that did not start or did not commit (the grid was not co-resident / a wait gave up) and were run by the
 * single-workgroup kernel instead - the caller saw DUST_OK either way. */
int dust_mpf_stats(dust_mpf *mpf, long long out[2]);
/* mpf.prior.sample([n]) / .log_prob(x): the controller draws its dynamics samples here (disco.py:171-172) */
int dust_mpf_prior_sample(dust_mpf *mpf, int n, uint64_t seed, float *samples);
int dust_mpf_prior_log_prob(dust_mpf *mpf, int n, const float *x, float *log_prob);
/* MPF.optimize's default bandwidth, `silvermans_rule(self.x.view(-1, 1)) * self.bw_scale` (mpf.py:68-73; KDEpy 1.1.0, third party: parity
 * unpinned), evaluated on the device (float64, numpy's linear-interpolation quartiles): one launch + a 4-byte read-back. */
int dust_mpf_silverman(dust_mpf *mpf, float *bw);
/* tf.compute_sigma_points(mpf.prior.mean, mpf.prior.variance.diag()) (disco.py:240-251 on the prior of mpf.py:26-38; utf.py:93-123) on
 * the device: mean and variance of the particle mixture (variance = bw^2 + the particles' spread), then the mean and mean +-
 * sqrt(scale var_p) e_p with scale = lambda + n.  out [2P + 1][P], host.  DUST_ERR_INVALID unless scale > 0. */
int dust_mpf_sigma_points(dust_mpf *mpf, float scale, float *out);
/* One control period of the dual loop (simulations.py:104-138; BASELINE north_star "DualSVMPC step() / forward()") in ONE call:
 * mpf.optimize(action_prev, state, bw, mpf_steps) (skipped when action_prev is NULL: the first period; mpf_bw <= 0: Silverman's rule of
 * the filter's particles, on the device) -> the controller's n_steps x [M][P] dynamics samples drawn from the filter's refreshed prior on
 * the device, into the controller's parameter buffer (dyn_dist = mpf.prior: simulations.py:79, disco.py:171) -> svmpc.optimize(n_steps) +
 * svmpc.forward().  a_seq [H][da], p_weights [N] or NULL; *bw_used (or NULL): the bandwidth of the filter update.  seed: Philox key of the
 * period's draws (the stream of dust_mpf_prior_sample).
 * A controller with sigma-point weights (dust_set_param_weights) takes the sigma points of the filter's prior instead of draws
 * (MultiDISCO._sigma_rollout, disco.py:240-251; the same points for each of the n_steps iterations; seed unused): DUST_ERR_UNSUPPORTED
 * without dust_set_sigma_scale or with params_log_space (disco.py:125), DUST_ERR_INVALID unless M = 2P + 1. */
int dust_dual_tick(dust_ctx *ctx, dust_mpf *mpf, const float *state, const float *action_prev, int n_steps, int mpf_steps, float mpf_bw,
                   uint64_t seed, float *a_seq, float *p_weights, float *bw_used);
/* One control period of the dual loop over an AMPPI controller (simulations.py:104-138 around amppi.py:227-260) in ONE call, ABI 3:
 *   1. mpf.optimize(action_prev, state, bw, mpf_steps) - skipped when action_prev is NULL; mpf_bw <= 0: Silverman's rule on the device;
 *   2. the parameters from the refreshed prior (model.params_dist = mpf.prior):
 *        no flag                      "extended": trajectory s rolls out on row s of dust_mpf_prior_sample(mpf, S, seed), which its lane
 *                                     draws inside the tick's kernel - no parameter buffer, no extra launch, no host copy;
 *        DUST_AMPPI_PARAMS_SHARED     "single": row 0 of dust_mpf_prior_sample(mpf, 1, seed), staged on the device;
 *        sigma weights and a scale    (dust_set_param_weights, dust_set_sigma_scale) the 2P + 1 points of dust_mpf_sigma_points(mpf, scale),
 *                                     staged on the device; seed unused;
 *   3. dust_amppi_update(state, actions, those parameters); actions NULL: device-drawn noise from the context's own stream;
 *   4. outputs, each may be NULL: costs [S], omega [S], a_seq [H][da] after the update and BEFORE the roll, params_out - the rows the
 *      tick used ([S][P], [1][P] or [2P + 1][P]) -, *bw_used (0 without a filter update);
 *   5. dust_amppi_roll(roll_steps) when roll_steps > 0.
 * DUST_ERR_INVALID / DUST_ERR_UNSUPPORTED: whatever dust_amppi_update refuses (n_policies != 1, sharded contexts, ...), dim_p != the
 * filter's P (this covers "none"), different devices, controller and filter naming different skid-steer / cart-pole parameters or column
 * orders (as dust_dual_tick), a log-space filter (amppi.py:134-139 hands samples to the model as drawn), sigma weights without a scale or
 * with n_params != 2P + 1, DUST_STORE_STATES.  With every output NULL the call returns without waiting for the device; the filter's
 * stream is ordered behind the tick's kernels, which read its particles in place. */
int dust_amppi_dual_tick(dust_ctx *ctx, dust_mpf *mpf, const float *state, const float *action_prev, const float *actions, int flags,
                         int mpf_steps, float mpf_bw, uint64_t seed, int roll_steps, float *costs, float *omega, float *a_seq,
                         float *params_out, float *bw_used);

/* ---- B dynamics filters of one configuration: the deep copies of the MPF the reference makes per episode (simulations.py:62,78) ----
 * One workgroup per environment runs the single-workgroup form of dust_mpf_optimize (mpf.hpp mpf_optimize_batch_kernel): environment b
 * computes what a lone filter created under DUST_MPF_GRID=0 computes on its inputs, bit for bit.  Limits: up to 1024 particles over
 * 1 .. 4 parameters, n_env in [1, 65535], no control-channel noise in the filter's model (its per-step actions are drawn on the host),
 * and one particle column per uncertain parameter of the model - at most 3 (Pendulum: g, mass, length), 1 (Particle: mass), 3
 * (skid-steer), 4 (cart-pole); a filter with more columns than its model has parameters is DUST_ERR_UNSUPPORTED.
 * dust_mpf_batch_create copies everything `proto` holds into every environment - particles, observation, past observation and past
 *   action, prior bandwidths, optimiser configuration, state and step count, model and occupancy grid; `proto` may be destroyed afterwards.
 * dust_mpf_batch_clone: copy.deepcopy.  _set_particles / _get_particles: [B][Mp][P].  _set_obs: every environment's observation [B][ds]
 *   (the state the next update's prediction starts from).  _get_prior_bw: [B][4] (the first P of a row are the environment's).
 * dust_mpf_batch_stats: out[0] kernel launches made for the filter side so far, out[1] calls (updates and dual ticks).
 * dust_mpf_batch_optimize = B x dust_mpf_optimize(action[b], new_obs[b], bw, n_steps) in one launch - plus one for Silverman's rule of
 *   every environment's particles when bw <= 0 (the bandwidths stay in device memory), plus one for the heading / angle terms of a
 *   skid-steer / cart-pole filter.  active [B] bytes or NULL: an environment with active[b] = 0 keeps everything, and its rows of
 *   bw_used [B] and grad_norms [B][n_steps] (each may be NULL) are not written. */
typedef struct dust_mpf_batch dust_mpf_batch;
int dust_mpf_batch_create(const dust_mpf *proto, int n_env, dust_mpf_batch **out);
void dust_mpf_batch_destroy(dust_mpf_batch *batch);
int dust_mpf_batch_clone(const dust_mpf_batch *batch, dust_mpf_batch **out);
int dust_mpf_batch_set_particles(dust_mpf_batch *batch, const float *x);
int dust_mpf_batch_get_particles(dust_mpf_batch *batch, float *x);
int dust_mpf_batch_set_obs(dust_mpf_batch *batch, const float *obs);
int dust_mpf_batch_get_prior_bw(dust_mpf_batch *batch, float *bw);
int dust_mpf_batch_stats(dust_mpf_batch *batch, long long out[2]);
int dust_mpf_batch_optimize(dust_mpf_batch *batch, const float *actions, const float *new_obs, float bw, int n_steps, const unsigned char *active,
                            float *bw_used, float *grad_norms);
/* Per-environment filter hyper-parameters: the B trials of a sweep over the filter's own settings (the reference's mpf_learning_rate,
 * mpf_obs_std, mpf_bandwidth, mpf_bandwidth_scaling of demo/.._config.yaml) as the environments of one batch.  Pendulum and Particle filters; rows
 * on a skid-steer or cart-pole batch are DUST_ERR_UNSUPPORTED.
 * dust_mpf_batch_set_hyper: rows [B], host, copied (and uploaded on the batch's stream) before the call returns; NULL: back to the
 *   prototype's values and the uniform kernels.  Particles, optimiser state, step counts, prior bandwidths and host rows are not touched.
 *   A row with a value that is not finite, or with lr, obs_std or bw_scale <= 0, is DUST_ERR_INVALID and leaves the stored rows as they
 *   were.  dust_mpf_batch_clone copies the rows.
 * dust_mpf_batch_get_hyper: the rows as they were set, or B times the prototype's values where none are set - bw is then 0 (the
 *   prototype has no bandwidth of its own: each call names one).
 * While rows are set the rows carry the bandwidths: the bw of dust_mpf_batch_optimize and the mpf_bw of every dual entry must be <= 0
 *   (> 0: DUST_ERR_INVALID ahead of any staging or launch).  Environment b updates under rows[b].bw when that is > 0, else under
 *   Silverman's rule on its own particles times rows[b].bw_scale; bw_used / bw_out and the refreshed prior bandwidths report that value.
 *   The launch count per update is the one of a call with bw <= 0 without rows, whatever B and the rows' values. */
typedef struct dust_mpf_hyper { /* one environment's row */
  double lr;      /* the optimiser's lr (dust_optim_config.lr) */
  float obs_std;  /* GaussianLikelihood's sigma */
  float bw;       /* > 0: this environment's fixed kernel bandwidth; <= 0: Silverman's rule on its particles */
  float bw_scale; /* the factor on Silverman's rule (MPF(bw_scale=)) */
  float reserved; /* 0 */
} dust_mpf_hyper;
int dust_mpf_batch_set_hyper(dust_mpf_batch *batch, const dust_mpf_hyper *rows /* [B], or NULL: back to the prototype's */);
int dust_mpf_batch_get_hyper(dust_mpf_batch *batch, dust_mpf_hyper *rows /* [B]: the prototype's values where none are set */);
/* One control period of the dual loop for B environments in one call = B x dust_amppi_dual_tick, on the AMPPI batch's stream in launch
 * order with no event, no synchronisation and no host round trip between the filters and the ticks; the number of kernel launches does
 * not depend on B.  states [B][ds]; actions_prev [B][da] or NULL (no filter update: the first period); actions [B][S][H][da] or NULL
 * (drawn on the device); mpf_bw <= 0: Silverman's rule per environment on the device; prior_seeds [B]: the Philox key of every
 * environment's draws (unused by sigma points).  Parameters as dust_amppi_dual_tick: "extended" drawn inside the tick's kernel
 * (amppi_prior_batch_kernel), DUST_AMPPI_PARAMS_SHARED and sigma points staged for all B by one launch.  Outputs, each may be NULL:
 * costs / omega [B][S], a_seq [B][H][da] after the update and before the roll, params_out [B][rows][P], bw_used [B] (0: no update).
 * An environment with active[b] = 0 keeps its particles, optimiser state, bandwidths, sequence and stream position; its output rows are
 * not written.  With every output NULL the call returns without waiting for the device.  Refused before any launch: what
 * dust_amppi_dual_tick and dust_amppi_batch_update refuse, batches of different n_env or on different devices. */
int dust_amppi_dual_batch_tick(dust_amppi_batch *batch, dust_mpf_batch *mpf, const float *states, const float *actions_prev, const float *actions,
                               int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds, int roll_steps, const unsigned char *active,
                               float *costs, float *omega, float *a_seq, float *params_out, float *bw_used);
/* dust_amppi_dual_batch_episode: n_periods periods of the dual loop over the AMPPI batch with the plants on the device - what n_periods
 * dust_amppi_dual_batch_tick calls with device-drawn noise and roll_steps >= 1 compute, with x_{t+1} = step(x_t, a_t) under the true
 * rows plant_params between them (dust_amppi_batch_episode's plant).  Arguments as that tick's, minus `actions`; prior_seeds [T][B]:
 * period t draws under row t; the records as dust_amppi_batch_episode's plus bw_out [T][B] (the bandwidth every period's update ran
 * with; 0: no update).  Per period, on the controller batch's stream: Silverman's rule and the filters' update reading their rows in
 * device memory, in the single and sigma modes the staging launch of the parameter rows, ONE launch of the period kernel, whose reducer
 * also conditions the environment's filter row for the next period.  The call waits once; afterwards both batches are where the ticks
 * leave them, and the pair (a_{T-1}, x_T) stays pending: pass actions_out[T - 1] as actions_prev of the next call.
 * Pendulum and Particle pairs; a skid-steer or cart-pole pair is DUST_ERR_UNSUPPORTED (their likelihood rows carry host fp64
 * trigonometry), as is every flag but DUST_AMPPI_PARAMS_SHARED.  Every refusal comes before anything is staged or launched. */
int dust_amppi_dual_batch_episode(dust_amppi_batch *batch, dust_mpf_batch *mpf, const float *states, const float *actions_prev, int n_periods,
                                  int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds, int roll_steps, const float *plant_params,
                                  const unsigned char *active, float *states_out, float *actions_out, float *costs_out, float *omega_out,
                                  float *bw_out, float *a_seq);
/* One control period of the DuSt-MPC loop for B environments in one call = B x dust_dual_tick, on the SVMPC batch's stream in launch
 * order with no event, no synchronisation and no host round trip between the filters and the ticks; the number of kernel launches does
 * not depend on B.  states [B][ds]; actions_prev [B][da] or NULL (no filter update: the first period); mpf_bw <= 0: Silverman's rule per
 * environment on the device; then ONE launch of n_steps SVGD iterations and forward() (svmpc_prior_batch_kernel, counted under
 * DUST_K_SVMPC_BATCH).  In iteration `it` the dynamics sample m of environment b is row it M + m of
 * dust_mpf_prior_sample(filter b after its update, n_steps M, prior_seeds[b]), drawn inside the tick's kernel.  eps
 * [B][n_steps][S][N][H][da] on the host, on the device with DUST_PTR_DEVICE, or NULL (drawn on the device from every environment's own
 * stream); DUST_SVMPC_BATCH_KEEP_ACTIONS as dust_svmpc_batch_tick.  Outputs, each may be NULL: a_seq [B][H][da] (the best particle
 * before the roll), p_weights [B][N], params_out [B][n_steps][M][P], bw_used [B] (0: no update; mpf_bw when that was given).  An
 * environment with active[b] = 0 keeps everything on both sides; its output rows are not written.  With every output NULL the call
 * returns without waiting for the device.  Refused before anything is staged or launched: what dust_svmpc_batch_tick refuses (sigma-point
 * weights among it: a batch does not run the sigma mode of dust_dual_tick; the navigation cost family is NOT among it - it ticks in
 * svmpc_skid_nav_prior_batch_kernel on the batch's one map), what dust_dual_tick refuses of a controller / filter pair,
 * what dust_mpf_batch_optimize refuses, batches of different n_env, NULL prior_seeds, n_steps < 1, mpf_steps < 0. */
int dust_svmpc_dual_batch_tick(dust_svmpc_batch *batch, dust_mpf_batch *mpf, const float *states, const float *actions_prev, int n_steps,
                               const void *eps, int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds,
                               const unsigned char *active, float *a_seq, float *p_weights, float *params_out, float *bw_used);
/* dust_svmpc_dual_batch_episode = T control periods of the DuSt-MPC loop (simulations.py:104-138) for B environments in one call: T
 * successive dust_svmpc_dual_batch_tick calls with device-drawn noise (eps NULL), and between them what the host would do -
 * x_{t+1} = step(x_t, a_t), a_t the raw a_seq[0] chosen before the roll - done on the device: the plant of dust_svmpc_batch_episode (the
 * family's own device step under the environment's TRUE parameter row, or the nominal model; deterministic).  Period t takes
 * states = x_t, actions_prev = a_{t-1} (period 0: the call's actions_prev; NULL skips that one update, as in the dual tick) and the key
 * row prior_seeds + t B.  Bit for bit on both sides: every getter of the SVMPC batch; the filters' particles, prior bandwidths, optimiser
 * slots, step counts and host rows; the Philox positions; dust_mpf_batch_stats (launches and calls advanced as by the T ticks).
 *   Flow: everything is staged once ahead of the first launch (states, mask, seeds, plant rows, the filters' per-environment input rows);
 *   all periods are then enqueued on the controller batch's stream, with no host wait, event or copy between them; the call waits once,
 *   for the records.  A period launches Silverman's rule (mpf_bw <= 0) and the filters' update when it has one - the kernels of
 *   dust_mpf_batch_optimize, reading their per-environment rows from device memory - and ONE launch of svmpc_dual_period_kernel
 *   (dust_amd/csrc/svmpc_episode.hpp, counted under DUST_K_SVMPC_BATCH): the tick of dust_svmpc_dual_batch_tick, the plant's step, the
 *   records, and GaussianLikelihood.condition (likelihoods.py:51-64) of the filter's row for the next period.  The launch count does not
 *   depend on B.
 *   states [B][ds], actions_prev [B][da] or NULL, prior_seeds [T][B], plant_params [B][P] or NULL (the columns and the space of the
 *   controller's dynamics samples), all host; flags: 0;
 *   records, host, copied back once after the last launch, the rows of inactive environments NOT written: states_out [T][B][ds] (the
 *     state after the step), actions_out [T][B][da] (the raw a_seq[0]), pw_out [T][B][N] or NULL, bw_out [T][B] or NULL (bw_used of the
 *     period's dual tick; 0 where no update ran), a_seq [B][H][da] or NULL (the last period's sequence, before the roll).
 * The pending pair: after T periods (a_{T-1}, x_T) has NOT been folded into the filters, exactly as after T dual ticks; hand
 * actions_out[T-1] and states_out[T-1] to the next call as actions_prev and states: two episodes chained that way equal one of T1 + T2
 * periods (a change of the true parameters mid-episode is two chained calls).
 * Refused before anything is staged or launched, both batches untouched.  DUST_ERR_INVALID: what dust_svmpc_dual_batch_tick refuses; NULL
 * states, states_out, actions_out or prior_seeds; n_periods outside [1, 4096]; n_steps < 1; mpf_steps < 0; plant_params with dim_p = 0.
 * DUST_ERR_UNSUPPORTED: any flag; a skid-steer or cart-pole pair, the navigation cost included (their filters' likelihood rows carry
 * sin / cos of the past heading from the host's libm: a device-side conditioning would not be bit-equal to the period-by-period loop). */
int dust_svmpc_dual_batch_episode(dust_svmpc_batch *batch, dust_mpf_batch *mpf, const float *states, const float *actions_prev,
                                  int n_periods, int n_steps, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds,
                                  const float *plant_params, int flags, const unsigned char *active,
                                  float *states_out, float *actions_out, float *pw_out, float *bw_out, float *a_seq);
/* dust_svmpc_dual_batch_optimize = one WARM-UP period of the DuSt-MPC loop (simulations.py:104-117 while step < warm_up) for B
 * environments: dust_svmpc_dual_batch_tick WITHOUT forward() - the filters' update for (actions_prev[b], states[b]) (skipped when
 * actions_prev is NULL), then ONE launch of svmpc_prior_batch_kernel (or the navigation instance) with do_forward = 0.  No roll, no prior
 * refresh, no a_seq and no weights; the Philox position and the optimiser count move as dust_svmpc_batch_optimize moves them.  The
 * controller batch is left, bit for bit, where dust_svmpc_batch_optimize fed params_out would leave it; the filters where
 * dust_mpf_batch_optimize leaves them.  Refusals, staging order, the filter side's launch count and the commit of the filters' host rows
 * are the dual tick's. */
int dust_svmpc_dual_batch_optimize(dust_svmpc_batch *batch, dust_mpf_batch *mpf, const float *states, const float *actions_prev, int n_steps,
                                   const void *eps, int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds,
                                   const unsigned char *active, float *params_out, float *bw_used);
/* dust_svmpc_dual_batch_simulate = dust_svmpc_dual_batch_episode under the reference's episode rules (dust_episode_rules, as
 * dust_svmpc_batch_simulate reads them): the loop of run_pendulum_simulation(mpf=...) (simulations.py:104-138) with its warm-up and its
 * cost, and the Particle loop's crash and goal, for B environments in one call.  Period t of the call is period g = t0 + t of the
 * episode.  For an environment that is still running:
 *   filter    when the period has an action (t >= 1, or actions_prev), Silverman's rule (mpf_bw <= 0) and the filters' update, reading
 *             the per-environment rows in device memory - ALSO while the episode warms up;
 *   period    ONE launch of svmpc_dual_sim_period_kernel (Pendulum, Particle; counted under DUST_K_SVMPC_BATCH): the PRIOR tick under
 *             the key row prior_seeds + t B, with forward() only when g >= warm_up - below, the plant gets the zero action, no pw_out
 *             row is written and the particles do not roll;
 *   cost      the plant steps under the true row; the family's instantaneous cost of the new state goes to costs_out[t][b] and is added
 *             in fp32 to loss[b];
 *   stops     crash (status 2, loss = +inf; wins) and goal (status 1), the predicates of dust_svmpc_batch_simulate;
 *   next      the filter's row is conditioned for period t + 1 unless this is the call's last period or the environment has just
 *             stopped: a stop leaves (a_{n-1}, x_n) pending, exactly as the last period of a call does.
 * A stopping environment clears its byte of a device-resident run mask (staged once as active[b] && status[b] == 0) with the launch's
 * last store; every later launch of the call takes that mask, so a stopped environment takes no further filter update and no tick.  The
 * host queues T period launches whatever stops and waits once.
 * THE CONTRACT: afterwards environment b is, on both sides, where n_run[b] per-period calls would have left it -
 * dust_svmpc_dual_batch_optimize while warming up and dust_svmpc_dual_batch_tick afterwards, with the environment inactive from its
 * stop on: getters, counters and noise streams; the filters' particles, prior bandwidths, optimiser slots and step counts; the filters'
 * host rows (observation, past observation, past action, step count), committed per environment from n_run[b] and not from T.
 * Rows t >= n_run[b] of states_out / actions_out / pw_out / bw_out / costs_out are NOT written, nor anything of an inactive environment;
 * bw_out[t][b] is 0 where no update ran; a_seq receives an environment's row only when one of its periods ran forward().  An environment
 * entering with status != 0 does nothing: only n_run[b] = 0 is written.  With warm_up = 0, no goal and no crash rule the call computes,
 * bit for bit, what dust_svmpc_dual_batch_episode computes.  The filters' particles are recorded per period only while
 * dust_svmpc_batch_set_history(DUST_HIST_FILTER) is on; otherwise read them after the call.
 * Refused before anything is staged or launched, both batches and the in-out arrays unchanged.  DUST_ERR_INVALID: what
 * dust_svmpc_dual_batch_episode refuses; NULL rules, loss, status, n_run or costs_out; t0 < 0 or warm_up < 0; a goal or radius that is
 * not finite; an entry status outside 0 .. 2.  DUST_ERR_UNSUPPORTED: stop_on_crash without a Particle with_obstacle map; a skid-steer or
 * cart-pole pair; per-environment hyper rows; any flag. */
int dust_svmpc_dual_batch_simulate(dust_svmpc_batch *batch, dust_mpf_batch *mpf, const float *states, const float *actions_prev,
                                   int n_periods, int n_steps, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds /* [T][B] */,
                                   const float *plant_params, const dust_episode_rules *rules, int flags, const unsigned char *active,
                                   float *states_out, float *actions_out, float *pw_out, float *bw_out, float *costs_out /* [T][B] */,
                                   float *loss /* [B] in-out */, int *status /* [B] in-out */, int *n_run /* [B] out */, float *a_seq);

/* ---- AMPPI episodes under the reference's episode rules (ABI 3, additive) ----
 * dust_amppi_batch_simulate = dust_amppi_batch_episode under dust_episode_rules: the use_svmpc=False branch of run_particle_episode
 * (simulations.py:217-260; particle_example.py:191-242) and the AMPPI loop of run_pendulum_simulation (simulations.py:124-160) for B
 * environments in one call - what the per-period host loop (dust_amppi_batch_update, read back, a host plant, host cost and predicates,
 * dust_amppi_batch_roll) does, without the host between two periods.  This branch of the reference has no warm-up: warm_up must be 0.
 * Period t is ONE launch of amppi_sim_period_kernel / amppi_skid_nav_sim_period_kernel (amppi_episode.hpp, counted under DUST_K_AMPPI):
 * the period of dust_amppi_batch_episode, and in the reducer workgroup of a running environment
 *   cost     the family's own instantaneous cost (dust_svmpc_batch_simulate's) of the state AFTER the step, with a zero action:
 *            inst_costs_out[t][b], and loss[b] += cost as an fp32 running sum in period order;
 *   crash    stop_on_crash: the new position lies on an occupied cell of Particle's map or of the navigation cost's -> loss[b] = +inf,
 *            status[b] = 2, stop;
 *   goal     goal_radius > 0: the fp32 predicate of dust_svmpc_batch_simulate -> status[b] = 1, stop.  The crash rule wins.
 * A stopping environment still rolls; it then clears its byte of a device-resident run mask (staged once as active[b] && status[b] == 0),
 * which every later launch of the call takes.  The host queues T launches whatever stops and waits once.
 * THE CONTRACT: afterwards environment b is where n_run[b] x (dust_amppi_batch_update on the recorded states, dust_amppi_batch_roll)
 * would have left it, bit for bit, with the environment inactive from its stop on: sequences, stream positions, and the last period's
 * actions through dust_amppi_batch_get_actions for every environment that ran a period.  Rows t >= n_run[b] of every record are NOT
 * written, nor anything of an inactive environment; a_seq [B][H][da] (may be NULL) receives the sequence of the environment's LAST period,
 * before its roll.  An environment entering with status != 0 does nothing: only n_run[b] = 0 is written.  loss / status are read at entry
 * and rules->t0 is accepted, so calls chain (a mid-episode change of the true parameters is two chained calls).  With no goal and no crash
 * rule the call computes, bit for bit, what dust_amppi_batch_episode computes.
 * Refused before anything is staged or launched, the batch and the in-out arrays unchanged.  DUST_ERR_INVALID: what
 * dust_amppi_batch_episode refuses; NULL rules, loss, status, n_run or inst_costs_out; warm_up != 0; t0 < 0; a goal or radius that is not
 * finite; an entry status outside 0 .. 2.  DUST_ERR_UNSUPPORTED: stop_on_crash without an occupancy map (Particle's with_obstacle map, or
 * the navigation cost's); every flag but DUST_AMPPI_PARAMS_SHARED.  The staging and record caps are dust_amppi_batch_episode's. */
int dust_amppi_batch_simulate(dust_amppi_batch *batch, const float *states, int n_periods, const float *params, int flags, int roll_steps,
                              const float *plant_params, const dust_episode_rules *rules, const unsigned char *active, float *states_out,
                              float *actions_out, float *costs_out, float *omega_out, float *inst_costs_out /* [T][B] */,
                              float *loss /* [B] in-out */, int *status /* [B] in-out */, int *n_run /* [B] out */, float *a_seq);
/* dust_amppi_dual_batch_simulate = dust_amppi_dual_batch_episode under the same rules: the AMPPI loop of
 * run_pendulum_simulation(mpf=...) (simulations.py:124-160) with its cost, and the Particle loop's crash and goal (217-260).  The run mask
 * is taken by every launch of the call - Silverman's rule, the filters' update, the parameter staging of the single / sigma modes, the
 * period kernels amppi_sim_period_kernel / amppi_prior_sim_period_kernel -, so a stopped environment takes no further update and no tick,
 * and the filter-side launch count depends neither on B nor on the stops.  A stopping environment does not condition its filter row:
 * (a_{n-1}, x_n) stays pending, exactly as behind a call's last period.
 * THE CONTRACT: afterwards environment b is, on both sides, where n_run[b] dust_amppi_dual_batch_tick calls would have left it, with the
 * environment inactive from its stop on: what dust_amppi_batch_simulate lists, and the filters' particles, prior bandwidths, optimiser
 * slots, step counts, dust_mpf_batch_stats and host rows (committed per environment from n_run[b]).  bw_out[t][b] is 0 where no update
 * ran.  Everything else - records, chaining, rules off - as dust_amppi_batch_simulate, against dust_amppi_dual_batch_episode.
 * Refused as there, and what dust_amppi_dual_batch_episode refuses.  DUST_ERR_UNSUPPORTED: stop_on_crash without a Particle with_obstacle
 * map; a skid-steer or cart-pole pair; every flag but DUST_AMPPI_PARAMS_SHARED. */
int dust_amppi_dual_batch_simulate(dust_amppi_batch *batch, dust_mpf_batch *mpf, const float *states, const float *actions_prev, int n_periods,
                                   int flags, int mpf_steps, float mpf_bw, const uint64_t *prior_seeds /* [T][B] */, int roll_steps,
                                   const float *plant_params, const dust_episode_rules *rules, const unsigned char *active, float *states_out,
                                   float *actions_out, float *costs_out, float *omega_out, float *bw_out, float *inst_costs_out /* [T][B] */,
                                   float *loss /* [B] in-out */, int *status /* [B] in-out */, int *n_run /* [B] out */, float *a_seq);

#ifdef __cplusplus
}
#endif
#endif
