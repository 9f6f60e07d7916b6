"""The cases of tests/test_gpu_svmpc_sweep.py and tests/test_svmpc_sweep_cpu.py: per-environment hyper-parameters in the batched SVMPC tick
and its episodes (dust_svmpc_batch_set_hyper, csrc/svmpc_batch.hpp svmpc_sweep_kernel, csrc/svmpc_episode.hpp svmpc_sweep_episode_kernel).

The shapes are the smallest that reach every branch of a row's use: four model families, SGD and Adam (the one place lr is read), K1 and
IMQ, one and two action channels (a row's two sigmas), n_steps 1 and 3, the one- and the two-softmax path side by side in one launch
(alpha * temperature == 1 or not), weighted and unweighted priors side by side, N = S = M = H = 1, and the LDS corner of the box
(N 64, D 128).  Every comparison of the tests is np.array_equal: the feature adds no arithmetic, so there is no tolerance to derive.
No device is needed to import this module or to build its rows."""
import numpy as np

F32 = lambda v: float(np.float32(v))  # a Context carries a plain optimiser's lr and every sigma in fp32: the rows hold those values

# id, family, N, S, M, H, the Context's options, n_steps of the three ticks, B
CASES = [
    dict(id="pend", family="pendulum", N=3, S=32, M=2, H=8, opts=dict(optimizer="SGD", kernel="K1"), iters=(1, 3, 1), B=5),
    dict(id="part", family="particle", N=4, S=16, M=1, H=6, opts=dict(optimizer="Adam", kernel="IMQ", roll_strategy="mean"), iters=(2, 1, 2), B=5,
         lr=1.0),  # (Adam steps by lr whatever the gradient's size)
    dict(id="skid", family="skid_steer", N=2, S=8, M=2, H=5, opts=dict(optimizer="SGD", kernel="K1"), iters=(2, 1, 2), B=5),
    dict(id="cart", family="cartpole", N=2, S=8, M=1, H=5, opts=dict(optimizer="Adam", kernel="K1"), iters=(2, 1, 2), B=5),
    dict(id="ones", family="pendulum", N=1, S=1, M=1, H=1, opts=dict(optimizer="SGD", kernel="K1"), iters=(1, 2, 1), B=2),
    dict(id="corner", family="particle", N=64, S=4, M=1, H=64, opts=dict(optimizer="SGD", kernel="K1"), iters=(1, 2, 1), B=5),
]
IDS = [c["id"] for c in CASES]
BY_ID = {c["id"]: c for c in CASES}
EPISODE_IDS = ["pend", "part", "ones"]
T_EPISODE = 4

FAMILY = {
    "pendulum": dict(da=1, ds=2, lr=2.0, sigma_a=(2.0,), sigma_p=(2.0,), scale=1.0, state=(3.0, 0.0)),
    # two channels with different sigmas inside a row
    "particle": dict(da=2, ds=4, lr=100.0, sigma_a=(5.0, 3.0), sigma_p=(4.0, 6.0), scale=1.0, state=(-9.0, -9.0, 0.0, 0.0)),
    "skid_steer": dict(da=2, ds=5, lr=0.05, sigma_a=(0.3, 0.25), sigma_p=(0.3, 0.4), scale=0.3, state=None),
    "cartpole": dict(da=1, ds=4, lr=0.05, sigma_a=(0.6,), sigma_p=(0.6,), scale=0.5, state=None),
}
FIELDS = ("lr", "alpha", "temperature", "sigma_a", "chol_a", "sigma_p", "weighted_prior")


def family(case):
    return FAMILY[case["family"]]


def n_params(case):
    """P: the columns of a dynamics sample / a true row (0: no uncertain parameters)"""
    if case["family"] == "pendulum":
        return 2 if case["M"] > 1 or case["id"] == "pend" else (1 if case["id"] == "ones" else 0)
    return {"particle": 0, "skid_steer": 2, "cartpole": 4}[case["family"]]


def base_row(case):
    """the prototype's own values: alpha = temperature = 1"""
    f = family(case)
    sa, sp = np.array(f["sigma_a"], np.float32), np.array(f["sigma_p"], np.float32)
    return dict(lr=F32(case.get("lr", f["lr"])), alpha=np.float32(1.0), temperature=np.float32(1.0), sigma_a=sa, chol_a=sa.copy(), sigma_p=sp, weighted_prior=0)


def _mod(row, **kw):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in row.items()}
    out.update(kw)
    return out


def env_rows(case):
    """the five rows of the table (environment b -> a dict of one row's fields); `ones` (B = 2) takes the last two"""
    r = base_row(case)
    sa15 = (r["sigma_a"] * np.float32(1.5)).astype(np.float32)
    rows = [
        _mod(r),                                                            # 0: the prototype's own values
        _mod(r, lr=r["lr"] * 4.0),                                          # 1: lr x 4
        _mod(r, alpha=np.float32(0.5), temperature=np.float32(2.0)),        # 2: the product is 1: the one-softmax path
        _mod(r, alpha=np.float32(2.0), temperature=np.float32(1.5)),        # 3: the two-softmax path beside it
        _mod(r, sigma_a=sa15, chol_a=sa15.copy(), sigma_p=(r["sigma_p"] * np.float32(0.5)).astype(np.float32), weighted_prior=1),  # 4
    ]
    return rows[-case["B"]:]


def stack(rows):
    """a list of rows -> the dict of arrays `SvmpcBatch.set_hyper` takes"""
    out = {}
    for k in FIELDS:
        v = np.stack([np.asarray(r[k]) for r in rows])
        out[k] = v.astype(np.float64 if k == "lr" else (np.int64 if k == "weighted_prior" else np.float32))
    return out


def row_equal(x, y):
    return all(np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for k in FIELDS)


# one field of a row changed (environment 2 of the power test), and the getter where the change must show
VARIANTS = {
    "lr": (lambda r: _mod(r, lr=r["lr"] * 0.5), ("THETA",)),
    "alpha": (lambda r: _mod(r, alpha=np.float32(r["alpha"] * np.float32(3.0))), ("LOG_L", "SCORE")),
    "temperature": (lambda r: _mod(r, temperature=np.float32(r["temperature"] * np.float32(3.0))), ("A_MAT", "A_MIX")),
    "sigma_a": (lambda r: _mod(r, sigma_a=(r["sigma_a"] * np.float32(1.25)).astype(np.float32),
                               chol_a=(r["chol_a"] * np.float32(1.25)).astype(np.float32)), ("COSTS",)),
    "sigma_p": (lambda r: _mod(r, sigma_p=(r["sigma_p"] * np.float32(0.75)).astype(np.float32)), ("LOG_P",)),
    "weighted_prior": (lambda r: _mod(r, weighted_prior=1 - r["weighted_prior"]), ("PRIOR_MIX",)),
}


def context_kwargs(case, row=None):
    """Context keywords of the case's prototype built with `row`'s values (None: the base row); Particle's `grid` is the caller's"""
    r = base_row(case) if row is None else row
    hyper = dict(lr=float(r["lr"]), alpha=float(r["alpha"]), temperature=float(r["temperature"]), sigma_a=np.asarray(r["sigma_a"], np.float32),
                 chol_a=np.asarray(r["chol_a"], np.float32), sigma_p=np.asarray(r["sigma_p"], np.float32), weighted_prior=bool(r["weighted_prior"]))
    kw = dict(case["opts"], seed=77, **hyper)
    N, S, M, H = case["N"], case["S"], case["M"], case["H"]
    if case["family"] == "pendulum":
        kw.update(model="pendulum", N=N, S=S, M=M, H=H)
        P = n_params(case)
        if P:
            kw["uncertain_params"] = ("length", "mass")[:P]
        return kw
    if case["family"] == "particle":
        kw.update(model="particle", N=N, S=S, M=M, H=H)
        return kw
    if case["family"] == "skid_steer":
        import skid_cases as sc

        return sc.controller_kwargs(sc.R("sweep", N, S, H, M, ("x_icr", "wheel_radius"), "uniform", None, 0, **sc.XW), **kw)
    import cartpole_cases as cc

    return cc.controller_kwargs(dict(cc.ROLLOUT_BY_TAG["params_log"], N=N, S=S, H=H, M=M), **kw)


def start_state(case):
    f = family(case)
    if f["state"] is not None:
        return np.array(f["state"], np.float32)
    if case["family"] == "skid_steer":
        import skid_cases as sc

        return np.asarray(sc.STATE0, np.float32)
    import cartpole_cases as cc

    return np.asarray(cc.STATE0, np.float32)


def draw_params(case, rng, shape):
    """dynamics samples / true rows of `shape` + (P,), or None without uncertain parameters"""
    P = n_params(case)
    if P == 0:
        return None
    if case["family"] == "pendulum":
        return (1.0 + 0.1 * rng.standard_normal(shape + (P,))).astype(np.float32)
    if case["family"] == "skid_steer":
        import skid_cases as sc

        return rng.uniform(np.asarray(sc.XW["lo"]), np.asarray(sc.XW["hi"]), shape + (P,)).astype(np.float32)
    import cartpole_cases as cc

    s = cc.ROLLOUT_BY_TAG["params_log"]
    return (np.asarray(s["loc"]) + np.asarray(s["scale"]) * rng.standard_normal(shape + (P,))).astype(np.float32)


def env_inputs(case, n_env=None, ticks=3, seed=11):
    """every environment's own particles, prior means, a_mat, start state, Philox key, recorded noise and dynamics samples per tick; the
    episodes' true rows"""
    f = family(case)
    B = case["B"] if n_env is None else n_env
    N, S, M, H, da = case["N"], case["S"], case["M"], case["H"], f["da"]
    rng = np.random.default_rng(seed)
    mu = (f["scale"] * rng.standard_normal((B, N, H, da))).astype(np.float32)
    th = (mu + 2 * f["scale"] * rng.standard_normal((B, N, H, da))).astype(np.float32)
    am = (f["scale"] * rng.standard_normal((B, N, H, da))).astype(np.float32)
    st = np.tile(start_state(case), (B, 1))
    st = (st + 0.05 * rng.standard_normal(st.shape)).astype(np.float32)
    eps = [rng.standard_normal((B, n, S, N, H, da)).astype(np.float32) for n in case["iters"][:ticks]]
    params = [draw_params(case, rng, (B, n, M)) for n in case["iters"][:ticks]]
    return dict(mu=mu, th=th, am=am, st=st, eps=eps, params=params, seeds=[1000 + 13 * b for b in range(B)], plant=draw_params(case, rng, (B,)),
                ep_params=draw_params(case, rng, (T_EPISODE + 1, B, case["iters"][0], M)))
