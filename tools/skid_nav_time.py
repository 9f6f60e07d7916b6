"""First-pass time of the skid-steer rollout kernels with and without the navigation cost's obstacle term, per library build:
    python tools/skid_nav_time.py libA.so [libB.so ...]
Each build runs in its own process, three alternating rounds; N = 1024, S = 128, H = 30, M = 5 (P = 2), device-drawn noise; microseconds per
launch of the first pass (profile kind `states_kernel`) over blocks of 60 launches: plain, the map staged into LDS (80 x 80 cells), the map
read from device memory (DUST_NAV_GRID_HBM=1), and the sigma-point instances.  A build without dust_set_obstacle_cost reports the plain
kernels only."""
import os, subprocess, sys
code = r'''
import os, sys
sys.path.insert(0, os.environ["DUST_REPO_ROOT"])
import numpy as np
from dust_amd import Context, _lib
N, S, H, M = 1024, 128, 30, 5
rng = np.random.default_rng(0)
th = (1.5 + 0.5 * rng.standard_normal((N, H, 2))).astype(np.float32)
params = rng.uniform((0.1, 0.05), (0.3, 0.08), (M, 2)).astype(np.float32)
state = np.array([0.33, -0.24, 0.4, 0.1, -0.05], np.float32)
grid = np.kron((rng.random((27, 27)) < 0.4).astype(np.float32), np.ones((3, 3), np.float32))[:80, :80]
have = b"dust_set_obstacle_cost" in open(_lib.LIB_PATH, "rb").read()  # (its name in the symbol table: nothing is loaded for the question)
if not have:  # an earlier build: the binding must not ask it for the entry point
    _lib.SYMBOLS.pop("dust_set_obstacle_cost")
def run(w_obs, ut):
    kw = dict(grid=grid, w_obs=w_obs, cell_size=0.05) if w_obs else {}
    c = Context(model="skid_steer", N=N, S=S, M=M, H=H, dt=0.1, sigma_a=1.0, sigma_p=1.0, temperature=20.0, alpha=0.05, uncertain_params=("x_icr", "wheel_radius"),
                min_a=-3.0, max_a=3.0, goal=(1.2, 0.6, 0.3, 0, 0), w_quad_state=(2, 2, 0.5, 0.1, 0.05), w_quad_term=(20, 20, 2, 0, 0), seed=3, **kw)
    if ut:
        c.set_param_weights(np.array([0.0, 0.25, 0.25, 0.25, 0.25], np.float32))
    c.set_theta(th); c.set_a_mat(th)
    for _ in range(10):
        c.likelihood_sample(state, None, params)
    best = []
    for blk in range(5):
        c.sync(); c.profile(True)
        for _ in range(60):
            c.likelihood_sample(state, None, params)
        c.sync()
        ms, n = c.profile_get()["states_kernel"]
        best.append(1e3 * ms / n)
        c.profile(False)
    c.close()
    return "%.1f-%.1f" % (min(best), max(best))
out = ["plain " + run(0.0, False), "plain-ut " + run(0.0, True)]
if have:
    out += ["nav-lds " + run(10.0, False), "nav-lds-ut " + run(10.0, True)]
    os.environ["DUST_NAV_GRID_HBM"] = "1"
    out += ["nav-mem " + run(10.0, False)]
print("  ".join(out))
'''
libs = sys.argv[1:]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for rnd in range(int(os.environ.get("AB_ROUNDS", "3"))):
    for lib in libs:
        env = dict(os.environ, DUST_AMD_LIB=os.path.abspath(lib), DUST_REPO_ROOT=root)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
        print("round %d  %-28s %s" % (rnd, os.path.basename(os.path.dirname(lib)) + "/" + os.path.basename(lib),
                                      out.stdout.strip().split("\n")[-1] if out.returncode == 0 else "ERR " + out.stderr[-400:]), flush=True)
        if out.returncode != 0:  # nothing more is started on a device after a failed run
            sys.exit(1)
