"""Inputs shared by tests/test_complete_cpu.py and tests/test_gpu_complete.py: the CPU test checks that the reference alone meets
the conditions the GPU tests impose on these very inputs (objective decrease on every row, the trajectory's rounding spread)."""
import numpy as np

from conftest import make_arch, synth_batch
from oracle import vae_assoc_oracle as O

TWO = dict(archs=[make_arch("image", 784, 64, 48, 20), make_arch("joint", 147, 40, 32, 20)], binary=[True, False],
           weights=[50.0, 1.0], lam=8.0, B=32)
THREE = dict(archs=[make_arch("a", 60, 32, 24, 8), make_arch("b", 21, 16, 16, 8), make_arch("c", 33, 24, 16, 8)],
             binary=[True, False, False], weights=[2.0, 1.0, 0.5], lam=0.7, B=64)
NETS = {"two": TWO, "three": THREE}

T_TRAJ, LR, PRIOR = 20, 0.05, 1.0
# Trajectory test (net "two", softplus, pattern "random", T_TRAJ iterations, fp32 kernels against the fp64 reference): the largest
# deviation between the reference run in fp64 and the same reference run with float32 arithmetic on these inputs, measured on the
# CPU (test_complete_cpu.py re-measures and prints them): z relative to max |z|, objective relative per entry.  The GPU may
# deviate 4 times as much (a different summation order).
TRAJ_DEV_Z, TRAJ_DEV_OBJ = 8.1e-7, 2.9e-7
TRAJ_BOUND_Z, TRAJ_BOUND_OBJ = 4 * TRAJ_DEV_Z, 4 * TRAJ_DEV_OBJ


def params0(net, seed=3):
    """xavier weights, non-zero biases (float32, flat)"""
    rng = np.random.default_rng(seed)
    flat = O.flatten_params(net["archs"], O.init_params(net["archs"], rng)).astype(np.float32)
    off = 0
    for na in net["archs"]:
        for _, shp in O.layer_shapes(na):
            n = int(np.prod(shp))
            if len(shp) == 1:
                flat[off:off + n] = 0.05 * rng.standard_normal(n)
            off += n
    return flat


def inputs(net, rows, pattern, seed=5):
    """-> (X, observed, z0) for ``rows`` rows.  Patterns: "random" = a random element mask on every modality (row 0 of modality 0
    with nothing observed, row 1 with everything); "none_last" = the last modality None, the others randomly masked; "full_last" =
    the last modality fully observed (observed[m] = None), modality 0 with its second half missing; "all" = everything observed
    (observed = None)."""
    rng = np.random.default_rng(seed)
    M = len(net["archs"])
    widths = [na["n_input"] for na in net["archs"]]
    X = synth_batch(rng, rows, widths, net["binary"])
    obs = [rng.random((rows, w)) < 0.6 for w in widths]
    z0 = (0.5 * rng.standard_normal((rows, net["archs"][0]["n_z"]))).astype(np.float32)
    if pattern == "random":
        obs[0][:1] = False
        if rows > 1:
            obs[0][1] = True
    elif pattern == "none_last":
        X[M - 1] = None
        obs[M - 1] = None
    elif pattern == "full_last":
        obs[M - 1] = None
        obs[0][:] = True
        obs[0][:, widths[0] // 2:] = False
    elif pattern == "all":
        obs = None
    else:
        raise ValueError(pattern)
    return X, obs, z0
