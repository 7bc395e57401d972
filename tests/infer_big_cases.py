"""The inputs and references of tests/test_gpu_infer_big.py and tests/test_gpu_complete_big.py, in one place:
tests/test_infer_big_cpu.py checks without a device that every input is seeded, every reference finite and the measured
trajectory bound non-zero.

Set A is tests/test_gpu_big_ragged.py's: batch 3999, n_z = 40, hidden [1003, 605] / [1003, 640] on 784 (Bernoulli) / 147 (Gaussian)
inputs -- the smallest shape whose single-item launches reach the 128x128 tiles.  Set S (serving) puts the decoders' first layer on
both sides of k_serve_in's bounds, NET_NZ64 has n_z + 1 = 65 > 64, and C2_BIG is the benchmark's C2 at batch_size 1024.

Every reference is computed once per process (functools.lru_cache) and handed out as it is: callers do not modify it."""
import functools

import numpy as np

import complete_cases
import complete_reference as CR
import impute_reference as IR
from conftest import make_arch, synth_batch
from oracle import vae_assoc_oracle as O
from scoring_reference import ref_loglik, ref_scores
from test_gpu_big_ragged import B_A, BIN, NZ_A, SET_A
from test_gpu_scoring_edges import ACT, c2, host_params

DTYPES = ("fp32", "bf16")
W_A, LAM_A = [5.0, 1.0], 0.5
NET_A = dict(archs=SET_A, binary=BIN, weights=W_A, lam=LAM_A, B=B_A)       # complete_cases' form
TAIL_A = 159
ROWS_A = B_A + TAIL_A                    # a full chunk and a 159-row one inside the 3999-row plan
GEN_ROWS = (ROWS_A, B_A, 65, 64)         # 65 rows: still the 3999-row plan; 64: the 64-row bucket, 16-slice k_serve_in
N_LL, K_LL = 1400, 3                     # log_likelihood / impute: passes of 1333 x 3 = 3999 and 67 x 3 = 201 decoded rows

# Set S: batch_size 96 (buckets 64 and 96), n_z = 20; (first decoder layer of modality 0, of modality 1) -> fused staging launch?
NZ_S, B_S = 20, 96
S_ROWS = (1, 64, 65, 96, 200)
S_FIRST = {(1024, 40): True, (1003, 130): True, (1025, 64): False}


def set_s(first):
    return [make_arch("a", 784, 0, 0, NZ_S, n_hidden=[first[0], 48]), make_arch("b", 147, 0, 0, NZ_S, n_hidden=[first[1], 40])]


NET_NZ64 = [make_arch("a", 784, 0, 0, 64, n_hidden=[96, 80]), make_arch("b", 147, 0, 0, 64, n_hidden=[40, 24])]
C2_BIG_B = 1024
C2_BIG = c2()[0]


def noise(seed, *shape):
    """seeded standard-normal float32 rows: every z and eps below"""
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def quant_of(dtype):
    return None if dtype == "fp32" else "bf16"


@functools.lru_cache(maxsize=None)
def params_a():
    """Set A's parameters as per-modality dicts (test_gpu_scoring_edges.host_params: fp32-exact, non-zero biases)"""
    return host_params(SET_A, 71)


def oracle(archs, params, dtype, B, weights=None, lam=0.5):
    """fp64 oracle for fp32 compute (relu), quant='bf16' oracle for bf16 compute (softplus): the scoring files' pairing"""
    return O.OracleAssocVAE(archs, BIN, ACT[dtype], weights or W_A, lam, 1e-3, B, params_flat=O.flatten_params(archs, params),
                            quant=quant_of(dtype))


@functools.lru_cache(maxsize=None)
def oracle_a(dtype):
    return oracle(SET_A, params_a(), dtype, B_A)


@functools.lru_cache(maxsize=None)
def data_a():
    """-> (X [ROWS_A rows per modality], eps [ROWS_A, n_z], per-modality eps of reconstruct)"""
    rng = np.random.default_rng(72)
    X = synth_batch(rng, ROWS_A, [a["n_input"] for a in SET_A], BIN)
    eps = rng.standard_normal((ROWS_A, NZ_A)).astype(np.float32)
    eps_m = [rng.standard_normal((ROWS_A, NZ_A)).astype(np.float32) for _ in SET_A]
    return X, eps, eps_m


@functools.lru_cache(maxsize=None)
def gen_a(dtype):
    """-> (z [ROWS_A, n_z], decoder outputs per modality); a call of n rows takes the first n of both"""
    z = noise(73, ROWS_A, NZ_A)
    return z, oracle_a(dtype).generate(z)


@functools.lru_cache(maxsize=None)
def recon_a(dtype):
    X, _, eps_m = data_a()
    return oracle_a(dtype).reconstruct(X, eps=eps_m)


@functools.lru_cache(maxsize=None)
def score_a(dtype):
    X, eps, _ = data_a()
    return ref_scores(oracle_a(dtype), X, eps, cross=True)


@functools.lru_cache(maxsize=None)
def loglik_a(dtype):
    """-> (X [N_LL rows], eps [N_LL, K_LL, n_z], reference)"""
    X = [x[:N_LL] for x in data_a()[0]]
    eps = noise(74, N_LL, K_LL, NZ_A)
    return X, eps, ref_loglik(oracle_a(dtype), X, eps)


@functools.lru_cache(maxsize=None)
def impute_a(dtype):
    """-> (X, present, eps, fp64 reference, float32 definition's deviation per modality (mean, var), (mu, logvar) deviations)"""
    X = [x[:N_LL] for x in data_a()[0]]
    p = IR.pattern_rows(N_LL, len(SET_A))
    eps = noise(75, N_LL, K_LL, NZ_A)
    return (X, p, eps) + IR.rounding_spread(oracle_a(dtype), X, p, K_LL, eps)


@functools.lru_cache(maxsize=None)
def train_a(dtype):
    """-> (X [B_A rows], eps, cost of the step's forward pass): the training step that follows the forward-only calls"""
    X, eps, _ = data_a()
    X, eps = [x[:B_A] for x in X], eps[:B_A]
    return X, eps, oracle_a(dtype).evaluate_cost(X, eps)


@functools.lru_cache(maxsize=None)
def small_case(key, dtype):
    """generate on Set S (key = a first-layer pair), the n_z = 64 net ("nz64") or C2 at batch_size 1024 ("c2"):
    -> (archs, B, params, z [max rows, n_z], decoder outputs per modality)"""
    if key == "nz64":
        archs, B, rows = NET_NZ64, B_S, max(S_ROWS)
    elif key == "c2":
        archs, B, rows = C2_BIG, C2_BIG_B, C2_BIG_B + 64
    else:
        archs, B, rows = set_s(key), B_S, max(S_ROWS)
    params = host_params(archs, 76)
    z = noise(77, rows, archs[0]["n_z"])
    return archs, B, params, z, oracle(archs, params, dtype, B).generate(z)


# ----------------------------------------------------------------------------- complete
PATTERNS = ("random", "none_last")
SETTINGS = (("softplus", "fp32"), ("softplus", "bf16"), ("relu", "fp32"))
T_TRAJ = 5
# The five-iteration trajectory (Set A, softplus, pattern "random", B_A rows, fp32 kernels against the fp64 reference): the largest
# deviation of complete_reference run in float32 arithmetic from the same reference in fp64 on these inputs, measured on the CPU
# (test_infer_big_cpu.py re-measures and prints them): z relative to max |z|, objective relative per entry.  The kernels may
# deviate 4 times as much (a different summation order).
TRAJ_DEV_Z, TRAJ_DEV_OBJ = 2.96e-6, 3.3e-7
TRAJ_BOUND_Z, TRAJ_BOUND_OBJ = 4 * TRAJ_DEV_Z, 4 * TRAJ_DEV_OBJ


# x of complete() in bf16 (absolute; tests/test_gpu_complete.py's bound on its 64-unit nets is 2e-3).  At fan-in 1003 / 605 / 640 the
# quant='bf16' reference itself moves by more than that with the precision of its sums: decode32_bf16 (the same roundings to bf16,
# float32 products and sums between them) against the fp64-summing reference on the complete() cases' z0 differs by 5.4e-4 on the 784
# sigmoid outputs and by 2.66e-3 on the 147 linear ones (max |x| 2.58; 373 of 611,226 entries above 1e-3, in 15 rows of 7 different
# 256-row tiles and 135 of the 147 columns; 12 above 2e-3, in rows 805, 1797, 1822 and 3732: a hidden activation whose bf16 rounding
# flips moves every output of its row).  The kernels' fp32 accumulators are
# that float32 restatement, so the bound is the project's rule since R5: 4x the restatement's worst error on the same inputs.
X_DEV_BF16 = 2.66e-3
X_BOUND_BF16 = 4 * X_DEV_BF16


@functools.lru_cache(maxsize=None)
def x_spread_bf16():
    """-> per modality, max |decode32_bf16(z0) - decode(z0, quant='bf16')| on the complete() cases' z0 (the same for every pattern)"""
    z0 = complete_inputs("random", ROWS_A)[2]
    params = O.unflatten_params(SET_A, params0_a().astype(np.float64), np.float64)
    want = complete_ref_smooth("random", "bf16")["x"]
    return [float(np.abs(IR.decode32_bf16(na, p, z0, "softplus", b) - w).max()) for na, p, b, w in zip(SET_A, params, BIN, want)]


@functools.lru_cache(maxsize=None)
def params0_a():
    return complete_cases.params0(NET_A)


@functools.lru_cache(maxsize=None)
def complete_inputs(pattern, rows):
    """complete_cases.inputs on Set A -> (X, observed, z0)"""
    return complete_cases.inputs(NET_A, rows, pattern)


def complete_ref(pattern, rows, act, dtype, n_iters=0, masks0=None, np_dtype=np.float64):
    X, obs, z0 = complete_inputs(pattern, rows)
    return CR.complete(SET_A, params0_a(), X, obs, z0, BIN, W_A, act, n_iters, complete_cases.LR, complete_cases.PRIOR,
                       quant=quant_of(dtype), dtype=np_dtype, masks0=masks0)


@functools.lru_cache(maxsize=None)
def complete_ref_smooth(pattern, dtype):
    """softplus, n_iters = 0, ROWS_A rows (a 3999-row chunk and a 159-row one): no relu decisions to hand over, so it is cached"""
    return complete_ref(pattern, ROWS_A, "softplus", dtype)


@functools.lru_cache(maxsize=None)
def trajectory_ref():
    """the fp64 reference of the five-iteration trajectory"""
    return complete_ref("random", B_A, "softplus", "fp32", T_TRAJ)


@functools.lru_cache(maxsize=None)
def trajectory():
    """-> (fp64 reference, z deviation of the float32 run relative to max |z|, its worst relative objective deviation)"""
    r64 = trajectory_ref()
    r32 = complete_ref("random", B_A, "softplus", "fp32", T_TRAJ, np_dtype=np.float32)
    assert r32["z"].dtype == np.float32 and r32["objective"].dtype == np.float32
    dz = np.abs(r32["z"] - r64["z"]).max() / np.abs(r64["z"]).max()
    dj = (np.abs(r32["objective"] - r64["objective"]) / np.abs(r64["objective"])).max()
    return r64, float(dz), float(dj)
