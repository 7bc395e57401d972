"""CPU checks of tests/infer_big_cases.py, the inputs and references of tests/test_gpu_infer_big.py and
tests/test_gpu_complete_big.py: every input is seeded (built twice, equal bits), every reference is finite, and the trajectory
bound of the five-iteration complete() case is re-measured here on those very inputs.  The GPU tests exclude nothing from their
comparisons, so there is no exclusion for the reference to stay within."""
import numpy as np
import pytest

import infer_big_cases as cases


def _finite(tree):
    if isinstance(tree, dict):
        return all(_finite(v) for v in tree.values())
    if isinstance(tree, (list, tuple)):
        return all(_finite(v) for v in tree)
    return tree is None or bool(np.all(np.isfinite(np.asarray(tree, np.float64))))


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b))


def test_inputs_are_seeded():
    makers = [cases.params_a, cases.data_a, cases.params0_a, lambda: cases.small_case.__wrapped__("nz64", "fp32")[2:],
              lambda: cases.complete_inputs.__wrapped__("random", 70), lambda: cases.complete_inputs.__wrapped__("none_last", 70),
              lambda: cases.noise(73, 5, 7)]          # every z and eps is cases.noise(seed, shape)
    for make in makers:
        make = getattr(make, "__wrapped__", make)
        assert _same(make(), make())
    z = cases.gen_a("fp32")[0]
    assert z.shape == (cases.ROWS_A, cases.NZ_A) and cases.ROWS_A == 3999 + 159 and z is cases.gen_a("fp32")[0]


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_set_a_references_are_finite(dtype):
    assert _finite(cases.gen_a(dtype)) and _finite(cases.recon_a(dtype)) and _finite(cases.score_a(dtype))
    assert _finite(cases.loglik_a(dtype)) and _finite(cases.train_a(dtype))
    X, p, eps, want, dev, lat = cases.impute_a(dtype)
    assert _finite(want["mu"]) and _finite(want["logvar"]) and _finite(want["mean"]) and _finite(want["var"])
    # the yardstick of impute's mean and variance is the float32 definition's own deviation: it must not be zero
    assert all(dm > 0 and dv > 0 for dm, dv in dev), dev
    assert len({tuple(r) for r in p.tolist()}) == 4 and want["mean"][0].shape == (cases.N_LL, 784)
    assert [o.shape for o in cases.gen_a(dtype)[1]] == [(cases.ROWS_A, 784), (cases.ROWS_A, 147)]
    assert cases.score_a(dtype)["cross"].shape == (cases.ROWS_A, 2, 2)
    # the sample passes of log_likelihood and impute on a 3999-row handle: 1333 rows x 3 = a full bucket, then 67 x 3 = 201
    n = cases.B_A // cases.K_LL
    assert n * cases.K_LL == cases.B_A and (cases.N_LL - n) * cases.K_LL == 201


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_small_references_are_finite(dtype):
    for key in list(cases.S_FIRST) + ["nz64", "c2"]:
        archs, B, params, z, want = cases.small_case(key, dtype)
        assert _finite(want) and want[0].shape == (len(z), 784) and want[1].shape == (len(z), 147), key


@pytest.mark.parametrize("pattern", cases.PATTERNS)
def test_complete_references_are_finite(pattern):
    for dtype in cases.DTYPES:
        r = cases.complete_ref_smooth(pattern, dtype)
        assert _finite(r) and r["objective"].shape == (1, cases.ROWS_A) and np.abs(r["grad0"]).max() > 0
    X, obs, z0 = cases.complete_inputs(pattern, cases.ROWS_A)
    assert (X[1] is None) == (pattern == "none_last") and z0.shape == (cases.ROWS_A, cases.NZ_A)
    assert obs[0][0].any() == (pattern != "random")           # "random": row 0 of modality 0 has nothing observed


def test_trajectory_rounding_spread_of_the_gpu_tests_inputs():
    """fp64 reference against the same reference in float32 arithmetic on the trajectory test's inputs: the measured spread is what
    infer_big_cases.TRAJ_DEV_* record (the GPU test allows 4 times as much), and the bound is not zero."""
    r64, dz, dj = cases.trajectory()
    print("trajectory spread fp32 vs fp64: z %.3e of max|z|, objective %.3e relative" % (dz, dj))
    assert _finite(r64) and r64["objective"].shape == (cases.T_TRAJ + 1, cases.B_A)
    assert cases.TRAJ_BOUND_Z > 0 and cases.TRAJ_BOUND_OBJ > 0
    assert cases.TRAJ_DEV_Z / 4 <= dz <= 2 * cases.TRAJ_DEV_Z, dz
    assert cases.TRAJ_DEV_OBJ / 4 <= dj <= 2 * cases.TRAJ_DEV_OBJ, dj


def test_bf16_x_spread_of_the_gpu_tests_inputs():
    """complete()'s x in bf16: the quant='bf16' reference with float32 sums against itself with fp64 sums, on the GPU test's z0 --
    what infer_big_cases.X_DEV_BF16 records (the GPU test allows 4 times as much)."""
    dev = cases.x_spread_bf16()
    print("bf16 x spread, float32 sums vs fp64 sums: %s" % ["%.3e" % d for d in dev])
    assert cases.X_BOUND_BF16 > 0 and cases.X_DEV_BF16 / 4 <= max(dev) <= 2 * cases.X_DEV_BF16, dev
    z0 = [cases.complete_inputs(p, cases.ROWS_A)[2] for p in cases.PATTERNS]
    assert np.array_equal(z0[0], z0[1])
