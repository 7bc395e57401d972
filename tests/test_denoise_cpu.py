"""CPU checks of denoising training (include/avae.h): the reference of tests/denoise_reference.py against
central differences and against the plain oracle, the statistics and the keying of the corruption stream, and the marshalling
of ``inputs`` / ``corruption`` with its error messages."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from conftest import make_arch, synth_batch
from denoise_reference import corrupt, denoise_cost_and_grads, drop_mask, drop_threshold, normals
from oracle import vae_assoc_oracle as O

MLP = dict(archs=[make_arch("image", 40, 14, 10, 4), make_arch("joint", 13, 10, 8, 4)], binary=[True, False],
           weights=[3.0, 1.0], lam=0.8, B=16)
CONV = dict(archs=[dict(make_arch("image", 784, 4, 6, 3), hidden_conv=True, n_hidden_gener_1=6, n_hidden_gener_2=4),
                   make_arch("joint", 13, 10, 8, 3)], binary=[True, False], weights=[3.0, 1.0], lam=0.8, B=4)
CASES = {"softplus": dict(MLP, act="softplus"), "tanh": dict(MLP, act="tanh"), "relu": dict(MLP, act="relu"),
         "conv": dict(CONV, act="softplus")}


def _setup(case, seed):
    """parameters, clean batch, eps and the corrupted inputs: 30 % of the image dropped, sigma = 0.5 on the joint"""
    rng = np.random.default_rng(seed)
    archs = case["archs"]
    flat = O.flatten_params(archs, O.init_params(archs, rng))
    X = [x.astype(np.float64) for x in synth_batch(rng, case["B"], [na["n_input"] for na in archs], case["binary"])]
    eps = rng.standard_normal((case["B"], archs[0]["n_z"]))
    X_in = [corrupt(X[0], 5, 0, 0, drop=0.3)[0], corrupt(X[1], 5, 0, 1, noise=0.5)[0]]
    return rng, flat, X, X_in, eps


def _ref(case, flat, X, X_in, eps, **kw):
    return denoise_cost_and_grads(case["archs"], flat, X, X_in, eps, case["binary"], case["weights"], case["lam"], case["act"], **kw)


def _tensor_diffs(archs, a, b):
    """max |a - b| of every parameter tensor, as a fraction of that tensor's largest |b|"""
    out, off = [], 0
    for na in archs:
        for _, shp in O.layer_shapes(na):
            n = int(np.prod(shp))
            out.append(float(np.abs(a[off:off + n] - b[off:off + n]).max() / np.abs(b[off:off + n]).max()))
            off += n
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_reference_gradient_by_central_differences(name):
    """backward(forward(X_in), X) is the gradient of loss_terms(forward(X_in), X): 60 random parameters, 1e-6 of the gradient's
    largest entry"""
    case = CASES[name]
    rng, flat, X, X_in, eps = _setup(case, 2)
    _, g = _ref(case, flat, X, X_in, eps)
    _, g_plain = _ref(case, flat, X, X, eps)
    assert max(_tensor_diffs(case["archs"], g, g_plain)) > 0.05           # the corrupted step is another step
    h, worst = 1e-6, 0.0
    for i in rng.choice(flat.size, 60, replace=False):
        e = np.zeros_like(flat)
        e[i] = h
        fd = (_ref(case, flat + e, X, X_in, eps)[0] - _ref(case, flat - e, X, X_in, eps)[0]) / (2 * h)
        worst = max(worst, abs(fd - g[i]))
    print("central differences, %s: worst %.3e of the largest entry" % (name, worst / np.abs(g).max()))
    assert worst <= 1e-6 * np.abs(g).max()


@pytest.mark.parametrize("name", ["relu", "conv"])
def test_clean_inputs_give_the_plain_oracle_bitwise(name):
    case = CASES[name]
    _, flat, X, _, eps = _setup(case, 3)
    ref = O.OracleAssocVAE(case["archs"], binary=case["binary"], transfer_fct=case["act"], weights=case["weights"],
                           assoc_lambda=case["lam"], batch_size=case["B"], params_flat=flat)
    for bg in (None, 3 * case["B"]):
        c0, g0, _ = ref.cost_and_grads(X, eps, batch_global=bg)
        c1, g1 = _ref(case, flat, X, X, eps, batch_global=bg)
        assert c1 == float(c0) and np.array_equal(g1, g0)


def test_masked_reference_composes_by_pattern():
    """all present = the unmasked reference (up to the order of the sums); an absent (row, m) reads neither X nor X_in"""
    case = CASES["tanh"]
    rng, flat, X, X_in, eps = _setup(case, 4)
    B = case["B"]
    c0, g0 = _ref(case, flat, X, X_in, eps)
    c1, g1 = _ref(case, flat, X, X_in, eps, present=np.ones((B, 2), bool))
    assert abs(c1 - c0) <= 1e-12 * abs(c0)
    np.testing.assert_allclose(g1, g0, rtol=1e-10, atol=1e-12)
    p = rng.random((B, 2)) < 0.6
    p[0], p[1] = False, True
    c2, g2 = _ref(case, flat, X, X_in, eps, present=p)
    Xn, In = [x.copy() for x in X], [x.copy() for x in X_in]
    for m in range(2):
        Xn[m][~p[:, m]] = np.nan
        In[m][~p[:, m]] = np.nan
    c3, g3 = _ref(case, flat, Xn, In, eps, present=p)
    assert c3 == c2 and np.array_equal(g3, g2) and np.isfinite(c2)


STREAM_SHAPES = [(80, 784, 0, 0.3), (80, 147, 1, 0.1), (20, 147, 1, 0.5)]


@pytest.mark.parametrize("seed", [3, 11, 77])
@pytest.mark.parametrize("step", [0, 1, 20])
@pytest.mark.parametrize("shape", STREAM_SHAPES)
def test_stream_statistics(seed, step, shape):
    """drop fraction, mean and variance of the normals within 4 standard errors (binomial, 1/sqrt(N), sqrt(2/N))"""
    rows, cols, m, p = shape
    N = rows * cols
    d = drop_mask(seed, step, rows, cols, m, p)
    n = normals(seed, step, rows, cols, m)
    assert d.shape == n.shape == (rows, cols)
    dev = (abs(d.mean() - p) / np.sqrt(p * (1 - p) / N), abs(n.mean()) * np.sqrt(N), abs(n.var() - 1.0) / np.sqrt(2.0 / N))
    print("seed %d step %d %s: %.2f / %.2f / %.2f standard errors" % ((seed, step, shape) + dev))
    assert max(dev) <= 4.0


def test_streams_of_modalities_and_steps_are_independent():
    """p = 0.5 masks of two modalities, and of two steps, agree on half of 80 x 147 elements (0.5 +- 0.014 = 3 standard errors)"""
    a = drop_mask(3, 0, 80, 147, 0, 0.5)
    for other in (drop_mask(3, 0, 80, 147, 1, 0.5), drop_mask(3, 1, 80, 147, 0, 0.5)):
        agree = float((a == other).mean())
        print("agreement %.3f" % agree)
        assert abs(agree - 0.5) <= 0.014
    # the two streams of one element are different blocks too
    assert abs(np.corrcoef(normals(3, 0, 80, 147, 0).ravel(), a.ravel())[0, 1]) < 0.04
    # a step counter past 2^32 reaches the fourth counter word
    assert not np.array_equal(drop_mask(3, 1 << 32, 20, 147, 0, 0.5), drop_mask(3, 0, 20, 147, 0, 0.5))


def test_stream_is_keyed_by_the_global_row():
    for m, cols in ((0, 784), (1, 147)):
        assert np.array_equal(drop_mask(11, 2, 40, cols, m, 0.3, row_offset=40), drop_mask(11, 2, 80, cols, m, 0.3)[40:])
        assert np.array_equal(normals(11, 2, 40, cols, m, row_offset=40), normals(11, 2, 80, cols, m)[40:])


def test_corrupt_semantics():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((20, 147))
    x[3, 5] = np.nan
    out, d = corrupt(x, 7, 4, 1, drop=0.5, noise=0.25, drop_value=-1.0)
    assert np.all(out[d] == -1.0)                                                  # a select: NaN under a drop is gone
    keep = ~d & np.isfinite(x)
    np.testing.assert_allclose(out[keep], (x + 0.25 * normals(7, 4, 20, 147, 1))[keep], rtol=0, atol=1e-15)
    assert np.isnan(out[3, 5]) == (not d[3, 5])
    same, none = corrupt(x, 7, 4, 1)
    assert none is None and np.array_equal(same, x, equal_nan=True)
    assert drop_threshold(0.0) == 0 and drop_threshold(0.5) == 1 << 23 and drop_threshold(np.float32(0.3)) == int(np.float32(0.3) * 2.0 ** 24)


# ----------------------------------------------------------------------------- marshalling (no GPU, no library)
def test_inputs_marshal_like_X():
    from vae_assoc_amd._marshal import dev_inputs, dev_modalities
    widths = (784, 147)
    wide, wide_in = torch.rand(12, 931), torch.rand(12, 931)
    X = [wide[:, :784], wide[:, 784:]]
    ts, _, _, _, _ = dev_modalities(X, widths, "cpu", 12, "batch_size")
    its, ptrs, lds = dev_inputs([wide_in[:, :784], wide_in[:, 784:]], ts, widths, "cpu", 12, "batch_size")
    assert [t.data_ptr() for t in its] == [wide_in.data_ptr(), wide_in.data_ptr() + 784 * 4]      # column views: no copy
    assert list(lds) == [931, 931] and [ptrs[0], ptrs[1]] == [t.data_ptr() for t in its]
    its, ptrs, lds = dev_inputs([None, np.zeros((12, 147))], ts, widths, "cpu", 12)
    assert its[0] is None and ptrs[0] is None and list(lds) == [0, 147] and its[1].dtype == torch.float32
    with pytest.raises(ValueError, match="12 rows"):
        dev_inputs([None, np.zeros((11, 147))], ts, widths, "cpu", 12, "batch_size")
    with pytest.raises(ValueError, match=r"\[rows, 147\]"):
        dev_inputs([None, np.zeros((12, 146))], ts, widths, "cpu", 12)
    with pytest.raises(ValueError, match="list of 2"):
        dev_inputs([None], ts, widths, "cpu", 12)
    with pytest.raises(ValueError, match=r"inputs\[1\] is given while X\[1\] is None"):
        dev_inputs([None, np.zeros((12, 147))], [ts[0], None], widths, "cpu", 12)


def test_corruption_fields_and_their_errors():
    from vae_assoc_amd._marshal import corruption_fields
    assert corruption_fields(None, 0.3, 2.0, 3) == ([0.0] * 3, [0.0] * 3, [0.0] * 3)
    p, s, d = corruption_fields(0.25, [0.0, 0.5], -1.0, 2)
    assert p == [0.25, 0.25] and s == [0.0, 0.5] and d == [-1.0, -1.0]
    assert corruption_fields(0.3, 0.0, 0.0, 1)[0] == [float(np.float32(0.3))]                       # what the library is handed
    for kw, needle in ((dict(drop=1.0), "drop_prob"), (dict(drop=-0.1), "drop_prob"), (dict(drop=[0.1, float("nan")]), "drop_prob"),
                       (dict(noise=-1.0), "noise_std"), (dict(noise=float("inf")), "noise_std"),
                       (dict(drop_value=float("nan")), "drop_value"), (dict(drop=[0.1, 0.2, 0.3]), "drop must be")):
        args = dict(drop=0.0, noise=0.0, drop_value=0.0)
        args.update(kw)
        with pytest.raises(ValueError, match=needle):
            corruption_fields(args["drop"], args["noise"], args["drop_value"], 2)


def test_bucketed_step_forwards_inputs_only_when_given():
    from vae_assoc_amd import parallel

    class Replica:
        def __init__(self):
            self.calls = []

        def _stage(self, *a, **kw):
            self.calls.append((a, kw))

        def _grad_tensor(self):
            return None

    r = Replica()
    parallel.dp_train_step_bucketed(r, None, [], "X", "eps")
    parallel.dp_train_step_bucketed(r, None, [], "X", "eps", "IN")
    assert r.calls == [(("X", "eps"), {}), (("X", "eps"), {"inputs": "IN"})]


def test_denoise_entry_points_are_in_the_abi_and_the_model_surface():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import _capi
    from vae_assoc_amd.vae_assoc import AssocVariationalAutoEncoder
    L = _capi.lib()
    for name in ("avae_set_corruption", "avae_train_steps_in", "avae_eval_cost_in", "avae_stage_batches_in"):
        assert name in _capi.SYMBOLS and hasattr(L, name)
    assert C.sizeof(_capi.Corruption) == 3 * 4 * _capi.AVAE_MAX_MODALITIES
    assert [f[0] for f in _capi.Corruption._fields_] == ["drop_prob", "drop_value", "noise_std"]      # the header's order
    for meth in ("partial_fit", "partial_fit_steps", "evaluate_cost", "_stage"):
        sig = inspect.signature(getattr(AssocVariationalAutoEncoder, meth))
        assert "inputs" in sig.parameters and sig.parameters["inputs"].default is None
    assert inspect.signature(AssocVariationalAutoEncoder.__init__).parameters["corruption"].default is None
    sig = inspect.signature(AssocVariationalAutoEncoder.set_corruption)
    assert [sig.parameters[k].default for k in ("drop", "noise", "drop_value")] == [0.0, 0.0, 0.0]
    # a NULL handle is refused by every new call without touching a device
    assert L.avae_set_corruption(None, None) != 0
