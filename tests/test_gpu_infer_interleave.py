"""Every inference call on ONE handle, one after another, on a real MI355X: the forward-only entry points share host helpers,
the encoders' / decoders' activation buffers, the serving slot and their first-use device scratch, so a call must leave nothing
behind that the next one reads.  Each result is compared bitwise with the same call made on a fresh handle of its own with the
same parameters; all noise is given explicitly (eps, z0), so that no result depends on a handle's draw counter.

The smoke nets (784-96-80 / 147-72-40, n_z 20, Bernoulli + Gaussian), batch_size 48, N = 53 rows: two chunks, the second ragged
(5 rows).  log_likelihood runs with K = 3 (16 rows per pass) and K = 50 >= batch_size (one row spans two passes: 48 + 2), impute
with K = 0 and with K = 5 under a mask whose rows lack each modality in turn, and one row both."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, NZ = 48, 53, 20
WIDTHS = (784, 147)


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


def _archs():
    from conftest import make_arch
    return [make_arch("image", 784, 96, 80, NZ), make_arch("joint", 147, 72, 40, NZ)]


def _model(V, dtype, use_graph, flat=None):
    model = V.AssocVariationalAutoEncoder(_archs(), binary=[True, False], transfer_fct="relu", weights=[50, 1], assoc_lambda=8.0,
                                          learning_rate=1e-3, batch_size=B, compute_dtype=dtype, device=0, seed=3,
                                          use_graph=use_graph)
    if flat is not None:
        model.set_params(flat)
    return model


def _inputs():
    from conftest import synth_batch
    rng = np.random.default_rng(11)
    X = synth_batch(rng, N, WIDTHS, [True, False])
    present = np.ones((N, 2), bool)
    present[1::5, 0] = False            # rows without the image, in both chunks (1, 6, ..., 51)
    present[3::7, 1] = False            # rows without the joint vector (3, 10, ..., 52)
    present[50] = False                 # a row with neither, in the ragged chunk
    assert (~present[:, 0] & present[:, 1]).any() and (present[:, 0] & ~present[:, 1]).any() and (~present.any(1)).any()
    observed = [rng.random((N, 784)) < 0.5, None]
    std = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(X=X, present=present, observed=observed, eps=std(N, NZ), eps3=std(N, 3, NZ), eps50=std(N, 50, NZ),
                eps5=std(N, 5, NZ), z0=std(N, NZ), z=std(N, NZ), eps_rec=[std(N, NZ), std(N, NZ)])


def _calls(d):
    """(name, call on a model) in the order handle A makes them"""
    X, p = d["X"], d["present"]
    return [
        ("score_samples", lambda m: m.score_samples(X, eps=d["eps"], cross_modal=True)),
        ("log_likelihood K=3", lambda m: m.log_likelihood(X, n_samples=3, eps=d["eps3"])),
        ("log_likelihood K=50", lambda m: m.log_likelihood(X, n_samples=50, eps=d["eps50"])),
        ("impute K=0", lambda m: m.impute(X, n_samples=0)),
        ("impute K=5 masked", lambda m: m.impute(X, present=p, n_samples=5, eps=d["eps5"])),
        ("complete", lambda m: m.complete(X, observed=d["observed"], n_iters=3, z0=d["z0"])),
        ("generate", lambda m: m.generate(d["z"])),
        ("reconstruct", lambda m: m.reconstruct(X, d["eps_rec"])),
        ("score_samples_masked", lambda m: m.score_samples_masked(X, p, eps=d["eps"], cross_modal=True)),
        ("log_likelihood_masked", lambda m: m.log_likelihood_masked(X, p, n_samples=3, eps=d["eps3"])),
        ("score_samples again", lambda m: m.score_samples(X, eps=d["eps"], cross_modal=True)),
    ]


def _leaves(r, path=""):
    """(path, array) of every array in a result: dicts and lists of arrays, None leaves kept"""
    if isinstance(r, dict):
        return [l for k in sorted(r) for l in _leaves(r[k], "%s[%r]" % (path, k))]
    if isinstance(r, (list, tuple)):
        return [l for i, v in enumerate(r) for l in _leaves(v, "%s[%d]" % (path, i))]
    return [(path, None if r is None else np.ascontiguousarray(np.asarray(r, np.float32)).copy())]


def _assert_same_bits(a, b, what):
    """bit patterns, so that NaNs (the masked calls' absent entries) compare too"""
    assert [p for p, _ in a] == [p for p, _ in b], what
    for (path, x), (_, y) in zip(a, b):
        assert (x is None) == (y is None), what + path
        if x is None:
            continue
        assert x.shape == y.shape, "%s%s: shape %s against %s" % (what, path, x.shape, y.shape)
        diff = x.view(np.uint32) != y.view(np.uint32)
        assert not diff.any(), "%s%s: %d of %d elements differ, first at %s" % (
            what, path, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist())


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_interleaved_calls_equal_fresh_handles(V, dtype, use_graph):
    d = _inputs()
    calls = _calls(d)
    A = _model(V, dtype, use_graph)
    flat = A.get_params()
    m0, v0, step0 = A.get_opt_state()
    g0 = A.get_grads()
    got = [_leaves(call(A)) for _, call in calls]
    for (name, call), a in zip(calls, got):
        assert any(x is not None and x.size for _, x in a), name
        fresh = _model(V, dtype, use_graph, flat)
        _assert_same_bits(a, _leaves(call(fresh)), "%s on the shared handle against a fresh one: " % name)
        del fresh
    _assert_same_bits(got[-1], got[0], "score_samples after every other call against its first result: ")
    # forward only: the handle's parameters, optimiser state and gradient buffer are what they were
    m1, v1, step1 = A.get_opt_state()
    assert step1 == step0
    for what, x, y in (("params", flat, A.get_params()), ("adam m", m0, m1), ("adam v", v0, v1), ("grads", g0, A.get_grads())):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what
