"""The forward-only entry points on the big nets' tile plans (MI355X): generate, avae_decode, reconstruct, score_samples,
log_likelihood and impute on Set A of tests/test_gpu_big_ragged.py (batch 3999, hidden [1003, 605] / [1003, 640] on 784 / 147
inputs, n_z = 40), and generate on the serve plans' route bounds (Set S, n_z = 64, C2 at batch_size 1024).

Until here every test of these plans ran nets of at most 500 units on batches of 16 to 256 rows: K_FWD_OUT_STORE never ran on
128x128 or 64x64 tiles, the serve plan never at a bucket where its fused staging launch does not fit, k_serve_in never beyond two
column slices, and the row kernels of scoring and imputation never read a 784 / 147-wide out32 over thousands of rows.  Every
target is asserted from a dump first (AVAE_DEBUG_SYNC=1 for the by-modality route, AVAE_PLAN_DUMP=1 for the serve plan), then the
numbers go against the fp64 oracle (fp32 compute, relu) or the quant='bf16' oracle (bf16 compute, softplus) at the tolerances of
each entry point's own test file; inputs and references are tests/infer_big_cases.py's, checked on the CPU by
tests/test_infer_big_cpu.py.  One handle per (net, dtype, route) is shared by the module and released at its end."""
import ctypes as C

import numpy as np
import pytest
import torch

import infer_big_cases as cases
from infer_big_cases import B_A, BIN, LAM_A, NZ_A, ROWS_A, SET_A, W_A
from plan_dump import K_FWD_HIDDEN, K_FWD_OUT_STORE, parse, parse_serve, serve_plan, slices, with_switches
from test_gpu_impute import _lat_tol, _same_bits
from test_gpu_loglik import assert_columns
from test_gpu_parity import build_pair
from test_gpu_scoring_edges import ACT, make_pair

pytestmark = pytest.mark.gpu

TOL_X = {"fp32": 1e-5, "bf16": 2e-3}          # generate / reconstruct / decode: of max(1, max |ref|)
TOL_COL = {"fp32": 1e-5, "bf16": 3e-3}        # scores and log-likelihoods: of each column's maximum
TOL_COST = {"fp32": 1e-5, "bf16": 5e-5}       # the training step's cost (check_step_parity's)
SENTINEL = -0x21524111                        # int32 bits of the guard rows (0xDEADBEEF)


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from vae_assoc_amd import vae_assoc
    assert torch.cuda.is_available()
    return vae_assoc


@pytest.fixture(scope="module")
def set_a(V):
    """Set A's handles, one per (dtype, use_graph), built on first use"""
    cache = {}

    def get(dtype, use_graph=True):
        if (dtype, use_graph) not in cache:
            cache[dtype, use_graph] = make_pair(V, SET_A, BIN, W_A, LAM_A, ACT[dtype], B_A, dtype, cases.params_a(), use_graph=use_graph)[0]
        return cache[dtype, use_graph]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _err(got, want):
    """(max |got - want| / max(1, max |want|), where) of one output"""
    d = np.abs(np.asarray(got, np.float64) - want)
    return d.max() / max(1.0, np.abs(want).max()), np.unravel_index(d.argmax(), d.shape)


def _print_columns(what, got, want):
    """worst error of each output relative to its column's maximum (assert_columns' measure), before it is asserted"""
    worst = {}
    for key, r in want.items():
        g2, r2 = np.asarray(got[key], np.float64).reshape(len(r), -1), r.reshape(len(r), -1)
        worst[key] = max(np.abs(g2[:, c] - r2[:, c]).max() / max(np.abs(r2[:, c]).max(), 1e-30) for c in range(r2.shape[1]))
    print(what + ", ".join("%s %.2e" % kv for kv in worst.items()))


def _guarded(rows, cols):
    t = torch.empty((rows + 8, cols), dtype=torch.float32, device="cuda")
    t.view(torch.int32).fill_(SENTINEL)
    return t


def _guard_intact(t, rows):
    return bool((t[rows:].view(torch.int32) == SENTINEL).all())


def _generate_capi(model, zt, rows):
    outs = [_guarded(rows, a["n_input"]) for a in SET_A]
    ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    assert model._L.avae_generate(model._h, zt.data_ptr(), rows, ptrs, model._stream()) == 0, model._L.avae_last_error(model._h)
    torch.cuda.synchronize()
    return outs


def _decode_capi(model, zt, rows):
    outs = [_guarded(rows, a["n_input"]) for a in SET_A]
    for m, o in enumerate(outs):
        assert model._L.avae_decode(model._h, m, zt.data_ptr(), rows, o.data_ptr(), model._stream()) == 0, model._L.avae_last_error(model._h)
    torch.cuda.synchronize()
    return outs


# ----------------------------------------------------------------------------- the plans Set A reaches
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_set_a_plans(V, monkeypatch, capfd, dtype):
    """Computed by hand from finish_launch and found as expected, both dtypes.  By modality (single-item launches): inf_dec
    N = 1003 on 128x128 tiles (cfg 1, 256 tiles), N = 605 / 640 on 64x64 (cfg 0), inf_out N = 784 on cfg 1 and N = 147 on cfg 0.
    Serve plan, bucket 3999: the fused staging launch does not fit (K_SERVE_Z would need cfg 3), serve_dec1 (1003 + 1003) on the
    8-wave 256x128 tiles (cfg 2), serve_dec2 (605 + 640) and serve_out (784 + 147, K_FWD_OUT_STORE through the slot) on cfg 1.
    Bucket 64: fused and lean, k_serve_in with 16 column slices per modality on a grid of 2 x 16."""
    kw = dict(binary=BIN, transfer_fct=ACT[dtype])
    plans = serve_plan(V, monkeypatch, capfd, SET_A, B_A, dtype, B_A + 64, **kw)
    assert sorted(plans) == [64, B_A], sorted(plans)
    big = plans[B_A]
    assert not big["fused_in"] and not big["lean_in"], big
    assert [(n, c) for n, c, _i in big["plan"]] == [("serve_dec1", 2), ("serve_dec2", 1), ("serve_out", 1)], big["plan"]
    assert [(k, M, N) for k, M, N, _K in big["plan"][0][2]] == [(K_FWD_HIDDEN, B_A, 1003)] * 2
    assert [(k, M, N) for k, M, N, _K in big["plan"][1][2]] == [(K_FWD_HIDDEN, B_A, 605), (K_FWD_HIDDEN, B_A, 640)]
    assert [(k, M, N) for k, M, N, _K in big["plan"][2][2]] == [(K_FWD_OUT_STORE, B_A, 784), (K_FWD_OUT_STORE, B_A, 147)]
    small = plans[64]
    assert small["fused_in"] and small["lean_in"] and small["in_lean_grid"] == 2 * 16, small
    assert slices(small) == [16, 16] and small["plan"][0][1] == 3, small["plan"][0]
    assert [n for n, _c, _i in small["plan"]] == ["serve_in+serve_dec1", "serve_dec2", "serve_out"]
    # by modality: AVAE_DEBUG_SYNC=1 runs eagerly, and with it modality by modality
    m = with_switches(monkeypatch, {"AVAE_DEBUG_SYNC": "1"},
                      lambda: V.AssocVariationalAutoEncoder(SET_A, batch_size=B_A, compute_dtype=dtype, **kw))
    capfd.readouterr()
    m.generate(np.zeros((B_A, NZ_A), np.float32))
    m.synchronize()
    plan = parse(capfd.readouterr().err)
    del m
    got = [(n, c, its[0][1], its[0][2]) for n, c, its in plan if n in ("inf_dec", "inf_out")]
    assert got == [("inf_dec", 1, B_A, 1003), ("inf_dec", 0, B_A, 605), ("inf_out", 1, B_A, 784),
                   ("inf_dec", 1, B_A, 1003), ("inf_dec", 0, B_A, 640), ("inf_out", 0, B_A, 147)], got
    assert all(len(its) == 1 for n, _c, its in plan if n in ("inf_dec", "inf_out"))


# ----------------------------------------------------------------------------- 1. generate and avae_decode
@pytest.mark.parametrize("rows", cases.GEN_ROWS)
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_generate_and_decode(set_a, dtype, rows):
    """generate (serve route) and avae_decode (by modality) of 3999 + 159, 3999, 65 and 64 rows: 159 and 65 valid rows run inside
    the 3999-row plan (sp->rows far below the plan's M), 64 rows go to the 64-row bucket.  Through the C ABI the destinations are
    8 rows longer than the call and pre-filled: the extra rows keep their bits.
    Measured on the MI355X, worst error of max(1, max |ref|) over the four row counts, both routes alike: fp32 1.7e-7 (784 columns)
    and 6.5e-7 (147) against 1e-5, bf16 4.7e-4 and 5.6e-4 against 2e-3.  The bitwise tie between the serve route (cfg 2 / 1 / 1)
    and the by-modality route (cfg 1 / 0 / 1 and 1 / 0 / 0) holds at every row count in both dtypes: every tile configuration
    adds a K column in the same order.  It is asserted for bf16, as on the small nets; fp32 is printed."""
    model = set_a(dtype)
    z, want = cases.gen_a(dtype)
    z = z[:rows]
    gen = model.generate(z)
    zt = torch.from_numpy(z).cuda()
    srv, dec = _generate_capi(model, zt, rows), _decode_capi(model, zt, rows)
    for m in range(2):
        assert gen[m].shape == (rows, SET_A[m]["n_input"])
        assert _guard_intact(srv[m], rows) and _guard_intact(dec[m], rows), "rows beyond the call were written (modality %d)" % m
        s, d = srv[m][:rows].cpu().numpy(), dec[m][:rows].cpu().numpy()
        assert _same_bits(s, gen[m]), m                      # the Python surface is the C call
        (es, ws), (ed, wd) = _err(s, want[m][:rows]), _err(d, want[m][:rows])
        tie = _same_bits(s, d)
        print("generate %s rows=%d modality %d: serve err %.3e at %s, by-modality err %.3e at %s (bound %.0e); bitwise tie: %s"
              % (dtype, rows, m, es, ws, ed, wd, TOL_X[dtype], tie))
        assert es <= TOL_X[dtype] and ed <= TOL_X[dtype], (m, es, ws, ed, wd)
        assert tie or dtype == "fp32", (rows, m)             # bf16: bitwise, as tests/test_gpu_parity.py asserts on the small nets


# ----------------------------------------------------------------------------- 2. reconstruct
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_reconstruct(set_a, dtype):
    """3999 + 159 rows with given eps: inf_enc / inf_head, then the decoder's by-modality launches.  Measured: fp32 1.7e-7 / 7.4e-7
    against 1e-5, bf16 1.7e-3 / 1.5e-3 against 2e-3 (the encoder's bf16 roundings come on top of the decoder's)."""
    X, _, eps_m = cases.data_a()
    got, want = set_a(dtype).reconstruct(X, eps=eps_m), cases.recon_a(dtype)
    for m in range(2):
        e, where = _err(got[m], want[m])
        print("reconstruct %s modality %d: err %.3e at %s (bound %.0e)" % (dtype, m, e, where, TOL_X[dtype]))
        assert e <= TOL_X[dtype], (m, e, where)


# ----------------------------------------------------------------------------- 3. scores and log-likelihoods
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_score_samples_cross_modal(set_a, dtype):
    """3999 + 159 rows: the row kernels read out32 with ld32 of a 784 / 147-wide output over thousands of rows.  Measured, worst
    column of each output relative to its maximum: fp32 recon 2.8e-7, latent 8.4e-7, assoc 5.8e-7, cost 3.2e-7, cross 2.6e-7
    against 1e-5; bf16 2.9e-4, 4.8e-4, 2.3e-4, 7.5e-5, 3.4e-4 against 3e-3."""
    X, eps, _ = cases.data_a()
    got = set_a(dtype).score_samples(X, eps=eps, cross_modal=True)
    _print_columns("set A %s score (bound %.0e): " % (dtype, TOL_COL[dtype]), got, cases.score_a(dtype))
    assert_columns(got, cases.score_a(dtype), TOL_COL[dtype], "set A %s score " % dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_log_likelihood(set_a, dtype):
    """K = 3 on 1400 rows: the first SampleBlocks pass decodes 1333 x 3 = 3999 rows, a full bucket, the last 67 x 3 = 201.
    Measured: fp32 marginal 2.9e-7, joint 2.5e-7, conditional 2.2e-7 against 1e-5; bf16 1.8e-4, 1.4e-4, 2.8e-4 against 3e-3."""
    X, eps, want = cases.loglik_a(dtype)
    got = set_a(dtype).log_likelihood(X, n_samples=cases.K_LL, eps=eps)
    _print_columns("set A %s loglik (bound %.0e): " % (dtype, TOL_COL[dtype]), got, want)
    assert_columns(got, want, TOL_COL[dtype], "set A %s loglik " % dtype)


# ----------------------------------------------------------------------------- 4. impute
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_impute_both_routes(set_a, dtype):
    """K = 3, N = 1400, every presence pattern of two modalities: the default (serve) route and use_graph=0 (by modality), each
    against the definition: mu / logvar at _lat_tol, mean and variance within 4x the float32 definition's own deviation from fp64
    on these inputs (impute_reference.rounding_spread).  Measured, kernel / float32 definition, both routes alike: fp32 mean
    2.1e-7 / 1.6e-7 and 4.1e-7 / 3.2e-7, variance 1.3e-6 / 1.1e-6 and 9.0e-7 / 6.0e-7; bf16 mean 8.0e-4 / 8.0e-4 and 7.3e-4 / 5.9e-4,
    variance 4.6e-3 / 4.7e-3 and 3.8e-3 / 3.0e-3.  The two routes are bitwise equal in both dtypes, as on the small nets."""
    X, p, eps, want, dev, _lat = cases.impute_a(dtype)
    res = {}
    for route, use_graph in (("serve", True), ("by modality", False)):
        got = res[route] = set_a(dtype, use_graph).impute(X, p, n_samples=cases.K_LL, eps=eps)
        for key in ("mu", "logvar"):
            assert np.abs(got[key] - want[key]).max() <= _lat_tol(dtype, want[key]), (route, key)
        fails = []
        for d in range(2):
            sm, sv = np.abs(want["mean"][d]).max(), want["var"][d].max()
            em, ev = np.abs(got["mean"][d] - want["mean"][d]).max() / sm, np.abs(got["var"][d] - want["var"][d]).max() / sv
            print("impute %s %s modality %d: mean err %.3e (float32 definition %.3e), var err %.3e (float32 definition %.3e)"
                  % (dtype, route, d, em, dev[d][0], ev, dev[d][1]))
            assert np.all(got["var"][d] >= 0)
            if em > 4 * dev[d][0] or ev > 4 * dev[d][1]:
                fails.append((d, em, dev[d][0], ev, dev[d][1]))
        assert not fails, (route, fails)
    a, b = res["serve"], res["by modality"]
    assert _same_bits(a["mu"], b["mu"]) and _same_bits(a["logvar"], b["logvar"])        # the encoders' launches are the same
    ties = [_same_bits(a[k][d], b[k][d]) for k in ("mean", "var") for d in range(2)]
    print("impute %s: routes bitwise equal (mean0, mean1, var0, var1): %s" % (dtype, ties))
    assert all(ties), ties                                   # as tests/test_gpu_impute.py asserts on the small nets


# ----------------------------------------------------------------------------- 5. the serve plan's route bounds
@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("first", list(cases.S_FIRST))
def test_set_s_route_and_generate(V, monkeypatch, capfd, first, dtype):
    """batch_size 96, n_z = 20, first decoder layers (1024, 40), (1003, 130), (1025, 64): 1024 is k_serve_in's c.N <= 1024 bound
    (16 slices beside a one-slice modality whose workgroups 1-15 idle), 1003 leaves its last slice partial (beside three slices),
    1025 is past the bound (launch_serve + a graph).  The handle is created with AVAE_PLAN_DUMP=1, which only prints: a handle
    without it prints nothing and gives the same bits.  Measured, worst of the five row counts (fp32 against 1e-5 / bf16 against
    2e-3): (1024, 40) 1.6e-7 / 4.0e-4, (1003, 130) 2.4e-7 / 8.9e-8, (1025, 64) 1.9e-7 / 8.3e-5."""
    archs, B, params, z, want = cases.small_case(first, dtype)
    model = with_switches(monkeypatch, {"AVAE_PLAN_DUMP": "1"},
                          lambda: make_pair(V, archs, BIN, W_A, LAM_A, ACT[dtype], B, dtype, params)[0])
    capfd.readouterr()
    got = {rows: model.generate(z[:rows]) for rows in cases.S_ROWS}
    model.synchronize()
    plans = parse_serve(capfd.readouterr().err)
    assert sorted(plans) == [64, 96], sorted(plans)
    for b, sv in plans.items():
        assert sv["fused_in"] == sv["lean_in"] == cases.S_FIRST[first], (b, sv)
        if sv["fused_in"]:
            assert slices(sv) == [(n + 63) // 64 for n in first] and max(slices(sv)) == 16, slices(sv)
            assert sv["in_lean_grid"] == (b + 31) // 32 * 16 and sv["plan"][0][1] == 3, sv
        else:
            assert [n for n, _c, _i in sv["plan"]] == ["serve_dec1", "serve_dec2", "serve_out"], sv["plan"]
    worst = 0.0
    for rows, gen in got.items():
        for m in range(2):
            e, where = _err(gen[m], want[m][:rows])
            worst = max(worst, e)
            assert e <= TOL_X[dtype], (rows, m, e, where)
    if first == (1003, 130):       # without the switch: nothing printed, the same bits
        plain = make_pair(V, archs, BIN, W_A, LAM_A, ACT[dtype], B, dtype, params)[0]
        capfd.readouterr()
        again = {rows: plain.generate(z[:rows]) for rows in cases.S_ROWS}
        plain.synchronize()
        assert "[avae]" not in capfd.readouterr().err
        assert all(_same_bits(again[rows][m], got[rows][m]) for rows in cases.S_ROWS for m in range(2))
    print("set S %s %s: worst generate err %.2e (bound %.0e)" % (first, dtype, worst, TOL_X[dtype]))


@pytest.mark.parametrize("key,buckets", [("nz64", {64: False, 96: False}), ("c2", {64: True, cases.C2_BIG_B: False})])
def test_unfused_serve_plans(V, monkeypatch, capfd, key, buckets):
    """n_z = 64 (n_z + 1 > 64): unfused at both buckets.  C2's nets at batch_size 1024: the staging launch would be 192 tiles of
    64x64, above cfg 3's 128, so bucket 1024 is unfused and bucket 64 fused.  fp32 through test_gpu_parity.build_pair against the
    fp64 oracle, bf16 against the quant='bf16' oracle.  Measured: n_z = 64 2.2e-7 / 2.0e-5, C2 4.0e-7 / 5.4e-4 (bounds 1e-5 / 2e-3)."""
    figures = []
    for dtype in cases.DTYPES:
        archs, B, params, z, want = cases.small_case(key, dtype)
        if dtype == "fp32":
            make = lambda: build_pair(V, archs, BIN, W_A, LAM_A, ACT[dtype], B, dtype, p0=cases.O.flatten_params(archs, params))[0]  # noqa: E731
        else:
            make = lambda: make_pair(V, archs, BIN, W_A, LAM_A, ACT[dtype], B, dtype, params)[0]  # noqa: E731
        model = with_switches(monkeypatch, {"AVAE_PLAN_DUMP": "1"}, make)
        capfd.readouterr()
        row_counts = cases.S_ROWS if key == "nz64" else (64, B, B + 64)
        got = {rows: model.generate(z[:rows]) for rows in row_counts}
        model.synchronize()
        plans = parse_serve(capfd.readouterr().err)
        assert {b: sv["fused_in"] for b, sv in plans.items()} == buckets, (dtype, plans)
        worst = 0.0
        for rows, gen in got.items():
            for m in range(2):
                e, where = _err(gen[m], want[m][:rows])
                worst = max(worst, e)
                assert e <= TOL_X[dtype], (key, dtype, rows, m, e, where)
        figures.append("%s %.2e (bound %.0e)" % (dtype, worst, TOL_X[dtype]))
        del model
    print("%s: worst generate err %s" % (key, ", ".join(figures)))


# ----------------------------------------------------------------------------- 7. a plan rebuilt for another row count
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_rebuilt_plans_give_the_same_bits(set_a, dtype):
    """3999 + 159 rows, then 70 rows, then 3999 + 159 again: build_inference rebuilds the by-modality plan whenever the row count
    changes (3999 -> 159 -> 70 -> 3999 -> 159), the serve route changes bucket; the two long results are bitwise equal."""
    model = set_a(dtype)
    z = cases.gen_a(dtype)[0]
    zt = torch.from_numpy(z).cuda()
    first = [o.clone() for o in _decode_capi(model, zt, ROWS_A)], model.generate(z)
    _decode_capi(model, zt[:70].contiguous(), 70)
    model.generate(z[:70])
    again = _decode_capi(model, zt, ROWS_A), model.generate(z)
    for m in range(2):
        assert torch.equal(first[0][m], again[0][m]) and _same_bits(first[1][m], again[1][m]), m


# ----------------------------------------------------------------------------- 6. training after the forward-only calls
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_training_step_after_forward_only_calls(set_a, dtype):
    """After the calls above on the same handle (in file order; alone, after the calls made here), one partial_fit: its cost is
    the oracle's within the training tolerance (1e-5 / 5e-5), so the forward-only plans left padding rows and constant-1 columns
    intact.  Measured: 3.0e-8 (fp32) and 3.3e-8 (bf16) relative.  The handle's parameters are put back for whoever uses it next."""
    model = set_a(dtype)
    X, eps, want = cases.train_a(dtype)
    model.generate(cases.gen_a(dtype)[0][:65])
    model.score_samples([x[:70] for x in X], eps=eps[:70], cross_modal=True)
    theta = model.get_params()
    try:
        cost = model.partial_fit(X, eps)
    finally:
        model.set_params(theta)
        model.set_opt_state(np.zeros_like(theta), np.zeros_like(theta), 0)
    rel = abs(cost - want) / abs(want)
    print("set A %s: cost after the forward-only calls %.6f, oracle %.6f (rel %.2e, bound %.0e)" % (dtype, cost, want, rel, TOL_COST[dtype]))
    assert rel <= TOL_COST[dtype]
