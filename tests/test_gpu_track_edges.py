"""k_motion_track's exits, classes and edges on a real MI355X (csrc/avae_track.hip), with the helpers, the
bound and the references of tests/test_gpu_track.py: ``iterations``, ``accepted`` and ``status`` are the definition's, the values lie
within 4x the restatement's own error, on cases on which definition and restatement take the same decisions (asserted first, and
without a GPU in tests/test_track_cpu.py).

1. tries the backward pass rejects (a gain not finite as float, a pivot that is NaN) and the try after one; 2. the limit term's
lower branch and the other D classes, E in every class, full and singular, the longest row; 3. a workspace full of stale bytes, and
one that is only 8-byte aligned; 4. factor, lam_max and tol as only the C call takes them; 5. non-finite values where the input scan
ends; 6. the Python call's conversions and chunks.  (The D class tops and the T strides are ``track_cases.SHAPES``'s new shapes, in
test_gpu_track.py.)"""
import numpy as np
import pytest
import torch

import track_cases as TC
from test_gpu_track import OUTPUTS, DTYPES, V, _against, _model, _plan, _same, _track  # noqa: F401  (V: the module's fixture)

pytestmark = pytest.mark.gpu

VALUES = ("trajectory", "controls", "cost0", "cost", "track_rmse")


def _all_same(a, b, rows=slice(None)):
    return all(_same(a[k][rows], b[k][rows]) for k in OUTPUTS)


# ------------------------------------------------------------------------------------------------ 1. the backward pass's exits
REJECTED = tuple((dict(TC.SUBNORMAL, **opt), d, s) for opt, d, s in TC.SUBNORMAL_RUNS) + ((TC.OVERFLOW, "ppppp", 1),)


@pytest.mark.parametrize("run", range(len(REJECTED)), ids=("cap", "lam_max", "then-r", "pivot"))
def test_backward_pass_rejects_every_try(V, run):
    """``track_cases.subnormal_case``: K ~ 1 / dt is finite as double and infinite as float ('cap': five such tries; 'lam_max': three
    and out by lam > lam_max with status 2; 'then-r': six, then six the cost rejects, on the LDS and the gains the rejected ones
    left); 'pivot': l_qq overflows in float and a pivot is NaN.  Nothing may move: the outputs are those of n_iters = 0, bit for bit."""
    model = _model(V)
    c = TC.subnormal_case()
    opt, decisions, status = REJECTED[run]
    r64, r32 = TC.refs(c, **opt)
    assert r64["decisions"] == [decisions] * 3 and (r64["status"] == status).all()
    got = _track(model, c, **opt)
    _against(got, r64, r32, "subnormal dt, %s" % decisions)
    assert (got["accepted"] == 0).all() and _same(got["cost"], got["cost0"])
    still = _track(model, c, **dict(opt, n_iters=0))
    assert all(_same(got[k], still[k]) for k in VALUES)


def test_try_after_a_rejected_backward_pass(V):
    """``track_cases.huge_case``: row 1 takes 'pap' -- its second try starts from the V, G and L and the gains the first left half
    rewritten.  Its float controls hold inf (the doubles are 1e40): non-finite exactly where the restatement's are, within the bound
    elsewhere.  Its neighbours are the rows of the case without the huge value, bit for bit."""
    model = _model(V)
    c = TC.huge_case()
    r64, r32 = TC.refs(c, **TC.HUGE)
    assert r64["decisions"] == ["aaa", "pap", "aaa"]
    got = _track(model, c, **TC.HUGE)
    near = [0, 2]
    _against(*({k: r[k][near] for k in OUTPUTS} for r in (got, r64, r32)), "the neighbours of the huge row")
    assert _all_same(got, _track(model, TC.smooth_case((3, 5, 3)), **TC.HUGE), near)
    g, d, s = ({k: np.array(r[k][1:2], dtype=np.float64) for k in OUTPUTS} for r in (got, r64, r32))
    for k in ("iterations", "accepted", "status"):
        assert np.array_equal(got[k][1:2], r64[k][1:2]), k
    for k in ("trajectory", "controls"):
        off = ~np.isfinite(s[k])
        assert np.array_equal(~np.isfinite(g[k]), off), k
        g[k][off], d[k][off], s[k][off] = 0.0, 0.0, 0.0
    assert (~np.isfinite(r32["controls"][1])).any() and all(np.isfinite(g[k]).all() for k in VALUES)
    err, own = TC.errors(g, d), TC.errors(s, d)
    err.update(cost0=TC.rel_err(g["cost0"], d["cost0"]), track_rmse=TC.rel_err(g["track_rmse"], d["track_rmse"]))
    own.update(cost0=TC.rel_err(s["cost0"], d["cost0"]),                         # (track_rmse: a float output, as in _against)
               track_rmse=max(TC.rel_err(s["track_rmse"], d["track_rmse"]), float(np.finfo(np.float32).eps) / 4))
    print("the huge row kernel / restatement: %s" % ", ".join("%s %.2e / %.2e" % (k, err[k], own[k]) for k in err))
    # This row's costs are its effort term, 1e78, next to which the walk's float error (of a track term of 1e2) is nothing: the
    # restatement's cost0 is the definition's to the bit, and 4x its error asks the kernel for NumPy's order of summation.  The
    # kernel's (lanes, then the butterfly) is another: m = T (2 D^2 + 2 D + 8) roundings of sums of non-negative terms move
    # either result by at most m 2^-53 of it, so the two lie within 2 m 2^-53 = 3.6e-14.
    T, D = c["init"].shape[1:]
    floor = 2.0 * T * (2 * D * D + 2 * D + 8) * 2.0 ** -53
    for k in err:
        assert err[k] <= max(4.0 * own[k], floor if k in ("cost0", "cost") else 0.0), (k, err[k], own[k])


# ------------------------------------------------------------------------------------------------ 2. the terms in every class
@pytest.mark.parametrize("tries", (1, 4))
@pytest.mark.parametrize("name", TC.TERM_CASES)
def test_limit_and_effort_terms(V, name, tries):
    """boxes that bind from below, from above and from both sides at D = 3, 7 and 16; E = I + 0.3 N(0, 1) at D = 3, 4 and 16, and
    with a null direction that lam alone carries; E, a box and R together"""
    model = _model(V)
    c, opt = TC.named(name)
    opt = dict(opt, n_iters=tries, tol=0.0)
    r64, r32 = TC.refs(c, **opt)
    got = _track(model, c, **opt)
    _against(got, r64, r32, "%s after %d" % (name, tries))
    if name in TC.BOXED_CASES:
        live = TC.outside(c, got["trajectory"])
        assert all(TC.outside(c, c["init"])) and live[0] and live[1] and live[3], "the box does not bind on both sides"
    py = model.motion_track(c["path"], c["chain"], init=c["init"], effort=c.get("effort"), limits=c.get("limits"), **opt)
    assert all(_same(py[k], got[k]) for k in OUTPUTS)


def test_longest_widest_row(V):
    """(1, 1024, 16): kTrackMaxT points in the widest class, one try (the restatement's own cost error is 1e-2 there)"""
    model = _model(V)
    c = TC.smooth_case(TC.LONGEST)
    r64, r32 = TC.refs(c, n_iters=1, tol=0.0)
    _against(_track(model, c, n_iters=1, tol=0.0), r64, r32, "smooth-1-1024-16 after 1")


# ------------------------------------------------------------------------------------------------ 3. the workspace
def _on(model, c, ws, offset, **opt):
    n, T, D = c["init"].shape
    return _track(model, c, pointers=dict(workspace=ws.data_ptr() + offset), workspace_bytes=_plan(model, n, T, D), **opt)


@pytest.mark.parametrize("name", ("rejecting", "smooth-2-257-16"))
def test_stale_workspace_bytes_do_not_leak(V, name):
    """a workgroup reads back only what it wrote itself: a workspace of zeros, of 0xFF (every double and float in it a NaN) and one
    another shape has just used give the bits of a fresh one -- at the allocator's alignment and 8 bytes past it"""
    model = _model(V)
    c, opt = TC.named(name)
    opt = dict(opt, tol=0.0, n_iters=8 if name == "rejecting" else 4)
    other = TC.smooth_case((65, 8, 7))
    fresh = _track(model, c, **opt)
    if name == "rejecting":
        assert TC.refs(c, **opt)[0]["decisions"] == ["aaarrrra"]
    size = max(_plan(model, *c["init"].shape), _plan(model, 65, 8, 7)) + 256
    ws = torch.empty((size,), dtype=torch.uint8, device=model.device)
    assert ws.data_ptr() % 256 == 0
    for offset in (0, 8):
        for fill in (0x00, 0xFF):
            ws.fill_(fill)
            assert _all_same(_on(model, c, ws, offset, **opt), fresh), (offset, fill)
        _on(model, other, ws, offset, n_iters=3, tol=0.0)
        assert _all_same(_on(model, c, ws, offset, **opt), fresh), (offset, "after another shape")


def test_workspace_alignment_error(V):
    """4 bytes past an aligned address: refused, and no output written"""
    model = _model(V)
    c = TC.smooth_case((3, 4, 5))
    ws = torch.empty((_plan(model, 3, 4, 5) + 256,), dtype=torch.uint8, device=model.device)
    shapes = dict(trajectory=(3, 4, 5), controls=(3, 3, 5))
    guard = {k: torch.full(shapes.get(k, (3,)), 7, dtype=DTYPES[k], device=model.device) for k in OUTPUTS}
    msg = _track(model, c, expect=2, n_iters=1, workspace_bytes=_plan(model, 3, 4, 5),
                 pointers=dict({k: v.data_ptr() for k, v in guard.items()}, workspace=ws.data_ptr() + 4))
    assert "avae_motion_track" in msg and "aligned to 8 bytes" in msg, msg
    torch.cuda.synchronize()
    assert all((v == 7).all().item() for v in guard.values())


# ------------------------------------------------------------------------------------------------ 4. options of the C call alone
@pytest.mark.parametrize("run", range(len(TC.ABI_RUNS)), ids=tuple(r[0].replace(" ", "-") for r in TC.ABI_RUNS))
def test_options_only_the_c_call_takes(V, run):
    """factor = 2; a lam_max that ends a row after accepted tries (status 0); a tol that ends every row on its first try -- at 0.3
    from the seed repeated by a gain below tol J and above tol J' (asserted in tests/test_track_cpu.py): the old cost is the measure"""
    model = _model(V)
    label, make, opt, decisions, status = TC.ABI_RUNS[run]
    c = make()
    r64, r32 = TC.refs(c, **opt)
    assert all(d == decisions for d in r64["decisions"]) and (r64["status"] == status).all()
    _against(_track(model, c, **opt), r64, r32, label)


# ------------------------------------------------------------------------------------------------ 5. the input scans
@pytest.mark.parametrize("T", (65, 64))
def test_non_finite_last_elements(V, T):
    """NaN and -inf in the last element of a row's path and of its first guess, where the lane-strided scan ends (T = 65: in the
    middle of a wave; T = 64, D = 3: on its last lane): status 3 for that row alone"""
    model = _model(V)
    c = TC.smooth_case((6, T, 3))
    opt = dict(n_iters=2, tol=0.0)
    clean = _track(model, c, **opt)
    path, init = c["path"].copy(), c["init"].copy()
    path[0, -1, -1], init[2, -1, -1], path[3, -1, -1], init[5, -1, -1] = np.nan, np.nan, -np.inf, -np.inf
    got = _track(model, dict(c, path=path, init=init), **opt)
    bad = np.array([True, False, True, True, False, True])
    assert (got["status"][bad] == 3).all() and (got["iterations"][bad] == 0).all() and (got["accepted"][bad] == 0).all()
    assert all(np.isnan(got[k][bad]).all() for k in VALUES)
    assert (clean["status"] == 1).all() and _all_same(got, clean, ~bad)


def test_non_finite_lower_limit_and_single_point_rows(V):
    model = _model(V)
    c = TC.smooth_case((6, 65, 3))
    lim = c["chain"].limits.astype(np.float32)
    lim[2, 0] = np.nan                                             # the last joint's lo: the scan's last but one element
    got = _track(model, dict(c, limits=lim), n_iters=1, limit_weight=1.0)
    assert (got["status"] == 3).all() and all(np.isnan(got[k]).all() for k in VALUES)
    one = TC.smooth_case((3, 1, 3))                                # T = 1: no controls, no try
    clean = _track(model, one)
    init = one["init"].copy()
    init[1, 0, 2] = np.nan
    got = _track(model, dict(one, init=init))
    assert list(got["status"]) == [0, 3, 0] and np.isnan(got["trajectory"][1]).all() and np.isnan(got["cost"][1])
    assert _all_same(got, clean, [0, 2]) and got["controls"].shape == (3, 0, 3)


def test_bad_row_with_optional_outputs_absent(V):
    """controls, cost and track_rmse NULL and a non-finite row among good ones: the outputs asked for lie apart in one arena of
    7s, and every byte of it outside them stays 7"""
    model = _model(V)
    c = TC.smooth_case((6, 65, 3))
    init = c["init"].copy()
    init[4, -1, -1] = np.nan
    bad = dict(c, init=init)
    opt = dict(n_iters=2, tol=0.0)
    whole = _track(model, bad, **opt)
    want = ("trajectory", "cost0", "iterations", "accepted", "status")
    sizes = dict(trajectory=6 * 65 * 3 * 4, cost0=6 * 8, iterations=6 * 4, accepted=6 * 4, status=6 * 4)
    at, end = {}, 512
    for k in want:
        at[k], end = end, end + (sizes[k] + 511) // 256 * 256     # at least 256 bytes of 7s between two outputs
    arena = torch.full((end + 512,), 7, dtype=torch.uint8, device=model.device)
    pointers = {k: arena.data_ptr() + at[k] for k in want}
    pointers.update(controls=None, cost=None, track_rmse=None)
    assert _track(model, bad, want=(), pointers=pointers, **opt) == {}
    host = arena.cpu().numpy()
    inside = np.zeros(host.shape, dtype=bool)
    for k in want:
        inside[at[k]:at[k] + sizes[k]] = True
        assert np.array_equal(host[at[k]:at[k] + sizes[k]], np.ascontiguousarray(whole[k]).view(np.uint8).reshape(-1)), k
    assert (host[~inside] == 7).all()
    assert whole["status"][4] == 3 and (np.delete(whole["status"], 4) == 1).all() and np.isnan(whole["trajectory"][4]).all()


# ------------------------------------------------------------------------------------------------ 6. the Python surface
def test_python_surface_conversions_and_chunks(V):
    model = _model(V)
    c, _ = TC.named("figure")                                      # 5 rows
    opt = dict(n_iters=2, tol=0.0)
    want = _track(model, c, **opt)
    dev = model.motion_track(torch.from_numpy(c["path"]).to(model.device), c["chain"], init=torch.from_numpy(c["init"]).to(model.device), **opt)
    assert all(isinstance(v, torch.Tensor) and v.device == torch.device(model.device) for v in dev.values())
    assert all(_same(dev[k].cpu().numpy(), want[k]) for k in OUTPUTS)
    wide = np.zeros((5, 100, 6))
    wide[:, :, ::2] = c["path"]
    strided = wide[:, :, ::2]
    assert strided.dtype == np.float64 and not strided.flags["C_CONTIGUOUS"]
    assert _all_same(model.motion_track(strided, c["chain"], init=c["init"], **opt), want)
    for chunk in (1, 4):
        try:
            model._track_chunk = chunk
            py = model.motion_track(c["path"], c["chain"], init=c["init"], **opt)
        finally:
            model._track_chunk = None
        assert _all_same(py, want), chunk
    # limits=True is the chain's own
    box, lopt = TC.named("binding")
    lopt = dict(lopt, **opt)
    own = dict(box, limits=box["chain"].limits)
    a = model.motion_track(own["path"], own["chain"], init=own["init"], limits=True, **lopt)
    b = model.motion_track(own["path"], own["chain"], init=own["init"], limits=own["chain"].limits, **lopt)
    assert _all_same(a, b) and _all_same(a, _track(model, own, **lopt))
    assert not _same(a["trajectory"], _track(model, box, **lopt)["trajectory"])      # (and the limits are read)
