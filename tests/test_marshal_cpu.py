"""CPU checks of the host code every entry point shares: argument marshalling (vae_assoc_amd/_marshal.py) on CPU tensors, the
initial parameter draw pinned by hash, and the construction of the library's config with the constructor's checks.  None of it
needs a GPU or libavae.so."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from vae_assoc_amd import _capi
from vae_assoc_amd import _marshal as Mh
from vae_assoc_amd.vae_assoc import build_config, initial_params

CPU = torch.device("cpu")
WIDTHS = (6, 4)


# ----------------------------------------------------------------------------- one array, leading dimension
def test_column_slice_of_a_wide_matrix_passes_without_a_copy():
    wide = torch.arange(5 * 10, dtype=torch.float32).reshape(5, 10)
    view = wide[:, 6:]
    t, was_np = Mh.dev_array(view, 4, CPU)
    assert not was_np and t.data_ptr() == view.data_ptr() == wide.data_ptr() + 6 * 4
    assert Mh.ld_of(t) == 10
    ts, rows, was_np, ptrs, lds = Mh.dev_modalities([wide[:, :6], view], WIDTHS, CPU)
    assert rows == 5 and was_np is False
    assert list(ptrs) == [wide.data_ptr(), view.data_ptr()] and list(lds) == [10, 10]
    assert isinstance(ptrs, C.c_void_p * 2) and isinstance(lds, C.c_int32 * 2)


def test_one_row_reports_the_width_as_leading_dimension():
    wide = torch.zeros(3, 10)
    t, _ = Mh.dev_array(wide[1:2, 6:], 4, CPU)
    assert t.shape == (1, 4) and t.data_ptr() == wide[1:2, 6:].data_ptr() and Mh.ld_of(t) == 4
    assert list(Mh.dev_modalities([wide[:1, :6], wide[:1, 6:]], WIDTHS, CPU)[4]) == [6, 4]


def test_non_unit_column_stride_and_overlapping_rows_are_copied():
    wide = torch.arange(40, dtype=torch.float32).reshape(5, 8)
    t, _ = Mh.dev_array(wide[:, ::2], 4, CPU)
    assert t.data_ptr() != wide.data_ptr() and t.is_contiguous() and torch.equal(t, wide[:, ::2]) and Mh.ld_of(t) == 4
    row = torch.arange(4, dtype=torch.float32)
    t, _ = Mh.dev_array(row.expand(3, 4), 4, CPU)            # row stride 0 < width
    assert t.is_contiguous() and Mh.ld_of(t) == 4 and torch.equal(t[2], row)


def test_numpy_and_other_dtypes_become_float32():
    t, was_np = Mh.dev_array(np.arange(8, dtype=np.float64).reshape(2, 4), 4, CPU)
    assert was_np and t.dtype == torch.float32 and t.shape == (2, 4)
    t, was_np = Mh.dev_array([[1, 2, 3, 4]], 4, CPU)
    assert was_np and t.dtype == torch.float32
    t, was_np = Mh.dev_array(torch.ones(2, 4, dtype=torch.float64), 4, CPU)
    assert not was_np and t.dtype == torch.float32


@pytest.mark.parametrize("bad", [np.zeros((3, 5)), np.zeros(4), np.zeros((2, 2, 4)), None, torch.zeros(3, 5)])
def test_a_wrong_shape_is_a_value_error(bad):
    with pytest.raises(ValueError):
        Mh.dev_array(bad, 4, CPU)


# ----------------------------------------------------------------------------- a list of modalities
def test_none_modality_is_null_with_ld_zero_only_where_allowed():
    x1 = torch.zeros(3, 4)
    ts, rows, was_np, ptrs, lds = Mh.dev_modalities([None, x1], WIDTHS, CPU, allow_none=True)
    assert ts[0] is None and ts[1] is x1 and rows == 3 and was_np is False
    assert ptrs[0] is None and ptrs[1] == x1.data_ptr() and list(lds) == [0, 4]
    with pytest.raises(ValueError):
        Mh.dev_modalities([None, x1], WIDTHS, CPU)
    ts, rows, was_np, ptrs, lds = Mh.dev_modalities([None, None], WIDTHS, CPU, rows=7, what="present has 7", allow_none=True)
    assert ts == [None, None] and rows == 7 and was_np is None and list(ptrs) == [None, None] and list(lds) == [0, 0]
    assert Mh.dev_modalities([None, None], WIDTHS, CPU, allow_none=True)[1] is None


def test_numpy_flag_is_the_first_given_modalitys():
    a, b = np.zeros((2, 6), np.float32), torch.zeros(2, 4)
    assert Mh.dev_modalities([a, b], WIDTHS, CPU)[2] is True
    assert Mh.dev_modalities([torch.zeros(2, 6), b.numpy()], WIDTHS, CPU)[2] is False
    assert Mh.dev_modalities([None, b.numpy()], WIDTHS, CPU, allow_none=True)[2] is True


def test_row_args_take_rows_and_the_fallback_numpy_flag_from_present():
    a, b = np.zeros((3, 6), np.float32), torch.zeros(3, 4)
    ts, rows, was_np, ptrs, lds, p = Mh.dev_row_args([a, b], WIDTHS, CPU)
    assert rows == 3 and was_np is True and p is None and list(lds) == [6, 4]
    pres = np.array([[1, 0], [0, 2], [0, 0]])
    ts, rows, was_np, ptrs, lds, p = Mh.dev_row_args([None, b], WIDTHS, CPU, pres)
    assert rows == 3 and was_np is False and p.dtype == torch.uint8 and p.tolist() == [[1, 0], [0, 1], [0, 0]]
    assert list(ptrs) == [None, b.data_ptr()] and list(lds) == [0, 4]
    assert Mh.dev_row_args([None, None], WIDTHS, CPU, pres)[1:3] == (3, True)                 # nothing given: present decides
    assert Mh.dev_row_args([None, None], WIDTHS, CPU, torch.from_numpy(pres))[1:3] == (3, False)
    assert Mh.dev_row_args([None, None], WIDTHS, CPU, pres[:0])[1] == 0
    with pytest.raises(ValueError, match=r"modality 1: expected 2 rows \(present has 2\), got 3"):
        Mh.dev_row_args([None, b], WIDTHS, CPU, pres[:2])
    with pytest.raises(ValueError, match=r"present must be \[rows, 2\], got \(3,\)"):
        Mh.dev_row_args([a, b], WIDTHS, CPU, pres[:, 0])
    with pytest.raises(ValueError):
        Mh.dev_row_args([None, b], WIDTHS, CPU)                                              # None needs a presence


def test_row_count_sources_and_their_errors():
    a, b = torch.zeros(3, 6), torch.zeros(2, 4)
    with pytest.raises(ValueError, match=r"modality 1: expected 3 rows \(as modality 0\), got 2"):
        Mh.dev_modalities([a, b], WIDTHS, CPU)
    with pytest.raises(ValueError, match=r"modality 0: expected 2 rows \(batch_size\), got 3"):
        Mh.dev_modalities([a, b], WIDTHS, CPU, rows=2, what="batch_size")
    with pytest.raises(ValueError, match="expected a list of 2 modalities, got 1"):
        Mh.dev_modalities([a], WIDTHS, CPU)
    with pytest.raises(ValueError, match=r"expected a \[rows, 4\] array"):
        Mh.dev_modalities([a, torch.zeros(3, 5)], WIDTHS, CPU)
    assert Mh.dev_modalities([a[:0], b[:0]], WIDTHS, CPU)[1] == 0


# ----------------------------------------------------------------------------- presence
@pytest.mark.parametrize("make", [
    lambda v: v.astype(bool), lambda v: v.astype(np.int8) * -3, lambda v: v.astype(np.float64) * 0.25,
    lambda v: torch.from_numpy(v.astype(bool)), lambda v: torch.from_numpy(v.astype(np.int8) * 5),
    lambda v: torch.from_numpy(v.astype(np.float32) * -0.5), lambda v: torch.from_numpy(v.astype(np.int64)).t().contiguous().t(),
    lambda v: v.tolist()])
def test_presence_from_bool_int_and_float_arrays_and_tensors(make):
    v = np.array([[1, 0], [0, 0], [1, 1], [0, 1]], dtype=np.uint8)
    p = Mh.dev_flags(make(v), 2, CPU)
    assert p.dtype == torch.uint8 and p.is_contiguous() and p.device == CPU and np.array_equal(p.numpy(), v)
    assert Mh.dev_flags(make(v), 2, CPU, rows=4, what="batch_size").shape == (4, 2)


def test_presence_shape_errors_state_both_shapes():
    with pytest.raises(ValueError, match=r"present must be \[rows, 2\], got \(4, 3\)"):
        Mh.dev_flags(np.ones((4, 3)), 2, CPU)
    with pytest.raises(ValueError, match=r"present must be \[8 \(batch_size x n_steps\), 2\], got \(4, 2\)"):
        Mh.dev_flags(np.ones((4, 2)), 2, CPU, rows=8, what="batch_size x n_steps")
    with pytest.raises(ValueError, match=r"observed\[1\] must be \[4 \(as X\[1\]\), 2\], got \(8,\)"):
        Mh.dev_flags(np.ones(8), 2, CPU, rows=4, what="as X[1]", name="observed[1]")


# ----------------------------------------------------------------------------- eps and the optional pointer
def test_eps_forms_and_the_optional_pointer():
    assert Mh.dev_dense(None, 5, CPU, 3) is None and Mh.dev_dense3(None, (3, 2, 5), CPU) is None and Mh.ptr(None) is None
    wide = torch.zeros(3, 9)
    e = Mh.dev_dense(wide[:, :5], 5, CPU, 3)
    assert e.is_contiguous() and e.shape == (3, 5) and Mh.ptr(e) == e.data_ptr() != wide.data_ptr()
    assert Mh.dev_dense(np.zeros((3, 5)), 5, CPU).dtype == torch.float32
    with pytest.raises(ValueError, match=r"eps must be \[4, 5\], got \(3, 5\)"):
        Mh.dev_dense(np.zeros((3, 5)), 5, CPU, 4)
    with pytest.raises(ValueError, match=r"z0 must be \[4 \(batch_size\), 5\], got \(3, 5\)"):
        Mh.dev_dense(np.zeros((3, 5)), 5, CPU, 4, "batch_size", name="z0")
    with pytest.raises(ValueError):
        Mh.dev_dense(np.zeros((3, 6)), 5, CPU, 3)
    e3 = Mh.dev_dense3(np.zeros((3, 2, 5)), (3, 2, 5), CPU)
    assert e3.dtype == torch.float32 and e3.is_contiguous()
    assert Mh.dev_dense3(torch.zeros(3, 5, 2, dtype=torch.float64).transpose(1, 2), (3, 2, 5), CPU).is_contiguous()
    with pytest.raises(ValueError, match=r"eps must be \[3, 2, 5\], got \(3, 5\)"):
        Mh.dev_dense3(np.zeros((3, 5)), (3, 2, 5), CPU)


# ----------------------------------------------------------------------------- one scalar
def refusal(call, *args):
    with pytest.raises(ValueError) as e:
        call(*args)
    return str(e.value)


@pytest.mark.parametrize("v", [0, 7, np.int8(7), np.uint64(7), np.int64(0)])
def test_as_int_and_as_index_take_python_and_numpy_integers(v):
    assert Mh.as_int(v, "n", 0) == int(v) and type(Mh.as_int(v, "n", 0, 7)) is int
    assert Mh.as_index(v, "m", 8) == int(v) and type(Mh.as_index(v, "m", 8)) is int
    assert Mh.as_int(2 ** 64 - 1, "seed", 0, 2 ** 64 - 1) == 2 ** 64 - 1 and Mh.as_int(-3, "n", -3) == -3


@pytest.mark.parametrize("bad", [True, np.bool_(False), 1.0, np.float32(2), "1", None, [1], -1, 9], ids=repr)
def test_as_int_and_as_index_refuse_with_the_shared_wording(bad):
    assert refusal(Mh.as_int, bad, "n_iters", 0, 8) == "n_iters must be an integer in [0, 8], got %r" % (bad,)
    assert refusal(Mh.as_index, bad, "modality", 9) == "modality must be an index in [0, 9), got %r" % (bad,)
    if not isinstance(bad, int) or isinstance(bad, bool) or bad < 0:
        assert refusal(Mh.as_int, bad, "state: iteration", 0) == "state: iteration must be an integer >= 0, got %r" % (bad,)


def test_as_int_formats_a_64_bit_upper_end_and_a_tuple_value():
    assert refusal(Mh.as_int, 2 ** 64, "seed", 0, 2 ** 64 - 1) == "seed must be an integer in [0, 18446744073709551615], got 18446744073709551616"
    assert refusal(Mh.as_int, (1, 2), "k", 1) == "k must be an integer >= 1, got (1, 2)"
    assert refusal(Mh.as_index, 0, "source", 0) == "source must be an index in [0, 0), got 0"


def test_need_type_names_the_class_and_the_type_it_got():
    from vae_assoc_amd.motion import MotionBasis
    assert Mh.need_type(MotionBasis(n_basis=3, n_dof=2, n_points=5), MotionBasis, "basis") is None
    assert refusal(Mh.need_type, "basis", MotionBasis, "basis") == "basis must be a MotionBasis, got 'str'"
    assert refusal(Mh.need_type, None, dict, "state") == "state must be a dict, got 'NoneType'"


def test_to_device32_gives_a_contiguous_float32_copy():
    t = Mh.to_device32(np.arange(6, dtype=np.float64).reshape(2, 3).T, CPU)
    assert t.dtype == torch.float32 and t.is_contiguous() and t.tolist() == [[0.0, 3.0], [1.0, 4.0], [2.0, 5.0]]


def test_posterior_rows_concatenates_in_list_order_and_masks_non_finite_rows():
    from vae_assoc_amd._args import posterior_rows
    mu, lv = np.arange(12, dtype=np.float32).reshape(3, 4), np.zeros((3, 4), np.float32)
    m, l, fin, was_np = posterior_rows((mu, lv), 4, CPU, True)
    assert was_np and l is not None and np.array_equal(m.numpy(), mu) and fin.tolist() == [True] * 3
    m, l, fin, was_np = posterior_rows((torch.from_numpy(mu), None), 4, CPU, False)
    assert not was_np and l is None and m.data_ptr() == torch.from_numpy(mu).data_ptr()              # one pair: no copy
    mu2, lv2 = mu[:2].copy(), lv[:2].copy()
    mu2[0, 1], lv2[1, 3] = np.nan, np.inf
    m, l, fin, was_np = posterior_rows([(torch.from_numpy(mu), torch.from_numpy(lv)), (mu2, lv2)], 4, CPU, True)
    assert not was_np and m.shape == l.shape == (5, 4) and m.is_contiguous() and fin.tolist() == [True, True, True, False, False]
    assert np.array_equal(m.numpy()[:3], mu) and np.array_equal(l.numpy()[3:], lv2)
    m, l, fin, _ = posterior_rows([(mu, lv), (mu2, lv2)], 4, CPU, False)                              # logvar not looked at
    assert l is None and fin.tolist() == [True, True, True, False, True]
    assert posterior_rows((mu[:0], None), 4, CPU, False)[2].shape == (0,)


def test_posterior_rows_refusals():
    from vae_assoc_amd._args import posterior_rows
    mu = np.zeros((3, 4), np.float32)
    for bad in ([], mu, [(mu, mu), mu], None, ((mu, mu, mu),)):
        assert refusal(posterior_rows, bad, 4, CPU, True) == ("posteriors must be a (mu, logvar) pair or a non-empty list of such "
                                                              "pairs, got %r" % type(bad).__name__)
    assert refusal(posterior_rows, [(mu, mu), (mu, mu[:2])], 4, CPU, True) == "posteriors[1]: logvar must be [3 (as mu), 4], got (2, 4)"
    assert refusal(posterior_rows, (np.zeros((3, 5)), None), 4, CPU, False) == "posteriors[0]: expected a [rows, 4] array, got (3, 5)"
    assert posterior_rows([(mu, mu), (mu, mu[:2])], 4, CPU, False)[0].shape == (6, 4)


# ----------------------------------------------------------------------------- the initial draw
IMG = dict(scope='image', hidden_conv=False, n_hidden_recog_1=96, n_hidden_recog_2=80,
           n_hidden_gener_1=96, n_hidden_gener_2=80, n_input=784, n_z=20)
JNT = dict(scope='joint', hidden_conv=False, n_hidden_recog_1=72, n_hidden_recog_2=40,
           n_hidden_gener_1=72, n_hidden_gener_2=40, n_input=147, n_z=20)
CONV = dict(scope='image', hidden_conv=True, n_hidden_recog_1=16, n_hidden_recog_2=64,
            n_hidden_gener_1=64, n_hidden_gener_2=16, n_input=784, n_z=20)
DEEP = dict(scope='deep', hidden_conv=False, n_hidden=[48, 40, 32], n_hidden_recog_1=0, n_hidden_recog_2=0,
            n_hidden_gener_1=0, n_hidden_gener_2=0, n_input=60, n_z=20)


@pytest.mark.parametrize("archs, seed, n_params, digest", [
    ([IMG, JNT], 3, 185315, "8f23f52d2ba776478f4db10c719646e3678119971db580ab1aca3fbf1c158f33"),
    ([CONV, JNT], 0, 804628, "a0d1049938743d2ed6ba9a9df5ac06e9dd529b5fdccd16d878add6bb6f12abc4"),
    ([DEEP, JNT], 2 ** 31 + 5, 39455, "44d03d11bc02e938abff1920eeb1fab7b660440d7cfbce9cc4cd405041a22d87"),
], ids=["mlp", "conv", "deep"])
def test_initial_draw_is_the_one_it_has_always_been(archs, seed, n_params, digest):
    flat = initial_params(archs, seed)
    assert flat.dtype == np.float32 and flat.shape == (n_params,)
    assert hashlib.sha256(flat.tobytes()).hexdigest() == digest


# ----------------------------------------------------------------------------- the config
def config(archs=(IMG, JNT), binary=(True, False), weights=(50, 1), transfer_fct="relu", assoc_lambda=8.0, learning_rate=1e-3,
           batch_size=48, compute_dtype="bf16", seed=3, use_graph=True, comm=None, comm_buckets=2, wire_dtype="fp32",
           placement=lambda: (0, 1, 0)):
    return build_config(list(archs), list(binary), list(weights), transfer_fct, assoc_lambda, learning_rate, batch_size,
                        compute_dtype, seed, use_graph, comm, comm_buckets, wire_dtype, placement)


def test_config_of_the_smoke_model():
    cfg, binary, weights, act, comm = config(seed=-1, comm="ipc", comm_buckets=1, wire_dtype="bf16", placement=lambda: (2, 4, 3))
    assert (binary, weights, act, comm) == ([True, False], [50, 1], "relu", "ipc")
    assert cfg.abi_version == _capi.AVAE_ABI_VERSION and cfg.n_modalities == 2 and cfg.n_z == 20
    assert [cfg.mod[m].n_input for m in range(2)] == [784, 147]
    assert [list(cfg.mod[m].n_hidden[:cfg.mod[m].n_hidden_layers]) for m in range(2)] == [[96, 80], [72, 40]]
    assert [(cfg.mod[m].binary, cfg.mod[m].weight, cfg.mod[m].hidden_conv) for m in range(2)] == [(1, 50.0, 0), (0, 1.0, 0)]
    assert (cfg.batch_size, cfg.batch_global, cfg.row_offset, cfg.device) == (48, 48 * 4, 3 * 48, 2)
    assert cfg.compute_dtype == _capi.DTYPE_IDS["bf16"] == 1 and cfg.activation == _capi.ACT_IDS["relu"]
    assert cfg.seed == 0xFFFFFFFFFFFFFFFF and cfg.use_graph == 1
    assert (cfg.comm_buckets, cfg.wire_dtype) == (1, _capi.DTYPE_IDS["bf16"])
    assert (cfg.assoc_lambda, cfg.learning_rate) == (8.0, np.float32(1e-3)) and cfg.beta1 == cfg.beta2 == cfg.adam_eps == 0.0
    assert cfg.use_comm == _capi.COMM_NONE and cfg.workspace is None            # the collective and the workspace come later
    cfg, binary, weights, act, comm = build_config([IMG, JNT], True, 1.0, None, 1.0, 0.001, 100, "fp32", 3, False, None, 2, "fp32",
                                                   lambda: (0, 1, 0))
    assert (binary, weights, act, comm) == ([True, True], [1.0, 1.0], "identity", "torch")
    assert (cfg.batch_global, cfg.row_offset, cfg.compute_dtype, cfg.use_graph, cfg.seed) == (100, 0, 0, 0, 3)
    cfg = config(archs=(CONV, JNT))[0]
    assert cfg.mod[0].hidden_conv == 1 and list(cfg.mod[0].n_hidden[:2]) == [16, 64] and list(cfg.mod[0].conv_gener) == [64, 16]
    cfg = config(archs=(DEEP, JNT))[0]
    assert cfg.mod[0].n_hidden_layers == 3 and list(cfg.mod[0].n_hidden[:3]) == [48, 40, 32]


@pytest.mark.parametrize("kw", [
    dict(archs=(IMG, dict(JNT, n_z=21))),
    dict(archs=(JNT,) * 5, binary=(False,) * 5, weights=(1,) * 5),
    dict(archs=(dict(DEEP, n_hidden=[8] * 9), JNT)),
    dict(compute_dtype="fp16"),
    dict(comm="mpi"), dict(comm_buckets=3), dict(wire_dtype="fp8"),
    dict(archs=(dict(CONV, n_input=1024), JNT)),
    dict(archs=(CONV, JNT), binary=(False, False)),
    dict(transfer_fct="gelu"),
], ids=["n_z", "modalities", "hidden", "compute_dtype", "comm", "comm_buckets", "wire_dtype", "conv_width", "conv_binary", "act"])
def test_config_refuses(kw):
    with pytest.raises(ValueError):
        config(**kw)


def test_config_checks_keep_the_constructors_order():
    """The architecture and dtype checks come before the device and the process group are opened, the collective's after."""
    def no_device():
        raise RuntimeError("no device")
    with pytest.raises(ValueError, match="share n_z"):
        config(archs=(IMG, dict(JNT, n_z=21)), comm="mpi", placement=no_device)
    with pytest.raises(ValueError, match="compute_dtype"):
        config(compute_dtype="fp16", placement=no_device)
    with pytest.raises(RuntimeError, match="no device"):
        config(comm="mpi", placement=no_device)
    with pytest.raises(AssertionError):
        config(binary=(True,))
    with pytest.raises(ValueError, match="comm must be"):
        config(comm="mpi", archs=(dict(DEEP, n_hidden=[8] * 9), JNT))
